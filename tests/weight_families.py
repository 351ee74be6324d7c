"""Models with other weights than the three shipped ones, made at test time from seeds and from
the shipped ``.dbw`` files (a plain module, no committed fixtures).

The shipped models share one corner of the weight space: every batch-norm gamma is positive,
kernels have a standard deviation of 1.3 .. 4.9, pre-BN activations reach 3.5e7.  A step that is
only right for a positive BN scale (BN applied before a max-pool, ``|scale|``) computes the same
bits as the right one there.  The families below leave that corner:

* ``flipped``       the same function exactly, half of every BN's output channels negated;
* ``random_model``  freshly initialised sizes: He kernels, BN scales near +-1, some exactly 0;
* ``ranged``        the same function, pre-BN2 activations 2^a times larger;
* ``dead``          every ReLU of conv1d_2 .. conv1d_19 outputs 0;
* ``constant``      conv1d_20's kernel zero: the logits are ``relu(bias)`` whatever the input.
"""
import numpy as np

from deepbinner_amd.model_format import BN_CHANNELS, BN_EPSILON, ModelWeights, conv_shapes

# batch normalisation i (1-based) -> the convolutions (1-based) that read its output; BN4 reaches
# conv1d_10 through the average pool, which is linear and so keeps a negated channel negated
BN_CONSUMERS = {1: [2], 2: [5], 3: [8], 4: [10, 11, 12, 14], 5: [17], 6: [18], 7: [20]}


def _copy(weights):
    convs = [(k.copy(), b.copy()) for k, b in weights.convs]
    bns = [tuple(a.copy() for a in bn) for bn in weights.bns]
    return convs, bns


def flipped(weights, seed, frac=0.5):
    """For a random ``frac`` of each BN's channels: gamma and beta negated (so scale and shift are,
    and the BN output), and the rows of every consumer kernel that read those channels negated.
    Negation is exact in every precision and zero padding stays zero: the same function."""
    rng = np.random.default_rng(seed)
    convs, bns = _copy(weights)
    for i, c_n in enumerate(BN_CHANNELS, start=1):
        ch = np.sort(rng.choice(c_n, int(round(frac * c_n)), replace=False))
        gamma, beta, mean, var = bns[i - 1]
        gamma[ch] = -gamma[ch]
        beta[ch] = -beta[ch]
        for j in BN_CONSUMERS[i]:
            kernel = convs[j - 1][0]
            kernel[:, ch, :] = -kernel[:, ch, :]
    return ModelWeights(weights.n_classes, convs, bns, input_size=weights.input_size)


def random_model(seed, n_classes, negative=0.3, input_size=1024):
    """Kernels N(0, variance 2 / (k C_in)) (He), biases N(0, std 0.1), gamma +-exp(N(0, std 0.5))
    with ``negative`` of the channels negative and two channels of every BN exactly 0, beta
    N(0, std 0.5), moving mean N(0.5, std 0.5), moving variance exp(N(0, std 1))."""
    rng = np.random.default_rng([seed, n_classes])
    convs = []
    for _, k, cin, cout, _, _ in conv_shapes(n_classes):
        kernel = rng.standard_normal((k, cin, cout)) * np.sqrt(2.0 / (k * cin))
        bias = rng.standard_normal(cout) * 0.1
        convs.append((kernel.astype(np.float32), bias.astype(np.float32)))
    bns = []
    for c_n in BN_CHANNELS:
        gamma = np.exp(rng.standard_normal(c_n) * 0.5)
        gamma[rng.random(c_n) < negative] *= -1.0
        gamma[rng.choice(c_n, 2, replace=False)] = 0.0
        beta = rng.standard_normal(c_n) * 0.5
        mean = 0.5 + rng.standard_normal(c_n) * 0.5
        var = np.exp(rng.standard_normal(c_n))
        bns.append(tuple(a.astype(np.float32) for a in (gamma, beta, mean, var)))
    return ModelWeights(n_classes, convs, bns, input_size=input_size)


def ranged(weights, a):
    """conv1d_4's kernel and bias and BN2's moving mean times 2^a, BN2's variance
    (var + eps) 4^a - eps: BN2's scale is 2^-a times what it was and its shift the same, so the
    function is the same with pre-BN2 activations 2^a times larger (up to the rounding of the new
    variance to fp32).  a > 0 only: a < 0 would make the variance negative."""
    assert a > 0
    convs, bns = _copy(weights)
    kernel, bias = convs[3]
    convs[3] = (np.ldexp(kernel, a), np.ldexp(bias, a))
    gamma, beta, mean, var = bns[1]
    var = (var.astype(np.float64) + BN_EPSILON) * 4.0 ** a - BN_EPSILON
    assert np.isfinite(var.astype(np.float32)).all()
    bns[1] = (gamma, beta, np.ldexp(mean, a), var.astype(np.float32))
    return ModelWeights(weights.n_classes, convs, bns, input_size=weights.input_size)


DEAD_BIAS = -1.0e6


def dead(weights):
    """The biases of conv1d_2 .. conv1d_19 at -1e6: every ReLU behind stage A outputs 0, so the
    stages B .. G are the BN shifts at every position.  For models whose activations stay far
    below 1e6 (``random_model``: below 2,000)."""
    convs, bns = _copy(weights)
    for i in range(1, 19):
        convs[i] = (convs[i][0], np.full_like(convs[i][1], DEAD_BIAS))
    return ModelWeights(weights.n_classes, convs, bns, input_size=weights.input_size)


def bn_shift(bn, dtype=np.float64):
    """The shift of oracle/network_ref.py: batch_norm, which is BN(0)."""
    gamma, beta, mean, var = (a.astype(dtype) for a in bn)
    return beta - mean * (gamma / np.sqrt(var + dtype(BN_EPSILON)))


def constant(weights, bias):
    """conv1d_20's kernel zero and its bias ``bias`` (which sets the class count): the logits are
    ``relu(bias)`` for every window whatever happens upstream."""
    bias = np.asarray(bias, dtype=np.float32)
    convs, bns = _copy(weights)
    convs[-1] = (np.zeros((1, 48, len(bias)), dtype=np.float32), bias.copy())
    return ModelWeights(len(bias), convs, bns, input_size=weights.input_size)


def constant_biases(n_classes):
    """name -> conv1d_20 bias: exact ties for the top place (two barcodes; three from 3 classes
    on, the last class among them), a spread above 200 with the top in a barcode class and
    negative entries (logit 0 after the ReLU), and all equal."""
    rng = np.random.default_rng(n_classes)
    ties = np.round(rng.uniform(-2.0, 6.0, n_classes) * 8) / 8          # below the top, exact
    top = [1] if n_classes == 2 else sorted({1, n_classes // 2, n_classes - 1})
    ties[top] = 7.5
    if n_classes == 2:
        ties[0] = 7.5
    spread = np.linspace(-20.0, 230.0, n_classes)
    spread = spread[rng.permutation(n_classes)]
    j = int(np.argmax(spread))
    if j == 0:                                    # the top place goes to a barcode
        spread[[0, 1]] = spread[[1, 0]]
    return {'ties': ties.astype(np.float32), 'spread': spread.astype(np.float32),
            'equal': np.full(n_classes, 3.0, dtype=np.float32)}


def constant_logits(bias, n_windows):
    """The closed form: relu(bias) for every window, in float64."""
    z = np.maximum(np.asarray(bias, dtype=np.float32).astype(np.float64), 0.0)
    return np.repeat(z[None, :], n_windows, axis=0)


# ---- the models and inputs of the device tests (tests/test_gpu_weight_families.py), by name, so
# that tests/test_weight_families.py can hold every one of them to the conditioning cap -------
RANDOM_CLASSES = [2, 13, 17, 32]
RANDOM_SEEDS = [0, 1, 2]
# the general path: the shipped size forced, and three sizes of general_fixtures.PARITY_GEOMETRIES
GENERAL_GEOMETRIES = [(1024, 13), (98, 13), (1502, 17), (16382, 13)]
# ... and the smallest sizes of that list with their own class counts, for ``random_model`` alone
RANDOM_ONLY_GEOMETRIES = [(96, 2), (112, 33), (160, 256)]


def persistent_models():
    """name -> (builder, inputs: 'all' | 'normalised', side, classify checks too?)."""
    from conftest import PLAN
    from general_fixtures import STARTS, shipped
    out = {}
    for k, (model, side) in enumerate(PLAN):
        out['flipped-' + model] = (lambda m=model, k=k: flipped(shipped(m), 100 + k), 'all', side,
                                   True)
    for c in RANDOM_CLASSES:
        for seed in RANDOM_SEEDS:
            out['random-C{}-s{}'.format(c, seed)] = (
                lambda c=c, seed=seed: random_model(seed, c), 'all', 'start', seed == 0)
    out['ranged-24'] = (lambda: ranged(shipped(STARTS), 24), 'normalised', 'start', False)
    out['ranged-28'] = (lambda: ranged(shipped(STARTS), 28), 'normalised', 'start', True)
    out['dead'] = (lambda: dead(random_model(0, 13)), 'all', 'start', False)
    return out


def general_models():
    """name -> (builder, inputs: 'all' | 'normalised')."""
    from general_fixtures import geometry
    out = {}
    for size, c in GENERAL_GEOMETRIES:
        tag = 'L{}-C{}'.format(size, c)
        out['flipped-' + tag] = (lambda size=size, c=c: flipped(geometry(size, c), size), 'all')
        out['random-' + tag] = (lambda size=size, c=c: random_model(size, c, input_size=size),
                                'all')
        out['ranged-40-' + tag] = (lambda size=size, c=c: ranged(geometry(size, c), 40),
                                   'normalised')
    for size, c in RANDOM_ONLY_GEOMETRIES:
        out['random-L{}-C{}'.format(size, c)] = (
            lambda size=size, c=c: random_model(size, c, input_size=size), 'all')
    out['dead-L1024-C13'] = (lambda: dead(random_model(0, 13)), 'all')
    return out


def family_windows(input_size=1024, inputs='all'):
    """Shipped size: the first 40 golden start windows (z-normalised) plus the five synthetic
    windows of test_gpu_log_space.py - 45, not a multiple of the group of four.  Other sizes: the
    windows of the seven golden reads at three scan steps, plus the synthetic five.  'normalised'
    leaves the synthetic ones (the 50x amplitude window among them) out and takes three more
    golden windows at the shipped size, 43: not a multiple of four either."""
    import os
    from conftest import GOLD
    from general_fixtures import golden_signals
    from oracle import classify_ref
    from test_gpu_log_space import synthetic_windows
    if input_size == 1024:
        x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)
        x = x[:40 if inputs == 'all' else 43]
    else:
        x = classify_ref.make_windows(golden_signals(), input_size, 3 * (input_size // 2),
                                      'start').reshape(-1, input_size)
        x = x[np.abs(x).max(axis=1) > 0]           # (steps past the end of a short read)
    x = x.astype(np.float32)
    if inputs == 'all':
        x = np.concatenate([x, synthetic_windows(input_size, input_size)])
    return x


STAGE_TOL = 2e-5           # of tests/test_gpu_parity.py: test_stage_activations
STAGES = ['A', 'B', 'C', 'D', 'E', 'F', 'G', 'logits']


def stage_ratios(got, want):
    """stage -> max |got - want| / (STAGE_TOL x max(1, max |want|)); <= 1 passes."""
    out = {}
    for s in STAGES:
        g, w = np.asarray(got[s], dtype=np.float64), np.asarray(want[s], dtype=np.float64)
        assert g.shape == w.shape, (s, g.shape, w.shape)
        err = np.abs(g - w).max() if np.isfinite(g).all() else np.inf
        out[s] = float(err / (STAGE_TOL * max(1.0, np.abs(w).max())))
    return out
