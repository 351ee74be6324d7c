"""A helper, not a test: the training step's first half restated in NumPy - the Deepbinner graph
(reference ``network_architecture.py:18-95``) in Keras's training phase, the categorical
cross-entropy of ``train_network.py:53-55`` and the analytic gradient of the mean loss with respect
to every trainable parameter.  It is the contract of ``include/deepbinner_hip.h``, "training"
(DESIGN.md section 17), and what ``dbh_gradients`` is held to; ``tests/test_train_reference.py``
pins it against ``oracle/network_ref.forward`` and against central differences.

Everything runs in ``dtype`` (float64 for the reference proper, float32 to measure what plain fp32
arithmetic loses on a case).  ``model=True`` keeps fp64 arithmetic and rounds to fp32 where DESIGN.md
section 17 says the device does - every tensor it stores, and the matrix pipe's short sums - so its
distance from the fp64 run is what the device's arithmetic may lose on a case, without sharing a
line with the kernels.  The layer primitives are ``oracle.network_ref``'s, so the edge rules
(SAME padding, the average pool's valid-tap count, the 'valid' max-pool) are the inference
oracle's.  Not restated here: GaussianNoise (the caller's to add) and Keras's clipping of the
probability to [1e-7, 1 - 1e-7].
"""
import os

import numpy as np

import weight_families as wf
from deepbinner_amd.model_format import (BN_CHANNELS, BN_EPSILON, ModelWeights, conv_shapes,
                                         param_count)
from oracle import network_ref

M32 = 0xFFFFFFFF
SEED = 20181018                              # the dropout seed of the device cases
HIGH_SEED = SEED + (0x9e3779b9 << 32)        # ... and one whose high half matters


def _mix(h):
    """32-bit integer hash step on uint64 arrays holding 32-bit values."""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7feb352d)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846ca68b)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(16))
    return h


def dropout_keep(seed, layer, n_windows, length, channels, rate):
    """Boolean [n_windows, length, channels]: which elements dropout layer ``layer`` (1..7) keeps.
    The function written out in include/deepbinner_hip.h."""
    seed = int(seed) & (2 ** 64 - 1)
    lo, hi = seed & M32, seed >> 32
    h = _mix(np.uint64((lo + layer * 0x9e3779b9) & M32))
    h = _mix(h ^ np.uint64(hi))
    window = np.arange(n_windows, dtype=np.uint64)[:, None, None]
    h = _mix((h + window) & np.uint64(M32))
    counter = (np.arange(length, dtype=np.uint64)[None, :, None] * np.uint64(256)
               + np.arange(channels, dtype=np.uint64)[None, None, :])
    h = _mix(h ^ counter)
    threshold = int(float(np.float32(rate)) * 16777216.0)
    return (h >> np.uint64(8)) >= np.uint64(threshold)


def dropout_scale(rate):
    """(float)(1 / (1 - rate)) as the device forms it; exactly 1 at rate 0."""
    return float(np.float32(1.0 / (1.0 - float(np.float32(rate)))))


def _pads(length, k, stride, padding):
    if padding == 'same':
        out = -(-length // stride)
        total = max((out - 1) * stride + k - length, 0)
        return out, total // 2, total - total // 2
    return (length - k) // stride + 1, 0, 0


def conv1d_backward(x, kernel, stride, padding, dz):
    """Gradients of ``network_ref.conv1d`` given dz at its output: (dx, dkernel, dbias)."""
    n, length, cin = x.shape
    k = kernel.shape[0]
    out, left, right = _pads(length, k, stride, padding)
    assert dz.shape[1] == out
    xp = np.pad(x, ((0, 0), (left, right), (0, 0)))
    dxp = np.zeros_like(xp)
    dkernel = np.empty_like(kernel)
    span = (out - 1) * stride + 1
    flat = dz.reshape(-1, dz.shape[2])
    for j in range(k):
        dkernel[j] = xp[:, j:j + span:stride, :].reshape(-1, cin).T @ flat
        dxp[:, j:j + span:stride, :] += dz @ kernel[j].T
    return dxp[:, left:left + length, :], dkernel, flat.sum(axis=0)


def _pairs(x):
    n, length, c = x.shape
    half = length // 2
    return x[:, :2 * half, :].reshape(n, half, 2, c)


def max_pool2_first(x, tie_first=True):
    """Which of each pair the 'valid' pool takes: True = the first (it wins exact ties; with
    ``tie_first`` off the second does, which is not the contract - the tie tests show that they
    would notice)."""
    pairs = _pairs(x)
    if tie_first:
        return pairs[:, :, 0, :] >= pairs[:, :, 1, :]
    return pairs[:, :, 0, :] > pairs[:, :, 1, :]


def max_pool2_backward(x, g, tie_first=True):
    first = max_pool2_first(x, tie_first)
    half = first.shape[1]
    dx = np.zeros_like(x)                   # a dropped last position keeps 0
    dx[:, 0:2 * half:2, :] = g * first
    dx[:, 1:2 * half:2, :] = g * ~first
    return dx


def avg_pool3_backward(g):
    n, length, c = g.shape
    count = np.full((length, 1), 3.0, dtype=g.dtype)
    count[0] = 2.0
    count[-1] = 2.0
    if length == 1:
        count[0] = 1.0
    gp = np.pad(g / count, ((0, 0), (1, 1), (0, 0)))
    return gp[:, 0:length] + gp[:, 1:length + 1] + gp[:, 2:length + 2]


# ---- the device's arithmetic, restated from DESIGN.md section 17 (model=True) -------------------
def _r32(a):
    """Rounded to fp32 and back: a tensor as the device stores it."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _short(a, b):
    """a @ b summed in fp32, as the matrix pipe forms a short sum; the result in fp64."""
    return np.matmul(np.ascontiguousarray(a, dtype=np.float32),
                     np.ascontiguousarray(b, dtype=np.float32)).astype(np.float64)


def _short_rows(a, b):
    """[n, l, 16] x [16, c] summed in fp32 like _short, by a loop that treats every row alike: equal
    rows give equal sums whatever their position, as they do on the device (a BLAS blocks the rows,
    and would break the exact ties behind a constant layer)."""
    return np.einsum('nlc,co->nlo', np.ascontiguousarray(a, dtype=np.float32),
                     np.ascontiguousarray(b, dtype=np.float32)).astype(np.float64)


def _orders(order):
    """The order in which a short sum takes its 16 channels, and its 64 rows: as they lie for
    ``order`` 0, else a permutation drawn from it - another draw of the same roundings."""
    if order == 0:
        return np.arange(16), np.arange(64)
    rng = np.random.default_rng(order)
    return rng.permutation(16), rng.permutation(64)


def model_conv1d(x, kernel, bias, stride, padding, order=0):
    """The pre-activation as stored: one tap's 16 channels summed in fp32, those sums and the bias
    added in fp64, one rounding to fp32.  conv1d_1 (one input channel): fp32 fused multiply-adds
    over the taps, then the bias."""
    n, length, cin = x.shape
    k, _, cout = kernel.shape
    out, left, right = _pads(length, k, stride, padding)
    xp = np.pad(x, ((0, 0), (left, right), (0, 0)))
    span = (out - 1) * stride + 1
    y = np.zeros((n, out, cout))
    if cin == 1:
        for j in range(k):
            y = _r32(xp[:, j:j + span:stride, :] * kernel[j] + y)     # the product is exact in fp64
        return _r32(y + bias)
    p16, _ = _orders(order)
    for j in range(k):
        for c0 in range(0, cin, 16):
            y += _short_rows(xp[:, j:j + span:stride, c0 + p16], kernel[j, c0 + p16, :])
    return _r32(y + bias)


def model_conv1d_backward(x, kernel, stride, padding, dz, order=0):
    """(dx, dkernel, dbias) as the device forms them from the fp32 tensors x and dz: the data
    gradient like the convolution (16 output channels of a tap in fp32, then fp64, one rounding);
    the kernel's from fp32 sums over 64 consecutive rows added in fp64; the bias's in fp64."""
    n, length, cin = x.shape
    k, _, cout = kernel.shape
    out, left, right = _pads(length, k, stride, padding)
    xp = np.pad(x, ((0, 0), (left, right), (0, 0)))
    dxp = np.zeros_like(xp)
    dkernel = np.empty_like(kernel)
    span = (out - 1) * stride + 1
    flat = dz.reshape(-1, cout)
    fill = -flat.shape[0] % 64
    p16, p64 = _orders(order)
    z64 = np.pad(flat, ((0, fill), (0, 0))).reshape(-1, 64, cout)[:, p64, :]
    for j in range(k):
        rows = np.pad(xp[:, j:j + span:stride, :].reshape(-1, cin), ((0, fill), (0, 0)))
        dkernel[j] = _short(rows.reshape(-1, 64, cin)[:, p64, :].transpose(0, 2, 1), z64).sum(axis=0)
        for c0 in range(0, cout, 16):
            dxp[:, j:j + span:stride, :] += _short_rows(dz[:, :, c0 + p16], kernel[j][:, c0 + p16].T)
    return _r32(dxp[:, left:left + length, :]), dkernel, flat.sum(axis=0)


def model_avg_pool3_same(x):
    """The valid taps added left to right in fp32, then the division in fp32."""
    length = x.shape[1]
    xp = np.pad(x, ((0, 0), (1, 1), (0, 0))).astype(np.float32)
    count = np.full((length, 1), 3.0, dtype=np.float32)
    count[0] = count[-1] = 2.0 if length > 1 else 1.0
    return (((xp[:, 0:length] + xp[:, 1:length + 1]) + xp[:, 2:length + 2]) / count).astype(np.float64)


def model_avg_pool3_backward(g):
    """Each output's share g / count in fp32, the up to three of them added left to right in fp32."""
    length = g.shape[1]
    count = np.full((length, 1), 3.0, dtype=np.float32)
    count[0] = count[-1] = 2.0 if length > 1 else 1.0
    gp = np.pad(g.astype(np.float32) / count, ((0, 0), (1, 1), (0, 0)))
    return ((gp[:, 0:length] + gp[:, 1:length + 1]) + gp[:, 2:length + 2]).astype(np.float64)


def close_decisions(exact, model):
    """How many ReLU and pool decisions of the fp64 run ``exact`` the device's rounding could turn:
    with d = |model - fp64| of a pre-activation or a pool pair's difference, floored at 1/16 of
    its layer's largest, those with |value| < 8 d.  Pool pairs count where their maximum is
    positive (behind a ReLU the others are 0 and 0).  A value that is exactly 0 in both runs is a
    tie by construction (equal inputs, or the tie cases' constant layers), not one that rounding
    made or could break, and does not count."""
    count = 0
    for (value, counts), (other, _) in zip(exact.decisions, model.decisions):
        d = np.abs(other - value)
        d = np.maximum(d, d.max() / 16)
        near = (np.abs(value) < 8 * d) & ~((value == 0) & (other == 0))
        if counts is not None:
            near &= counts
        count += int(near.sum())
    return count


def same_patterns(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a.patterns, b.patterns))


class Result:
    """loss, n_correct, grads (flat, the blob's layout, dtype), stats (960: mean then variance per
    BN layer), probs, logits, patterns (every ReLU mask and pool choice, for flip detection),
    decisions (per pattern the values decided on: a ReLU's pre-activations with None, or a pool's
    pair differences with the mask of pairs whose maximum is positive)."""


def loss_and_gradients(weights, x, labels, rate=0.15, seed=0, dtype=np.float64, backward=True,
                       model=False, order=0, tie_first=True):
    dtype = np.dtype(dtype).type
    assert not model or dtype is np.float64
    stored = _r32 if model else (lambda a: a)    # a tensor written to memory between two kernels
    x = np.asarray(x, dtype=dtype)
    if x.ndim == 2:
        x = x[:, :, None]
    n = x.shape[0]
    labels = np.asarray(labels).astype(np.int64)
    shapes = conv_shapes(weights.n_classes)
    scale = dtype(dropout_scale(rate))
    eps = dtype(BN_EPSILON)
    patterns = []
    decisions = []
    tape = []                                # the backward pass, last step first when reversed
    grads_conv = [None] * 20
    grads_bn = [None] * 7
    stats = []

    def conv(i, t):
        kernel, bias = (a.astype(dtype) for a in weights.convs[i - 1])
        _, _, _, _, stride, padding = shapes[i - 1]
        # the head (conv1d_20 on) is fp64 on the device, and so are conv1d_1's gradients
        piped = model and 1 < i < 20
        if model and i < 20:
            pre = model_conv1d(t, kernel, bias, stride, padding, order)
        else:
            pre = network_ref.conv1d(t, kernel, bias, stride, padding)
        y = network_ref.relu(pre)
        live = y > 0                         # ReLU'(0) = 0
        patterns.append(live)
        decisions.append((pre, None))

        def back(g):
            if piped:
                dx, dk, db = model_conv1d_backward(t, kernel, stride, padding, g * live, order)
            else:
                dx, dk, db = conv1d_backward(t, kernel, stride, padding, g * live)
            grads_conv[i - 1] = (dk, db)
            return stored(dx)
        tape.append(back)
        return y

    def pool(t):
        patterns.append(max_pool2_first(t, tie_first))
        pairs = _pairs(t)
        decisions.append((pairs[:, :, 0, :] - pairs[:, :, 1, :], pairs.max(axis=2) > 0))
        tape.append(lambda g: max_pool2_backward(t, g, tie_first))
        return network_ref.max_pool2(t)

    def bn(i, t):
        gamma, beta = (a.astype(dtype) for a in weights.bns[i - 1][:2])
        rows = dtype(t.shape[0] * t.shape[1])
        mean = t.mean(axis=(0, 1))
        var = ((t - mean) ** 2).mean(axis=(0, 1))            # biased, two passes
        stats.extend([mean, var])
        istd = dtype(1) / np.sqrt(var + eps)
        xhat = (t - mean) * istd
        keep = dropout_keep(seed, i, t.shape[0], t.shape[1], t.shape[2], rate) * scale

        def back(g):
            g = stored(g * keep)
            dbeta = g.sum(axis=(0, 1))
            dgamma = (g * xhat).sum(axis=(0, 1))
            grads_bn[i - 1] = (dgamma, dbeta)
            return stored((gamma * istd) * (g - dbeta / rows - xhat * (dgamma / rows)))
        tape.append(back)
        # (the device rounds xhat, the scaling, the shift and the dropout factor, one at a time;
        # its backward pass forms xhat again in fp64)
        return stored(stored(stored(stored(xhat) * gamma) + beta) * keep)

    def run_back(g, upto):
        while len(tape) > upto:
            g = tape.pop()(g)
        return g

    t = bn(1, conv(1, x))
    t = bn(2, pool(conv(4, conv(3, conv(2, t)))))
    t = bn(3, pool(conv(7, conv(6, conv(5, t)))))
    t = bn(4, pool(conv(9, conv(8, t))))
    trunk = len(tape)
    d = t
    marks = [len(tape)]
    x1 = conv(10, model_avg_pool3_same(d) if model else network_ref.avg_pool3_same(d))
    marks.append(len(tape))
    x2 = conv(11, d)
    marks.append(len(tape))
    x3 = conv(13, conv(12, d))
    marks.append(len(tape))
    x4 = conv(16, conv(15, conv(14, d)))
    marks.append(len(tape))
    branch_tapes = [tape[marks[k]:marks[k + 1]] for k in range(4)]
    del tape[trunk:]
    cat = np.concatenate([x1, x2, x3, x4], axis=2)

    def inception_back(g):
        total = None
        # (the device adds the branches' data gradients from conv1d_14's to conv1d_10's, in fp32)
        for k in ((3, 2, 1, 0) if model else (0, 1, 2, 3)):
            gb = g[:, :, 48 * k:48 * (k + 1)]
            for step in reversed(branch_tapes[k]):
                gb = step(gb)
            if k == 0:
                gb = model_avg_pool3_backward(gb) if model else avg_pool3_backward(gb)
            total = gb if total is None else stored(total + gb)
        return total
    tape.append(inception_back)
    t = bn(5, pool(cat))
    t = bn(6, conv(17, t))
    t = bn(7, pool(conv(19, conv(18, t))))
    z = conv(20, t)
    l7 = z.shape[1]
    logits = z.mean(axis=1)
    mx = logits.max(axis=1, keepdims=True)
    e = np.exp(logits - mx)
    se = e.sum(axis=1, keepdims=True)
    probs = e / se
    losses = (mx[:, 0] + np.log(se[:, 0])) - logits[np.arange(n), labels]

    out = Result()
    out.loss = float(losses.astype(np.float64).sum() / n) if dtype is np.float64 else float(losses.mean())
    out.n_correct = int((np.argmax(logits, axis=1) == labels).sum())   # lowest index on ties
    out.probs, out.logits, out.patterns, out.decisions = probs, logits, patterns, decisions
    out.stats = stored(np.concatenate(stats))
    out.grads = None
    if backward:
        dlogits = probs.copy()
        dlogits[np.arange(n), labels] -= 1
        dlogits /= dtype(n)
        g = np.repeat(stored(dlogits / dtype(l7))[:, None, :], l7, axis=1)
        run_back(g, 0)
        parts = []
        for dk, db in grads_conv:
            parts += [dk.ravel(), db.ravel()]
        for (dgamma, dbeta), c in zip(grads_bn, BN_CHANNELS):
            parts += [dgamma, dbeta, np.zeros(2 * c, dtype=dtype)]
        out.grads = stored(np.concatenate(parts))
        assert out.grads.size == param_count(weights.n_classes)
    return out


def tensor_slices(n_classes):
    """name -> slice of the flat blob, the 54 trainable tensors in blob order."""
    out = {}
    pos = 0
    for name, k, cin, cout, _, _ in conv_shapes(n_classes):
        out[name + '/kernel'] = slice(pos, pos + k * cin * cout)
        pos += k * cin * cout
        out[name + '/bias'] = slice(pos, pos + cout)
        pos += cout
    moving = []
    for i, c in enumerate(BN_CHANNELS, start=1):
        out['bn_%d/gamma' % i] = slice(pos, pos + c)
        out['bn_%d/beta' % i] = slice(pos + c, pos + 2 * c)
        moving.append(slice(pos + 2 * c, pos + 4 * c))
        pos += 4 * c
    assert pos == param_count(n_classes) and len(out) == 54
    return out, moving


# ---- the cases of tests/test_gpu_gradients.py, with their references ----------------------------
def case_inputs(size, n, classes, draw=None):
    """(weights, windows, labels) of a case.  ``draw`` None: the case as first written - the
    shipped starts model on golden windows at (1024, 20, 13), a random model on normal windows
    elsewhere.  A number: a random model on the ``draw``-th set of normal windows, the one that
    GUARDED names because no decision on it is close (tests/test_train_reference.py)."""
    if draw is None and (size, n, classes) == (1024, 20, 13):
        from conftest import GOLD
        from general_fixtures import shipped
        weights = shipped()
        x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)[:n]
        x = np.ascontiguousarray(x, dtype=np.float32)
    else:
        weights = wf.random_model(size + n, classes, input_size=size)
        key = [size, n, classes] if draw is None else [size, n, classes, draw]
        x = np.random.default_rng(key).standard_normal((n, size)).astype(np.float32)
    if classes == 256:
        labels = np.full(n, 77, dtype=np.int32)            # every window the same label
    else:
        labels = np.random.default_rng(size).integers(classes, size=n).astype(np.int32)
        labels[0], labels[-1] = 0, classes - 1
    return weights, x, labels


# (input size, windows, classes, dropout rate, dropout seed, draw): the direct cases held to the
# model's bound.  A turned ReLU or pool choice moves a tensor by 1e-3 .. 1e-1 of its size, which
# no tolerance covers, so each case runs on a draw of its windows (the lowest found) on which no
# decision is close (close_decisions() == 0) and the model's loss is within 1e-6 of the fp64 one;
# tests/test_train_reference.py asserts both for every entry.  The choice looks at the reference
# alone, never at the device.  (1024, 20, 13) - 3.7 M decisions - is not here: of 16 draws at each
# rate every one had close decisions (2 .. 14 of them), so that shape stays with the fp32
# reference's rule alone and (1024, 4, 13) stands in for it; at 3.0 M decisions, (16384, 1, 3)
# needs some hundred draws.
GUARDED = [
    (96, 3, 2, 0.0, SEED, 2), (96, 3, 2, 0.15, SEED, 3),
    (130, 5, 13, 0.0, SEED, 0), (130, 5, 13, 0.15, SEED, 0),
    (200, 2, 33, 0.0, SEED, 0), (200, 2, 33, 0.15, SEED, 0),
    (1024, 3, 256, 0.0, SEED, 5), (1024, 3, 256, 0.15, SEED, 0),
    (1024, 4, 13, 0.0, SEED, 1),
    # one window: at 96, BN7 sees one element - variance 0, xhat 0, 51 of the 54 gradients exactly 0
    (96, 1, 2, 0.0, SEED, 0), (96, 1, 2, 0.15, SEED, 0),
    (1024, 1, 13, 0.0, SEED, 0), (1024, 1, 13, 0.15, SEED, 2),
    # lengths 1025, 512 .. 16: an odd length at the first pool, 16 positions into the head
    (2050, 3, 13, 0.0, SEED, 0), (2050, 3, 13, 0.15, SEED, 51),
    # the largest input: 128 positions into the head
    (16384, 1, 3, 0.0, SEED, 116), (16384, 1, 3, 0.15, SEED, 178),
    # 64 window numbers through the dropout hash
    (96, 64, 5, 0.0, SEED, 0), (96, 64, 5, 0.15, SEED, 5),
    # threshold 2^23 and scale 2; a seed whose high half takes part
    (130, 5, 13, 0.5, SEED, 1), (130, 5, 13, 0.5, HIGH_SEED, 0),
]


def case_id(case):
    return 'L{}-N{}-C{}-rate{}-{}-draw{}'.format(*case[:4], 'high' if case[4] >> 32 else 'low', case[5])


# conv1d_i (pooled) with a zero kernel and bias 0.5: every pool pair behind it is an exact positive
# tie, the data gradient through it is 0 (so everything upstream has gradient exactly 0), and its
# own kernel's gradient depends on which of a pair took the gradient.  Windows must not be
# constant: both positions of a tie would then see the same inputs.
TIE_LAYERS = [(4,), (7,), (9,), (19,), (10, 11, 13, 16)]
TIE_SHAPE = (130, 5, 13)
# what lies upstream of each (convolutions, batch normalisations), all 1-based
TIE_UPSTREAM = {4: (range(1, 4), [1]), 7: (range(1, 7), [1, 2]), 9: (range(1, 9), [1, 2, 3]),
                19: (range(1, 19), range(1, 7)), 10: ([*range(1, 10), 12, 14, 15], [1, 2, 3, 4])}


def tie_inputs(layers):
    size, n, classes = TIE_SHAPE
    weights, x, labels = case_inputs(size, n, classes, draw=0)
    convs = [(k.copy(), b.copy()) for k, b in weights.convs]
    for i in layers:
        convs[i - 1] = (np.zeros_like(convs[i - 1][0]), np.full_like(convs[i - 1][1], 0.5))
    bns = list(weights.bns)
    if 9 in layers:
        # BN4 then puts out its beta at every position, and the average pool's (c + c + c) / 3 is
        # c in fp32 only where 3 c needs no rounding; else conv1d_10's pool pairs at the window's
        # ends, ties in exact arithmetic, would go by an fp32 rounding.  Multiples of 1 / 256 do.
        gamma, beta, mean, var = bns[3]
        bns[3] = (gamma, (np.round(beta * 256) / 256).astype(np.float32), mean, var)
    return ModelWeights(classes, convs, bns, input_size=size), x, labels


ORDERS = 8
_references = {}


def references(key, make_inputs, rate, seed):
    """(fp64, fp32, model) results of a case: computed once, shared among the tests of a session,
    never changed.  The model's result is that of order 0 and carries ``close`` (close_decisions
    against the fp64 run), ``same`` (no pattern of any order differs from the fp64 run's),
    ``n_decisions``, and ``draws``: (loss, grads, stats) of each of ORDERS orders of the short
    sums.  The patterns and decisions themselves are dropped to keep a session's references small.

    Why several orders: on a small case a handful of roundings (those in front of a batch
    normalisation over two to five elements) carry most of every tensor's error, so one order's
    error is one draw of a quantity that varies several-fold, and 4 x one draw is below another
    draw - the device's - about one time in six.  e_model is therefore the largest error among
    ORDERS draws: the size of the error, not one sample of it."""
    if key not in _references:
        weights, x, labels = make_inputs()
        exact = loss_and_gradients(weights, x, labels, rate=rate, seed=seed)
        plain = loss_and_gradients(weights, x, labels, rate=rate, seed=seed, dtype=np.float32)
        model = loss_and_gradients(weights, x, labels, rate=rate, seed=seed, model=True)
        model.close = close_decisions(exact, model)
        model.same = same_patterns(exact, model)
        model.n_decisions = sum(value.size for value, _ in exact.decisions)
        model.draws = [(model.loss, model.grads, model.stats)]
        for order in range(1, ORDERS):
            other = loss_and_gradients(weights, x, labels, rate=rate, seed=seed, model=True,
                                       order=order)
            model.same = model.same and same_patterns(exact, other)
            model.draws.append((other.loss, other.grads, other.stats))
        for r in (exact, plain, model):
            r.patterns = r.decisions = None
        _references[key] = (exact, plain, model)
    return _references[key]


def model_error(exact, model, sl=None):
    """e_model of a tensor (``sl`` a slice of the gradient blob) or, without one, of the loss: the
    largest error among the model's draws, relative to max |fp64 tensor|; 0 for a zero tensor."""
    if sl is None:
        return max(abs(loss - exact.loss) for loss, _, _ in model.draws) / abs(exact.loss)
    scale = np.abs(exact.grads[sl]).max()
    if scale == 0:
        return 0.0
    return max(np.abs(grads[sl] - exact.grads[sl]).max() for _, grads, _ in model.draws) / scale


def guarded_references(case):
    size, n, classes, rate, seed, draw = case
    return references(case, lambda: case_inputs(size, n, classes, draw), rate, seed)


def tie_references(layers):
    return references(('tie',) + tuple(layers), lambda: tie_inputs(layers), 0.0, SEED)
