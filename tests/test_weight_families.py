"""The weight families of tests/weight_families.py without a device: they are what they claim to
be, the fp32 oracle stays well inside every bound the device tests use on them, and three faults
that are invisible (two of them bit-exactly) on the shipped weights fail the comparator there."""
import numpy as np
import pytest

import weight_families as wf
from conftest import MODELS
from general_fixtures import STARTS, shipped
from oracle import network_ref
from oracle_compare import log_space_ratio

PERSISTENT = wf.persistent_models()
GENERAL = wf.general_models()


def oracle(weights, x, dtype=np.float64):
    return network_ref.forward(weights, x, dtype=dtype, return_stages=True)


# ---- the families are what they claim --------------------------------------------------------
@pytest.mark.parametrize('model', MODELS)
def test_flipped_is_the_same_function_bit_for_bit(weights, model):
    x = wf.family_windows()
    w, f = weights[model], wf.flipped(weights[model], 7)
    for bn_w, bn_f in zip(w.bns, f.bns):
        assert (np.sign(bn_w[0]) != np.sign(bn_f[0])).sum() == len(bn_w[0]) // 2
    p64, s64 = oracle(w, x)
    q64, t64 = oracle(f, x)
    assert np.array_equal(s64['logits'], t64['logits']) and np.array_equal(p64, q64)
    assert np.array_equal(network_ref.forward(w, x, dtype=np.float32),
                          network_ref.forward(f, x, dtype=np.float32))
    # and it is not the same model: half the channels of every BN output changed sign
    assert not np.array_equal(s64['C'], t64['C'])
    assert np.array_equal(np.abs(s64['C']), np.abs(t64['C']))


def test_the_shipped_models_have_no_gamma_at_or_below_zero(weights):
    """The gap: why the device tests need ``flipped`` and ``random_model``."""
    for w in weights.values():
        assert all((bn[0] > 0).all() for bn in w.bns)


@pytest.mark.parametrize('a', [24, 28, 40])
def test_ranged_is_the_same_function_with_larger_activations(weights, a):
    x = wf.family_windows(inputs='normalised')
    w = weights[STARTS]
    _, s64 = oracle(w, x)
    p, t64 = oracle(wf.ranged(w, a), x)
    ratio = log_space_ratio(p, logits=s64['logits'])
    print('ranged({}) against the shipped model: error / bound {:.2e}'.format(a, ratio))
    assert ratio <= 1e-3
    assert max(wf.stage_ratios(t64, s64).values()) <= 1e-3


def largest_conv_output(weights, x, monkeypatch):
    """The largest output of any convolution (before its ReLU), from the fp64 oracle."""
    seen = []
    conv1d = network_ref.conv1d

    def spy(*args):
        y = conv1d(*args)
        seen.append(float(np.abs(y).max()))
        return y
    with monkeypatch.context() as mp:
        mp.setattr(network_ref, 'conv1d', spy)
        network_ref.forward(weights, x, dtype=np.float64)
    assert len(seen) == 20
    return max(seen)


def test_ranged_activations_lie_where_the_device_tests_need_them(weights, monkeypatch):
    """The persistent kernel holds activations times 2^-60: 24 and 28 stay inside 2^48 .. 2^56
    on the windows the device tests use, 40 goes beyond 2^60 (general path only)."""
    x = wf.family_windows(inputs='normalised')
    base = largest_conv_output(weights[STARTS], x, monkeypatch)
    assert 2.0 ** 25 < base < 2.0 ** 26
    for a in (24, 28):
        top = largest_conv_output(wf.ranged(weights[STARTS], a), x, monkeypatch)
        assert top == base * 2.0 ** a and 2.0 ** 48 < top < 2.0 ** 56
    assert largest_conv_output(wf.ranged(weights[STARTS], 40), x, monkeypatch) > 2.0 ** 60


def test_dead_stages_are_the_bn_shifts(monkeypatch):
    x = wf.family_windows()
    live = wf.random_model(0, 13)
    assert largest_conv_output(live, x, monkeypatch) < 1e-2 * -wf.DEAD_BIAS
    w = wf.dead(live)
    for dtype in (np.float64, np.float32):
        _, stages = oracle(w, x, dtype)
        for i, s in enumerate('BCDEFG', start=2):
            shift = wf.bn_shift(w.bns[i - 1], dtype)
            assert np.array_equal(stages[s], np.broadcast_to(shift, stages[s].shape)), s
        assert np.abs(stages['A']).max() > 10          # stage A is alive


@pytest.mark.parametrize('n_classes', [2, 17, 32, 33, 256])
def test_constant_logits_are_the_closed_form(n_classes):
    x = wf.family_windows()
    for name, bias in wf.constant_biases(n_classes).items():
        w = wf.constant(wf.random_model(1, n_classes), bias)
        _, stages = oracle(w, x[:6])
        assert np.array_equal(stages['logits'], wf.constant_logits(bias, 6)), name
        z = np.maximum(bias, 0)
        top = np.flatnonzero(z == z.max())
        if name == 'ties':
            assert len(top) >= 2 and (n_classes == 2 or 0 not in top) and n_classes - 1 in top
        elif name == 'spread':
            assert z.max() - z.min() > 200 and len(top) == 1 and top[0] != 0
        else:
            assert len(top) == n_classes


def test_random_models_are_not_degenerate():
    x = wf.family_windows()
    for c in wf.RANDOM_CLASSES:
        for seed in wf.RANDOM_SEEDS:
            w = wf.random_model(seed, c)
            for gamma, _, _, var in w.bns:
                assert (gamma == 0).sum() == 2 and (gamma < 0).sum() >= 0.1 * len(gamma)
                assert (var > 0).all()
            probs, stages = oracle(w, x)
            assert np.isfinite(probs).all()
            for s in 'ABCDEFG':            # alive, and different from window to window
                assert (stages[s].std(axis=0) > 0).mean() > 0.5, (c, seed, s)
            assert np.abs(stages['logits']).max() > 88       # beyond exp's fp32 range
            # (an untrained model may favour one class everywhere, a ReLU may hold a logit at 0)
            assert (stages['logits'].std(axis=0) > 0).sum() >= min(2, c - 1)


# ---- the conditioning cap --------------------------------------------------------------------
def conditioning(weights, x):
    """fp32 oracle against fp64 oracle: the worst stage ratio and the log-space ratio."""
    _, s64 = oracle(weights, x)
    p32, s32 = oracle(weights, x, np.float32)
    return max(wf.stage_ratios(s32, s64).values()), log_space_ratio(p32, logits=s64['logits'])


@pytest.mark.parametrize('name', list(PERSISTENT))
def test_persistent_models_are_well_conditioned(name):
    """A condition, not a measurement: on every model the device tests use, plain fp32 arithmetic
    stays within 1/4 of each bound.  A seed that breaks the cap is replaced, not excused."""
    build, inputs = PERSISTENT[name][:2]
    stage, log = conditioning(build(), wf.family_windows(inputs=inputs))
    print('{}: fp32 oracle / bound: stages {:.3f}, log space {:.3f}'.format(name, stage, log))
    assert stage <= 0.25 and log <= 0.25


@pytest.mark.parametrize('name', list(GENERAL))
def test_general_models_are_well_conditioned(name):
    build, inputs = GENERAL[name]
    w = build()
    stage, log = conditioning(w, wf.family_windows(w.input_size, inputs))
    print('{}: fp32 oracle / bound: stages {:.3f}, log space {:.3f}'.format(name, stage, log))
    assert stage <= 0.25 and log <= 0.25


def test_general_geometries_come_from_the_parity_list():
    from general_fixtures import PARITY_GEOMETRIES
    sizes = [s for s, _ in PARITY_GEOMETRIES]
    assert all(s in sizes or s == 1024 for s, _ in wf.GENERAL_GEOMETRIES)
    assert all(g in PARITY_GEOMETRIES for g in wf.RANDOM_ONLY_GEOMETRIES)


# ---- planted faults --------------------------------------------------------------------------
def planted_forward(weights, x, fault=None):
    """oracle/network_ref.py: forward in fp64 with one fault at every site where it applies:

    'bn_before_pool'   BN applied before the max-pool instead of after it (the same for a
                       positive scale: an increasing map commutes with max);
    'shift_padding'    the zero padding of a k = 3 convolution behind a BN (conv1d_2, 8, 17, 18)
                       filled with the BN shift - what padding before the BN would give;
    'abs_scale'        |scale| for scale, the shift as it should be.
    """
    from deepbinner_amd.model_format import BN_EPSILON, conv_shapes
    r = network_ref
    x = np.asarray(x, dtype=np.float64)[:, :, None]
    shapes = conv_shapes(weights.n_classes)

    def bn_terms(i):
        gamma, beta, mean, var = (a.astype(np.float64) for a in weights.bns[i - 1])
        scale = gamma / np.sqrt(var + BN_EPSILON)
        return (np.abs(scale) if fault == 'abs_scale' else scale), beta - mean * scale

    def bn(i, t):
        scale, shift = bn_terms(i)
        return t * scale + shift

    def pool_bn(i, t):
        return r.max_pool2(bn(i, t)) if fault == 'bn_before_pool' else bn(i, r.max_pool2(t))

    def conv(i, t, behind_bn=None):
        kernel, bias = (a.astype(np.float64) for a in weights.convs[i - 1])
        _, k, _, _, stride, padding = shapes[i - 1]
        if fault == 'shift_padding' and behind_bn and k == 3:
            length = t.shape[1]
            total = max((-(-length // stride) - 1) * stride + k - length, 0)
            left = total // 2
            pad = np.broadcast_to(bn_terms(behind_bn)[1], (t.shape[0], 1, t.shape[2]))
            t = np.concatenate([pad] * left + [t] + [pad] * (total - left), axis=1)
            padding = 'valid'
        return r.relu(r.conv1d(t, kernel, bias, stride, padding))

    stages = {}
    x = stages['A'] = bn(1, conv(1, x))
    x = stages['B'] = pool_bn(2, conv(4, conv(3, conv(2, x, behind_bn=1))))
    x = stages['C'] = pool_bn(3, conv(7, conv(6, conv(5, x))))
    x = stages['D'] = pool_bn(4, conv(9, conv(8, x, behind_bn=3)))
    branches = [conv(10, r.avg_pool3_same(x)), conv(11, x), conv(13, conv(12, x)),
                conv(16, conv(15, conv(14, x)))]
    x = stages['E'] = pool_bn(5, np.concatenate(branches, axis=2))
    x = stages['F'] = bn(6, conv(17, x, behind_bn=5))
    x = stages['G'] = pool_bn(7, conv(19, conv(18, x, behind_bn=6)))
    stages['logits'] = conv(20, x).mean(axis=1)
    return r.softmax(stages['logits']), stages


def verdict(weights, x, fault):
    """(worst stage ratio, log-space ratio, bit-equal?) of the faulty forward pass against the
    right one, under the two rules of the device tests."""
    p64, s64 = oracle(weights, x)
    p, s = planted_forward(weights, x, fault)
    return (max(wf.stage_ratios(s, s64).values()), log_space_ratio(p, logits=s64['logits']),
            np.array_equal(p, p64) and all(np.array_equal(s[k], s64[k]) for k in s))


NEW_MODELS = {'flipped-' + STARTS: lambda: wf.flipped(shipped(STARTS), 100),
              'random-C13-s0': lambda: wf.random_model(0, 13),
              'random-C2-s1': lambda: wf.random_model(1, 2),
              'random-C32-s2': lambda: wf.random_model(2, 32)}


@pytest.mark.parametrize('model', MODELS)
def test_planted_forward_without_a_fault_is_the_oracle(weights, model):
    for w in (weights[model], wf.random_model(0, 13)):
        stage, log, same = verdict(w, wf.family_windows(), None)
        assert same and stage == 0.0 and log < 1e-5      # (log p of the same bits, rounded twice)


@pytest.mark.parametrize('fault', ['bn_before_pool', 'abs_scale'])
@pytest.mark.parametrize('model', MODELS)
def test_sign_faults_are_invisible_on_the_shipped_weights(weights, model, fault):
    """Bit-exact there (every scale is positive): the gap the families close."""
    stage, log, same = verdict(weights[model], wf.family_windows(), fault)
    assert same and stage == 0.0 and log < 1e-5


@pytest.mark.parametrize('fault', ['bn_before_pool', 'abs_scale', 'shift_padding'])
@pytest.mark.parametrize('name', list(NEW_MODELS))
def test_planted_faults_fail_on_the_new_families(name, fault):
    stage, log, same = verdict(NEW_MODELS[name](), wf.family_windows(), fault)
    print('{} {}: stages {:.3g} x bound, log space {:.3g} x bound'.format(name, fault, stage, log))
    assert not same and stage > 10 and log > 10


@pytest.mark.parametrize('model', MODELS)
def test_shift_padding_still_fails_on_the_shipped_weights(weights, model):
    """The control: a fault the old tests see is seen with the families' comparator too."""
    stage, log, same = verdict(weights[model], wf.family_windows(), 'shift_padding')
    assert not same and stage > 10 and log > 10
