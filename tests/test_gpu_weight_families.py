"""Both forward paths on weights unlike the three shipped models (tests/weight_families.py): BN
scales of both signs and exactly zero, freshly initialised kernel sizes, activations up to 2^54
in the persistent kernel and beyond 2^60 on the general path, dead ReLUs, and closed-form logits
with exact ties.  Against the fp64 oracle per stage and in log space, and - for ``flipped``, which
is the same function exactly - against the unflipped model on the device, bit for bit.

Every check prints its worst error / bound; tests/test_weight_families.py holds plain fp32
arithmetic to a quarter of each bound on every model used here."""
import numpy as np
import pytest

import weight_families as wf
from conftest import PLAN
from general_fixtures import geometry, golden_signals
from oracle import classify_ref, network_ref
from oracle_compare import assert_log_close, oracle_call_batch
from test_gpu_general_models import compare_calls
from test_gpu_log_space import golden_windows, ragged_reads

pytestmark = pytest.mark.gpu

PERSISTENT = wf.persistent_models()
GENERAL = wf.general_models()
CLASSIFIED = [n for n in PERSISTENT if PERSISTENT[n][3]]


class Case:
    def __init__(self, hip, weights, inputs, general):
        self.weights = weights
        self.model = hip.HipModel(weights, device=0, general=general)
        assert self.model.kind == (1 if general else 0)
        self.x = wf.family_windows(weights.input_size, inputs)
        _, self.stages = network_ref.forward(weights, self.x, dtype=np.float64, return_stages=True)


@pytest.fixture(scope='module')
def cases(hip):
    out = {}

    def get(name, general=False):
        key = (name, general)
        if key not in out:
            entry = GENERAL[name] if general else PERSISTENT[name]
            out[key] = Case(hip, entry[0](), entry[1], general)
        return out[key]
    yield get
    for case in out.values():
        case.model.close()


def largest_conv_output(weights, windows, monkeypatch):
    """The largest output of any convolution on these windows, from the fp64 oracle."""
    seen = []
    conv1d = network_ref.conv1d

    def spy(*args):
        y = conv1d(*args)
        seen.append(float(np.abs(y).max()))
        return y
    with monkeypatch.context() as mp:
        mp.setattr(network_ref, 'conv1d', spy)
        network_ref.forward(weights, windows, dtype=np.float64)
    return max(seen)


def assert_inside_the_persistent_range(name, weights, windows, monkeypatch):
    """``ranged`` on the persistent kernel: large, and inside its 2^60 (dbh_layout.h)."""
    if name.startswith('ranged'):
        top = largest_conv_output(weights, windows, monkeypatch)
        print('{}: largest convolution output 2^{:.1f}'.format(name, np.log2(top)))
        assert 2.0 ** 48 < top < 2.0 ** 56


# ---- the persistent kernel -----------------------------------------------------------------
@pytest.mark.parametrize('name', list(PERSISTENT))
def test_persistent_stages(cases, monkeypatch, name):
    """debug_stage at A .. G and the logits against the fp64 oracle, bound 2e-5 x max(1, max|want|)
    (the bound of test_stage_activations)."""
    case = cases(name)
    assert len(case.x) % 4
    assert_inside_the_persistent_range(name, case.weights, case.x, monkeypatch)
    got = {s: case.model.debug_stage(case.x, s) for s in wf.STAGES}
    got['logits'] = got['logits'][:, :case.weights.n_classes]
    ratios = wf.stage_ratios(got, case.stages)
    print('stages {}: error / bound {}'.format(
        name, ', '.join('{} {:.3f}'.format(s, ratios[s]) for s in wf.STAGES)))
    bad = [s for s in wf.STAGES if not ratios[s] <= 1.0]
    if bad:
        s = bad[0]
        err = np.abs(got[s].astype(np.float64) - case.stages[s])
        at = np.unravel_index(np.argmax(err), err.shape)
        over = err > wf.STAGE_TOL * max(1.0, np.abs(case.stages[s]).max())
        raise AssertionError('{}: first failing stage {} at {:.3g} x bound; worst at (window, '
                             'position, channel) {}; {} of {} values over the bound, in {} '
                             'windows'.format(name, s, ratios[s], at, int(over.sum()), over.size,
                                              int(over.reshape(len(over), -1).any(axis=1).sum())))


@pytest.mark.parametrize('name', list(PERSISTENT))
def test_persistent_predict(cases, name):
    case = cases(name)
    assert_log_close(case.model.predict(case.x), logits=case.stages['logits'],
                     what='persistent predict ' + name)


@pytest.mark.parametrize('side', ['start', 'end'])
@pytest.mark.parametrize('scan', [512, 6144])
@pytest.mark.parametrize('name', CLASSIFIED)
def test_persistent_classify(cases, all_signals, monkeypatch, name, scan, side):
    """scan 512: the forward kernel's fused renormalise-and-call; 6144: the merge kernel."""
    case = cases(name)
    signals = all_signals + ragged_reads(1024, 3)
    windows = classify_ref.make_windows(signals, 1024, scan, side).reshape(-1, 1024)
    assert_inside_the_persistent_range(name, case.weights, windows, monkeypatch)
    probs, calls = case.model.classify_signals(signals, side, scan, 0.5)
    o_calls, o_probs, scale = oracle_call_batch(case.weights, signals, scan, 0.5, side)
    assert np.isfinite(o_probs).all()
    compare_calls(calls, probs, o_calls, o_probs)
    assert_log_close(probs, probs=o_probs, scale=scale,
                     what='persistent classify {} {} {}'.format(name, side, scan))


@pytest.mark.parametrize('k', range(len(PLAN)))
def test_flipped_equals_shipped_on_the_persistent_kernel(cases, hip_models, all_signals, k):
    """Metamorphic: negating a BN output channel and the kernel rows that read it changes the sign
    of exact intermediate values only - scale and shift are negated exactly on the host (fp64
    division, then rounding, both odd-symmetric), and so are fma(x, scale, shift), the Winograd
    transforms of data and kernels, and every product of the consumer; the sums are the same sums.
    So the probabilities are the same bits."""
    model, side = PLAN[k]
    case = cases('flipped-' + model)
    x = np.concatenate([golden_windows(side), case.x])
    want = hip_models[model].predict(x)
    got = case.model.predict(x)
    diff = int((got != want).sum())
    print('flipped against shipped, {}: {} windows, {} of {} values differ'.format(
        model, len(x), diff, got.size))
    assert np.array_equal(got, want)
    signals = all_signals + ragged_reads(1024, 3)
    for scan in (512, 6144):
        p0, c0 = hip_models[model].classify_signals(signals, side, scan, 0.5)
        p1, c1 = case.model.classify_signals(signals, side, scan, 0.5)
        assert np.array_equal(p0, p1) and np.array_equal(c0, c1)


def test_persistent_predict_off_the_counter(cases, hip_models):
    """More windows than workgroups x 4, not a multiple of 4 (the counter hands out groups of 4,
    then 2, then single windows): a random model of 17 classes against the oracle, and flipped
    against shipped bit for bit."""
    rng = np.random.default_rng(23)
    x = golden_windows('start')
    x = x[rng.integers(0, len(x), 1539)] * rng.uniform(0.5, 1.5, (1539, 1)).astype(np.float32)
    assert len(x) > 256 * 4 and len(x) % 4
    case = cases('random-C17-s0')
    _, stages = network_ref.forward(case.weights, x, dtype=np.float64, return_stages=True)
    assert_log_close(case.model.predict(x), logits=stages['logits'],
                     what='persistent predict random-C17-s0, 1539 windows')
    model, _ = PLAN[0]
    assert np.array_equal(cases('flipped-' + model).model.predict(x), hip_models[model].predict(x))


def constant_case(hip, n_classes, which, kind):
    bias = wf.constant_biases(n_classes)[which]
    model = hip.HipModel(wf.constant(wf.random_model(1, n_classes), bias), device=0)
    assert model.kind == kind
    return bias, model


def check_constant(model, bias, all_signals, what):
    """Per window and per read against the closed form: logits = relu(bias) for every window."""
    x = wf.family_windows()
    logits = wf.constant_logits(bias, len(x))
    got = model.predict(x)
    assert_log_close(got, logits=logits, what=what + ' predict')
    z = logits[0]
    top = np.flatnonzero(z == z.max())
    if len(top) > 1:
        # tied logits are the same number through the same arithmetic: equal probabilities
        assert (got[:, top] == got[:, top[:1]]).all()
    assert (got == got[:1]).all()                       # every window the same
    signals = all_signals + ragged_reads(1024, 3)
    closed = network_ref.softmax(logits[:1])

    def predict(w):
        return np.repeat(closed, len(w), axis=0)
    for scan, side in ((512, 'start'), (6144, 'start'), (6144, 'end')):
        probs, calls = model.classify_signals(signals, side, scan, 0.5)
        o_calls, o_probs = classify_ref.call_batch(predict, signals, 1024, scan, 0.5, side)
        assert np.isfinite(o_probs).all()
        scale = np.full(len(signals), max(1.0, z.max()))
        assert_log_close(probs, probs=o_probs, scale=scale,
                         what='{} classify {} {}'.format(what, side, scan))
        compare_calls(calls, probs, o_calls, o_probs)
        if len(top) > 1:
            assert (calls == 0).all()                  # a tie for the top place: no call


@pytest.mark.parametrize('which', ['ties', 'spread', 'equal'])
@pytest.mark.parametrize('n_classes', [2, 17, 32])
def test_persistent_constant_logits(hip, all_signals, n_classes, which):
    bias, model = constant_case(hip, n_classes, which, kind=0)
    try:
        check_constant(model, bias, all_signals,
                       'persistent constant {} C={}'.format(which, n_classes))
    finally:
        model.close()


# ---- the general path ----------------------------------------------------------------------
@pytest.mark.parametrize('name', list(GENERAL))
def test_general_predict(cases, name):
    case = cases(name, general=True)
    assert_log_close(case.model.predict(case.x), logits=case.stages['logits'],
                     what='general predict ' + name)


@pytest.mark.parametrize('name', list(GENERAL))
def test_general_classify(cases, name):
    """Three scan steps, so the merge kernel runs."""
    case = cases(name, general=True)
    size = case.weights.input_size
    signals = golden_signals() + ragged_reads(size, size + 1)
    scan = 3 * (size // 2)
    probs, calls = case.model.classify_signals(signals, 'start', scan, 0.5)
    o_calls, o_probs, scale = oracle_call_batch(case.weights, signals, scan, 0.5, 'start')
    assert np.isfinite(o_probs).all()
    compare_calls(calls, probs, o_calls, o_probs)
    assert_log_close(probs, probs=o_probs, scale=scale, what='general classify ' + name)


@pytest.mark.parametrize('input_size,n_classes', wf.GENERAL_GEOMETRIES)
def test_flipped_equals_unflipped_on_the_general_path(cases, hip, input_size, n_classes):
    """As on the persistent kernel: the same bits."""
    case = cases('flipped-L{}-C{}'.format(input_size, n_classes), general=True)
    base = hip.HipModel(geometry(input_size, n_classes), device=0, general=True)
    try:
        want = base.predict(case.x)
        got = case.model.predict(case.x)
        print('flipped against unflipped, general L={}: {} of {} values differ'.format(
            input_size, int((got != want).sum()), got.size))
        assert np.array_equal(got, want)
        signals = golden_signals() + ragged_reads(input_size, input_size + 1)
        scan = 3 * (input_size // 2)
        p0, c0 = base.classify_signals(signals, 'start', scan, 0.5)
        p1, c1 = case.model.classify_signals(signals, 'start', scan, 0.5)
        assert np.array_equal(p0, p1) and np.array_equal(c0, c1)
    finally:
        base.close()


@pytest.mark.parametrize('which', ['ties', 'spread', 'equal'])
@pytest.mark.parametrize('n_classes', [33, 256])
def test_general_constant_logits(hip, all_signals, n_classes, which):
    """The general path's merge kernel has no entry point of its own: this hands it exact ties."""
    bias, model = constant_case(hip, n_classes, which, kind=1)
    try:
        check_constant(model, bias, all_signals,
                       'general constant {} C={}'.format(which, n_classes))
    finally:
        model.close()
