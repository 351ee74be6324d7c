"""Both forward paths against the fp64 oracle in log space (tests/oracle_compare.py), through their
production entry points: the persistent kernel's predict (counter hand-out included), its fused
one-step classify and its merge, its class-count endings; the general path at input sizes that
give every stage length both parities, and its classify across chunk seams."""
import os

import numpy as np
import pytest

from conftest import GOLD, PLAN
from general_fixtures import PARITY_GEOMETRIES, STARTS, ENDS, geometry, golden_signals, \
    synthetic_reads
from oracle import classify_ref
from oracle_compare import assert_log_close, oracle_call_batch, oracle_logits
from test_gpu_general_models import compare_calls

pytestmark = pytest.mark.gpu


def ragged_reads(input_size, seed):
    rng = np.random.default_rng(seed)
    return [np.zeros(0, dtype=np.int16),
            np.array([500], dtype=np.int16),
            np.full(300, 480, dtype=np.int16),                        # std == 0
            rng.integers(300, 700, input_size // 2 - 1).astype(np.int16),
            rng.integers(300, 700, input_size + 1).astype(np.int16),
            rng.integers(0, 2047, 3 * input_size + 7).astype(np.int16),
            rng.integers(-32768, 32767, 2 * input_size).astype(np.int16)]   # full int16 range


def synthetic_windows(input_size, seed):
    """All zeros, constant, a single spike, 50x amplitude, a right-padded short read."""
    rng = np.random.default_rng(seed)
    x = np.zeros((5, input_size), dtype=np.float32)
    x[1] = 1.0
    x[2, input_size // 3] = 8.0
    x[3] = rng.standard_normal(input_size) * 50
    x[4, :37] = rng.standard_normal(37)
    return x


def golden_windows(side):
    return np.load(os.path.join(GOLD, 'windows_%s.npy' % side)).reshape(-1, 1024)


# ---- the persistent kernel -----------------------------------------------------------------
@pytest.mark.parametrize('model,side', PLAN)
def test_persistent_predict_in_log_space(hip_models, weights, model, side):
    x = golden_windows(side)
    assert len(x) == 444
    _, logits = oracle_logits(weights[model], x)
    assert hip_models[model].kind == 0
    assert_log_close(hip_models[model].predict(x), logits=logits,
                     what='persistent predict ' + model)


def test_persistent_predict_off_the_counter_in_log_space(hip_models, weights):
    """More windows than CUs x 4, not a multiple of 4: the counter hands out groups of 4, then 2,
    then single windows to the end of the launch."""
    model = 'EXP-NBD103_read_starts'
    x = golden_windows('start')
    _, logits = oracle_logits(weights[model], x)
    idx = np.random.default_rng(11).integers(0, len(x), 1539)
    assert len(idx) > 256 * 4 and len(idx) % 4
    got = hip_models[model].predict(x[idx])
    assert_log_close(got, logits=logits[idx], what='persistent predict, 1539 windows')


@pytest.mark.parametrize('model,side', PLAN)
@pytest.mark.parametrize('scan', [512, 6144])
def test_persistent_classify_in_log_space(hip_models, weights, all_signals, model, side, scan):
    """scan 512: one step, finished in the forward kernel's fused renormalise-and-call; 6144: the
    merge kernel."""
    signals = all_signals + ragged_reads(1024, 3)
    probs, calls = hip_models[model].classify_signals(signals, side, scan, 0.5)
    o_calls, o_probs, scale = oracle_call_batch(weights[model], signals, scan, 0.5, side)
    compare_calls(calls, probs, o_calls, o_probs)
    assert_log_close(probs, probs=o_probs, scale=scale,
                     what='persistent classify {} {} {}'.format(model, side, scan))


@pytest.mark.parametrize('n_classes', [2, 16, 17, 32])
def test_persistent_class_counts_in_log_space(hip, weights, n_classes):
    """The models of test_other_class_counts: classes 16..31 reach the softmax through LDS."""
    from deepbinner_amd.model_format import ModelWeights
    base = weights['EXP-NBD103_read_starts']
    rng = np.random.default_rng(n_classes)
    convs = list(base.convs[:-1]) + [
        ((rng.standard_normal((1, 48, n_classes)) * 0.2).astype(np.float32),
         (rng.standard_normal(n_classes) * 0.1).astype(np.float32))]
    w = ModelWeights(n_classes, convs, base.bns)
    model = hip.HipModel(w, device=0)
    try:
        assert model.kind == 0
        x = np.concatenate([golden_windows('start')[:148], synthetic_windows(1024, n_classes)])
        _, logits = oracle_logits(w, x)
        assert_log_close(model.predict(x), logits=logits,
                         what='persistent predict, {} classes'.format(n_classes))
    finally:
        model.close()


# ---- the general path ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def general_models(hip):
    out = {}

    def get(input_size, n_classes, name=STARTS):
        key = (input_size, n_classes, name)
        if key not in out:
            out[key] = hip.HipModel(geometry(input_size, n_classes, name=name), device=0,
                                    general=True)
        return out[key]
    yield get
    for m in out.values():
        m.close()


@pytest.mark.parametrize('input_size,n_classes', PARITY_GEOMETRIES)
def test_general_predict_in_log_space(general_models, input_size, n_classes):
    model = general_models(input_size, n_classes)
    assert model.kind == 1
    half = input_size // 2
    x = classify_ref.make_windows(golden_signals(), input_size, 3 * half, 'start')
    x = np.concatenate([x.reshape(-1, input_size).astype(np.float32),
                        synthetic_windows(input_size, input_size)])
    _, logits = oracle_logits(model.weights, x)
    assert_log_close(model.predict(x), logits=logits,
                     what='general predict L={} C={}'.format(input_size, n_classes))


def chunk_windows(model, scan_size):
    """Windows per chunk of the general path, from the public workspace size: the workspace is
    the 256-aligned per-window probabilities plus the activations of min(windows, chunk)."""
    steps = scan_size // (model.input_size // 2)

    def activations(n_reads):
        probs = n_reads * steps * model.n_classes * 4
        return model.workspace_bytes(n_reads, scan_size) - ((probs + 255) & ~255)
    per_window = activations(1) // steps
    assert activations(1) == steps * per_window and per_window > 0
    whole = activations(1 << 20)
    assert whole % per_window == 0
    chunk = whole // per_window
    assert activations(-(-chunk // steps)) == whole and chunk < (1 << 20) * steps
    assert activations(chunk // steps) == (chunk // steps) * steps * per_window
    return chunk


@pytest.mark.parametrize('input_size,scan_steps', [(16384, 3), (4096, 6)])
@pytest.mark.parametrize('side', ['start', 'end'])
def test_general_classify_across_chunk_seams(general_models, hip, all_signals, input_size,
                                             scan_steps, side):
    name = STARTS if side == 'start' else ENDS
    model = general_models(input_size, 13, name)
    scan = scan_steps * (input_size // 2)
    chunk = chunk_windows(model, scan)
    signals = (all_signals + synthetic_reads(input_size, scan, input_size)
               + ragged_reads(input_size, input_size + 1))
    n = len(signals)
    windows = n * scan_steps
    # at least two seams, and a read whose windows lie on both sides of one
    assert windows > 2 * chunk and chunk % scan_steps
    straddle = [r for r in range(n)
                if (r * scan_steps) // chunk != (r * scan_steps + scan_steps - 1) // chunk]
    assert straddle
    print('L={} steps={} chunk={} windows={} reads across a seam: {}'.format(
        input_size, scan_steps, chunk, windows, straddle))

    probs, calls = model.classify_signals(signals, side, scan, 0.5)
    o_calls, o_probs, scale = oracle_call_batch(model.weights, signals, scan, 0.5, side)
    compare_calls(calls, probs, o_calls, o_probs)
    assert_log_close(probs, probs=o_probs, scale=scale,
                     what='general classify L={} {} steps {}'.format(input_size, scan_steps, side))

    # the device entry points give the same bits
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in signals])
    samples = np.concatenate(signals + [np.zeros(1, np.int16)]).astype(np.int16)
    d_s = hip.DeviceBuffer.from_array(samples)
    d_o = hip.DeviceBuffer.from_array(offsets)
    d_p = hip.DeviceBuffer(n * 13 * 4)
    d_c = hip.DeviceBuffer(n * 4)
    d_w = hip.DeviceBuffer(model.workspace_bytes(n, scan))
    model.classify_dev(d_s.ptr, d_o.ptr, n, side, scan, 0.5, d_p.ptr, d_c.ptr, d_w.ptr)
    hip.synchronize()
    assert np.array_equal(d_p.download((n, 13), np.float32), probs)
    assert np.array_equal(d_c.download((n,), np.int32), calls)
    for batch in (1, 5):
        assert batch == 1 or n % batch
        d_p.upload(np.zeros((n, 13), np.float32))
        d_c.upload(np.full(n, -1, np.int32))
        model.classify_batched_dev(d_s.ptr, d_o.ptr, n, batch, side, scan, 0.5, d_p.ptr, d_c.ptr)
        hip.synchronize()
        assert np.array_equal(d_p.download((n, 13), np.float32), probs)
        assert np.array_equal(d_c.download((n,), np.int32), calls)

    # each read alone: the same bits as in the big call
    for r, s in enumerate(signals):
        p1, c1 = model.classify_signals([s], side, scan, 0.5)
        assert np.array_equal(p1[0], probs[r]) and c1[0] == calls[r], r
