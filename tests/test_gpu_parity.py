"""
Parity of the HIP path with the oracle — the tests proper (need an MI355X; `-m gpu`).
Everything goes through the C ABI (deepbinner_amd.hip_backend -> libdeepbinner_hip.so).

Tolerances: softmax probabilities within 1e-4 absolute of the fp64 oracle (BASELINE.json
north_star); the fp32-vs-fp64 spread of the oracle itself is < 2e-6, so the checks below use
tighter bounds where the arithmetic allows.  Integer work (calls) must be identical.
"""
import argparse
import io
import os
import tempfile

import numpy as np
import pytest

from conftest import GOLD, PLAN, MODEL_DIR
from oracle import classify_ref, network_ref

pytestmark = pytest.mark.gpu
PROB_TOL = 1e-4


def pack(signals):
    offsets = np.zeros(len(signals) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in signals])
    samples = (np.concatenate(signals) if len(signals) and offsets[-1] else
               np.zeros(0)).astype(np.int16)
    return samples, offsets


def call_names(calls):
    return ['none' if c == 0 else str(int(c)) for c in calls]


def test_native_library_is_loaded(hip):
    maps = open('/proc/self/maps').read()
    assert 'libdeepbinner_hip.so' in maps
    info = hip.forward_kernel_info()
    assert info['threads_per_block'] == 512 and info['lds_bytes'] > 100000


# ---- per-stage activations -----------------------------------------------------------------
@pytest.mark.parametrize('stage', ['A', 'B', 'C', 'D', 'E', 'F', 'G', 'logits'])
def test_stage_activations(hip_models, stage):
    g = np.load(os.path.join(GOLD, 'stages_EXP-NBD103_read_starts.npz'))
    got = hip_models['EXP-NBD103_read_starts'].debug_stage(g['x'], stage)
    want = g[stage]
    if stage == 'logits':
        got = got[:, :want.shape[1]]
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err < 2e-5 * scale, 'stage %s: max err %.3e (scale %.2f)' % (stage, err, scale)


# ---- seam b1: predict ------------------------------------------------------------------------
@pytest.mark.parametrize('model_name,side', PLAN)
def test_predict_matches_oracle(hip_models, model_name, side):
    x = np.load(os.path.join(GOLD, 'windows_%s.npy' % side)).reshape(-1, 1024)
    want = np.load(os.path.join(GOLD, 'window_probs_%s_%s.npy' % (model_name, side)))
    got = hip_models[model_name].predict(x[:, :, None], batch_size=256)
    assert got.dtype == np.float32 and got.shape == want.shape and got.flags.writeable
    assert np.abs(got - want).max() < PROB_TOL
    assert np.array_equal(got.argmax(axis=1), want.argmax(axis=1))
    assert np.abs(got.sum(axis=1) - 1).max() < 1e-5


def test_predict_more_windows_than_workgroups(hip_models):
    """Seam b1 through the persistent loop: 1,500 windows on 256 workgroups (every workgroup walks
    several, each on the cold path of stage A - the fp32 windows bring no prefetch - and the
    batched tail runs with full and partial batches): row for row what the same windows give 50 at
    a time (one workgroup per window)."""
    x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)
    rng = np.random.default_rng(5)
    big = x[rng.integers(0, len(x), 1500)] * rng.uniform(0.5, 1.5, (1500, 1)).astype(np.float32)
    model = hip_models['EXP-NBD103_read_starts']
    got = model.predict(big[:, :, None])
    want = np.concatenate([model.predict(big[a:a + 50, :, None]) for a in range(0, 1500, 50)])
    assert np.array_equal(got, want)


def test_timeline_kernel_stamps_every_window(hip_models):
    """The cycle-stamp build of the forward kernel (dbh_timeline::dbh_forward_kernel, launched from
    dbh_kernels.hip), on fp32 windows and on int16 reads: 5 windows are one group of four and one of
    one, two workgroups.  Every wave takes stamp 0 (shader clock) and stamp 62 (100 MHz clock) at the
    top of every window."""
    model = hip_models['EXP-NBD103_read_starts']
    x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)[:5]
    reads = (np.random.default_rng(11).standard_normal((5, 1024)) * 80 + 500).astype(np.int16)
    for stamps in (model.timeline(x), model.timeline_i16(reads)):
        assert stamps.shape == (5, 8, 64) and stamps.dtype == np.int64
        assert (stamps[:, :, 0] != 0).all() and (stamps[:, :, 62] != 0).all()


def test_predict_edge_inputs(hip_models, weights):
    model = hip_models['EXP-NBD103_read_starts']
    assert model.predict(np.zeros((0, 1024, 1))).shape == (0, 13)
    rng = np.random.default_rng(1)
    x = np.zeros((5, 1024), dtype=np.float32)
    x[1] = 1.0
    x[2] = rng.standard_normal(1024) * 50          # large amplitude
    x[3, :7] = rng.standard_normal(7)              # nearly empty (short read, right padded)
    x[4, -300:] = rng.standard_normal(300)         # left padded (end side)
    got = model.predict(x)
    want = network_ref.forward(weights['EXP-NBD103_read_starts'], x, dtype=np.float64)
    assert np.abs(got - want).max() < PROB_TOL
    with pytest.raises(ValueError):
        model.predict(np.zeros((3, 1000, 1)))


def test_predict_is_order_and_batch_independent(hip_models):
    """Size-independent properties at BASELINE config-2 size (10k windows)."""
    model = hip_models['EXP-NBD103_read_starts']
    base = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)
    rng = np.random.default_rng(20260927)
    idx = rng.integers(0, len(base), size=10000)
    x = base[idx] + (rng.standard_normal((10000, 1024)) * 0.01).astype(np.float32)
    full = model.predict(x)
    assert np.abs(full.sum(axis=1) - 1).max() < 1e-5 and np.isfinite(full).all()
    perm = rng.permutation(10000)
    assert np.array_equal(model.predict(x[perm]), full[perm])          # bit-exact
    parts = np.concatenate([model.predict(x[i:i + 256]) for i in range(0, 10000, 256)])
    assert np.array_equal(parts, full)
    dup = model.predict(np.repeat(x[:3], 4, axis=0))
    assert np.array_equal(dup[0], dup[3]) and np.array_equal(dup[4], dup[7])
    # spot check against the oracle
    from deepbinner_amd.model_format import ModelWeights
    w, _ = ModelWeights.load(os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'))
    want = network_ref.forward(w, x[:64], dtype=np.float64)
    assert np.abs(full[:64] - want).max() < PROB_TOL


def test_read_length_hint_never_changes_results(hip, weights):
    """dbh_model_set_read_length_hint: right, wrong, too-small-capacity and ragged cases all give
    bit-identical probabilities and calls (the device re-fetches wherever the offsets disagree)."""
    model = hip.HipModel(weights['EXP-NBD103_read_starts'], device=0)
    rng = np.random.default_rng(5)
    uniform = rng.integers(200, 900, size=(300, 1024)).astype(np.int16)
    ragged = [rng.integers(200, 900, size=int(n)).astype(np.int16)
              for n in rng.integers(0, 3000, size=200)]

    def run(reads, scan, side):
        samples = np.concatenate([np.asarray(r).reshape(-1) for r in reads]) if len(reads) else \
            np.empty(0, np.int16)
        lengths = np.array([len(r) for r in reads], dtype=np.int64)
        offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
        d_s = hip.DeviceBuffer.from_array(samples if samples.size else np.zeros(1, np.int16))
        d_o = hip.DeviceBuffer.from_array(offsets)
        n = len(reads)
        d_p = hip.DeviceBuffer(n * model.n_classes * 4)
        d_c = hip.DeviceBuffer(n * 4)
        model.classify_batched_dev(d_s.ptr, d_o.ptr, n, 64, side, scan, 0.5, d_p.ptr, d_c.ptr,
                                   None)
        hip.synchronize()
        return d_p.download((n, model.n_classes), np.float32), d_c.download((n,), np.int32)

    for reads, scan, side in ((uniform, 512, 'start'), (uniform, 1024, 'end'),
                              (ragged, 512, 'start'), (ragged, 1024, 'end')):
        model.set_read_length_hint(0)
        want = run(reads, scan, side)
        total = sum(len(r) for r in reads)
        for hint, cap in ((1024, total), (1024, total // 2), (1000, total), (1024, 10 * total),
                          (4096, total)):
            model.set_read_length_hint(hint, min(cap, total))      # never beyond the buffer
            got = run(reads, scan, side)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), \
                (hint, cap, scan, side)
    model.set_read_length_hint(0)


@pytest.mark.parametrize('model_name,side,batch,scan,length', [
    ('EXP-NBD103_read_starts', 'start', 512, 512, 1024),      # BASELINE configs[2], start model
    ('EXP-NBD103_read_ends', 'end', 512, 512, 1024),          # BASELINE configs[2], end model
    ('SQK-RBK004_read_starts', 'start', 256, 512, 1024),      # BASELINE configs[3]
    ('EXP-NBD103_read_starts', 'start', 256, 6144, 6656),     # the CLI's default geometry
])
def test_baseline_configurations_match_oracle(hip, hip_models, weights, model_name, side, batch,
                                              scan, length):
    """The device-resident batched entry point on the other BASELINE.json configurations
    (tools/config_rates.py times them at full size): calls identical to the oracle's C port and
    probabilities within tolerance on 768 synthetic reads, with and without the length hint."""
    from bench import synthetic_reads
    from oracle import dbref
    n = 768
    reads = np.ascontiguousarray(
        np.tile(synthetic_reads(n, 20260927), (1, -(-length // 1024)))[:, :length])
    assert reads.shape == (n, length)
    offsets = np.arange(n + 1, dtype=np.int64) * length
    want_probs, want_calls = dbref.CModel(weights[model_name]).classify(
        reads.reshape(-1), offsets, side, scan, 0.5)
    model = hip_models[model_name]
    d_s, d_o = hip.DeviceBuffer.from_array(reads), hip.DeviceBuffer.from_array(offsets)
    d_p, d_c = hip.DeviceBuffer(n * model.n_classes * 4), hip.DeviceBuffer(n * 4)
    for hint in (0, length):
        model.set_read_length_hint(hint, reads.size)
        model.classify_batched_dev(d_s.ptr, d_o.ptr, n, batch, side, scan, 0.5, d_p.ptr, d_c.ptr,
                                   None)
        hip.synchronize()
        assert np.array_equal(d_c.download((n,), np.int32), want_calls)
        assert np.abs(d_p.download((n, model.n_classes), np.float32) - want_probs).max() < PROB_TOL
    model.set_read_length_hint(0)


def _classify_resident(hip, model, d_samples, d_offsets, n, batch, side, stream=None):
    d_p, d_c = hip.DeviceBuffer(n * model.n_classes * 4), hip.DeviceBuffer(n * 4)
    model.classify_batched_dev(d_samples.ptr, d_offsets.ptr, n, batch, side, 512, 0.5, d_p.ptr,
                               d_c.ptr, stream)
    hip.synchronize()
    return d_p.download((n, model.n_classes), np.float32), d_c.download((n,), np.int32)


def test_config2_at_full_size(hip, hip_models, weights):
    """BASELINE.json configs[2] as stated: 100,000 signals (bench.py's, with real-read windows in
    them) through the EXP-NBD103 start AND end models, batch 512, combine_calls (require_either)
    on the device.  Parity with the oracle's C port + combine_calls on every read that gets a
    barcode from either model plus 2,000 random ones; on all of it: the combined calls follow the oracle's table, a
    different batch size and the reversed read order give the same bits."""
    from bench import config_reads
    from oracle import dbref
    n = 100000
    reads = config_reads(n, 20260927)
    offsets = np.arange(n + 1, dtype=np.int64) * 1024
    d_s, d_o = hip.DeviceBuffer.from_array(reads), hip.DeviceBuffer.from_array(offsets)
    start, end = hip_models['EXP-NBD103_read_starts'], hip_models['EXP-NBD103_read_ends']
    p_s, c_s = _classify_resident(hip, start, d_s, d_o, n, 512, 'start')
    p_e, c_e = _classify_resident(hip, end, d_s, d_o, n, 512, 'end')
    d_cs, d_ce = hip.DeviceBuffer.from_array(c_s), hip.DeviceBuffer.from_array(c_e)
    d_f = hip.DeviceBuffer(n * 4)
    hip.combine_calls_dev(d_cs.ptr, d_ce.ptr, n, 'require_either', d_f.ptr)
    hip.synchronize()
    final = d_f.download((n,), np.int32)
    name = lambda c: 'none' if c == 0 else str(int(c))                # noqa: E731
    table = np.array([[0 if classify_ref.combine_calls(name(a), name(b), 'require_either') == 'none'
                       else int(classify_ref.combine_calls(name(a), name(b), 'require_either'))
                       for b in range(13)] for a in range(13)], dtype=np.int32)
    assert np.array_equal(final, table[c_s, c_e])
    assert (c_s != 0).sum() > 100 and (final != 0).sum() > 100       # the real windows do classify
    # the oracle on EVERY read either model gives a barcode (the ones that matter: the rest of the
    # set is synthetic and calls none) and on 2,000 more spread over the whole set: probabilities
    # within tolerance and every call identical - no read of these sets sits in the 1e-5 band
    # around score_diff where fp32 and the port may fall on different sides
    rng = np.random.default_rng(20260929)
    pick = np.unique(np.concatenate([np.flatnonzero((c_s != 0) | (c_e != 0)),
                                     rng.choice(n, 2000, replace=False)]))
    sub = np.ascontiguousarray(reads[pick])
    sub_off = np.arange(len(pick) + 1, dtype=np.int64) * 1024
    for model_name, side, probs, calls in (('EXP-NBD103_read_starts', 'start', p_s, c_s),
                                           ('EXP-NBD103_read_ends', 'end', p_e, c_e)):
        want_probs, want_calls = dbref.CModel(weights[model_name]).classify(
            sub.reshape(-1), sub_off, side, 512, 0.5)
        assert np.abs(probs[pick] - want_probs).max() < PROB_TOL
        assert np.array_equal(calls[pick], want_calls), \
            '%d calls differ from the oracle' % (calls[pick] != want_calls).sum()
        assert (want_calls != 0).sum() > (100 if side == 'start' else 10)
    # invariants on all of it: batch size, read order
    p2, c2 = _classify_resident(hip, start, d_s, d_o, n, 4096, 'start')
    assert np.array_equal(p2, p_s) and np.array_equal(c2, c_s)
    d_r = hip.DeviceBuffer.from_array(np.ascontiguousarray(reads[::-1]))
    p3, c3 = _classify_resident(hip, end, d_r, d_o, n, 512, 'end')
    assert np.array_equal(p3[::-1], p_e) and np.array_equal(c3[::-1], c_e)


def test_config3_at_full_size(hip, hip_models, weights):
    """BASELINE.json configs[3]: SQK-RBK004_read_starts, batch 256.  One GPU's 125,000-read shard
    of the 1,000,000 against the oracle's C port (every read that gets a barcode + 2,000 random
    ones: calls identical, none in the threshold band); then all 1,000,000 reads
    on this GPU (what `bench.py --config 3` times at N = 1): probabilities are distributions, the
    first shard's results are unchanged inside the whole, and reversing the order of the reads
    reverses the results bit for bit."""
    from bench import config_reads
    from oracle import dbref
    model = hip_models['SQK-RBK004_read_starts']
    n = 1000000
    reads = config_reads(n, 20260927)
    shard = 125000
    offsets = np.arange(n + 1, dtype=np.int64) * 1024
    d_o = hip.DeviceBuffer.from_array(offsets)
    d_s = hip.DeviceBuffer.from_array(reads[:shard])
    p_shard, c_shard = _classify_resident(hip, model, d_s, d_o, shard, 256, 'start')
    cmodel = dbref.CModel(weights['SQK-RBK004_read_starts'])

    def against_the_oracle(probs, calls, upto, seed):
        """every read with a barcode + 2,000 random ones of reads[:upto]: same call, |dp| < 1e-4"""
        rng = np.random.default_rng(seed)
        pick = np.unique(np.concatenate([np.flatnonzero(calls[:upto] != 0),
                                         rng.choice(upto, 2000, replace=False)]))
        sub = np.ascontiguousarray(reads[pick])
        want_probs, want_calls = cmodel.classify(
            sub.reshape(-1), np.arange(len(pick) + 1, dtype=np.int64) * 1024, 'start', 512, 0.5)
        assert np.abs(probs[pick] - want_probs).max() < PROB_TOL
        assert np.array_equal(calls[pick], want_calls), \
            '%d calls differ from the oracle' % (calls[pick] != want_calls).sum()
        return int((want_calls != 0).sum())

    assert against_the_oracle(p_shard, c_shard, shard, 1) > 100
    del d_s
    d_all = hip.DeviceBuffer.from_array(reads)
    p_all, c_all = _classify_resident(hip, model, d_all, d_o, n, 256, 'start')
    assert np.array_equal(p_all[:shard], p_shard) and np.array_equal(c_all[:shard], c_shard)
    assert np.abs(p_all.sum(axis=1) - 1).max() < 1e-5 and p_all.min() >= 0
    assert ((c_all >= 0) & (c_all < 13)).all() and (c_all != 0).sum() > 100
    against_the_oracle(p_all, c_all, n, 2)      # ... and over the whole million
    del d_all
    d_rev = hip.DeviceBuffer.from_array(np.ascontiguousarray(reads[::-1]))
    p_rev, c_rev = _classify_resident(hip, model, d_rev, d_o, n, 1024, 'start')
    assert np.array_equal(p_rev[::-1], p_all) and np.array_equal(c_rev[::-1], c_all)


@pytest.mark.parametrize('n_classes', [2, 13, 16, 17, 25, 32])
def test_other_class_counts(hip, weights, all_signals, n_classes):
    """Both endings of the kernel - every class in one N tile (<= 16, no LDS round) and two N
    tiles (17..32) - on models whose last convolution is redrawn for n_classes outputs."""
    from deepbinner_amd.model_format import ModelWeights
    from oracle import dbref
    base = weights['EXP-NBD103_read_starts']
    rng = np.random.default_rng(n_classes)
    convs = list(base.convs[:-1]) + [
        ((rng.standard_normal((1, 48, n_classes)) * 0.2).astype(np.float32),
         (rng.standard_normal(n_classes) * 0.1).astype(np.float32))]
    w = ModelWeights(n_classes, convs, base.bns)
    model = hip.HipModel(w, device=0)
    x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)[:40]
    got = model.predict(x)
    want = network_ref.forward(w, x, dtype=np.float64)
    assert got.shape == (40, n_classes) and np.abs(got - want).max() < PROB_TOL
    # seam b2 with one and with several scan steps against the C port
    samples = np.concatenate(all_signals)
    offsets = np.concatenate(([0], np.cumsum([len(s) for s in all_signals]))).astype(np.int64)
    cm = dbref.CModel(w)
    for side, scan in (('start', 512), ('end', 512), ('start', 6144)):
        probs, calls = model.classify_signals(all_signals, side, scan, 0.05)
        want_probs, want_calls = cm.classify(samples, offsets, side, scan, 0.05)
        assert np.abs(probs - want_probs).max() < PROB_TOL
        # a call may legitimately differ only where best - second sits on the threshold
        for i in np.flatnonzero(calls != want_calls):
            top = np.sort(want_probs[i])[::-1]
            assert abs((top[0] - top[1]) - 0.05) < 1e-5, (side, scan, i)


def test_live_kernel_timing_brackets(hip_models):
    """dbh_forward_timing_*: one event pair per run of `span` launches at every n-th launch; only
    closed brackets are reported, and timing does not change results."""
    model = hip_models['EXP-NBD103_read_starts']
    base = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)[:32]
    want = model.predict(base)
    model.timing_enable(4, 2)
    for _ in range(10):                      # launches 0..9: brackets {0,1}, {4,5}, {8,9}
        assert np.array_equal(model.predict(base), want)
    ms, launches, windows = model.timing_read()
    assert launches == 6 and windows == 6 * 32 and ms > 0
    # tens of microseconds per launch, plus whatever the host did between the two blocking
    # predict() calls of a bracket (seen: 9 ms once, in the middle of the full suite)
    assert 0.005 < ms / launches < 100.0
    model.timing_enable(3, 3)
    for _ in range(5):                       # bracket {0,1,2} closed, {3,4,..} still open
        model.predict(base)
    ms, launches, windows = model.timing_read()
    assert launches == 3 and windows == 3 * 32
    model.timing_enable(False)
    model.predict(base)
    assert model.timing_read()[1] == 0


# ---- seam b2: classify_i16 -------------------------------------------------------------------
@pytest.mark.parametrize('model_name,side', PLAN)
def test_classify_matches_reference_call_batch(hip_models, gold, all_signals, model_name, side):
    probs, calls = hip_models[model_name].classify_signals(all_signals, side, 6144, 0.5)
    assert call_names(calls) == gold['calls']['%s/%s' % (model_name, side)]
    ref = np.load(os.path.join(GOLD, 'merged_%s_%s.npy' % (model_name, side)))
    assert np.abs(probs - ref).max() < PROB_TOL


@pytest.mark.parametrize('side', ['start', 'end'])
def test_normalise_kernel(hip, gold, all_signals, side):
    """int16 -> windows on the device == the reference's normalise + padding (float32 of fp64)."""
    lib = hip.load_library()
    samples, offsets = pack(all_signals)
    d_s = hip.DeviceBuffer.from_array(samples)
    d_o = hip.DeviceBuffer.from_array(offsets)
    n = len(all_signals)
    d_w = hip.DeviceBuffer(n * 12 * 1024 * 4)
    hip.check(lib.dbh_normalise_windows_dev(d_s.ptr, d_o.ptr, n, 0 if side == 'start' else 1,
                                            6144, d_w.ptr, None))
    got = d_w.download((n, 12, 1024), np.float32)
    ref = np.load(os.path.join(GOLD, 'windows_%s.npy' % side)).transpose(1, 0, 2)
    # exact integer sums on the device vs NumPy's float64 reductions: <= 1 ulp of float32
    assert np.abs(got - ref).max() <= 2.4e-7 * max(1.0, float(np.abs(ref).max()))
    assert np.array_equal(got == 0, ref == 0)      # padding lands in exactly the same places


def test_classify_ragged_and_degenerate_reads(hip_models, weights):
    """Empty, tiny, flat, exactly-window-sized and long reads (classify.py:337-358 edge cases)."""
    rng = np.random.default_rng(7)
    signals = [np.zeros(0, dtype=np.int16),
               np.array([500], dtype=np.int16),
               np.full(300, 480, dtype=np.int16),                       # std == 0
               rng.integers(300, 700, 511).astype(np.int16),
               rng.integers(300, 700, 1024).astype(np.int16),
               rng.integers(300, 700, 1025).astype(np.int16),
               rng.integers(300, 700, 6144).astype(np.int16),
               rng.integers(0, 2047, 20000).astype(np.int16),
               rng.integers(-32768, 32767, 7000).astype(np.int16)]      # full int16 range
    w = weights['EXP-NBD103_read_starts']
    for side in ('start', 'end'):
        for scan in (6144, 512, 1024):
            probs, calls = hip_models['EXP-NBD103_read_starts'].classify_signals(
                signals, side, scan, 0.5)
            o_calls, o_probs = classify_ref.call_batch(
                lambda x: network_ref.forward(w, x.astype(np.float32), dtype=np.float64),
                signals, 1024, scan, 0.5, side)
            assert call_names(calls) == o_calls
            assert np.abs(probs - o_probs).max() < PROB_TOL
    p, c = hip_models['EXP-NBD103_read_starts'].classify_signals([], 'start', 6144, 0.5)
    assert p.shape == (0, 13) and c.shape == (0,)


def test_merge_kernel_rules(hip):
    """min for class 0 / max for barcodes / renormalise / top-2 threshold, incl. ties."""
    lib = hip.load_library()
    rng = np.random.default_rng(3)
    n, steps, C = 1000, 12, 13
    raw = rng.random((n, steps, C)).astype(np.float32) ** 4
    raw /= raw.sum(axis=2, keepdims=True)
    raw[0] = 1.0 / C                              # all-equal: best is class 0 by tie rule
    raw[1, :, :] = 0
    raw[1, :, 5] = 0.75
    raw[1, :, 0] = 0.25                           # diff exactly 0.5 -> called
    d_in = hip.DeviceBuffer.from_array(raw)
    d_p = hip.DeviceBuffer(n * C * 4)
    d_c = hip.DeviceBuffer(n * 4)
    hip.check(lib.dbh_merge_calls_dev(d_in.ptr, n, steps, C, 0.5, d_p.ptr, d_c.ptr, None))
    probs = d_p.download((n, C), np.float32)
    calls = d_c.download((n,), np.int32)
    merged = classify_ref.merge_steps(list(raw.transpose(1, 0, 2)))
    want = np.stack([classify_ref.make_sum_to_one(r) for r in merged])
    assert np.abs(probs - want).max() < 1e-6
    assert call_names(calls) == [classify_ref.barcode_call(r, 0.5) for r in want]
    assert calls[0] == 0 and calls[1] == 5


def test_classify_many_reads_properties(hip_models, all_signals):
    """100k-read scale (config 3 size) via invariants: tiling the 37 real reads must reproduce
    their calls everywhere, in any order."""
    reps = 2703                                    # 37 * 2703 = 100,011 reads
    signals = [s[:7000] for s in all_signals] * reps
    model = hip_models['EXP-NBD103_read_starts']
    probs, calls = model.classify_signals(signals, 'start', 6144, 0.5)
    base_p, base_c = probs[:37], calls[:37]
    assert np.array_equal(calls.reshape(reps, 37), np.tile(base_c, (reps, 1)))
    assert np.array_equal(probs.reshape(reps, 37, 13), np.broadcast_to(base_p, (reps, 37, 13)))
    assert np.abs(probs.sum(axis=1) - 1).max() < 1e-5


# ---- the drop-in surface on the real backend ---------------------------------------------------
def test_end_to_end_fast5_classification(hip, capsys):
    """reference tests/test_classify.py:143-160 + :272-296 through the real HipModel."""
    import deepbinner_amd.classify as classify
    import deepbinner_amd.load_fast5s as load_fast5s
    from test_oracle_golden import EXPECTED_START, EXPECTED_END
    args = argparse.Namespace(verbose=True, batch_size=128, scan_size=6144, score_diff=0.5,
                              require_either=True, require_start=False, require_both=False)
    fast5s = load_fast5s.find_all_fast5s(os.path.join(GOLD, 'fast5', 'single'))
    sm, si, em, ei, osz, cnt = classify.load_and_check_models(
        os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'),
        os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw'), 6144, out_dest=io.StringIO())
    assert type(sm).__name__ == 'HipModel' and (si, ei, osz, cnt) == (1024, 1024, 13, 2)
    classifications, _ = classify.classify_fast5_files(fast5s, sm, si, em, ei, osz, args,
                                                       full_output=True, summary_table=False)
    assert classifications == EXPECTED_START
    lines = capsys.readouterr().out.splitlines()
    row = ['0.00', '0.00', '0.00', '1.00'] + ['0.00'] * 9
    assert ('177c3867-6812-4476-a6da-9e4d5c43b760\t3\t' + '\t'.join(row + ['3'] + row + ['3'])) \
        in lines
    args.require_either, args.require_both = False, True
    classifications, _ = classify.classify_fast5_files(fast5s, sm, si, em, ei, osz, args,
                                                       full_output=False)
    assert classifications == EXPECTED_END


def test_b1_and_b2_seams_agree(hip_models, gold, all_signals):
    """call_batch via model.predict (host windowing) == call_batch fully on the device."""
    import deepbinner_amd.classify as classify
    model = hip_models['EXP-NBD103_read_ends']
    args = argparse.Namespace(scan_size=6144, batch_size=256, score_diff=0.5)

    class PredictOnly:
        def predict(self, x, batch_size=None):
            return model.predict(x, batch_size)

    ids = ['r%d' % i for i in range(len(all_signals))]
    c1, p1 = classify.call_batch(1024, 13, ids, all_signals, PredictOnly(), args, 'end')
    c2, p2 = classify.call_batch(1024, 13, ids, all_signals, model, args, 'end')
    assert c1 == c2
    assert np.abs(np.array(p1) - np.array(p2)).max() < 2e-6


@pytest.mark.parametrize('side,scan,batch', [('start', 6144, 8), ('end', 6144, 5), ('start', 512, 3),
                                             ('end', 1024, 64)])
def test_batched_pipeline_matches_single_call(hip, hip_models, all_signals, side, scan, batch):
    """dbh_classify_i16_batched_dev (3-stream pipeline, slot reuse) == one big classify call."""
    model = hip_models['EXP-NBD103_read_ends']
    signals = [s[:7000] if side == 'start' else s[-7000:] for s in all_signals] * 3
    signals.insert(5, np.zeros(0, dtype=np.int16))
    signals.insert(11, np.full(100, 512, dtype=np.int16))
    want_p, want_c = model.classify_signals(signals, side, scan, 0.5)
    samples, offsets = pack(signals)
    d_s = hip.DeviceBuffer.from_array(samples)
    d_o = hip.DeviceBuffer.from_array(offsets)
    n = len(signals)
    d_p = hip.DeviceBuffer(n * 13 * 4)
    d_c = hip.DeviceBuffer(n * 4)
    for _ in range(2):      # second round re-uses the pipeline's streams, events and slots
        model.classify_batched_dev(d_s.ptr, d_o.ptr, n, batch, side, scan, 0.5, d_p.ptr, d_c.ptr)
        hip.synchronize()
        assert np.array_equal(d_c.download((n,), np.int32), want_c)
        assert np.array_equal(d_p.download((n, 13), np.float32), want_p)


@pytest.mark.parametrize('cap', [1, 3, 4])
def test_long_shares_of_windows_per_workgroup(hip, hip_models, weights, all_signals, cap,
                                              monkeypatch):
    """The production kernel is persistent: a workgroup walks many windows, prefetching the next
    one's samples and statistics under the current one's last stages and finishing them eight at
    a time (the batched tail).  DEEPBINNER_GRID_CAP makes the shares long out of few windows: the
    results must equal, bit for bit, those of one window per workgroup (what fewer windows than
    CUs get), on both seams, for full, partial and single-window tail batches."""
    wide = hip_models['EXP-NBD103_read_starts']
    monkeypatch.setenv('DEEPBINNER_GRID_CAP', str(cap))
    narrow = hip.HipModel(weights['EXP-NBD103_read_starts'], device=0)
    monkeypatch.delenv('DEEPBINNER_GRID_CAP')
    base = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)
    rng = np.random.default_rng(cap)
    for n in (1, 2, 3, 8 * cap, 8 * cap + 1, 17 * cap + 2, 37):
        x = base[rng.integers(0, len(base), size=n)] + \
            (rng.standard_normal((n, 1024)) * 0.01).astype(np.float32)
        assert np.array_equal(narrow.predict(x), wide.predict(x)), n
    signals = [all_signals[i % len(all_signals)][:int(rng.integers(0, 3000))] for i in range(45)]
    for side, scan in (('start', 512), ('end', 512), ('start', 2048)):
        want_p, want_c = wide.classify_signals(signals, side, scan, 0.5)
        got_p, got_c = narrow.classify_signals(signals, side, scan, 0.5)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_p, want_p), (side, scan)


def test_windows_off_the_counter_and_in_fixed_shares_give_the_same(hip, hip_models, weights,
                                                                   all_signals, monkeypatch):
    """The workgroups of a production launch take their windows off a counter in global memory,
    which the launch's last taker puts back to zero for the next launch on that stream;
    DEEPBINNER_STATIC_WINDOWS=1 keeps round 2's fixed shares (b, b + grid, ...).  Same results
    either way, launch after launch (a counter left dirty would skip or repeat windows), with
    more windows than workgroups and with fewer, on several streams of one model."""
    counted = hip_models['EXP-NBD103_read_starts']
    monkeypatch.setenv('DEEPBINNER_STATIC_WINDOWS', '1')
    monkeypatch.setenv('DEEPBINNER_GRID_CAP', '5')
    fixed = hip.HipModel(weights['EXP-NBD103_read_starts'], device=0)
    monkeypatch.delenv('DEEPBINNER_STATIC_WINDOWS')
    few = hip.HipModel(weights['EXP-NBD103_read_starts'], device=0)      # counter, 5 workgroups
    monkeypatch.delenv('DEEPBINNER_GRID_CAP')
    rng = np.random.default_rng(11)
    for n in (700, 3, 61, 700, 1, 257):
        signals = [all_signals[i % len(all_signals)][:int(rng.integers(0, 4000))] for i in range(n)]
        want_p, want_c = fixed.classify_signals(signals, 'start', 512, 0.5)
        for model in (counted, few, few):
            got_p, got_c = model.classify_signals(signals, 'start', 512, 0.5)
            assert np.array_equal(got_c, want_c) and np.array_equal(got_p, want_p), n
    # the host-buffer pipeline: three slots, each with its own stream and counter
    signals = [all_signals[i % len(all_signals)] for i in range(900)]
    samples, offsets = pack(signals)
    want = fixed.classify_packed(samples, offsets, 'end', 2048, 0.5)
    for model in (counted, few):
        model.set_host_group(512)
        try:
            for _ in range(2):
                got = model.classify_packed(samples, offsets, 'end', 2048, 0.5)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        finally:
            model.set_host_group(0)
    fixed.close()
    few.close()


@pytest.mark.parametrize('side,scan', [('start', 6144), ('end', 6144), ('start', 512), ('end', 512)])
def test_fused_kernel_equals_three_kernel_path(hip, hip_models, all_signals, side, scan):
    """slice+normalise (and, at one scan step, renormalise+call) fused into the CNN kernel must
    reproduce normalise kernel -> CNN kernel -> merge kernel bit for bit."""
    lib = hip.load_library()
    model = hip_models['EXP-NBD103_read_starts']
    signals = list(all_signals) + [np.zeros(0, dtype=np.int16), np.full(9, 3, dtype=np.int16)]
    n, steps = len(signals), scan // 512
    samples, offsets = pack(signals)
    d_s, d_o = hip.DeviceBuffer.from_array(samples), hip.DeviceBuffer.from_array(offsets)
    d_w = hip.DeviceBuffer(n * steps * 1024 * 4)
    d_wp = hip.DeviceBuffer(n * steps * 13 * 4)
    d_p, d_c = hip.DeviceBuffer(n * 13 * 4), hip.DeviceBuffer(n * 4)
    code = 0 if side == 'start' else 1
    hip.check(lib.dbh_normalise_windows_dev(d_s.ptr, d_o.ptr, n, code, scan, d_w.ptr, None))
    model.predict_dev(d_w.ptr, n * steps, d_wp.ptr)
    hip.check(lib.dbh_merge_calls_dev(d_wp.ptr, n, steps, 13, 0.5, d_p.ptr, d_c.ptr, None))
    hip.synchronize()
    want_p, want_c = d_p.download((n, 13), np.float32), d_c.download((n,), np.int32)
    got_p, got_c = model.classify_signals(signals, side, scan, 0.5)
    assert np.array_equal(got_c, want_c)
    assert np.array_equal(got_p, want_p)


def test_packed_batches_from_the_native_loader_go_to_the_gpu_as_they_are(hip_models):
    """classify_packed on what f5_load_batch returns (first and last scan_size + 512 samples of
    long reads, back to back) == classify_signals on the whole signals, both sides, and the same
    through classify_fast5_files with either reader."""
    import argparse
    import io
    import contextlib
    from conftest import REPO
    from deepbinner_amd import classify, fast5_native, load_fast5s
    folder = os.path.join(REPO, 'tests', 'golden', 'fast5', 'single')
    files = sorted(os.path.join(folder, f) for f in os.listdir(folder)) * 40
    whole = [load_fast5s._python_get_read_id_and_signal(f)[1] for f in files[:7]] * 40
    for scan in (6144, 512, 3072):
        ids, samples, offsets, status = fast5_native.load_batch(files, scan + 512, 4)
        assert (status == 0).all()
        for name, side in PLAN:
            model = hip_models[name]
            got_p, got_c = model.classify_packed(samples, offsets, side, scan, 0.5)
            want_p, want_c = model.classify_signals(whole, side, scan, 0.5)
            assert np.array_equal(got_c, want_c) and np.array_equal(got_p, want_p), (scan, name)
    with pytest.raises(ValueError):
        model.classify_packed(samples, offsets[:-1], 'start', 6144, 0.5)
    p, c = model.classify_packed(np.zeros(0, np.int16), np.zeros(1, np.int64), 'start', 6144, 0.5)
    assert p.shape == (0, model.n_classes) and c.shape == (0,)

    # the CLI loop: native reader (packed fast path) and Python reader print the same table
    args = argparse.Namespace(verbose=True, batch_size=64, scan_size=6144, score_diff=0.5,
                              require_either=True, require_start=False, require_both=False,
                              loader_procs=0)
    tables = {}
    for reader in ('native', 'python'):
        os.environ['DEEPBINNER_FAST5_READER'] = reader
        try:
            out = io.StringIO()
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
                classify.classify_fast5_files(
                    files[:100], hip_models['EXP-NBD103_read_starts'], 1024,
                    hip_models['EXP-NBD103_read_ends'], 1024, 13, args, verified_single_read=True)
            tables[reader] = out.getvalue()
        finally:
            del os.environ['DEEPBINNER_FAST5_READER']
    assert tables['native'] == tables['python'] and tables['native'].count('\n') == 101

    # realtime on multi-read containers: packed chunks (native) == per-read lists (Python reader)
    import shutil
    import deepbinner_amd.realtime as realtime
    from conftest import MODEL_DIR
    multi = os.path.join(REPO, 'tests', 'golden', 'fast5', 'multi')
    rows = {}
    for reader in ('native', 'python'):
        os.environ['DEEPBINNER_FAST5_READER'] = reader
        work = tempfile.mkdtemp()
        try:
            in_dir, out_dir = os.path.join(work, 'in'), os.path.join(work, 'out')
            shutil.copytree(multi, in_dir)
            rt_args = argparse.Namespace(
                in_dir=in_dir, out_dir=out_dir, stop=True, scan_size=6144.0, score_diff=0.5,
                start_model=os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'),
                end_model=os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw'), batch_size=7,
                require_either=True, require_start=False, require_both=False)
            realtime.POLL_SECONDS, keep_poll = 0, realtime.POLL_SECONDS
            which, shutil.which = shutil.which, (lambda name: None)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    realtime.realtime(rt_args)
            finally:
                realtime.POLL_SECONDS, shutil.which = keep_poll, which
            with open(os.path.join(out_dir, 'multi_read_classifications.tsv')) as f:
                rows[reader] = sorted(line.split('\t')[:2] for line in f.read().splitlines())
        finally:
            del os.environ['DEEPBINNER_FAST5_READER']
            shutil.rmtree(work)
    assert rows['native'] == rows['python'] and len(rows['native']) == 30


def test_combine_calls_on_the_device(hip, gold):
    """dbh_combine_calls_dev against the ORACLE: the reference's own truth table
    (tests/test_combine_calls.py as committed in calls.json:combine_table, produced by the
    reference's combine_calls) and oracle.classify_ref.combine_calls for every pair of calls in
    every mode, in place and out of place, and on 1M random pairs through the oracle's 13 x 13
    table."""
    grid = np.arange(13, dtype=np.int32)
    starts, ends = np.repeat(grid, 13), np.tile(grid, 13)
    name = lambda c: 'none' if c == 0 else str(int(c))                # noqa: E731
    number = lambda s: 0 if s == 'none' else int(s)                   # noqa: E731
    rng = np.random.default_rng(9)
    big_s = rng.integers(0, 13, size=1000003).astype(np.int32)
    big_e = np.where(rng.random(1000003) < 0.5, big_s, rng.integers(0, 13, size=1000003)) \
        .astype(np.int32)
    table = gold['calls']['combine_table']
    assert len(table) == 15
    for mode in ('require_either', 'require_start', 'require_both'):
        want = np.array([number(classify_ref.combine_calls(name(a), name(b), mode))
                         for a, b in zip(starts, ends)], dtype=np.int32)
        d_s, d_e = hip.DeviceBuffer.from_array(starts), hip.DeviceBuffer.from_array(ends)
        d_o = hip.DeviceBuffer(len(starts) * 4)
        hip.combine_calls_dev(d_s.ptr, d_e.ptr, len(starts), mode, d_o.ptr)
        hip.synchronize()
        got = d_o.download((len(starts),), np.int32)
        assert np.array_equal(got, want), mode
        for key, answer in table.items():          # the reference's own rows
            m, a, b = key.split('|')
            if m == mode:
                assert got[number(a) * 13 + number(b)] == number(answer), key
        hip.combine_calls_dev(d_s.ptr, d_e.ptr, len(starts), mode, d_s.ptr)      # in place
        hip.synchronize()
        assert np.array_equal(d_s.download((len(starts),), np.int32), got)
        d_s, d_e = hip.DeviceBuffer.from_array(big_s), hip.DeviceBuffer.from_array(big_e)
        d_o = hip.DeviceBuffer(len(big_s) * 4)
        hip.combine_calls_dev(d_s.ptr, d_e.ptr, len(big_s), mode, d_o.ptr)
        hip.synchronize()
        assert np.array_equal(d_o.download((len(big_s),), np.int32),
                              want.reshape(13, 13)[big_s, big_e]), mode
    hip.combine_calls_dev(None, None, 0, 'require_both', None)                   # nothing to do
    with pytest.raises(Exception):
        hip.check(hip.load_library().dbh_combine_calls_dev(d_s.ptr, d_e.ptr, 5, 7, d_o.ptr, None))


def _run_bench(extra_args, env_extra, launcher=None):
    import json
    import socket
    import subprocess
    import sys
    from conftest import REPO
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.update(env_extra)
    cmd = [sys.executable]
    if launcher:
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        cmd += ['-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(launcher),
                '--master-addr', '127.0.0.1', '--master-port', str(port)]
    cmd += [os.path.join(REPO, 'bench.py')] + extra_args
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_share_one_gpu(hip):
    """bench.py's one-process-per-GPU path as the driver launches it (torch.distributed.run env,
    own rendezvous, sharded reads, gather, MAX-over-ranks timing, one JSON line from rank 0) on a
    one-GPU box: both ranks use device 0, so the calls are gathered through host memory (RCCL
    refuses two ranks per device)."""
    result = _run_bench(['--gpus', '2', '--steps', '3', '--warmup', '1'],
                        {'DEEPBINNER_DEVICE_ORDINALS': '0,0', 'DEEPBINNER_COMM': 'host'},
                        launcher=2)
    assert result['n_gpus'] == 2 and result['steps'] == 3 and result['value'] > 0
    assert result['scaling'] == 'weak' and 'roofline' in result
    assert result['gather']['transport'] == 'host'
    assert result['config']['reads_per_step'] == 20000
    # three steps as ONE launch and one exchange per rank (--steps-per-launch defaults to 10 for
    # this configuration, cut down to a divisor of --steps); the line says which rank's launches
    # and which rank's wait in the exchange were the longest (round-4 verdict, item 6)
    assert result['config']['steps_per_launch'] == 3 and result['steps_of_a_launch_agree'] is True
    per_rank = result['roofline']['avg_launch_ms_per_rank']
    assert len(per_rank['per_rank']) == 2 and per_rank['slowest_rank'] in (0, 1)
    assert per_rank['min'] <= result['roofline']['avg_launch_ms'] <= per_rank['max']
    waits = result['gather']['wait_ms_per_exchange']
    assert len(waits['per_rank']) == 2 and waits['max'] > 0 and waits['longest_on_rank'] in (0, 1)
    assert result['gather']['steps_per_exchange'] == 3


def test_bench_one_process_two_devices(hip):
    """`python bench.py --gpus 2` started plainly: one process, a thread per device, grouped
    all-gather behind the C ABI (device copies here, since both "devices" are GPU 0)."""
    result = _run_bench(['--gpus', '2', '--steps', '3', '--warmup', '1'],
                        {'DEEPBINNER_DEVICE_ORDINALS': '0,0'})
    assert result['n_gpus'] == 2 and result['value'] > 0 and 'roofline' in result
    assert result['gather']['transport'] == 'copy'
    # device copies run on a side stream against double-buffered call arrays (sharding.SideGather)
    assert result['gather']['queued_on'].startswith('side stream')
    assert result['gather']['ms_per_step'] > 0
    assert result['config']['reads_per_step'] == 20000
    assert result['calls_not_none_rank0'] > 0          # the real-read windows classify
    assert len(result['roofline']['avg_launch_ms_per_rank']['per_rank']) == 2
    assert len(result['gather']['wait_ms_per_exchange']['per_rank']) == 2
    # one launch and one exchange per step (the form of rounds 1-4) gives the same calls
    single = _run_bench(['--gpus', '2', '--steps', '3', '--warmup', '1', '--steps-per-launch', '1',
                         '--no-side-rates', '--no-cpu-baseline'],
                        {'DEEPBINNER_DEVICE_ORDINALS': '0,0'})
    assert single['config']['steps_per_launch'] == 1 and single['gather']['steps_per_exchange'] == 1
    assert single['calls_not_none_rank0'] == result['calls_not_none_rank0']


def test_bench_rccl_path_single_rank(hip):
    """The RCCL code path of bench.py (rendezvous, ncclGetUniqueId / ncclCommInitRank through the
    C ABI, ncclAllGather of the calls on the launch stream, MAX-over-ranks) forced on with ONE rank
    under the driver's launcher - what the N = 2/4/8 runs execute, minus the peers."""
    result = _run_bench(['--gpus', '1', '--steps', '3', '--warmup', '1', '--full'],
                        {'DEEPBINNER_BENCH_FORCE_RANKS': '1', 'DEEPBINNER_COMM_FORCE': '1'},
                        launcher=1)
    assert result['n_gpus'] == 1 and result['value'] > 0 and 'roofline' in result
    assert result['gather']['transport'] == 'rccl' and result['gather']['fallback_reason'] is None
    # RCCL's collective stays on the classification stream (profiles/r04_gather_ab.txt); rank 0
    # brackets exchange + copy with events: the line says how long a step's gather took
    assert result['gather']['queued_on'] == 'classification stream'
    assert result['gather']['ms_per_step'] > 0
    assert result['cpu_baseline']['calls_match_gpu'] is True
    assert result['cpu_baseline']['calls_not_none_in_sample'] > 0
    assert result['cpu_baseline']['published']['source'] == 'README.md:213'
    from deepbinner_amd import misc
    assert result['cpu_baseline']['cores'] == misc.usable_cpus()     # the quota, not the 256 online
    assert result['cpu_baseline']['value_12_threads'] > 0
    assert 0 < result['roofline']['frac'] <= 1.0
    assert result['roofline']['frac_algorithmic_equivalent'] > result['roofline']['frac']
    assert result['config']['workload'].startswith(
        'BASELINE.json configs[1]: EXP-NBD103_read_starts model, 10000 synthetic')
    assert 'value_with_hint' in result and 'value_no_hint' not in result


def test_bench_rccl_single_process_form(hip):
    """ncclCommInitAll + grouped ncclAllGather (the `python bench.py --gpus N` form), one device."""
    result = _run_bench(['--gpus', '1', '--steps', '3', '--warmup', '1', '--no-cpu-baseline',
                         '--no-side-rates'], {'DEEPBINNER_COMM_FORCE': '1'})
    assert result['gather']['transport'] == 'rccl' and result['gather']['fallback_reason'] is None
    assert result['calls_not_none_rank0'] > 0


def test_bench_gather_on_the_side_stream_gives_the_same_calls(hip):
    """The side-stream form of the exchange forced for RCCL (one rank) over five steps - both
    sets of call arrays, each reused behind its release event: the calls that reach the host are
    the CPU port's, and the line says where the exchange was queued and how long it took."""
    result = _run_bench(['--gpus', '1', '--steps', '5', '--warmup', '2', '--no-side-rates',
                         '--full'],
                        {'DEEPBINNER_COMM_FORCE': '1', 'DEEPBINNER_BENCH_GATHER': 'side'})
    assert result['gather']['transport'] == 'rccl'
    assert result['gather']['queued_on'].startswith('side stream')
    assert result['gather']['ms_per_step'] > 0
    assert result['calls_not_none_rank0'] > 0
    assert result['cpu_baseline']['calls_match_gpu'] is True


def test_bench_dump_outputs_are_the_last_steps_results(hip, hip_models, tmp_path):
    """`bench.py --dump-outputs DIR` (a plain run, ten steps per launch cut down to three): the
    last step's calls and probabilities, float32, are what the model gives for the same seeded
    reads through the host entry point."""
    from bench import config_reads
    result = _run_bench(['--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path)], {})
    assert 'cpu_baseline' not in result and 'other_configs' not in result
    assert result['steps'] == 3 and result['config']['steps_per_launch'] == 3
    assert sorted(p.name for p in tmp_path.iterdir()) == ['calls.npy',
                                                          'probs_EXP-NBD103_read_starts.npy']
    calls = np.load(str(tmp_path / 'calls.npy'))
    probs = np.load(str(tmp_path / 'probs_EXP-NBD103_read_starts.npy'))
    assert calls.dtype == probs.dtype == np.float32
    assert calls.shape == (10000,) and probs.shape == (10000, 13)
    assert int((calls != 0).sum()) == result['calls_not_none_rank0'] > 0
    reads = config_reads(10000, 20260927)
    want_probs, want_calls = hip_models['EXP-NBD103_read_starts'].classify_packed(
        reads.reshape(-1), np.arange(10001, dtype=np.int64) * 1024, 'start', 512, 0.5)
    assert np.array_equal(calls, want_calls.astype(np.float32))
    assert float(np.abs(probs - want_probs).max()) < 1e-6


@pytest.mark.parametrize('config', [2, 3])
def test_bench_other_configs_run(hip, config):
    """--config 2 (two models + device combine, batch 512) and --config 3 (1M reads, RBK004)."""
    result = _run_bench(['--config', str(config), '--steps', '2', '--warmup', '1',
                         '--no-cpu-baseline'], {})
    assert result['value'] > 0 and 'roofline' in result
    assert result['config']['reads_per_step'] == (100000 if config == 2 else 1000000)
    assert result['scaling'] == ('weak' if config == 2 else 'strong')
    # sanity bounds only: a functional test must not turn red on a shared or throttled GPU (the
    # rate itself is tracked by bench.py / profiles/; DEEPBINNER_PERF_ASSERT=1 holds it to the
    # matrix pipe's busy fraction this kernel reaches on an idle MI355X)
    assert 0 < result['roofline']['frac'] <= 1.0
    # (a loose floor by default - a forward kernel at less than half its rate is a defect, not a busy
    # box: ADVICE round 5 -, the kernel's own figure when asked for)
    assert result['roofline']['frac'] > 0.3
    if os.environ.get('DEEPBINNER_PERF_ASSERT') == '1':
        assert result['roofline']['frac'] > 0.6
    assert result['roofline']['frac'] == result['roofline']['frac_executed']


def test_device_group_matches_single_device(hip, hip_models, weights, all_signals):
    """Two "devices" (both ordinal 0) through the single-process multi-device front: contiguous
    read shards, a model replica and a stream per device, the all-gather of the calls - the same
    calls and probabilities a single device gives, for ragged real reads and for a count that does
    not divide evenly."""
    from deepbinner_amd import sharding
    signals = (all_signals * 3)[:101]
    samples, offsets = pack(signals)
    want_probs, want_calls = hip_models['EXP-NBD103_read_starts'].classify_packed(
        samples, offsets, 'start', 6144, 0.5)
    for transport in ('copy', 'host'):
        group = sharding.DeviceGroup(weights['EXP-NBD103_read_starts'], 2, devices=[0, 0],
                                     transport=transport)
        assert group.transport == transport
        group.upload_sharded(samples, offsets)
        assert group.shard_sizes == [51, 50]
        group.run(lambda s: s.classify(8, 'start', 6144, 0.5))
        group.all_gather()
        group.synchronize()
        for device_index in (0, 1):        # every device holds the whole job's calls
            assert np.array_equal(group.gathered_calls(device_index), want_calls)
        probs = np.concatenate(group.run(
            lambda s: s.probs.download((s.n_reads, 13), np.float32, s.stream.ptr)))
        assert np.array_equal(probs, want_probs)
        group.close()


def test_device_group_with_rccl_itself(hip, hip_models, weights, all_signals, monkeypatch):
    """Round-2 verdict: the single-process form THROUGH DeviceGroup with RCCL underneath
    (ncclCommInitAll over [0], the grouped ncclAllGather on the shard's own stream, behind the
    classification) - what `python bench.py --gpus N` runs, with the one device this box has -
    and several steps queued back to back (the gather of step k must not be overtaken by the
    classification of step k+1: the stream orders them)."""
    from deepbinner_amd import sharding
    monkeypatch.setenv('DEEPBINNER_COMM_FORCE', '1')
    signals = (all_signals * 2)[:53]
    samples, offsets = pack(signals)
    want_probs, want_calls = hip_models['EXP-NBD103_read_starts'].classify_packed(
        samples, offsets, 'start', 6144, 0.5)
    group = sharding.DeviceGroup(weights['EXP-NBD103_read_starts'], 1, devices=[0],
                                 transport='rccl')
    assert group.transport == 'rccl' and group.comm is not None and group.fallback_reason is None
    assert (group.comm.n_ranks, group.comm.n_local) == (1, 1)
    group.upload_sharded(samples, offsets)
    assert group.shards[0].gathered is not group.shards[0].calls      # a real receive buffer
    for _ in range(3):
        group.run(lambda s: s.classify(8, 'start', 6144, 0.5))
        group.all_gather()
    group.synchronize()
    assert np.array_equal(group.gathered_calls(0), want_calls)
    group.close()


def test_copy_transport_steps_queued_back_to_back(hip, weights, all_signals):
    """with the COPY transport a device's next classification must wait until every
    other device has pulled its calls (the back edge).  Two shards on GPU 0, ten steps queued
    without a synchronisation in between, the reads swapped between the steps: after every
    odd/even step the gathered calls are that step's."""
    from deepbinner_amd import sharding
    signals = (all_signals * 2)[:60]
    variants = [pack(signals), pack(signals[::-1])]
    group = sharding.DeviceGroup(weights['EXP-NBD103_read_starts'], 2, devices=[0, 0],
                                 transport='copy')
    want = []
    for samples, offsets in variants:
        group.upload_sharded(samples, offsets)
        group.run(lambda s: s.classify(8, 'start', 6144, 0.5))
        group.all_gather()
        group.synchronize()
        want.append(group.gathered_calls(0).copy())
    assert not np.array_equal(want[0], want[1])
    group.upload_sharded(*variants[0])
    for step in range(10):
        group.run(lambda s: s.classify(8, 'start', 6144, 0.5))
        group.all_gather()
    group.synchronize()
    for device_index in (0, 1):
        assert np.array_equal(group.gathered_calls(device_index), want[0])
    group.close()


def test_bench_says_in_one_line_that_devices_are_missing(hip):
    """`bench.py --gpus N` with fewer than N devices visible: a one-line error and a non-zero
    exit, not a traceback per worker thread."""
    import subprocess
    import sys
    from conftest import REPO
    wanted = hip.device_count() + 1
    env = dict(os.environ)
    env.pop('DEEPBINNER_DEVICE_ORDINALS', None)
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', str(wanted),
                          '--steps', '1', '--warmup', '0'], env=env, capture_output=True,
                         text=True, timeout=600, cwd=REPO)
    assert out.returncode != 0
    message = [l for l in out.stderr.splitlines() if l.strip()]
    assert message[-1] == 'bench.py: {} devices wanted, {} visible'.format(wanted, wanted - 1)
    assert 'Traceback' not in out.stderr


def test_rccl_all_gather_through_the_c_abi(hip):
    """dbh_comm_* with RCCL itself: both forms of communicator set-up with the one GPU this box
    has (ncclCommInitAll over [0]; ncclGetUniqueId + ncclCommInitRank with one rank)."""
    from deepbinner_amd import sharding
    assert hip.load_library().dbh_comm_available() == 1
    data = np.arange(1000, dtype=np.int32) * 7 - 3
    for make in (lambda: sharding.Communicator.init_all([0]),
                 lambda: sharding.Communicator.init_rank(sharding.Rendezvous(0, 1))):
        hip.set_device(0)
        comm = make()
        assert (comm.n_ranks, comm.n_local, comm.transport) == (1, 1, sharding.TRANSPORT_RCCL)
        stream = hip.Stream()
        send = hip.DeviceBuffer.from_array(data)
        recv = hip.DeviceBuffer(data.nbytes)
        comm.all_gather_i32([send.ptr], [recv.ptr], len(data), [stream.ptr])
        assert np.array_equal(recv.download(data.shape, np.int32, stream.ptr), data)
        comm.close()
        stream.close()


def test_cli_classify_two_ranks_share_one_gpu(hip):
    """The real CLI under the driver's launcher with 2 ranks on this box's single GPU (calls
    gathered through host memory): every read printed once, in file order, with the reference's
    expected calls; rank 0 prints the summary."""
    import socket
    import subprocess
    import sys
    from conftest import REPO
    from test_oracle_golden import EXPECTED_END
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=REPO, DEEPBINNER_COMM='host', DEEPBINNER_DEVICE='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(port), '-m', 'deepbinner_amd',
           'classify', '--native', '--require_both', '--batch_size', '2',
           os.path.join(GOLD, 'fast5', 'single')]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    rows = dict(l.split('\t') for l in out.stdout.splitlines() if '\t' in l)
    assert rows.pop('read_ID') == 'barcode_call'
    assert rows == EXPECTED_END          # require_both column of the reference's tests
    assert 'Barcode     Count' in out.stderr


@pytest.mark.skipif(os.environ.get('DEEPBINNER_SOAK') != '1',
                    reason='minutes of CPU work: set DEEPBINNER_SOAK=1 (optionally '
                           'DEEPBINNER_SOAK_READS=n)')
def test_soak_against_c_port(hip, hip_models, weights):
    """A large sample (default 500,000 distinct synthetic reads, both sides) against the oracle's
    C port: identical calls except where best - second sits on the threshold, probabilities
    within tolerance everywhere."""
    from bench import synthetic_reads
    from oracle import dbref
    total = int(os.environ.get('DEEPBINNER_SOAK_READS', '500000'))
    model = hip_models['EXP-NBD103_read_starts']
    cm = dbref.CModel(weights['EXP-NBD103_read_starts'])
    worst, on_threshold, chunk = 0.0, 0, 50000
    for k, first in enumerate(range(0, total, chunk)):
        n = min(chunk, total - first)
        reads = synthetic_reads(n, 777 + k)
        # make the sample less benign: scale / offset / clip some reads
        rng = np.random.default_rng(k)
        scale = rng.uniform(0.3, 3.0, size=(n, 1))
        reads = np.clip(np.rint((reads - 450) * scale + rng.integers(0, 900, size=(n, 1))),
                        -32768, 32767).astype(np.int16)
        offsets = np.arange(n + 1, dtype=np.int64) * 1024
        side = 'start' if k % 2 == 0 else 'end'
        want_probs, want_calls = cm.classify(reads.reshape(-1), offsets, side, 512, 0.5)
        probs, calls = model.classify_signals(list(reads), side, 512, 0.5)
        worst = max(worst, float(np.abs(probs - want_probs).max()))
        for i in np.flatnonzero(calls != want_calls):
            top = np.sort(want_probs[i].astype(np.float64))[::-1]
            assert abs((top[0] - top[1]) - 0.5) < 1e-5, (k, i)
            on_threshold += 1
    print('soak: {} reads, max |dp| {:.3e}, {} calls on the threshold'.format(total, worst,
                                                                            on_threshold))
    assert worst < PROB_TOL



# ---- the reference's own command line, end to end, on the real backend --------------------------
def _reference_cli_cases():
    import json
    with open(os.path.join(GOLD, 'reference_cli.json')) as f:
        return json.load(f)


def test_realtime_as_the_reference_runs_it_on_the_gpu(hip, tmp_path, capsys, monkeypatch):
    """The reference's realtime.py end to end (oracle/make_cli_golden.py): same stdout, same files
    in the same bins, with the HIP kernels doing the classification."""
    import shutil
    from conftest import MODEL_DIR
    from deepbinner_amd import deepbinner as cli
    import deepbinner_amd.realtime as realtime
    want = _reference_cli_cases()['realtime_two_models']
    monkeypatch.setattr(realtime, 'POLL_SECONDS', 0)
    for k, reader in enumerate(('native', 'python')):
        monkeypatch.setenv('DEEPBINNER_FAST5_READER', reader)
        work = tmp_path / str(k)
        in_dir, out_dir = work / 'in', work / 'out'
        shutil.copytree(os.path.join(GOLD, 'fast5', 'single'), in_dir)
        capsys.readouterr()
        cli.main(['realtime', '--in_dir', str(in_dir), '--out_dir', str(out_dir), '--stop',
                  '-s', os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'),
                  '-e', os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw')])
        text = capsys.readouterr().out.replace(str(work), '<WORK>') \
            .replace(MODEL_DIR + '/', 'MODELS/').replace('.dbw', '')
        assert text == want['stdout']
        assert {d: sorted(os.listdir(out_dir / d)) for d in sorted(os.listdir(out_dir))} == \
            want['tree']
        assert sorted(os.listdir(in_dir)) == want['left_in_in_dir']


def test_dispatcher_two_device_queues_reproduce_the_reference(hip, tmp_path, capsys, monkeypatch):
    """BASELINE.json configs[4] in the small: the single-process multi-device dispatcher with TWO
    device queues (both on GPU 0: DEEPBINNER_DEVICE_ORDINALS=0,0), batches dealt round-robin,
    results re-ordered - `classify --devices 2` prints the reference's table, `realtime --devices 2`
    reproduces the reference's own realtime run (stdout and bins), and a multi-read container is
    tabulated with the calls the one-read files of the same reads get."""
    import shutil
    from conftest import MODEL_DIR, REPO
    from deepbinner_amd import classify, deepbinner as cli
    import deepbinner_amd.realtime as realtime
    monkeypatch.setenv('DEEPBINNER_DEVICE_ORDINALS', '0,0')
    cases = _reference_cli_cases()
    models = ['-s', os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'),
              '-e', os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw')]
    # classify: the two-model verbose case of the reference's command-line goldens, batch size 2
    # so that the seven reads are four batches over the two queues
    case = cases['native_preset_verbose']           # --native = EXP-NBD103 start + end models
    argv = [os.path.join(MODEL_DIR, a[7:] + '.dbw') if a.startswith('MODELS/')
            else os.path.join(REPO, a) if a.startswith('tests/') else a for a in case['argv']]
    capsys.readouterr()
    cli.main(argv + ['--devices', '2', '--batch_size', '2'])
    assert classify._DEVICES == [0, 0]
    captured = capsys.readouterr()
    rows = captured.out.splitlines()
    assert rows[0] == case['header'] and len(rows) - 1 == len(case['rows'])
    assert [r.split('\t')[:2] for r in sorted(rows[1:])] == \
        [r.split('\t')[:2] for r in case['rows']]
    assert captured.err.split('Barcode     Count')[-1].split() == case['summary']
    # realtime on one-read files: the reference's own run
    want = cases['realtime_two_models']
    monkeypatch.setattr(realtime, 'POLL_SECONDS', 0)
    work = tmp_path / 'single'
    in_dir, out_dir = work / 'in', work / 'out'
    shutil.copytree(os.path.join(GOLD, 'fast5', 'single'), in_dir)
    capsys.readouterr()
    cli.main(['realtime', '--in_dir', str(in_dir), '--out_dir', str(out_dir), '--stop',
              '--devices', '2', '--batch_size', '2'] + models)
    text = capsys.readouterr().out.replace(str(work), '<WORK>') \
        .replace(MODEL_DIR + '/', 'MODELS/').replace('.dbw', '')
    # four batches of two reads instead of the reference's one of seven: three more progress
    # updates on the line; everything else is the reference's output
    import re
    text = re.sub(r'\rClassifying fast5s: [246] / 7 \(\d+\.\d%\)', '', text)
    assert text == want['stdout']
    assert {d: sorted(os.listdir(out_dir / d)) for d in sorted(os.listdir(out_dir))} == want['tree']
    # realtime on a multi-read container: every read tabulated once, with the calls a single
    # device gives (chunks of 4 reads over the two queues)
    multi = sorted(os.listdir(os.path.join(GOLD, 'fast5', 'multi')))
    work = tmp_path / 'multi'
    in_dir, out_dir = work / 'in', work / 'out'
    os.makedirs(in_dir)
    for name in multi:
        shutil.copy(os.path.join(GOLD, 'fast5', 'multi', name), in_dir / name)
    monkeypatch.setattr(shutil, 'which', lambda tool: None)       # no multi_to_single_fast5
    cli.main(['realtime', '--in_dir', str(in_dir), '--out_dir', str(out_dir), '--stop',
              '--devices', '2', '--batch_size', '4'] + models)
    capsys.readouterr()
    table = [l.split('\t') for l in
             (out_dir / 'multi_read_classifications.tsv').read_text().splitlines()]
    monkeypatch.delenv('DEEPBINNER_DEVICE_ORDINALS')
    single_dir, single_out = tmp_path / 'multi1' / 'in', tmp_path / 'multi1' / 'out'
    os.makedirs(single_dir)
    for name in multi:
        shutil.copy(os.path.join(GOLD, 'fast5', 'multi', name), single_dir / name)
    cli.main(['realtime', '--in_dir', str(single_dir), '--out_dir', str(single_out), '--stop',
              '--batch_size', '4'] + models)
    assert classify._DEVICES is None
    capsys.readouterr()
    want_table = [l.split('\t') for l in
                  (single_out / 'multi_read_classifications.tsv').read_text().splitlines()]
    assert len(table) == len(want_table) > 20
    assert [r[:2] for r in table] == [r[:2] for r in want_table]


@pytest.mark.parametrize('name', sorted(k for k, v in _reference_cli_cases().items()
                                        if 'argv' in v))
def test_command_line_prints_the_reference_table(hip, name, capsys, monkeypatch):
    """tests/golden/reference_cli.json is what the reference's deepbinner.py / classify.py /
    load_fast5s.py (h5py) printed with the oracle's network behind model.predict
    (oracle/make_cli_golden.py).  The same command lines here, HIP kernels behind every seam:
    same header, same calls, same summary; printed probabilities ('%.2f') equal unless a value
    sits within 1e-4 of a rounding boundary."""
    from conftest import MODEL_DIR, REPO
    from deepbinner_amd import deepbinner as cli
    case = _reference_cli_cases()[name]
    argv = [os.path.join(MODEL_DIR, a[7:] + '.dbw') if a.startswith('MODELS/')
            else os.path.join(REPO, a) if a.startswith('tests/') else a for a in case['argv']]
    for reader in ('native', 'python'):
        monkeypatch.setenv('DEEPBINNER_FAST5_READER', reader)
        capsys.readouterr()
        cli.main(argv)
        captured = capsys.readouterr()
        rows = captured.out.splitlines()
        assert rows[0] == case['header']
        assert captured.err.split('Barcode     Count')[-1].split() == case['summary']
        got = sorted(rows[1:])
        assert len(got) == len(case['rows'])
        for mine, theirs in zip(got, case['rows']):
            if mine == theirs:
                continue
            a, b = mine.split('\t'), theirs.split('\t')
            assert len(a) == len(b)
            for x, y in zip(a, b):
                if x != y:          # both must be probabilities, one rounding step apart
                    assert abs(float(x) - float(y)) < 0.0101, (mine, theirs)


def test_the_readme_walkthrough_on_the_gpu(hip, tmp_path, capsys, monkeypatch):
    """BASELINE.json configs[0] on the real backend: sample_reads.tar.gz through classify
    --native and bin gives the table and the binned files the reference's own code gave."""
    from conftest import check_the_readme_walkthrough, run_the_readme_walkthrough
    want = _reference_cli_cases()['sample_reads_walkthrough']
    for k, reader in enumerate(('native', 'python')):
        monkeypatch.setenv('DEEPBINNER_FAST5_READER', reader)
        work = tmp_path / str(k)
        work.mkdir()
        check_the_readme_walkthrough(run_the_readme_walkthrough(work, capsys), want)
