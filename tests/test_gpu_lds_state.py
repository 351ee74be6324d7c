"""Output must not depend on what the LDS held when a workgroup started (needs an MI355X; `-m gpu`).

LDS is not cleared between workgroups (the first test shows it: a fill reaches every CU and a
survey finds every word of it afterwards).  A kernel that reads a word of its __shared__ arena
before it has written it - a sync word taken for zero, a halo row "published" by nobody, a dummy
region, a staging area that is only valid from the second group on - computes with what the
workgroup before left there, and passes every test that happens to run behind a well-behaved
kernel.  Here every unit with a __shared__ arena runs behind a fill of each of

    0x00000000  the control              0x3F800000  1.0: survives where NaN x 0 would be caught
    0xFFFFFFFF  NaN, -1 as a counter     0x00000009  a sync word that already looks "arrived"
    0x7F800000  +inf                     0x80000000  -0.0, a huge epoch as a counter

and must give the control's result TO THE BIT (``as_bits``: shape, type and bytes of every array of
the result - what ``same_bits`` of tests/test_gpu_forward_builds.py asks, for any type).  The control itself passes the comparison the operation's own test makes
against its reference - the fp64 oracle, the CPU model, the NumPy restatement - so a wrong control
cannot pass by agreeing with itself.  The fill goes on the null stream and is followed by a device
synchronise (``fill_lds``); LDS needs no stream order.

No kernel here accumulates with float atomics (the tally's are integer counts), so none needed a
tolerance in place of the bits."""
import functools
import os
import struct

import numpy as np
import pytest

import general_fixtures
from conftest import GOLD
from test_gpu_forward_builds import MODELS, builds, ragged      # noqa: F401 (builds: a fixture)

pytestmark = pytest.mark.gpu

CONTROL = 0x00000000
POISONS = [0xFFFFFFFF, 0x7F800000, 0x3F800000, 0x00000009, 0x80000000]
PROB_TOL = 1e-4               # tests/test_gpu_parity.py
STAGE_TOL = 2e-5              # ... test_stage_activations: of scale = max(1, |want|.max())


def fill(hip, pattern):
    """A fill counts only if it saw every CU."""
    seen, total = hip.fill_lds(pattern)
    assert seen == total > 0, (hex(pattern), seen, total)


def test_lds_fill_reaches_every_cu_and_persists(hip):
    """20 of 20 fills see every CU, and a survey straight after a fill finds the pattern in every
    word on every CU (profiles/lds_state/survey.txt): the hardware and the driver clear nothing
    between dispatches, so what the tests below put there is what the kernels find."""
    for _ in range(20):
        fill(hip, 0xA5A5A5A5)
    for pattern in [CONTROL] + POISONS:
        fill(hip, pattern)
        matching, looked_at, total = hip.survey_lds(pattern)
        assert len(looked_at) == total, (hex(pattern), len(looked_at), total)
        assert (looked_at >= hip.LDS_ARENA_WORDS).all() and (looked_at % hip.LDS_ARENA_WORDS == 0).all()
        assert np.array_equal(matching, looked_at), (hex(pattern), int((matching != looked_at).sum()))
    other, looked_at, _ = hip.survey_lds(0x12345678)      # (the survey counts, it does not flatter)
    assert not other.any() and looked_at.all()


def as_bits(a):
    """Any result - array, bytes, number, tuple of them - as a tuple of (shape, dtype, bytes)."""
    if isinstance(a, (tuple, list)):
        return tuple(x for item in a for x in as_bits(item))
    if a is None:
        return (None,)
    if isinstance(a, (bytes, bytearray, memoryview)):
        return (bytes(a),)
    a = np.ascontiguousarray(a)
    return ((a.shape, a.dtype.str, a.tobytes()),)


def behind_every_fill(hip, run, check, what):
    """``run`` behind a fill of zeros, held to its reference by ``check``; then behind every other
    fill, held to that control to the bit."""
    fill(hip, CONTROL)
    control = run()
    check(control)
    want = as_bits(control)
    for pattern in POISONS:
        fill(hip, pattern)
        got = as_bits(run())
        assert len(got) == len(want), (what, hex(pattern))
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, '{}: result {} behind a fill of {:08X} is not the control\'s'.format(
                what, i, pattern)


# ---- the persistent forward kernel ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_call_batch(name, n, seed, side, scan):
    """(call names, merged probabilities) of the fp64 oracle for ``ragged(all_signals, n, seed)``."""
    from oracle import classify_ref, network_ref
    w = general_fixtures.shipped(name)
    signals = ragged(golden_all_signals(), n, seed)
    return classify_ref.call_batch(
        lambda x: network_ref.forward(w, x.astype(np.float32), dtype=np.float64), signals, 1024,
        scan, 0.5, side)


@functools.lru_cache(maxsize=None)
def golden_all_signals():
    """conftest's all_signals, for the cached oracles (a fixture cannot be a cache key)"""
    reads = np.load(os.path.join(GOLD, 'reads.npz'))
    out = []
    for s, o in (('samples', 'offsets'), ('multi_samples', 'multi_offsets')):
        out += [reads[s][reads[o][i]:reads[o][i + 1]] for i in range(len(reads[o]) - 1)]
    return tuple(out)


def check_classified(name, n, seed, side, scan):
    """tests/test_gpu_parity.py::test_classify_ragged_and_degenerate_reads' comparison"""
    def check(result):
        probs, calls = result
        o_calls, o_probs = oracle_call_batch(name, n, seed, side, scan)
        assert ['none' if c == 0 else str(int(c)) for c in calls] == list(o_calls)
        assert np.abs(probs - o_probs).max() < PROB_TOL
    return check


@pytest.mark.parametrize('build', ['full', 'lean'])
@pytest.mark.parametrize('name', MODELS)
def test_forward_seam_b2(hip, builds, all_signals, name, build):
    """classify_signals on a few ragged reads: fewer reads than a group, one group, one more, two
    groups, one more; from the start and from the end; one window per read (the fused call) and two
    (per-window probabilities and the merge kernel).  Every launch here is a workgroup's first
    group: the cold path."""
    model = builds[name, 'wide', build]
    for n in (1, 3, 4, 5, 9):
        signals = ragged(all_signals, n, n)
        for side in ('start', 'end'):
            for scan in (512, 1024):
                behind_every_fill(hip, lambda: model.classify_signals(signals, side, scan, 0.5),
                                  check_classified(name, n, n, side, scan),
                                  'classify_signals {} {} n {} {} scan {}'.format(name, build, n, side, scan))


@pytest.mark.parametrize('build', ['full', 'lean'])
@pytest.mark.parametrize('name', MODELS)
def test_forward_seam_b1(hip, builds, name, build):
    """predict on five golden windows, against the golden probabilities of the fp64 oracle."""
    model = builds[name, 'wide', build]
    x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)[:5]
    want = np.load(os.path.join(GOLD, 'window_probs_%s_start.npy' % name))[:5]

    def check(got):
        assert got.shape == want.shape and np.abs(got - want).max() < PROB_TOL
        assert np.array_equal(got.argmax(axis=1), want.argmax(axis=1))
    behind_every_fill(hip, lambda: model.predict(x), check, 'predict {} {}'.format(name, build))


@pytest.mark.parametrize('setting', ['cap2', 'cap2_static'])
@pytest.mark.parametrize('build', ['full', 'lean'])
@pytest.mark.parametrize('name', MODELS)
def test_forward_long_shares_on_two_workgroups(hip, builds, all_signals, name, build, setting):
    """27 reads over two workgroups, so that later groups, the staged path, the shrinking groups
    and full and partial tail batches all run behind a fill."""
    model = builds[name, setting, build]
    signals = ragged(all_signals, 27, 27)
    for side, scan in (('start', 512), ('end', 1024)):
        behind_every_fill(hip, lambda: model.classify_signals(signals, side, scan, 0.5),
                          check_classified(name, 27, 27, side, scan),
                          'classify_signals {} {} {} {} scan {}'.format(name, build, setting, side, scan))


@pytest.mark.parametrize('build', ['full', 'lean'])
@pytest.mark.parametrize('name', MODELS)
def test_forward_zero_copy(hip, builds, all_signals, name, build):
    """The reads in a dbh_malloc_host buffer, which the kernel reads in place, through sweep_pair
    in one group.  The control's calls at every scan size and score_diff 0.5 are the oracle's."""
    import sweep_reference
    from test_gpu_sweep import pinned_copy
    model = builds[name, 'wide', build]
    n, steps = 9, 4
    signals = ragged(all_signals, n, n)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
    samples = np.concatenate(signals).astype(np.int16)

    def check(result):
        (best, margin), _ = result
        assert best.shape == margin.shape == (n, steps)
        for k in range(1, steps + 1):
            o_calls, _ = oracle_call_batch(name, n, n, 'start', k * 512)
            calls = sweep_reference.calls_at(best[:, k - 1], margin[:, k - 1], 0.5)
            assert ['none' if c == 0 else str(int(c)) for c in calls] == list(o_calls), k
    with pinned_copy(hip, samples) as pinned:
        behind_every_fill(hip, lambda: hip.sweep_pair(model, None, pinned, offsets, steps * 512),
                          check, 'sweep_pair of pinned reads {} {}'.format(name, build))


@functools.lru_cache(maxsize=None)
def oracle_stages(name):
    from oracle import network_ref
    x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)[:5].astype(np.float32)
    return network_ref.forward(general_fixtures.shipped(name), x, dtype=np.float64, return_stages=True)[1]


@pytest.mark.parametrize('stage', ['A', 'B', 'C', 'D', 'E', 'F', 'G', 'logits'])
@pytest.mark.parametrize('name', MODELS)
def test_forward_debug_stages(hip, builds, name, stage):
    """The debug stages 0-7 on five windows (the full kernel serves them for either build), each
    against its own control dump; the control against the fp64 oracle's activations by the rule of
    tests/test_gpu_parity.py::test_stage_activations."""
    model = builds[name, 'wide', 'full']
    x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)[:5]

    def check(got):
        want = np.asarray(oracle_stages(name)[stage]).reshape(5, -1)
        got = got.reshape(5, -1)[:, :want.shape[1]] if stage == 'logits' else got.reshape(5, -1)
        scale = max(1.0, float(np.abs(want).max()))
        assert float(np.abs(got - want).max()) < STAGE_TOL * scale
    behind_every_fill(hip, lambda: model.debug_stage(x, stage), check,
                      'debug stage {} {}'.format(stage, name))


# ---- every other unit with a __shared__ arena --------------------------------------------------------
def case_general(hip):
    """dbh_general.hip: front, head and merge kernels - 96 samples, 33 classes, 5 windows, with evidence"""
    import locate_reference
    from oracle import classify_ref, network_ref
    model = hip.HipModel(general_fixtures.geometry(96, 33), device=0, general=True)
    windows = classify_ref.make_windows(general_fixtures.golden_signals(), 96, 3 * 48, 'start')
    windows = np.ascontiguousarray(windows.reshape(-1, 96)[:5], dtype=np.float32)
    signals = general_fixtures.synthetic_reads(96, 144, 5)

    def run():
        return model.evidence(windows) + model.classify_signals(signals, 'end', 144, 0.5)

    def check(result):
        probs, evidence, merged, calls = result
        want = network_ref.forward(model.weights, windows, dtype=np.float64)
        assert float(np.abs(probs - want).max()) <= 1e-4
        _, e64, _ = locate_reference.evidence(model.weights, windows)
        assert float(np.abs(evidence - e64).max()) <= 2e-5 * max(1.0, float(np.abs(e64).max()))
        _, o_probs = classify_ref.call_batch(
            lambda w: network_ref.forward(model.weights, np.asarray(w, np.float32), dtype=np.float64),
            signals, 96, 144, 0.5, 'end')
        assert float(np.abs(merged - o_probs).max()) <= 1e-4
    return run, check, model.close


def case_sweep(hip):
    """dbh_sweep.hip: fold32 (32 lanes per read), fold256 (a workgroup per read) and the tally"""
    import sweep_reference as ref
    persistent = hip.HipModel(general_fixtures.geometry(1024, 13), device=0)
    general = hip.HipModel(general_fixtures.geometry(96, 256), device=0)
    probs13, probs256 = ref.hand_made(13, 12, seed=1), ref.hand_made(256, 12, seed=2)
    rng = np.random.default_rng(5)
    sides = [(rng.integers(0, 13, (40, 3)).astype(np.int32), rng.choice([0.2, 0.5, 0.7], (40, 3)))
             for _ in range(2)]
    labels = rng.integers(-1, 13, 40).astype(np.int32)

    def run():
        return (hip.sweep_windows(persistent, probs13), hip.sweep_windows(general, probs256),
                hip.sweep_tally(sides[0], sides[1], [0.5, 0.7], 13, labels))

    def check(result):
        for (best, margin), probs in zip(result[:2], (probs13, probs256)):
            want_best, want_margin = ref.sweep(probs)
            assert np.array_equal(best, want_best) and np.abs(margin - want_margin).max() <= 1e-12
        assert np.array_equal(result[2], ref.tally(sides[0], sides[1], [0.5, 0.7], 13, labels))

    def close():
        persistent.close()
        general.close()
    return run, check, close


def case_scan(hip):
    """dbh_scan.hip: the window offsets' prefix, the ragged front and the event pass"""
    import scan_reference as ref
    rng = np.random.default_rng(96)
    reads = [rng.integers(-3000, 3000, n).astype(np.int16) for n in ref.lengths_around(96)]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    samples = np.concatenate(reads).astype(np.int16)
    best, margin, track_offsets = ref.random_track(rng, np.array([1, 64, 65, 200]), 0.3)

    def run():
        events, total, interior = hip.scan_events(best, margin, track_offsets, 0.5, 1, 2)
        return (hip.scan_window_offsets(offsets, 96), hip.scan_windows(samples, offsets, 96, 'end'),
                events, total, interior)

    def check(result):
        got_offsets, windows, events, total, interior = result
        assert np.array_equal(got_offsets, ref.window_offsets([len(r) for r in reads], 96))
        want = ref.batch_windows(reads, 96, 'end')
        assert np.array_equal(np.ascontiguousarray(windows).view(np.uint32),
                              np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))
        want_events, want_total, want_interior = ref.events(best, margin, track_offsets, 0.5, 1, 2)
        assert total == want_total > 0 and np.array_equal(interior, want_interior)
        assert np.array_equal(events, want_events)
    return run, check, None


def case_locate(hip):
    """dbh_locate.hip: the rule's kernel against its CPU model"""
    import locate_reference as ref
    ev, calls, lengths, input_size = ref.random_case(*ref.RANDOM_CASES[2], seed=8)

    def run():
        return hip.locate_rule_dev(ev, calls, lengths, input_size, 'start')

    def check(got):
        want = hip.locate_rule(ev, calls, lengths, input_size, 'start')
        assert got.tobytes() == want.tobytes()
    return run, check, None


def case_inflate(hip):
    """dbh_inflate.hip: a fixed, a dynamic and a stored block of tests/deflate_cases.py (families A,
    C and D: the first accepted case of each), under both forms of the launch"""
    import deflate_cases as dc
    from test_inflate import pack_streams
    families = dc.families()
    cases = [next(c for c in families[f] if c[3]) for f in 'ACD']
    comp, records, out_bytes, places = pack_streams(
        hip, [(stream, wanted, hip.INFLATE_ZLIB) for _, stream, wanted, _ in cases])

    def run():
        result = []
        for pair in ('1', '0'):
            os.environ['DEEPBINNER_INFLATE_PAIR'] = pair
            try:
                out, status, _ = hip.inflate(comp, records, out_bytes)
            finally:
                del os.environ['DEEPBINNER_INFLATE_PAIR']
            result += [out, status]
        return tuple(result)

    def check(result):
        for out, status in (result[:2], result[2:]):
            assert not status.any()
            for (name, _, _, data), (at, cap) in zip(cases, places):
                assert out[at:at + cap].tobytes() == data + bytes(cap - len(data)), name
    return run, check, None


def case_zstd(hip):
    """dbh_zstd.hip: one frame of each family A-D of tests/zstd_written.py (of each, the valid one
    with the most content up to 70,000 bytes)"""
    import zstd_written as zw
    from zstd_gpu import VBZ_ZSTD, run as run_streams
    families = zw.families()
    cases = [max((c for c in families[f] if c[2] and len(c[2]) <= 70000), key=lambda c: len(c[2]))
             for f in 'ABCD']
    items = [(struct.pack('<I', 2 * ((len(content) + 7) // 8) + 34) + frame,
              2 * ((len(content) + 7) // 8) + 34, VBZ_ZSTD) for _, frame, content, _ in cases]

    def run():
        outs, status, slots = run_streams(hip, items)
        return tuple(outs) + (status,) + tuple(slots)

    def check(result):
        status, slots = result[len(cases)], result[len(cases) + 1:]
        for (name, _, content, _), st, slot in zip(cases, status, slots):
            assert st in (0, 1) and bytes(slot[:len(content)]) == content, (name, int(st))
    return run, check, None


def case_vbz(hip):
    """dbh_vbz.hip: a stream of every code length, more than one step of a wavefront long"""
    import vbz_reference as ref
    from zstd_gpu import run as run_streams
    rng = np.random.default_rng(3109)
    payloads = [ref.mixed_stream(rng, n) for n in (17, 1025, 3109)]
    items = [(p, 2 * n + 6, 2) for p, n in zip(payloads, (17, 1025, 3109))]

    def run():
        outs, status, _ = run_streams(hip, items)
        return tuple(outs) + (status,)

    def check(result):
        for (payload, out_bytes, _), out, st in zip(items, result, result[-1]):
            ok, want = ref.expected(payload, out_bytes)
            assert ok and st == 0 and np.array_equal(out.view(np.int16), want)
    return run, check, None


def case_text(hip):
    """dbh_text.hip: the parser against its CPU model, on strict lines and a malformed one"""
    import text_format_reference as fr
    labels, samples = fr.rows(65)
    text = fr.text(labels, samples) + b'7\t1,2,x\n' + fr.text(labels[:2], samples[:2])

    def run():
        return hip.parse_training_text(text, 65)

    def check(got):
        want = hip.parse_training_text_host(text, 65)
        assert got[3] == want[3] == 6 and np.array_equal(got[2], want[2])
        ok = got[2] == hip.TEXT_OK
        assert np.array_equal(got[0][ok], want[0][ok]) and np.array_equal(got[1][ok], want[1][ok])
        assert np.array_equal(got[0][:6], samples) and np.array_equal(got[1][:6], labels)
    return run, check, None


def case_format(hip):
    """dbh_format.hip: the formatter against its CPU model and Python's own formatting"""
    import text_format_reference as fr
    labels, samples = fr.rows(65)

    def run():
        return hip.format_training_text(labels, samples)

    def check(got):
        assert got == hip.format_training_text(labels, samples, host=True) == fr.text(labels, samples)
    return run, check, None


def case_feed(hip):
    """dbh_feed.hip: an augmented batch against the NumPy restatement"""
    import feed_reference as fr
    from test_gpu_feed import signal_windows
    length, slots, aug, seed, n, classes = 96, 8, 2.0, 1, 12, 5
    samples, labels = signal_windows(length, n, classes)
    indices = np.array([0, n - 1, n - 4, n - 3, n - 2, n - 1, 3, 0])
    data = hip.Dataset.from_arrays(samples, labels, classes)

    def run():
        return data.batch(indices, aug, seed)

    def check(got):
        want_x, want_labels = fr.batch(samples, labels, indices, aug, seed)
        assert np.array_equal(np.ascontiguousarray(got[0], dtype=np.float32).view(np.uint32),
                              np.ascontiguousarray(want_x, dtype=np.float32).view(np.uint32))
        assert (got[1] == want_labels).all()
        assert any(fr.slot_is_augmented(seed, w, fr.augment_threshold(aug)) for w in range(slots))
    return run, check, data.close


def case_random(hip):
    """dbh_random.hip: 64 signals of 102 values, every kind among them, against the CPU model"""
    import random_signal_reference as rr
    seed, n, size = 3 + 102, 64, 102

    def run():
        return hip.random_signals(seed, 0, n, size)

    def check(got):
        want, kinds, nearest = rr.signals(seed, 0, n, size)
        assert nearest > rr.GUARD and rr.MULTI_GAUSSIAN in set(kinds.tolist())
        assert np.array_equal(got, want)
        assert np.array_equal(got, hip.random_signals(seed, 0, n, size, host=True))
    return run, check, None


def case_train(hip):
    """dbh_train.hip: loss and gradients at the smallest batch of tests/test_gpu_gradients.py, held
    to that test's rule"""
    import test_gpu_gradients as tg
    size, n, classes = tg.CASES[0]
    weights, x, labels = tg.case_inputs(size, n, classes)

    def run():
        return hip.loss_and_gradients(weights, x, labels, dropout_rate=0.15, seed=tg.SEED)

    def check(got):
        r64, r32 = tg.reference(size, n, classes, 0.15)
        tg.check_against_reference(got, r64, r32, classes, 'L{} N{} C{}'.format(size, n, classes))
    return run, check, None


def case_kernels(hip):
    """dbh_kernels.hip: the normalise kernel on the golden reads, against the golden windows"""
    signals = golden_all_signals()
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
    samples = np.concatenate(signals).astype(np.int16)
    n = len(signals)

    def run():
        with hip.device_arrays(samples, offsets, n * 12 * 1024 * 4) as (d_s, d_o, d_w):
            hip.check(hip.load_library().dbh_normalise_windows_dev(d_s.ptr, d_o.ptr, n, 1, 6144,
                                                                   d_w.ptr, None))
            hip.synchronize()
            return d_w.download((n, 12, 1024), np.float32)

    def check(got):
        want = np.load(os.path.join(GOLD, 'windows_end.npy')).transpose(1, 0, 2)
        assert np.abs(got - want).max() <= 2.4e-7 * max(1.0, float(np.abs(want).max()))
        assert np.array_equal(got == 0, want == 0)
    return run, check, None


UNITS = {'general': case_general, 'sweep': case_sweep, 'scan': case_scan, 'locate': case_locate,
         'inflate': case_inflate, 'zstd': case_zstd, 'vbz': case_vbz, 'text': case_text,
         'format': case_format, 'feed': case_feed, 'random': case_random, 'train': case_train,
         'kernels': case_kernels}


@pytest.mark.parametrize('unit', list(UNITS))
def test_unit_behind_every_fill(hip, unit):
    """One case per unit, at the smallest input its own GPU test uses."""
    run, check, close = UNITS[unit](hip)
    try:
        behind_every_fill(hip, run, check, 'dbh_{}.hip'.format(unit))
    finally:
        if close:
            close()
