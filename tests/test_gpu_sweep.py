"""The sweep on the GPU: both forms of the fold against the NumPy restatement on hand-made window
probabilities; the whole entry against ``classify_pair`` at every scan size, device against device
and exact, down to the equality edge of ``>=``; the tally kernel against the restated tally; the
command beside ``classify``'s table."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import general_fixtures
import sweep_reference as ref
from conftest import GOLD

pytestmark = pytest.mark.gpu

SINGLE = os.path.join(GOLD, 'fast5', 'single')
STARTS, ENDS = 'EXP-NBD103_read_starts', 'EXP-NBD103_read_ends'
K = 12
INVALID = 1


# ---- the fold alone -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fold_models(hip):
    """class count -> model: persistent ones (32 lanes per read) and general ones of the smallest
    input size (one workgroup per read)."""
    made = {('persistent', c): hip.HipModel(general_fixtures.geometry(1024, c), device=0)
            for c in (2, 13, 32)}
    made.update({('general', c): hip.HipModel(general_fixtures.geometry(96, c), device=0)
                 for c in (2, 33, 256)})
    assert all(m.kind == (hip.KIND_PERSISTENT if kind == 'persistent' else hip.KIND_GENERAL)
               for (kind, _), m in made.items())
    yield made
    for model in made.values():
        model.close()


@pytest.mark.parametrize('kind,n_classes', [('persistent', 2), ('persistent', 13), ('persistent', 32),
                                            ('general', 2), ('general', 33), ('general', 256)])
def test_fold_against_the_restatement(hip, fold_models, kind, n_classes):
    model = fold_models[kind, n_classes]
    for n_reads in (1, 7, 8, 9, 300):          # eight reads share a workgroup in the 32-lane form
        for steps in (1, 2, 12, 31):
            window_probs = ref.hand_made(n_classes, steps, seed=n_reads * 100 + steps, n_reads=max(n_reads, 7))
            window_probs = window_probs[-n_reads:] if n_reads < 7 else window_probs
            best, margin = hip.sweep_windows(model, window_probs)
            want_best, want_margin = ref.sweep(window_probs)
            where = (kind, n_classes, n_reads, steps)
            assert np.array_equal(best, want_best), where
            # 256 fp64 additions of values <= 1, a division and a product: far inside 1e-12
            assert np.abs(margin - want_margin).max() <= 1e-12, where
    # the rows a fold can get wrong are among them, and come out as the contract says
    best, margin = hip.sweep_windows(model, ref.hand_made(n_classes, 12, seed=1))
    assert (best[3] == 0).all() and (margin[3] == 1.0).all()            # p0 == 1: the guarded division
    assert best[0, 0] == 1 and (n_classes == 2 or margin[0, 0] == 0.0)  # two barcodes tie
    assert (best[5, :-1] == 0).all() and best[5, -1] == n_classes - 1   # a barcode that comes late
    if n_classes > 2:
        assert best[4, 0] == 1 and best[4, 1] == 2                      # the maximum moves on


# ---- end to end, device against device ------------------------------------------------------------
def random_reads(input_size, steps, seed, real, n=300):
    """300 random int16 signals, the lengths that sit on a seam among them; every third one has a
    real read's start in front and its end behind (``real``: the golden reads), so that the models
    call barcodes on some and the thresholds have something to decide."""
    half = input_size // 2
    rng = np.random.default_rng(seed)
    lengths = [0, 1, half - 1, input_size, steps * half - 1, steps * half + input_size]
    lengths += rng.integers(0, steps * half + 2 * input_size, n - len(lengths)).tolist()
    parts = []
    for i, length in enumerate(lengths):
        part = rng.integers(200, 900, length).astype(np.int16)
        if i >= 6 and i % 3 == 0:
            signal = real[i % len(real)]
            ends = min(length // 2, len(signal))
            part[:ends] = signal[:ends]
            part[length - ends:] = signal[len(signal) - ends:]
        parts.append(part)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lengths, out=offsets[1:])
    return np.concatenate(parts), offsets


def edge_calls(hip, model, side, d_samples, d_offsets, n, scan_size, thresholds):
    """Read r classified alone at its own threshold: n one-read calls queued on the null stream."""
    c = model.n_classes
    d_probs, d_calls = hip.DeviceBuffer(n * c * 4), hip.DeviceBuffer(n * 4)
    d_work = hip.DeviceBuffer(max(model.workspace_bytes(1, scan_size), 256))
    try:
        for r in range(n):
            model.classify_dev(d_samples.ptr, d_offsets.ptr + 8 * r, 1, side, scan_size,
                               float(thresholds[r]), d_probs.ptr + 4 * c * r, d_calls.ptr + 4 * r,
                               d_work.ptr)
        hip.synchronize()
        return d_calls.download((n,), np.int32)
    finally:
        for buf in (d_probs, d_calls, d_work):
            buf.free()


def check_end_to_end(hip, start_model, end_model, input_size, seed, real, some_called=False):
    half = input_size // 2
    samples, offsets = random_reads(input_size, K, seed, real)
    n = len(offsets) - 1
    swept = hip.sweep_pair(start_model, end_model, samples, offsets, K * half)
    sides = [(name, model, got) for name, model, got in
             (('start', start_model, swept[0]), ('end', end_model, swept[1])) if model is not None]
    for name, model, (best, margin) in sides:
        assert best.shape == margin.shape == (n, K) and best.dtype == np.int32
        assert (best >= 0).all() and (best < model.n_classes).all() and np.isfinite(margin).all()
    if some_called:         # (the shipped models on real read ends: the thresholds decide something)
        assert all((best != 0).any() for _, _, (best, _) in sides)
    # every scan size at two fixed thresholds: the per-side calls of classify_pair
    for k in range(1, K + 1):
        for t in (0.5, 1.0):
            _, side_calls, _ = hip.classify_pair(start_model, end_model, samples, offsets, k * half,
                                                 t, want_sides=True)
            for (name, _, (best, margin)), calls in zip(sides, [c for c in side_calls if c is not None]):
                assert np.array_equal(calls, ref.calls_at(best[:, k - 1], margin[:, k - 1], t)), (name, k, t)
    # the equality edge of >=: every read at its own margin and at the next double above it
    d_samples = hip.DeviceBuffer.from_array(samples if samples.size else np.zeros(1, np.int16))
    d_offsets = hip.DeviceBuffer.from_array(offsets)
    try:
        for name, model, (best, margin) in sides:
            for k in range(1, K + 1):
                at = margin[:, k - 1]
                above = np.nextafter(at, np.inf)
                got_at = edge_calls(hip, model, name, d_samples, d_offsets, n, k * half, at)
                got_above = edge_calls(hip, model, name, d_samples, d_offsets, n, k * half, above)
                assert np.array_equal(got_at, best[:, k - 1]), (name, k)
                assert not got_above.any(), (name, k)
    finally:
        d_samples.free()
        d_offsets.free()
    # a batch split in two calls, and one read alone
    cut = offsets[150]
    first = hip.sweep_pair(start_model, end_model, samples[:cut], offsets[:151], K * half)
    second = hip.sweep_pair(start_model, end_model, samples[cut:], offsets[150:] - cut, K * half)
    r = 5
    alone = hip.sweep_pair(start_model, end_model, samples[offsets[r]:offsets[r + 1]],
                           offsets[r:r + 2] - offsets[r], K * half)
    for j, (name, model) in enumerate((('start', start_model), ('end', end_model))):
        if model is None:
            assert swept[j] == (None, None)
            continue
        for part in (0, 1):
            assert np.array_equal(np.concatenate([first[j][part], second[j][part]]), swept[j][part]), name
            assert np.array_equal(alone[j][part][0], swept[j][part][r]), name
    return samples, offsets, swept


@pytest.fixture(scope='module')
def native_sweep(hip, hip_models, all_signals):
    """The two shipped --native models over 300 random reads, checked end to end once; the tally
    tests count these arrays."""
    return check_end_to_end(hip, hip_models[STARTS], hip_models[ENDS], 1024, 11, all_signals,
                            some_called=True)


def test_native_pair_end_to_end(hip, hip_models, native_sweep):
    samples, offsets, swept = native_sweep
    # the same through several groups and the slots that come round again (50 reads per group)
    start, end = hip_models[STARTS], hip_models[ENDS]
    start.set_host_group(50 * K)
    try:
        again = hip.sweep_pair(start, end, samples, offsets, K * 512)
    finally:
        start.set_host_group(0)
    for j in (0, 1):
        for part in (0, 1):
            assert np.array_equal(again[j][part], swept[j][part])
    # one scan step: the persistent path's per-window output, not the fused one-launch call
    (best, margin), _ = hip.sweep_pair(start, None, samples, offsets, 512)
    assert np.array_equal(best[:, 0], swept[0][0][:, 0]) and np.array_equal(margin[:, 0], swept[0][1][:, 0])
    one = start.sweep_packed(samples, offsets, 'start', 512)
    assert np.array_equal(one[0], best) and np.array_equal(one[1], margin)


def test_general_model_end_to_end(hip, all_signals):
    model = hip.HipModel(general_fixtures.geometry(96, 33, name=ENDS), device=0)
    try:
        assert model.kind == hip.KIND_GENERAL
        check_end_to_end(hip, None, model, 96, 12, all_signals)
    finally:
        model.close()


# ---- the host-buffer pipeline the sweep shares with classify --------------------------------------
def same_sweep(got, want):
    return all((got[j][part] is None and want[j][part] is None) or
               np.array_equal(got[j][part], want[j][part]) for j in (0, 1) for part in (0, 1))


@contextlib.contextmanager
def pinned_copy(hip, samples):
    """``samples`` in a dbh_malloc_host buffer, which the DMA engine reads in place."""
    lib = hip.load_library()
    ptr = ctypes.c_void_p()
    hip.check(lib.dbh_malloc_host(ctypes.byref(ptr), samples.nbytes))
    try:
        pinned = np.ctypeslib.as_array(ctypes.cast(ptr.value, ctypes.POINTER(ctypes.c_int16)),
                                       shape=samples.shape)
        pinned[:] = samples
        assert hip.is_pinned(pinned) and not hip.is_pinned(samples)
        yield pinned
    finally:
        hip.check(lib.dbh_free_host(ptr))


@pytest.fixture(scope='module')
def ragged_sweep(hip, hip_models, native_sweep):
    """The fixture's 300 reads with a zero-length read and a 5-sample read appended, and their sweep
    in one group; the 300 come out as they did without the two."""
    samples, offsets, swept = native_sweep
    samples = np.concatenate([samples, np.arange(5, dtype=np.int16)])
    offsets = np.concatenate([offsets, offsets[-1:], offsets[-1:] + 5])
    whole = hip.sweep_pair(hip_models[STARTS], hip_models[ENDS], samples, offsets, K * 512)
    assert same_sweep([[a[:300] for a in side] for side in whole], swept)
    return samples, offsets, whole


def test_pinned_input_is_the_pageable_run(hip, hip_models, native_sweep):
    samples, offsets, swept = native_sweep
    with pinned_copy(hip, samples) as pinned:
        got = hip.sweep_pair(hip_models[STARTS], hip_models[ENDS], pinned, offsets, K * 512)
    assert same_sweep(got, swept)


@pytest.mark.parametrize('memory', ['pinned', 'pageable'])
@pytest.mark.parametrize('reads_per_group', [1, 7])
def test_group_shapes(hip, hip_models, ragged_sweep, reads_per_group, memory):
    """One read per group, and seven: 302 reads then make 44 groups, the last one short, and every
    slot comes round many times."""
    samples, offsets, whole = ragged_sweep
    start, end = hip_models[STARTS], hip_models[ENDS]
    with pinned_copy(hip, samples) if memory == 'pinned' else contextlib.nullcontext(samples) as held:
        start.set_host_group(reads_per_group * K)
        try:
            got = hip.sweep_pair(start, end, held, offsets, K * 512)
        finally:
            start.set_host_group(0)
    assert same_sweep(got, whole)


def test_one_slot_ring_two_tenants(hip, hip_models, ragged_sweep):
    """classify, sweep, classify, the start model's sweep alone, seven reads per group on the same two
    models: the slots' buffers hold layouts of different sizes in turn, and every call gives what it
    gives on its own in one group."""
    samples, offsets, whole = ragged_sweep
    start, end = hip_models[STARTS], hip_models[ENDS]

    def classify():
        return hip.classify_pair(start, end, samples, offsets, K * 512, 0.5, want_sides=True,
                                 want_probs=True)

    def same_classify(got, want):
        return np.array_equal(got[0], want[0]) and all(
            np.array_equal(got[i][j], want[i][j]) for i in (1, 2) for j in (0, 1))

    classified = classify()
    start_alone = hip.sweep_pair(start, None, samples, offsets, K * 512)
    assert same_sweep(start_alone, (whole[0], (None, None)))
    start.set_host_group(7 * K)
    end.set_host_group(7 * K)
    try:
        assert same_classify(classify(), classified)
        assert same_sweep(hip.sweep_pair(start, end, samples, offsets, K * 512), whole)
        assert same_classify(classify(), classified)
        assert same_sweep(hip.sweep_pair(start, None, samples, offsets, K * 512), start_alone)
    finally:
        start.set_host_group(0)
        end.set_host_group(0)


def test_general_model_through_groups(hip, all_signals):
    """A general model takes its group from the default 32,768 windows whatever set_host_group says:
    3,000 reads at K = 12 scan steps (2,730 reads per group) go in two groups, the second one short,
    and come out as their two halves do in a call - and so a group - of their own."""
    model = hip.HipModel(general_fixtures.geometry(96, 33, name=ENDS), device=0)
    try:
        samples, offsets = random_reads(96, K, 13, all_signals, n=3000)
        assert 32768 // K < 3000 and 1500 <= 32768 // K
        whole = hip.sweep_pair(None, model, samples, offsets, K * 48)
        cut = offsets[1500]
        first = hip.sweep_pair(None, model, samples[:cut], offsets[:1501], K * 48)
        second = hip.sweep_pair(None, model, samples[cut:], offsets[1500:] - cut, K * 48)
        assert whole[0] == (None, None) and whole[1][0].shape == whole[1][1].shape == (3000, K)
        for part in (0, 1):
            assert np.array_equal(whole[1][part], np.concatenate([first[1][part], second[1][part]]))
    finally:
        model.close()


# ---- the tally ------------------------------------------------------------------------------------
THRESHOLDS = [0.1, 0.5, 0.9, 1.0]


def labels_for(best, seed, n_classes):
    rng = np.random.default_rng(seed)
    labels = np.where(rng.random(len(best)) < 0.5, best[:, -1], rng.integers(-1, n_classes, len(best)))
    labels[:4] = [-1, 0, 0, n_classes - 1]
    return labels.astype(np.int32)


@pytest.mark.parametrize('which', ['both', 'start', 'end'])
@pytest.mark.parametrize('labelled', [True, False])
def test_tally_on_the_device(hip, native_sweep, which, labelled):
    _, _, (start, end) = native_sweep
    start, end = (start if which != 'end' else None), (end if which != 'start' else None)
    labels = labels_for((start or end)[0], 3, 13) if labelled else None
    got = hip.sweep_tally(start, end, THRESHOLDS, 13, labels)
    want = ref.tally(start, end, THRESHOLDS, 13, labels)
    assert got.shape == (K, len(THRESHOLDS), 3 if which == 'both' else 1, 16)
    assert np.array_equal(got, want)
    # accumulated over three calls = one call over all reads
    counts = None
    for a, b in ((0, 1), (1, 257), (257, 300)):
        part = lambda side: None if side is None else (side[0][a:b], side[1][a:b])      # noqa: E731
        counts = hip.sweep_tally(part(start), part(end), THRESHOLDS, 13,
                                 None if labels is None else labels[a:b], counts)
    assert np.array_equal(counts, want)


def test_tally_of_256_classes_and_the_device_entry(hip):
    """More classes than a workgroup has threads, a last chunk that is not full, and
    dbh_sweep_tally_dev on the caller's buffers and stream."""
    rng = np.random.default_rng(5)
    n, steps, c = 1000, 3, 256
    sides = [(rng.integers(0, c, (n, steps)).astype(np.int32), rng.choice([0.2, 0.5, 0.7], (n, steps)))
             for _ in range(2)]
    sides[1][0][::2] = sides[0][0][::2]                 # (half the reads agree)
    labels = rng.integers(-1, c, n).astype(np.int32)
    want = ref.tally(sides[0], sides[1], [0.5, 0.7], c, labels)
    assert np.array_equal(hip.sweep_tally(sides[0], sides[1], [0.5, 0.7], c, labels), want)
    stream = hip.Stream()
    bufs = [hip.DeviceBuffer.from_array(a) for a in
            (sides[0][0], sides[0][1], sides[1][0], sides[1][1], labels, np.array([0.5, 0.7]),
             np.zeros(want.size, np.int64))]
    try:
        for _ in range(2):                              # adds: twice the counts
            hip.check(hip.load_library().dbh_sweep_tally_dev(
                *[b.ptr for b in bufs[:5]], n, steps, c, bufs[5].ptr, 2, bufs[6].ptr, stream.ptr),
                'dbh_sweep_tally_dev')
        stream.synchronize()
        assert np.array_equal(bufs[6].download(want.shape, np.int64), 2 * want)
    finally:
        for b in bufs:
            b.free()
        stream.close()


# ---- arguments that need a model to be refused ----------------------------------------------------
def test_entries_refuse_before_any_device_work(hip, hip_models):
    lib = hip.load_library()
    start, ends = hip_models[STARTS], hip_models[ENDS]
    small = hip.HipModel(general_fixtures.geometry(96, 13), device=0)          # another input size
    wide = hip.HipModel(general_fixtures.geometry(1024, 14), device=0)         # another class count
    samples, offsets = np.zeros(2000, np.int16), np.array([0, 1000, 2000], np.int64)
    best = np.full((2, K), 7, np.int32)
    margin = np.full((2, K), 0.25)
    p = lambda a: a.ctypes.data                                               # noqa: E731
    try:
        pair = lambda s, e, scan, **kw: lib.dbh_sweep_pair_i16(                 # noqa: E731
            s.handle if s else None, e.handle if e else None, kw.get('samples', p(samples)),
            kw.get('offsets', p(offsets)), kw.get('n', 2), scan, kw.get('best', p(best)), p(margin),
            p(best), p(margin))
        assert pair(start, small, 6144) == INVALID and pair(start, wide, 6144) == INVALID
        assert pair(start, ends, 6000) == INVALID and pair(start, ends, 0) == INVALID     # steps < 1
        assert pair(start, ends, 6144, n=-1) == INVALID
        assert pair(start, ends, 6144, offsets=None) == INVALID
        assert pair(start, ends, 6144, samples=None) == INVALID
        assert pair(start, None, 6144, best=None) == INVALID
        back = np.array([0, 1000, 500], np.int64)
        assert pair(start, ends, 6144, offsets=p(back)) == INVALID
        size = ctypes.c_size_t(99)
        assert lib.dbh_sweep_workspace_bytes(start.handle, 2, 6000, ctypes.byref(size)) == INVALID
        assert lib.dbh_sweep_workspace_bytes(start.handle, -1, 6144, ctypes.byref(size)) == INVALID
        assert size.value == 99
        assert lib.dbh_sweep_windows_dev(start.handle, None, 2, 3, None, None, None) == INVALID
        assert lib.dbh_sweep_windows_dev(start.handle, 1, 2, 0, 1, 1, None) == INVALID
        assert lib.dbh_sweep_windows_dev(start.handle, 1, -1, 3, 1, 1, None) == INVALID
        assert lib.dbh_sweep_i16_dev(start.handle, None, None, 2, 0, 6144, None, None, None, None) == INVALID
        assert lib.dbh_sweep_i16_dev(start.handle, 1, 1, 2, 2, 6144, 1, 1, 1, None) == INVALID    # side
        assert lib.dbh_sweep_i16_dev(start.handle, 1, 1, 2, 0, 100, 1, 1, 1, None) == INVALID
        assert (best == 7).all() and (margin == 0.25).all()
        assert pair(start, ends, 6144, n=0) == 0 and (best == 7).all()
        with pytest.raises(ValueError):
            hip.sweep_pair(start, small, samples, offsets, 6144)
    finally:
        small.close()
        wide.close()


# ---- the command ----------------------------------------------------------------------------------
def test_command_beside_classify(hip, capsys):
    from deepbinner_amd import deepbinner as cli
    capsys.readouterr()
    cli.main(['classify', '--native', SINGLE])
    calls = [line.split('\t')[1] for line in capsys.readouterr().out.strip().split('\n')[1:]]
    assert len(calls) == 7
    cli.main(['sweep', '--native', '--batch_size', '3', SINGLE])
    first = capsys.readouterr().out
    cli.main(['sweep', '--native', '--batch_size', '3', SINGLE])
    assert capsys.readouterr().out == first                                  # the same bytes
    lines = [line.split('\t') for line in first.strip().split('\n')]
    assert lines[0][:6] == ['scan_size', 'score_diff', 'mode', 'reads', 'classified', 'none']
    assert len(lines) == 1 + 24 * 9 * 3
    (row,) = [r for r in lines[1:] if (r[0], r[1], r[2]) == ('6144', '0.5', 'either')]
    assert [int(v) for v in row[6:]] == [calls.count(str(c)) for c in range(1, 13)]
    assert int(row[3]) == 7 and int(row[5]) == calls.count('none')
