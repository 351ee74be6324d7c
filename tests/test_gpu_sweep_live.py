"""The early tally on the GPU: ``sweep_early_tally`` against the plain restatement
(tests/early_reference.py) on synthetic tracks whose margins sit on the thresholds, at the shapes
where the kernel takes another path - the workgroup's edge, one step and hundreds, the second tile
of the window and of the push histogram, 256 classes, sums past 2^32; against live sessions that
replay the same reads; the command beside its host stand-in; the refusals."""
import os

import numpy as np
import pytest

import early_reference as ref
import general_fixtures
import live_reference
from conftest import GOLD

pytestmark = pytest.mark.gpu

SINGLE = os.path.join(GOLD, 'fast5', 'single')
ENDS = 'EXP-NBD103_read_ends'
INVALID = 1


def same(got, want):
    for name, a, b in zip(('calls', 'early', 'windows', 'pushes'), got, want):
        assert (a is None) == (b is None), name
        if a is not None:
            assert a.dtype == np.int64 and a.shape == b.shape, name
            assert np.array_equal(a, b), (name, np.argwhere(a != b)[:5].tolist())


# ---- the tally alone ------------------------------------------------------------------------------
def thresholds_of(count):
    return [0.5] if count == 1 else [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]


def synthetic(seed, n, steps, n_classes, thresholds, input_size, labels):
    """Tracks with margins from {0, t - ulp, t, t + ulp, 1}, classes from both ends of the range;
    lengths at the seams, zero among them, and random up to 3 cap."""
    rng = np.random.default_rng(seed)
    values = [0.0, 1.0]
    for t in thresholds:
        values += [np.nextafter(t, 0.0), t, np.nextafter(t, 1.0)]
    classes = sorted({0, 0, 1, 2, n_classes - 1})
    sides = [(rng.choice(classes, (n, steps)).astype(np.int32), rng.choice(values, (n, steps)))
             for _ in range(2)]
    cap = (steps + 1) * (input_size // 2)
    lengths = (live_reference.seam_lengths(input_size, steps) +
               rng.integers(0, 3 * cap, n).tolist())[:n]
    known = {'none': None, 'unknown': np.full(n, -1, np.int32),
             'mixed': rng.integers(-1, min(n_classes, 4), n).astype(np.int32)}[labels]
    return sides[0], sides[1], known, np.array(lengths, dtype=np.int64)


def chunk_of(kind, input_size, steps):
    h = input_size // 2
    return {'1': 1, 'h+1': h + 1, '1600': 1600, 'cap': (steps + 1) * h, '2^62': 1 << 62}[kind]


# (reads, steps, classes, thresholds, chunk, input size, both sides, labels): every value of each
# dimension at least once; a chunk of 1 at steps <= 4 only, where P = cap stays below 4096 - with
# L = 1024 it is 2560 pushes, ten tiles of the push histogram; 300 steps of L = 96 in chunks of 49
# are 295 pushes and two tiles of each histogram
SHAPES = [
    (1, 1, 2, 1, '1', 96, False, 'none'),
    (255, 4, 13, 9, '1', 96, True, 'mixed'),
    (256, 4, 13, 1, '1', 1024, False, 'mixed'),
    (256, 12, 13, 9, 'h+1', 96, True, 'mixed'),
    (257, 63, 2, 1, '1600', 96, False, 'unknown'),
    (513, 64, 13, 1, 'cap', 96, True, 'none'),
    (257, 65, 256, 1, '2^62', 96, False, 'mixed'),
    (256, 256, 13, 1, 'h+1', 96, False, 'none'),
    (257, 300, 13, 1, 'h+1', 96, True, 'mixed'),
    (513, 12, 256, 9, '1600', 1024, True, 'mixed'),
    (1, 300, 2, 9, 'cap', 96, False, 'none'),
]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '-'.join(str(v) for v in s))
def test_tally_against_the_restatement(hip, shape):
    n, steps, n_classes, n_thresholds, chunk, input_size, both, labels = shape
    thresholds = thresholds_of(n_thresholds)
    start, end, known, lengths = synthetic(sum(shape[:4]), n, steps, n_classes, thresholds,
                                           input_size, labels)
    c = chunk_of(chunk, input_size, steps)
    want = ref.tally(start, end if both else None, thresholds, n_classes, known, lengths, input_size, c)
    got = hip.sweep_early_tally(start, end if both else None, thresholds, n_classes, known, lengths,
                                input_size, c)
    same(got, want)
    same(got, hip.sweep_early_host(start, end if both else None, thresholds, n_classes, known,
                                   lengths, input_size, c))
    assert (got[0][..., :n_classes].sum(axis=-1) <= n).all()
    if n > 1:
        assert got[1][0, 0, 0] > 0                           # some read was decided


@pytest.fixture(scope='module')
def middling():
    """257 reads of twelve steps, both sides, mixed labels, nine thresholds - and what the
    restatement counts on them, computed once."""
    thresholds = thresholds_of(9)
    start, end, labels, lengths = synthetic(77, 257, 12, 13, thresholds, 96, 'mixed')
    want = ref.tally(start, end, thresholds, 13, labels, lengths, 96, 49)
    return start, end, labels, lengths, thresholds, want


def test_order_and_split_change_nothing(hip, middling):
    start, end, labels, lengths, thresholds, want = middling
    order = np.random.default_rng(1).permutation(len(labels))
    take = lambda side, rows: (side[0][rows], side[1][rows])              # noqa: E731
    same(hip.sweep_early_tally(take(start, order), take(end, order), thresholds, 13, labels[order],
                               lengths[order], 96, 49), want)
    counts = None
    for rows in (slice(0, 1), slice(1, 1), slice(1, None)):              # 1 read, none, the rest
        counts = hip.sweep_early_tally(take(start, rows), take(end, rows), thresholds, 13,
                                       labels[rows], lengths[rows], 96, 49, counts=counts)
    same(counts, want)


def test_sides_labels_and_lengths_may_be_absent(hip, middling):
    start, end, labels, lengths, thresholds, want = middling
    for given_end, given_labels, given_lengths in ((None, labels, lengths), (end, None, lengths),
                                                   (end, labels, None), (None, None, None)):
        got = hip.sweep_early_tally(start, given_end, thresholds, 13, given_labels, given_lengths,
                                    96, 49)
        same(got, ref.tally(start, given_end, thresholds, 13, given_labels, given_lengths, 96, 49))
        if given_lengths is None:
            assert got[3] is None and not got[1][..., 6:].any()
        if given_labels is None:
            assert not got[0][..., 13:].any()
        if given_end is not None and given_labels is not None and given_lengths is not None:
            same(got, want)
        if given_end is None and given_lengths is not None:      # the start side's columns repeat
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])


def test_sums_are_64_bit_from_the_first_add(hip):
    """256 reads of 2^33 + 1 samples that all decide, in one workgroup: 2^41 + 256 samples."""
    n, long_read = 256, (1 << 33) + 1
    start = (np.full((n, 4), 3, np.int32), np.full((n, 4), 0.9))
    lengths = np.full(n, long_read, np.int64)
    for c, samples in ((1 << 62, n * long_read), (1600, n * 1600)):
        calls, early, windows, pushes = hip.sweep_early_tally(start, None, [0.5], 13, None, lengths,
                                                              1024, c)
        assert early[0, 0].tolist() == [n, n, 0, 0, 0, n, samples, n * long_read]
        assert pushes[0, 0, 0] == n and windows[3, 0, 3] == n and calls[0, 0, 0, 3] == n
    same(hip.sweep_early_tally(start, None, [0.5], 13, None, lengths, 1024, 1 << 62),
         ref.tally(start, None, [0.5], 13, None, lengths, 1024, 1 << 62))


def device_arrays_of(hip, arrays):
    return [None if a is None else hip.DeviceBuffer.from_array(np.ascontiguousarray(a)) for a in arrays]


def test_device_entry_and_refusals_leave_the_arrays_alone(hip, middling):
    """dbh_sweep_early_tally_dev on the caller's buffers and stream: it adds, takes a negative
    length as 0, and every refused call leaves the four arrays as they were."""
    start, end, labels, lengths, thresholds, _ = middling
    lengths = lengths.copy()
    lengths[::7] = -5
    want = ref.tally(start, end, thresholds, 13, labels, np.maximum(lengths, 0), 96, 49)
    n, steps = start[0].shape
    lib = hip.load_library()
    stream = hip.Stream()
    inputs = device_arrays_of(hip, [start[0], start[1], end[0], end[1], labels, lengths,
                                    np.array(thresholds)])
    outputs = device_arrays_of(hip, [np.full(w.shape, 5, np.int64) for w in want])
    ptr = lambda b: None if b is None else b.ptr                            # noqa: E731
    names = ['sb', 'sm', 'eb', 'em', 'labels', 'lengths', 'n', 'steps', 'classes', 'size', 'chunk',
             'thr', 'n_thr', 'calls', 'early', 'windows', 'pushes']
    good = [ptr(b) for b in inputs[:6]] + [n, steps, 13, 96, 49, inputs[6].ptr, len(thresholds)] + \
        [b.ptr for b in outputs]

    def with_(**changed):
        args = list(good)
        for name, value in changed.items():
            args[names.index(name)] = value
        return args

    try:
        for bad in (with_(sb=None), with_(sm=None), with_(eb=None), with_(em=None), with_(n=-1),
                    with_(steps=0), with_(classes=1), with_(classes=257), with_(size=97),
                    with_(size=0), with_(chunk=0), with_(size=9000, chunk=1), with_(thr=None),
                    with_(n_thr=0), with_(calls=None), with_(early=None), with_(windows=None),
                    with_(pushes=None), with_(lengths=None)):
            assert lib.dbh_sweep_early_tally_dev(*bad, stream.ptr) == INVALID, bad
        assert lib.dbh_sweep_early_tally_dev(*with_(n=0), stream.ptr) == 0
        stream.synchronize()
        for buf, w in zip(outputs, want):
            assert (buf.download(w.shape, np.int64) == 5).all()
        host = [np.full(w.shape, 5, np.int64) for w in want]
        with pytest.raises(hip.HipBackendError):                 # a negative length, host buffers
            hip.sweep_early_tally(start, end, thresholds, 13, labels, lengths, 96, 49, counts=host)
        assert all((a == 5).all() for a in host)
        for _ in range(2):                                       # adds: 5 + twice the counts
            hip.check(lib.dbh_sweep_early_tally_dev(*good, stream.ptr), 'dbh_sweep_early_tally_dev')
        stream.synchronize()
        same([buf.download(w.shape, np.int64) for buf, w in zip(outputs, want)],
             [5 + 2 * w for w in want])
    finally:
        for buf in inputs + outputs:
            buf.free()
        stream.close()


# ---- against a live session -----------------------------------------------------------------------
def replayed_reads(input_size, steps, seed, real, n=300):
    """300 reads at the seam lengths and random ones up to 3 cap; every third one has a golden
    read's start spliced in front, so that barcodes lead."""
    rng = np.random.default_rng(seed)
    cap = (steps + 1) * (input_size // 2)
    lengths = live_reference.seam_lengths(input_size, steps)
    lengths += rng.integers(0, 3 * cap, n - len(lengths)).tolist()
    reads = []
    for i, length in enumerate(lengths):
        part = rng.integers(200, 900, int(length)).astype(np.int16)
        if i % 3 == 0:
            signal = real[i % len(real)]
            front = min(int(length), len(signal))
            part[:front] = signal[:front]
        reads.append(part)
    return reads


def replay_through(session, reads, chunk, pair):
    """Every read on a channel of its own, delivered as the replay command delivers it: round r
    brings each open read to min(r c, len) samples, the push with r c >= len carries END.  -> per
    read its last start record, its last end record (or None) and the push that decided it (0: none)."""
    n = len(reads)
    last, ends, decided_at = [None] * n, [None] * n, [0] * n
    rounds = max(max(1, -(-len(read) // chunk)) for read in reads)
    for r in range(1, rounds + 1):
        channels = [ch for ch, read in enumerate(reads) if r <= max(1, -(-len(read) // chunk))]
        chunks = [reads[ch][(r - 1) * chunk:r * chunk] for ch in channels]
        final = [r * chunk >= len(reads[ch]) for ch in channels]
        if pair:
            records, end_records = session.push_pair(channels, chunks, begin=r == 1, end=final)
        else:
            records, end_records = session.push(channels, chunks, begin=r == 1, end=final), None
        for i, ch in enumerate(channels):
            last[ch] = records[i].copy()
            if pair:
                ends[ch] = end_records[i].copy()
            if decided_at[ch] == 0 and int(records[i]['decided_windows']) > 0:
                decided_at[ch] = r
    return last, ends, decided_at


def counted(records, finals, decided_at, m, steps, n_pushes, lengths):
    """early [8], windows [steps], pushes [P] from the session's own records."""
    early = np.zeros(8, np.int64)
    windows, pushes = np.zeros(steps, np.int64), np.zeros(n_pushes, np.int64)
    for record, final, push, length in zip(records, finals, decided_at, lengths):
        d = int(record['decided_windows'])
        if d == 0:
            continue
        call, final_call = int(record['call']), int(final['final_call'])
        early += [1, call == final_call, final_call not in (0, call), final_call == 0, d > m, d,
                  int(record['decided_samples']), length]
        windows[d - 1] += 1
        pushes[push - 1] += 1
    return early, windows, pushes


@pytest.fixture(scope='module')
def sessions(hip, all_signals):
    """name -> (start model, end model, scan size, reads, the sweep's tracks of both sides)."""
    made = {}
    for name, (size, n_classes, steps) in {'persistent': (1024, 13, 4), 'general': (96, 33, 12)}.items():
        start = hip.HipModel(general_fixtures.geometry(size, n_classes), device=0)
        end = hip.HipModel(general_fixtures.geometry(size, n_classes, name=ENDS, seed=5), device=0)
        scan_size = steps * (size // 2)
        reads = replayed_reads(size, steps, 21 + n_classes, all_signals)
        offsets = np.zeros(len(reads) + 1, np.int64)
        np.cumsum([len(read) for read in reads], out=offsets[1:])
        tracks = hip.sweep_pair(start, end, np.concatenate(reads), offsets, scan_size)
        made[name] = (start, end, scan_size, reads, tracks)
    assert made['persistent'][0].kind == hip.KIND_PERSISTENT
    assert made['general'][0].kind == hip.KIND_GENERAL
    yield made
    for start, end, _, _, _ in made.values():
        start.close()
        end.close()


@pytest.mark.parametrize('chunk', ['h+1', '1600'])
@pytest.mark.parametrize('name', ['persistent', 'general'])
def test_tally_says_what_live_sessions_decide(hip, sessions, name, chunk):
    start, end, scan_size, reads, (start_track, end_track) = sessions[name]
    size, n_classes = start.input_size, start.n_classes
    steps = scan_size // (size // 2)
    c = chunk_of(chunk, size, steps)
    n = len(reads)
    lengths = np.array([len(read) for read in reads], dtype=np.int64)
    labels = np.random.default_rng(3).integers(-1, n_classes, n).astype(np.int32)
    thresholds = [0.1, 0.5, 0.9]
    calls, early, windows, pushes = hip.sweep_early_tally(start_track, end_track, thresholds,
                                                          n_classes, labels, lengths, size, c)
    n_pushes = hip.sweep_early_pushes(size, scan_size, c)
    assert pushes.shape == (steps, 3, n_pushes)
    some_decided = 0
    for m, t in ((1, 0.5), (2, 0.5), (steps, 0.1), (1, 0.9)):
        options = dict(scan_size=scan_size, score_diff=t, min_windows=m)
        with hip.LiveSession(start, n, **options) as whole:          # never stopped: the final call
            finals, _, _ = replay_through(whole, reads, c, pair=False)
        assert all(int(f['status']) == hip.LIVE_FINAL for f in finals)
        cell = (m - 1, thresholds.index(t))
        for mode, rule in enumerate(('either', 'start', 'both')):
            with hip.LiveSession(start, n, stop_on_decision=True, end_model=end, combine=rule,
                                 **options) as session:
                records, ends, decided_at = replay_through(session, reads, c, pair=True)
            if mode == 0:
                got = counted(records, finals, decided_at, m, steps, n_pushes, lengths.tolist())
                where = (name, chunk, m, t)
                assert got[0].tolist() == early[cell].tolist(), where
                assert got[1].tolist() == windows[cell].tolist(), where
                assert got[2].tolist() == pushes[cell].tolist(), where
                some_decided += int(got[0][0])
                for record, final in zip(records, finals):       # stopping changes no decision
                    assert all(record[f] == final[f] for f in ('call', 'decided_windows',
                                                               'decided_samples'))
            want = np.zeros(n_classes + 3, np.int64)
            for record, label in zip(ends, labels.tolist()):
                assert int(record['status']) == hip.LIVE_FINAL
                call = int(record['read_call'])
                want[call] += 1
                if label >= 0:
                    want[n_classes + (0 if call == label else (1 if call != 0 else 2))] += 1
            assert want.tolist() == calls[cell][mode].tolist(), (name, chunk, m, t, rule)
    assert some_decided > 0


# ---- the command ----------------------------------------------------------------------------------
def test_command_beside_its_host_stand_in(hip, capsys, monkeypatch):
    import test_sweep_live
    from conftest import MODEL_DIR, OracleModel
    from deepbinner_amd import classify, sweep
    from deepbinner_amd import deepbinner as cli
    capsys.readouterr()
    cli.main(['sweep', '--live', '--native', '--max_scan_size', '6144', '--batch_size', '3', SINGLE])
    on_device = capsys.readouterr().out
    with monkeypatch.context() as patch:
        patch.setattr(classify, 'build_model', lambda w: OracleModel(w))
        sweep.sweep(test_sweep_live.options(end_model=os.path.join(MODEL_DIR, ENDS + '.dbw'),
                                            score_diffs='0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9',
                                            chunk_samples=None),
                    backend=ref.HostBackend())
    on_host = capsys.readouterr().out
    assert on_device == on_host
    lines = on_device.strip('\n').split('\n')
    assert len(lines) == 1 + 12 * 9 * 3 and lines[0].startswith('min_windows\tscore_diff\tmode\treads')
