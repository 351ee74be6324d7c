"""The scan on the GPU: the ragged front bit for bit against the NumPy restatement, the window
offsets of more reads than one workgroup takes per trip, the event pass against the restated rule on
random tracks, and the whole pass - front, network, fold, events - on the seven golden reads packed
end to end as ONE read (a synthetic junction at every seam), beside oracle/dbref; the command beside
``classify``."""
import ctypes
import os

import numpy as np
import pytest

import scan_reference as ref
from conftest import GOLD, PLAN

pytestmark = pytest.mark.gpu

STARTS, ENDS = 'EXP-NBD103_read_starts', 'EXP-NBD103_read_ends'
INVALID = 1


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def pack(signals):
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
    samples = np.concatenate([np.asarray(s, np.int16) for s in signals]) if signals else np.zeros(0, np.int16)
    return samples.astype(np.int16), offsets


# ---- the front -------------------------------------------------------------------------------------
def front_reads(input_size):
    """Every length at which the window count or the padding changes, a constant read, one that
    alternates between the ends of int16, a full-range random one, and an empty read between two
    others."""
    rng = np.random.default_rng(input_size)
    reads = [rng.integers(-3000, 3000, n).astype(np.int16) for n in ref.lengths_around(input_size)]
    long = 3 * input_size + 17
    reads.append(np.full(long, 1234, np.int16))
    reads.append(np.where(np.arange(long) % 2 == 0, -32768, 32767).astype(np.int16))
    reads.append(rng.integers(-32768, 32768, long).astype(np.int16))
    reads += [rng.integers(0, 900, input_size + 3).astype(np.int16), np.zeros(0, np.int16),
              rng.integers(0, 900, 2 * input_size).astype(np.int16)]
    return reads


@pytest.mark.parametrize('input_size', [96, 130, 1024])
@pytest.mark.parametrize('side', ['start', 'end'])
def test_front_bit_for_bit(hip, input_size, side):
    reads = front_reads(input_size)
    samples, offsets = pack(reads)
    want = ref.batch_windows(reads, input_size, side)
    window_offsets = ref.window_offsets([len(r) for r in reads], input_size)
    assert np.array_equal(hip.scan_window_offsets(offsets, input_size), window_offsets)
    got = hip.scan_windows(samples, offsets, input_size, side)
    assert got.shape == want.shape == (window_offsets[-1], input_size)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert not len(bad), (bad[:5], np.searchsorted(window_offsets, bad[:5], side='right') - 1)
    # a range of windows that begins and ends inside reads is that slice of the whole
    first, count = 5, int(window_offsets[-1]) - 9
    part = hip.scan_windows(samples, offsets, input_size, side, first, count)
    assert np.array_equal(bits(part), bits(want[first:first + count]))
    # windows behind the batch's last are zeros
    tail = hip.scan_windows(samples, offsets, input_size, side, int(window_offsets[-1]) - 1, 3)
    assert np.array_equal(bits(tail[0]), bits(want[-1])) and not tail[1:].any()


@pytest.mark.parametrize('side', ['start', 'end'])
def test_front_beside_the_classify_front_on_the_golden_reads(hip, all_signals, side):
    """The first 12 windows of every golden read (as many as it has): within 1 float32 ulp of
    dbh_normalise_windows_dev - exact integer sums here, float sums there - with zeros in the same
    places."""
    samples, offsets = pack(all_signals)
    n = len(all_signals)
    window_offsets = ref.window_offsets([len(s) for s in all_signals], 1024)
    got = hip.scan_windows(samples, offsets, 1024, side)
    held = [hip.DeviceBuffer.from_array(samples), hip.DeviceBuffer.from_array(offsets),
            hip.DeviceBuffer(n * 12 * 1024 * 4)]
    try:
        hip.check(hip.load_library().dbh_normalise_windows_dev(
            held[0].ptr, held[1].ptr, n, 0 if side == 'start' else 1, 6144, held[2].ptr, None))
        hip.synchronize()
        theirs = held[2].download((n, 12, 1024), np.float32)
    finally:
        for buf in held:
            buf.free()
    compared = 0
    for r in range(n):
        for k in range(min(12, int(window_offsets[r + 1] - window_offsets[r]))):
            mine, other = got[window_offsets[r] + k], theirs[r, k]
            assert np.abs(mine - other).max() <= 2.4e-7 * max(1.0, float(np.abs(other).max())), (r, k)
            assert np.array_equal(mine == 0, other == 0), (r, k)
            compared += 1
    assert compared > 10 * n


def test_window_offsets_of_70000_reads(hip):
    """More reads than the one workgroup takes per trip (1,024), of 1 to 3 windows - the empty read,
    which has one all-zero window, among them."""
    rng = np.random.default_rng(70000)
    for input_size in (96, 1024):
        half = input_size // 2
        lengths = rng.choice([0, 1, input_size, input_size + 1, input_size + half,
                              input_size + half + 1, input_size + 2 * half], 70000)
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        counts = hip.scan_window_count(input_size, lengths)
        assert counts.min() == 1 and counts.max() == 3
        want = np.concatenate([[0], np.cumsum(counts)])
        assert np.array_equal(hip.scan_window_offsets(offsets, input_size), want)
    assert hip.scan_window_offsets(np.zeros(1, np.int64), 96).tolist() == [0]


# ---- events ----------------------------------------------------------------------------------------
def check_events(hip, best, margin, offsets, threshold, min_windows, skip, max_events=None):
    want, total, interior = ref.events(best, margin, offsets, threshold, min_windows, skip, max_events)
    got, got_total, got_interior = hip.scan_events(best, margin, offsets, threshold, min_windows,
                                                   skip, max_events)
    assert got_total == total and np.array_equal(got_interior, interior)
    assert got.dtype == want.dtype and np.array_equal(got, want)        # the peak too: a maximum
    return total


@pytest.mark.parametrize('density', [0.02, 0.3, 0.9])
def test_events_against_the_restatement(hip, density):
    rng = np.random.default_rng(int(1000 * density))
    lengths = rng.integers(1, 201, 300)
    lengths[:4] = [1, 64, 65, 200]                         # one trip exactly, and one window more
    best, margin, offsets = ref.random_track(rng, lengths, density)
    for min_windows, skip in ((1, 0), (1, 12), (2, 3), (5, 70)):
        total = check_events(hip, best, margin, offsets, 0.5, min_windows, skip)
        assert total > 0 or (density < 0.1 and min_windows > 2)
    # another threshold: margins equal to it fire
    check_events(hip, best, margin, offsets, 0.75, 1, 2)
    total = check_events(hip, best, margin, offsets, 0.5, 1, 2)
    for capacity in (0, 1, total - 1, total, total + 5):
        check_events(hip, best, margin, offsets, 0.5, 1, 2, max_events=capacity)


def test_events_of_long_and_of_many_short_reads(hip):
    rng = np.random.default_rng(1500)
    # one read of 1,500 windows (24 trips), with one run longer than a trip and runs across seams
    best, margin, offsets = ref.random_track(rng, np.array([1500]), 0.3)
    best[100:250], margin[100:250] = 7, 0.625
    margin[200] = 1.0
    best[62:66], margin[62:66] = 3, 0.75
    best[1499], margin[1499] = 9, 0.5
    for min_windows, skip in ((1, 0), (2, 12), (100, 101), (150, 100), (151, 0)):
        check_events(hip, best, margin, offsets, 0.5, min_windows, skip)
    # 3,000 reads of one or two windows: runs never cross from one read into the next
    lengths = rng.integers(1, 3, 3000)
    best, margin, offsets = ref.random_track(rng, lengths, 0.9, n_classes=3)
    assert check_events(hip, best, margin, offsets, 0.5, 1, 1) > 1000
    check_events(hip, best, margin, offsets, 0.5, 2, 0, max_events=10)


# ---- the whole pass --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def packed_read(gold):
    """The seven golden reads end to end as ONE read of 188,245 samples."""
    samples, _ = pack(gold['signals'])
    assert len(gold['signals']) == 7 and len(samples) == 188245
    return samples, np.array([0, len(samples)], np.int64)


@pytest.fixture(scope='module')
def oracle_tracks(packed_read, weights):
    """(model, side) -> (the restatement's windows, oracle/dbref's probabilities on them, the
    restated track and events at threshold 0.5, skip_windows 2).  Computed once, on the host."""
    from oracle import dbref
    samples, offsets = packed_read
    made = {}
    for name, side in PLAN[:2]:
        x = ref.windows(samples, 1024, side)
        probs = dbref.CModel(weights[name]).predict(x)
        best, margin = ref.track(probs)
        made[name, side] = (x, probs, best, margin,
                            ref.events(best, margin, np.array([0, len(x)]), 0.5, 1, 2))
    return made


def check_whole_pass(hip, model, side, packed_read, oracle):
    samples, offsets = packed_read
    x_want, probs_want, best_want, margin_want, (events_want, total, interior) = oracle
    x = hip.scan_windows(samples, offsets, 1024, side)
    assert np.array_equal(bits(x), bits(x_want))
    probs = model.predict(x)
    assert np.abs(probs - probs_want).max() <= 1e-4
    events, best, margin, window_offsets = model.scan_packed(samples, offsets, side, 0.5, 1, 2,
                                                             track=True)
    assert window_offsets.tolist() == [0, len(x_want)]
    # the track is the sweep's fold at one step over these very probabilities
    fold_best, fold_margin = hip.sweep_windows(model, probs[:, None, :])
    assert np.array_equal(best, fold_best[:, 0]) and np.array_equal(margin, fold_margin[:, 0])
    # the events are the rule applied to the track, the peak included ...
    mine = ref.events(best, margin, window_offsets, 0.5, 1, 2)[0]
    assert np.array_equal(events, mine)
    # ... and - every oracle margin lying clear of the threshold - the oracle's own
    assert (np.abs(margin_want - 0.5) > 1e-3).all()
    for field in ('read', 'cls', 'first', 'last'):
        assert np.array_equal(events[field], events_want[field]), field
    assert total == len(events) and int((events['first'] >= 2).sum()) == int(interior[0])
    assert np.array_equal(model.scan_packed(samples, offsets, side, 0.5, 1, 2), events)
    return events, best, margin


def test_whole_pass_on_the_packed_golden_reads(hip, hip_models, packed_read, oracle_tracks):
    model = hip_models[STARTS]
    events, best, margin = check_whole_pass(hip, model, 'start', packed_read,
                                            oracle_tracks[STARTS, 'start'])
    # each golden read's own start call, where it begins: one or two windows each
    assert events['cls'].tolist() == [3, 2, 3, 1, 1, 2, 12]
    assert ((events['last'] - events['first']) <= 1).all() and (events['peak'] >= 0.99).all()
    assert events['first'][0] == 0 and (events['first'][1:] >= 2).all()
    outside = np.ones(len(best), bool)
    for e in events:
        outside[e['first']:e['last'] + 1] = False
    assert (best[outside] == 0).all()
    # small chunks (50 windows each: eight of them) give the same track bit for bit
    samples, offsets = packed_read
    model.set_host_group(50)
    try:
        again, best_again, margin_again, _ = model.scan_packed(samples, offsets, 'start', 0.5, 1, 2,
                                                               track=True)
    finally:
        model.set_host_group(0)
    assert np.array_equal(best_again, best) and np.array_equal(margin_again.view(np.uint64),
                                                              margin.view(np.uint64))
    assert np.array_equal(again, events)


def test_whole_pass_on_the_general_path(hip, weights, packed_read, oracle_tracks):
    model = hip.HipModel(weights[STARTS], device=0, general=True)
    try:
        assert model.kind == hip.KIND_GENERAL
        events, _, _ = check_whole_pass(hip, model, 'start', packed_read,
                                        oracle_tracks[STARTS, 'start'])
        assert events['cls'].tolist() == [3, 2, 3, 1, 1, 2, 12]
    finally:
        model.close()


def test_whole_pass_on_side_end(hip, hip_models, packed_read, oracle_tracks):
    events, _, _ = check_whole_pass(hip, hip_models[ENDS], 'end', packed_read,
                                    oracle_tracks[ENDS, 'end'])
    assert len(events) > 0 and events['first'][0] == 0


@pytest.mark.parametrize('name,side', PLAN[:2])
def test_golden_reads_alone_beside_the_golden_window_probabilities(hip, hip_models, all_signals,
                                                                   name, side):
    """Each golden read scanned as a read of its own: its first 12 windows (as many as it has) are
    call_batch's, and their probabilities the golden ones to the project's 1e-4."""
    samples, offsets = pack(all_signals)
    n = len(all_signals)
    golden = np.load(os.path.join(GOLD, 'window_probs_{}_{}.npy'.format(name, side))).reshape(12, n, -1)
    window_offsets = ref.window_offsets([len(s) for s in all_signals], 1024)
    probs = hip_models[name].predict(hip.scan_windows(samples, offsets, 1024, side))
    events, best, margin, got_offsets = hip_models[name].scan_packed(samples, offsets, side, 0.5,
                                                                     track=True)
    assert np.array_equal(got_offsets, window_offsets)
    want_best, want_margin = ref.track(probs)
    assert np.array_equal(best, want_best) and np.abs(margin - want_margin).max() <= 1e-12
    for r in range(n):
        k = min(12, int(window_offsets[r + 1] - window_offsets[r]))
        at = int(window_offsets[r])
        assert np.abs(probs[at:at + k] - golden[:k, r]).max() <= 1e-4, r


def test_no_read_and_a_read_of_one_sample(hip, hip_models):
    model = hip_models[STARTS]
    none = model.scan_packed(np.zeros(0, np.int16), np.zeros(1, np.int64), 'start', 0.5, track=True)
    assert len(none[0]) == 0 and len(none[1]) == 0 and none[3].tolist() == [0]
    for side in ('start', 'end'):
        x = hip.scan_windows(np.array([77], np.int16), np.array([0, 1]), 1024, side)
        assert x.shape == (1, 1024) and not x.any()           # x - mean = 0, then padding
        events, best, margin, window_offsets = model.scan_packed(
            np.array([77], np.int16), np.array([0, 1], np.int64), side, 0.5, track=True)
        assert window_offsets.tolist() == [0, 1] and best.shape == (1,)
        # (a window of zeros is what an empty read's window is, too)
        empty = model.scan_packed(np.zeros(0, np.int16), np.array([0, 0], np.int64), side, 0.5,
                                  track=True)
        assert empty[1].tolist() == best.tolist() and empty[2].tolist() == margin.tolist()


def test_host_entry_refuses_before_any_device_work(hip, hip_models):
    lib = hip.load_library()
    model = hip_models[STARTS]
    samples = np.zeros(3000, np.int16)
    offsets = np.array([0, 1000, 3000], np.int64)
    best, margin = np.full(6, 7, np.int32), np.full(6, 0.25)
    events = np.full(6, 9, hip.SCAN_EVENT)
    found, inside = ctypes.c_int64(-1), ctypes.c_int64(-1)
    p = lambda a: a.ctypes.data                                    # noqa: E731
    good = dict(samples=p(samples), offsets=p(offsets), n=2, side=0, threshold=0.5, min_windows=1,
                skip=0, events=p(events), capacity=6, found=ctypes.byref(found),
                inside=ctypes.byref(inside))

    def call(**changed):
        a = dict(good, **changed)
        return lib.dbh_scan_i16(model.handle, a['samples'], a['offsets'], a['n'], a['side'],
                                a['threshold'], a['min_windows'], a['skip'], p(best), p(margin),
                                a['events'], a['capacity'], a['found'], a['inside'])

    back = np.array([0, 1000, 500], np.int64)
    for bad in (dict(n=-1), dict(side=2), dict(side=-1), dict(min_windows=0), dict(skip=-1),
                dict(capacity=-1), dict(offsets=p(back)), dict(offsets=None), dict(samples=None),
                dict(events=None), dict(found=None), dict(inside=None),
                dict(threshold=float('nan'))):
        assert call(**bad) == INVALID, bad
    assert (best == 7).all() and (margin == 0.25).all() and (events['read'] == 9).all()
    assert found.value == -1 and inside.value == -1
    assert call(n=0) == 0 and found.value == 0 and inside.value == 0 and (best == 7).all()
    # reads of 1,000 and of 2,000 samples: one window and three
    assert call() == 0 and found.value >= 0
    assert not (best[:4] == 7).any() and (best[4:] == 7).all() and (margin[4:] == 0.25).all()


# ---- the command -----------------------------------------------------------------------------------
def test_command_beside_classify_and_the_restatement(hip, gold, hip_models, packed_read, tmp_path,
                                                     capsys):
    from deepbinner_amd import deepbinner as cli
    from deepbinner_amd import hdf5_write, scan
    reads = {'packed-read': packed_read[0], 'plain-0': gold['signals'][0], 'plain-5': gold['signals'][5]}
    for read_id, signal in reads.items():
        hdf5_write.write_single_read_fast5(str(tmp_path / (read_id + '.fast5')), read_id, signal)
    capsys.readouterr()
    cli.main(['classify', '--native', str(tmp_path)])
    calls = dict(line.split('\t')[:2] for line in capsys.readouterr().out.strip().split('\n')[1:])
    assert sorted(calls) == sorted(reads)
    cli.main(['scan', '--native', '--batch_size', '2', str(tmp_path)])
    out, err = capsys.readouterr()
    lines = [line.split('\t') for line in out.strip().split('\n')]
    assert lines[0] == ['read_ID', 'barcode_call', 'samples', 'interior_events', 'events']
    assert sorted(row[0] for row in lines[1:]) == sorted(reads)
    flagged = 0
    for read_id, call, n_samples, interior, column in lines[1:]:
        signal = reads[read_id]
        assert call == calls[read_id] and int(n_samples) == len(signal)
        want, inside = [], 0
        for side, name in (('start', STARTS), ('end', ENDS)):
            x = ref.windows(signal, 1024, side)
            best, margin = ref.track(hip_models[name].predict(x))
            events, _, per_read = ref.events(best, margin, np.array([0, len(x)]), 0.5, 1, 12)
            inside += int(per_read[0])
            want += [scan.event_text(side, e, len(signal), 1024) for e in events]
        assert column == (','.join(want) or '-') and int(interior) == inside, read_id
        flagged += inside > 0
    packed = [row for row in lines[1:] if row[0] == 'packed-read'][0]
    assert int(packed[3]) >= 5 and packed[4].startswith('start:3:0-')
    assert '3 reads, {} with at least one interior event'.format(flagged) in err
