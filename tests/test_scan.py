"""The scan without a GPU: the window count and bounds of the restatement against
oracle/classify_ref.py's windows, the event rule on hand-made tracks, the ``scan`` command - rows,
events column, summary, flags, refusals - against a host stand-in for its device entries; the new
symbols and what the entries refuse before any device work."""
import argparse
import ctypes
import os

import numpy as np
import pytest

import scan_reference as ref
from conftest import GOLD, MODEL_DIR, REPO
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import hip_backend, scan
from oracle import classify_ref

SINGLE = os.path.join(GOLD, 'fast5', 'single')
STARTS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw')
ENDS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw')
NEW_SYMBOLS = ['dbh_scan_window_count', 'dbh_scan_window_offsets_dev', 'dbh_scan_windows_dev',
               'dbh_scan_events_dev', 'dbh_scan_i16']
INVALID = 1


# ---- windows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('input_size', [96, 130, 1024])
@pytest.mark.parametrize('side', ['start', 'end'])
def test_window_count_and_bounds_against_classify_ref(input_size, side):
    rng = np.random.default_rng(input_size)
    half = input_size // 2
    for n in ref.lengths_around(input_size):
        signal = rng.integers(-500, 500, n).astype(np.int16)
        count = ref.window_count(n, input_size)
        assert count == hip_backend.scan_window_count(input_size, n)
        assert count == hip_backend.scan_window_count(input_size, np.array([n]))[0]
        # the last window reaches the read's other end and holds more than h samples (or all)
        a, b = ref.window_bounds(n, count - 1, input_size, side)
        assert (b == n if side == 'start' else a == 0) and (b - a > half or b - a == n)
        if count > 1:              # ... and the one before it does not reach it
            a, b = ref.window_bounds(n, count - 2, input_size, side)
            assert b < n if side == 'start' else a > 0
        # every window is call_batch's window of that step (classify.py:337-357)
        want = classify_ref.make_windows([signal], input_size, count * half, side)
        assert want.shape[0] == count
        got = ref.windows(signal, input_size, side)
        assert got.shape == (count, input_size)
        for k in range(count):
            a, b = ref.window_bounds(n, k, input_size, side)
            assert (a, b) == classify_ref.window_bounds(n, k, input_size, side)
            np.testing.assert_allclose(got[k], want[k, 0], rtol=1e-6, atol=1e-6)
            padding = got[k, b - a:] if side == 'start' else got[k, :input_size - (b - a)]
            assert not padding.any()


def test_window_offsets_of_the_restatement():
    assert ref.window_offsets([0, 1024, 1025, 1537, 5000], 1024).tolist() == [0, 1, 2, 4, 7, 16]
    with pytest.raises(ValueError):
        hip_backend.scan_window_count(97, 10)
    with pytest.raises(ValueError):
        hip_backend.scan_window_count(94, 10)


# ---- the event rule --------------------------------------------------------------------------------
def one_read(best, margin):
    return (np.array(best, np.int32), np.array(margin, np.float64), np.array([0, len(best)]))


def rows(events):
    return [(int(e['read']), int(e['cls']), int(e['first']), int(e['last']), float(e['peak']))
            for e in events]


def test_event_rule_on_hand_made_tracks():
    # a run across the skip boundary is not interior, one starting exactly at it is
    best, margin, offsets = one_read([0, 3, 3, 3, 0, 0, 5, 5, 0], [.9, .6, .8, .7, .9, .9, .5, .6, .9])
    events, total, interior = ref.events(best, margin, offsets, 0.5, 1, skip_windows=2)
    assert rows(events) == [(0, 3, 1, 3, 0.8), (0, 5, 6, 7, 0.6)] and total == 2
    assert interior.tolist() == [1]
    assert ref.events(best, margin, offsets, 0.5, 1, skip_windows=1)[2].tolist() == [2]
    assert ref.events(best, margin, offsets, 0.5, 1, skip_windows=6)[2].tolist() == [1]
    assert ref.events(best, margin, offsets, 0.5, 1, skip_windows=7)[2].tolist() == [0]
    # two classes back to back are two events; min_windows 2 drops the singles
    best, margin, offsets = one_read([2, 2, 7, 0, 4, 0, 9, 9], [.9, .8, .7, 1., .6, 1., .5, .5])
    assert rows(ref.events(best, margin, offsets, 0.5)[0]) == [
        (0, 2, 0, 1, 0.9), (0, 7, 2, 2, 0.7), (0, 4, 4, 4, 0.6), (0, 9, 6, 7, 0.5)]
    assert rows(ref.events(best, margin, offsets, 0.5, min_windows=2)[0]) == [
        (0, 2, 0, 1, 0.9), (0, 9, 6, 7, 0.5)]
    # a margin equal to the threshold fires, one below splits a run; class 0 never fires
    best, margin, offsets = one_read([4, 4, 4, 0, 0], [.5, .4999, .5, 1., 1.])
    assert rows(ref.events(best, margin, offsets, 0.5)[0]) == [(0, 4, 0, 0, 0.5), (0, 4, 2, 2, 0.5)]
    # W = 1, and runs never cross from one read into the next
    best = np.array([6, 6, 6, 0], np.int32)
    margin = np.array([.9, .8, .7, 1.])
    events, total, interior = ref.events(best, margin, np.array([0, 1, 3, 4]), 0.5, 1, 0)
    assert rows(events) == [(0, 6, 0, 0, 0.9), (1, 6, 0, 1, 0.8)] and interior.tolist() == [1, 1, 0]
    # capacity: the first max_events, the true total
    events, total, _ = ref.events(best, margin, np.array([0, 1, 3, 4]), 0.5, 1, 0, max_events=1)
    assert rows(events) == [(0, 6, 0, 0, 0.9)] and total == 2


@pytest.mark.parametrize('density', [0.02, 0.3, 0.9])
def test_event_rule_against_run_lengths(density):
    """The loop against another way to say it: split each read's firing classes where they change."""
    rng = np.random.default_rng(int(density * 100))
    lengths = rng.integers(1, 200, 40)
    best, margin, offsets = ref.random_track(rng, lengths, density)
    at_least = 1 if density < 0.1 else 2
    events, total, interior = ref.events(best, margin, offsets, 0.5, at_least, 3)
    want = []
    for r in range(len(lengths)):
        cls = np.where((best != 0) & (margin >= 0.5), best, 0)[offsets[r]:offsets[r + 1]]
        cuts = np.flatnonzero(np.diff(cls)) + 1
        for piece, first in zip(np.split(cls, cuts), np.concatenate([[0], cuts])):
            if piece[0] != 0 and len(piece) >= at_least:
                peak = margin[offsets[r] + first:offsets[r] + first + len(piece)].max()
                want.append((r, int(piece[0]), int(first), int(first + len(piece) - 1), float(peak)))
    assert rows(events) == want and total == len(want) and len(want) > 0
    assert interior.sum() == sum(1 for e in want if e[2] >= 3)


# ---- the command against a host stand-in -----------------------------------------------------------
def options(**given):
    base = dict(input=SINGLE, native=False, rapid=False, start_model=STARTS, end_model=ENDS,
                scan_size=6144.0, score_diff=0.5, require_either=True, require_start=False,
                require_both=False, min_windows=1, multi_read=False, batch_size=4, loader_procs=0,
                devices=0)
    base.update(given)
    return argparse.Namespace(**base)


def table(text):
    lines = text.strip('\n').split('\n')
    return lines[0].split('\t'), [line.split('\t') for line in lines[1:]]


@pytest.fixture()
def one_file(tmp_path, gold):
    """The two shortest golden reads packed end to end as ONE read, in a one-read file written by
    the project's own writer: a synthetic junction (the stand-in's network is NumPy: keep it small)."""
    from deepbinner_amd import hdf5_write
    a, b = sorted(range(len(gold['signals'])), key=lambda i: len(gold['signals'][i]))[:2]
    signal = np.concatenate([gold['signals'][a], gold['signals'][b]]).astype(np.int16)
    hdf5_write.write_single_read_fast5(str(tmp_path / 'packed.fast5'), 'packed-read', signal)
    return str(tmp_path), 'packed-read', signal


def test_command_rows_events_and_summary(oracle_backend, one_file, capsys):
    directory, read_id, signal = one_file
    backend = ref.HostBackend()
    capsys.readouterr()
    scan.scan(options(input=directory, scan_size=1024.0), backend=backend)
    out, err = capsys.readouterr()
    header, lines = table(out)
    assert header == ['read_ID', 'barcode_call', 'samples', 'interior_events', 'events']
    assert len(lines) == 1 and backend.batches == 1
    row = lines[0]
    assert row[0] == read_id and row[2] == str(len(signal))
    # barcode_call is classify's for the same read
    from conftest import OracleModel
    from deepbinner_amd.model_format import ModelWeights
    models = [OracleModel(ModelWeights.load(p)[0]) for p in (STARTS, ENDS)]
    calls = backend.classify_pair(models[0], models[1], signal, np.array([0, len(signal)]), 1024, 0.5)
    assert row[1] == ('none' if calls[0] == 0 else str(calls[0]))
    # the events column: the restatement's events of both sides at absolute sample positions
    want, interior = [], 0
    for side, model in zip(('start', 'end'), models):
        x = ref.windows(signal, 1024, side)
        best, margin = ref.track(model.predict(x[:, :, None]))
        events, _, inside = ref.events(best, margin, np.array([0, len(x)]), 0.5, 1, 2)
        interior += int(inside[0])
        for e in events:
            a, _ = ref.window_bounds(len(signal), int(e['first']), 1024, side)
            _, b = ref.window_bounds(len(signal), int(e['last']), 1024, side)
            if side == 'end':
                a, _ = ref.window_bounds(len(signal), int(e['last']), 1024, side)
                _, b = ref.window_bounds(len(signal), int(e['first']), 1024, side)
            want.append('{}:{}:{}-{}:{:.3f}'.format(side, e['cls'], a, b, e['peak']))
    assert want[0].startswith('start:') and want[0].split(':')[2].startswith('0-')
    assert interior >= 1                       # the second read's own barcode, now inside
    assert row[4] == ','.join(want) and row[3] == str(interior)
    assert '1 reads, 1 with at least one interior event' in err and 'interior events' in err


def test_command_with_one_model_and_min_windows(oracle_backend, one_file, capsys):
    directory, _, signal = one_file
    capsys.readouterr()
    scan.scan(options(input=directory, end_model=None, min_windows=3), backend=ref.HostBackend())
    _, lines = table(capsys.readouterr().out)
    assert all(not e.startswith('end:') for e in lines[0][4].split(','))
    capsys.readouterr()
    scan.scan(options(input=directory, end_model=None, min_windows=1000), backend=ref.HostBackend())
    _, lines = table(capsys.readouterr().out)
    assert lines[0][3] == '0' and lines[0][4] == '-'


def test_event_samples():
    assert scan.event_samples('start', 0, 1, 5000, 1024) == (0, 1536)
    assert scan.event_samples('start', 7, 8, 5000, 1024) == (3584, 5000)
    assert scan.event_samples('end', 0, 1, 5000, 1024) == (5000 - 1536, 5000)
    assert scan.event_samples('end', 7, 8, 5000, 1024) == (0, 5000 - 3584)
    for side in ('start', 'end'):
        for first, last in ((0, 0), (2, 5), (8, 8)):
            a = ref.window_bounds(5000, first, 1024, side)
            b = ref.window_bounds(5000, last, 1024, side)
            assert scan.event_samples(side, first, last, 5000, 1024) == (min(a[0], b[0]), max(a[1], b[1]))


@pytest.mark.parametrize('given,message', [
    (dict(start_model=None, end_model=None), 'you must provide at least one model'),
    (dict(devices=2), 'a scan runs on one GPU'),
    (dict(input=os.path.join(GOLD, 'training_data.txt')), 'have no interior'),
    (dict(min_windows=0), '--min_windows must be at least 1'),
    (dict(batch_size=0), '--batch_size must be at least 1'),
    (dict(scan_size=6000.0), '--scan_size must be a multiple of half the model input size'),
])
def test_command_refusals(oracle_backend, given, message):
    with pytest.raises(SystemExit) as e:
        scan.scan(options(**given), backend=ref.HostBackend())
    assert message in str(e.value)
    if 'input' in given:                          # the training-data file: one line
        assert '\n' not in str(e.value)


def test_command_line_entry(monkeypatch):
    seen = {}
    monkeypatch.setattr(scan, 'scan', lambda args: seen.update(vars(args)))
    cli.main(['scan', '--native', 'some_dir'])
    assert seen['scan_size'] == 6144 and seen['score_diff'] == 0.5 and seen['min_windows'] == 1
    assert os.path.basename(seen['start_model']).startswith('EXP-NBD103_read_starts')
    assert os.path.basename(seen['end_model']).startswith('EXP-NBD103_read_ends')
    assert seen['batch_size'] == 256 and not seen['multi_read'] and seen['require_either']
    assert seen['loader_procs'] == 0 and seen['devices'] == 0
    cli.main(['scan', '-s', STARTS, '--min_windows', '2', '--multi_read', 'some_dir'])
    assert seen['min_windows'] == 2 and seen['multi_read'] and seen['end_model'] is None
    with pytest.raises(SystemExit) as e:
        cli.main(['scan', 'some_dir'])
    assert 'you must provide at least one model' in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(['scan', '-s', STARTS, '--require_both', 'some_dir'])
    assert 'can only be used with two models' in str(e.value)
    for refused in ('prep', 'train'):
        with pytest.raises(SystemExit) as e:
            cli.main([refused])
        assert 'not part of this build' in str(e.value) and 'sweep' in str(e.value)
        assert 'scan' in str(e.value)


# ---- the C ABI without a device --------------------------------------------------------------------
def test_symbols_are_exported_and_listed():
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in hip_backend.EXPORTED_SYMBOLS, name
    header = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    for cite in ('classify.py:337-357', 'classify.py:285-295'):
        assert cite in header[header.index('---- scan:'):header.index('---- compressed input')]
    assert hip_backend.SCAN_EVENT == ref.EVENT


def test_bad_arguments_are_refused_before_any_device_work():
    lib = hip_backend.load_library()
    count = ctypes.c_int64(-7)
    for size, n in ((97, 10), (94, 10), (16386, 10), (1024, -1)):
        assert lib.dbh_scan_window_count(size, n, ctypes.byref(count)) == INVALID
    assert lib.dbh_scan_window_count(1024, 10, None) == INVALID and count.value == -7
    assert lib.dbh_scan_window_count(96, 97, ctypes.byref(count)) == 0 and count.value == 2
    assert lib.dbh_scan_window_count(16384, 0, ctypes.byref(count)) == 0 and count.value == 1
    # the device entries: 1 stands for a device pointer nobody may touch
    assert lib.dbh_scan_window_offsets_dev(1, -1, 1024, 1, None) == INVALID
    assert lib.dbh_scan_window_offsets_dev(1, 4, 1023, 1, None) == INVALID
    assert lib.dbh_scan_window_offsets_dev(None, 4, 1024, 1, None) == INVALID
    assert lib.dbh_scan_window_offsets_dev(1, 4, 1024, None, None) == INVALID
    good = [1, 1, 1, 4, 1024, 0, 0, 8, 1, None]
    for at, bad in ((3, -1), (4, 1022 + 1), (4, 64), (5, 2), (5, -1), (6, -1), (7, -1), (1, None),
                    (2, None), (8, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_scan_windows_dev(*args) == INVALID, (at, bad)
    assert lib.dbh_scan_windows_dev(*(good[:3] + [0] + good[4:])) == 0          # no read
    good = [1, 1, 1, 4, 0.5, 1, 0, 1, 8, 1, 1, None]
    for at, bad in ((0, None), (1, None), (2, None), (3, -1), (4, float('nan')), (5, 0), (6, -1),
                    (7, None), (8, -1), (10, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_scan_events_dev(*args) == INVALID, (at, bad)
    # the host entry: no model, and buffers untouched
    samples = np.zeros(3000, np.int16)
    offsets = np.array([0, 1000, 3000], np.int64)
    best = np.full(4, 7, np.int32)
    margin = np.full(4, 0.25)
    events = np.full(4, 9, hip_backend.SCAN_EVENT)
    found, inside = ctypes.c_int64(-1), ctypes.c_int64(-1)
    p = lambda a: a.ctypes.data                                    # noqa: E731
    assert lib.dbh_scan_i16(None, p(samples), p(offsets), 2, 0, 0.5, 1, 0, p(best), p(margin),
                            p(events), 4, ctypes.byref(found), ctypes.byref(inside)) == INVALID
    assert (best == 7).all() and (margin == 0.25).all() and (events['read'] == 9).all()
    assert found.value == -1 and inside.value == -1
