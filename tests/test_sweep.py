"""The sweep without a GPU: the prefix property it rests on, checked against oracle/classify_ref.py
and not assumed; the restated tally against a plain loop; the ``sweep`` command - checks, row order,
header, refusals - against a host stand-in for its device entries; the new symbols and what the
entries refuse before any device work."""
import argparse
import ctypes
import os

import numpy as np
import pytest

import sweep_reference as ref
from conftest import GOLD, MODEL_DIR, PLAN
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import hip_backend, sweep
from oracle import classify_ref

SINGLE = os.path.join(GOLD, 'fast5', 'single')
STARTS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw')
ENDS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw')
NEW_SYMBOLS = ['dbh_sweep_windows_dev', 'dbh_sweep_workspace_bytes', 'dbh_sweep_i16_dev',
               'dbh_sweep_pair_i16', 'dbh_sweep_tally_dev', 'dbh_sweep_tally']
INVALID = 1


def replay(per_step):
    """A ``predict`` for classify_ref.call_batch that hands back recorded per-step probabilities:
    call_batch predicts step 0, 1, ... in turn, and window s does not depend on the scan size."""
    steps = iter(per_step)
    return lambda windows: next(steps)


def check_prefixes(per_step, signals, input_size, side, thresholds):
    """per_step [K, N, C] float32: row k of the restatement against classify_ref.call_batch run at
    scan_size = k * input_size / 2 - merged probabilities and the call at every threshold."""
    window_probs = np.ascontiguousarray(np.transpose(per_step, (1, 0, 2)))
    probs = ref.renormalise(ref.fold(window_probs))
    best, margin = ref.best_and_margin(probs)
    half = input_size // 2
    for k in range(1, per_step.shape[0] + 1):
        for t in thresholds:
            calls, want = classify_ref.call_batch(replay(per_step), signals, input_size, k * half, t, side)
            np.testing.assert_allclose(probs[:, k - 1], want, rtol=1e-14, atol=0)
            mine = ['none' if c == 0 else str(c) for c in ref.calls_at(best[:, k - 1], margin[:, k - 1], t)]
            assert mine == calls, (k, t)


@pytest.mark.parametrize('model,side', PLAN[:2])
def test_prefix_property_on_the_golden_reads(all_signals, model, side):
    flat = np.load(os.path.join(GOLD, 'window_probs_{}_{}.npy'.format(model, side)))
    per_step = flat.reshape(12, len(all_signals), -1).astype(np.float32)
    check_prefixes(per_step, all_signals, 1024, side, (0.5, 1.0, 0.05))


@pytest.mark.parametrize('n_classes,steps', [(2, 1), (2, 5), (13, 12), (33, 7), (256, 3)])
def test_prefix_property_on_hand_made_windows(n_classes, steps):
    window_probs = ref.hand_made(n_classes, steps, seed=n_classes + steps)
    per_step = np.ascontiguousarray(np.transpose(window_probs, (1, 0, 2)))
    rows_with_barcodes = [i for i in range(len(window_probs)) if i not in (3, 5)]
    # (classify_ref divides 0 by 0 where p0 == 1 and the barcodes are zero: those two rows apart)
    signals = [np.zeros(0, np.int16)] * len(rows_with_barcodes)
    check_prefixes(per_step[:, rows_with_barcodes], signals, 96, 'start', (0.1, 0.5, 1.0))
    best, margin = ref.sweep(window_probs)
    assert (best[3] == 0).all() and (margin[3] == 1.0).all()         # the guarded division
    assert best[0, 0] == 1                                           # the lower of the tied two
    assert n_classes == 2 or margin[0, 0] == 0.0
    assert (best[2] == 0).all()
    if n_classes > 2 and steps > 1:
        assert best[4, 0] == 1 and best[4, 1] == 2                   # the maximum moved on
    assert (best[5, :-1] == 0).all() and best[5, -1] == n_classes - 1


def plain_tally(start, end, thresholds, n_classes, labels):
    sides = [s for s in (start, end) if s is not None]
    n, steps = sides[0][0].shape
    modes = ref.MODES if len(sides) == 2 else ('-',)
    counts = np.zeros((steps, len(thresholds), len(modes), n_classes + 3), np.int64)
    for i in range(n):
        for k in range(steps):
            for t, threshold in enumerate(thresholds):
                calls = ['none' if b[i, k] == 0 or not m[i, k] >= threshold else str(b[i, k])
                         for b, m in sides]
                for j, mode in enumerate(modes):
                    final = calls[0] if len(sides) == 1 else classify_ref.combine_calls(
                        calls[0], calls[1], 'require_' + mode)
                    call = 0 if final == 'none' else int(final)
                    counts[k, t, j, call] += 1
                    if labels is not None and labels[i] >= 0:
                        slot = 0 if call == labels[i] else (1 if call != 0 else 2)
                        counts[k, t, j, n_classes + slot] += 1
    return counts


def tally_case(seed, n=60, steps=3, n_classes=5):
    rng = np.random.default_rng(seed)
    sides = []
    for _ in range(2):
        best = rng.integers(0, n_classes, (n, steps)).astype(np.int32)
        margin = rng.choice([0.05, 0.3, 0.5, 0.75, 1.0], (n, steps))
        sides.append((best, margin))
    sides[1][0][:10] = 0                              # reads only the start side calls
    sides[0][0][10:20] = 0                            # ... and only the end side
    labels = rng.integers(-1, n_classes, n).astype(np.int32)      # -1 and 0 among them
    return sides[0], sides[1], labels


@pytest.mark.parametrize('which', ['both', 'start', 'end'])
@pytest.mark.parametrize('labelled', [True, False])
def test_tally_of_the_restatement(which, labelled):
    start, end, labels = tally_case(7)
    assert (labels == -1).any() and (labels == 0).any()
    start, end = (start if which != 'end' else None), (end if which != 'start' else None)
    thresholds = [0.3, 0.5, 1.0]
    got = ref.tally(start, end, thresholds, 5, labels if labelled else None)
    want = plain_tally(start, end, thresholds, 5, labels if labelled else None)
    assert np.array_equal(got, want)
    assert (got[..., :5].sum(axis=-1) == 60).all()
    if labelled:
        assert (got[..., 5:].sum(axis=-1) == (labels >= 0).sum()).all()
    else:
        assert not got[..., 5:].any()


# ---- the command against a host stand-in -------------------------------------------------------
def options(**given):
    base = dict(input=SINGLE, native=False, rapid=False, start_model=STARTS, end_model=ENDS,
                max_scan_size=6144.0, score_diffs='0.5', labels=None, multi_read=False,
                batch_size=4, loader_procs=0, devices=0)
    base.update(given)
    return argparse.Namespace(**base)


def table(text):
    lines = text.strip('\n').split('\n')
    return lines[0].split('\t'), [line.split('\t') for line in lines[1:]]


@pytest.fixture(scope='module')
def classify_table():
    """barcode -> reads of the table ``classify --native`` prints for the seven golden files under
    the oracle backend (scan size 6144, score difference 0.5, require_either)."""
    import contextlib
    import io
    from conftest import OracleModel
    import deepbinner_amd.classify as classify
    saved, classify.build_model = classify.build_model, (lambda w: OracleModel(w))
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
            cli.main(['classify', '-s', STARTS, '-e', ENDS, SINGLE])
    finally:
        classify.build_model = saved
    rows = [line.split('\t') for line in out.getvalue().strip().split('\n')[1:]]
    assert len(rows) == 7
    return rows


def test_command_matches_classify_and_orders_its_rows(oracle_backend, classify_table, capsys, tmp_path):
    backend = ref.HostBackend()
    labels = tmp_path / 'labels.tsv'
    # read 0 unknown, read 1 said to carry a barcode classify did not call, the rest what classify
    # called ('0': known to carry none)
    said = ['none', '11' if classify_table[1][1] == '12' else '12'] + [
        '0' if call == 'none' else call for _, call in classify_table[2:]]
    labels.write_text('read_ID\tbarcode_call\n' + ''.join(
        '{}\t{}\n'.format(rid, label) for (rid, _), label in zip(classify_table, said)))
    capsys.readouterr()
    sweep.sweep(options(score_diffs='0.9,0.5,0.1', labels=str(labels)), backend=backend)
    header, rows = table(capsys.readouterr().out)
    assert header == (['scan_size', 'score_diff', 'mode', 'reads', 'classified', 'none', 'right',
                       'wrong', 'missed'] + [str(c) for c in range(1, 13)])
    assert [(int(r[0]), float(r[1]), r[2]) for r in rows] == [
        (512 * k, t, mode) for k in range(1, 13) for t in (0.1, 0.5, 0.9)
        for mode in ('either', 'start', 'both')]
    assert backend.batches == 2 and all(r[3] == '7' for r in rows)       # --batch_size 4
    (row,) = [r for r in rows if (r[0], float(r[1]), r[2]) == ('6144', 0.5, 'either')]
    per_barcode = [sum(1 for _, call in classify_table if call == str(c)) for c in range(1, 13)]
    assert [int(v) for v in row[9:]] == per_barcode
    assert int(row[5]) == sum(1 for _, call in classify_table if call == 'none')
    assert int(row[4]) == sum(per_barcode)
    known = classify_table[2:]
    first_is_called = classify_table[1][1] != 'none'
    assert int(row[6]) == len(known)
    assert int(row[7]) == (1 if first_is_called else 0) and int(row[8]) == (0 if first_is_called else 1)
    for r in rows:
        assert int(r[4]) + int(r[5]) == 7 and sum(int(v) for v in r[6:9]) == 6


def test_command_with_one_model_and_no_labels(oracle_backend, capsys):
    sweep.sweep(options(end_model=None, max_scan_size=1024.0, score_diffs='0.5,1'),
                backend=ref.HostBackend())
    header, rows = table(capsys.readouterr().out)
    assert header == ['scan_size', 'score_diff', 'mode', 'reads', 'classified', 'none'] + [
        str(c) for c in range(1, 13)]
    assert [(r[0], r[1], r[2]) for r in rows] == [('512', '0.5', '-'), ('512', '1.0', '-'),
                                                  ('1024', '0.5', '-'), ('1024', '1.0', '-')]


def test_command_on_training_data(oracle_backend, capsys):
    path = os.path.join(GOLD, 'training_data.txt')
    sweep.sweep(options(input=path, end_model=None, max_scan_size=1024.0), backend=ref.HostBackend())
    header, rows = table(capsys.readouterr().out)
    assert header[6:9] == ['right', 'wrong', 'missed']          # the file's own labels
    with open(path) as text:
        n = sum(1 for line in text if line.strip())
    assert all(int(r[3]) == n and sum(int(v) for v in r[6:9]) == n for r in rows)
    with pytest.raises(SystemExit) as e:
        sweep.sweep(options(input=path), backend=ref.HostBackend())
    assert 'training data can only be classified using a single model' in str(e.value)


@pytest.mark.parametrize('given,message', [
    (dict(max_scan_size=6000.0), '--scan_size must be a multiple of half the model input size'),
    (dict(max_scan_size=0.0), '--max_scan_size must be at least half the model input size'),
    (dict(score_diffs='0.5,0'), 'every --score_diffs value must be in the range (0, 1]'),
    (dict(score_diffs='0.5,1.5'), 'every --score_diffs value must be in the range (0, 1]'),
    (dict(score_diffs='0.5,x'), '--score_diffs must be a comma-delimited list of numbers'),
    (dict(score_diffs=','), '--score_diffs must name at least one threshold'),
    (dict(devices=2), 'a sweep runs on one GPU'),
    (dict(start_model=None, end_model=None), 'you must provide at least one model'),
])
def test_command_refusals(oracle_backend, given, message):
    with pytest.raises(SystemExit) as e:
        sweep.sweep(options(**given), backend=ref.HostBackend())
    assert message in str(e.value)


def test_two_input_sizes_are_refused(oracle_backend, tmp_path):
    import general_fixtures
    other = general_fixtures.save(general_fixtures.geometry(input_size=96, name=general_fixtures.ENDS),
                                  tmp_path / 'ends_96.dbw')
    with pytest.raises(SystemExit) as e:
        sweep.sweep(options(end_model=other), backend=ref.HostBackend())
    assert 'must have the same input size (they have 1024 and 96)' in str(e.value)


def test_command_line_entry(monkeypatch):
    seen = {}
    monkeypatch.setattr(sweep, 'sweep', lambda args: seen.update(vars(args)))
    cli.main(['sweep', '--native', 'some_dir'])
    assert seen['max_scan_size'] == 12288 and seen['score_diffs'] == '0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9'
    assert os.path.basename(seen['start_model']).startswith('EXP-NBD103_read_starts')
    assert os.path.basename(seen['end_model']).startswith('EXP-NBD103_read_ends')
    assert seen['batch_size'] == 256 and not seen['multi_read'] and seen['labels'] is None
    with pytest.raises(SystemExit) as e:
        cli.main(['sweep', 'some_dir'])
    assert 'you must provide at least one model' in str(e.value)
    for refused in ('prep', 'train'):
        with pytest.raises(SystemExit) as e:
            cli.main([refused])
        assert 'not part of this build' in str(e.value) and 'sweep' in str(e.value)


# ---- the C ABI without a device ----------------------------------------------------------------
def test_symbols_are_exported_and_listed():
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in hip_backend.EXPORTED_SYMBOLS, name
    header = open(os.path.join(os.path.dirname(GOLD), '..', 'include', 'deepbinner_hip.h')).read()
    for cite in ('classify.py:325-393', 'classify.py:285-295', 'classify.py:298-322'):
        assert cite in header


def test_bad_arguments_are_refused_before_any_device_work():
    lib = hip_backend.load_library()
    best = np.full((4, 3), 7, np.int32)
    margin = np.full((4, 3), 0.25, np.float64)
    thresholds = np.array([0.5])
    counts = np.full(3 * 1 * 1 * (5 + 3), -1, np.int64)
    p = lambda a: a.ctypes.data                                    # noqa: E731
    size = ctypes.c_size_t(99)
    # no model: every entry that takes one
    assert lib.dbh_sweep_windows_dev(None, 1, 4, 3, 1, 1, None) == INVALID
    assert lib.dbh_sweep_workspace_bytes(None, 4, 6144, ctypes.byref(size)) == INVALID
    assert size.value == 99
    assert lib.dbh_sweep_i16_dev(None, 1, 1, 4, 0, 6144, 1, 1, 1, None) == INVALID
    offsets = np.zeros(5, np.int64)
    assert lib.dbh_sweep_pair_i16(None, None, None, p(offsets), 4, 6144, p(best), p(margin),
                                  p(best), p(margin)) == INVALID
    # the tally: null pointers, half a side, no side, counts below 1, a class count out of range
    good = [p(best), p(margin), None, None, None, 4, 3, 5, p(thresholds), 1, p(counts)]

    def with_(**changed):
        names = ['sb', 'sm', 'eb', 'em', 'labels', 'n', 'steps', 'classes', 'thr', 'n_thr', 'counts']
        args = list(good)
        for name, value in changed.items():
            args[names.index(name)] = value
        return args

    for bad in (with_(sm=None), with_(sb=None), with_(sb=None, sm=None), with_(eb=p(best)),
                with_(n=-1), with_(steps=0), with_(steps=-3), with_(classes=1), with_(classes=257),
                with_(thr=None), with_(n_thr=0), with_(counts=None)):
        assert lib.dbh_sweep_tally(*bad) == INVALID, bad
        assert lib.dbh_sweep_tally_dev(*bad, None) == INVALID, bad
    assert (counts == -1).all() and (best == 7).all()
    assert lib.dbh_sweep_tally(*with_(n=0)) == 0 and (counts == -1).all()       # nothing to count
    with pytest.raises(ValueError):
        hip_backend.sweep_steps(1024, 6000)
    assert hip_backend.sweep_steps(1024, 12288) == 24 and hip_backend.sweep_steps(96, 48) == 1
