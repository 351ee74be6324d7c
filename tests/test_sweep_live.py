"""The early tally without a GPU: its closed form (tests/early_reference.py) held to the live
contract (tests/live_reference.py: ``plan``) over seam lengths, chunkings, every min_windows and
thresholds the margins sit on; ``sweep_early_host`` - the lines the kernel compiles - against the
closed form, all four arrays; the rules in plain numbers; ``sweep --live`` against a host stand-in
beside ``replay``'s summary of the same reads; the refusals; ``sweep`` without the flag as before."""
import argparse
import contextlib
import io
import os

import numpy as np
import pytest

import early_reference as ref
import live_reference
import sweep_reference
from conftest import GOLD, MODEL_DIR, REPO
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import hip_backend, replay, sweep

SINGLE = os.path.join(GOLD, 'fast5', 'single')
STARTS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw')
ENDS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw')
NEW_SYMBOLS = ['dbh_sweep_early_pushes', 'dbh_sweep_early_tally_dev', 'dbh_sweep_early_tally',
               'dbh_sweep_early_host']
INVALID = 1
THRESHOLDS = (0.2, 0.5, 0.7)


def same(got, want):
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b)


# ---- the closed form against the live contract ----------------------------------------------------
@pytest.mark.parametrize('input_size,steps', [(1024, 4), (96, 12), (96, 1)])
def test_restatement_against_the_live_plan(input_size, steps):
    """A read delivered as ``replay`` delivers it - push r brings it to min(r c, len) samples, the
    push with r c >= len carries END - through ``live_reference.plan``: the last record's call,
    decided_windows, decided_samples and final_call, and the push at which the decision appeared."""
    rng = np.random.default_rng(input_size + steps)
    h = input_size // 2
    scan_size, cap = steps * h, steps * h + h
    lengths = live_reference.seam_lengths(input_size, steps) + \
        rng.integers(0, 3 * scan_size + 1, 30).tolist()
    checked = 0
    for length in lengths:
        for c in (1, h - 1, h, h + 1, 3 * h, 1600, cap, 5 * scan_size):
            parts = [min(c, length - a) for a in range(0, max(length, 1), c)]
            flags = [0] * len(parts)
            flags[0] |= live_reference.BEGIN
            flags[-1] |= live_reference.END
            best = rng.integers(0, 4, steps).astype(np.int32)
            margin = rng.choice([0.1, 0.2, 0.5, 0.7, 0.9], steps)      # margins on the thresholds
            for m in range(1, steps + 1):
                for t in THRESHOLDS:
                    records, _ = live_reference.plan(input_size, scan_size, parts, flags, best, margin,
                                                     score_diff=t, min_windows=m)
                    last = records[-1]
                    assert last['status'] == live_reference.FINAL
                    decided = np.flatnonzero(records['decided_windows'] > 0)
                    want = dict(call=int(last['call']), decided_windows=int(last['decided_windows']),
                                decided_samples=int(last['decided_samples']),
                                push=int(decided[0]) + 1 if len(decided) else 0,
                                final_call=int(last['final_call']))
                    got = ref.outcome(best, margin, m, t, length, input_size, c)
                    assert got == want, (length, c, m, t, best, margin)
                    checked += 1
    assert checked == len(lengths) * 8 * steps * 3


# ---- the host entry against the closed form -------------------------------------------------------
def tracks(rng, n, steps, n_classes, thresholds):
    """Tracks whose margins sit on, one unit in the last place beside, and far from the thresholds."""
    values = [0.0, 1.0]
    for t in thresholds:
        values += [np.nextafter(t, 0.0), t, np.nextafter(t, 1.0)]
    best = rng.integers(0, min(n_classes, 6), (n, steps)).astype(np.int32)
    return best, rng.choice(values, (n, steps))


@pytest.mark.parametrize('input_size,steps,n_classes,chunk', [
    (1024, 4, 13, 1600), (96, 12, 33, 49), (96, 1, 2, 1), (96, 12, 5, 1 << 62), (1024, 4, 13, 2560),
    (96, 70, 256, 1600)])
@pytest.mark.parametrize('both', [False, True])
def test_host_entry_against_the_restatement(input_size, steps, n_classes, chunk, both):
    rng = np.random.default_rng(steps * n_classes)
    n = 40
    thresholds = [0.2, 0.5, 0.7]
    start = tracks(rng, n, steps, n_classes, thresholds)
    end = tracks(rng, n, steps, n_classes, thresholds) if both else None
    labels = rng.integers(-1, min(n_classes, 6), n).astype(np.int32)
    lengths = np.array((live_reference.seam_lengths(input_size, steps) +
                        rng.integers(0, 3 * steps * input_size, n).tolist())[:n], dtype=np.int64)
    for given_labels, given_lengths in ((labels, lengths), (None, lengths), (labels, None)):
        want = ref.tally(start, end, thresholds, n_classes, given_labels, given_lengths, input_size,
                         chunk)
        got = hip_backend.sweep_early_host(start, end, thresholds, n_classes, given_labels,
                                           given_lengths, input_size, chunk)
        same(got, want)
        if given_lengths is None:
            assert got[3] is None and not got[1][..., 6:].any()
        again = hip_backend.sweep_early_host(start, end, thresholds, n_classes, given_labels,
                                             given_lengths, input_size, chunk, counts=got)
        assert again is got or all(a is b for a, b in zip(again, got))
        same(got, [None if w is None else 2 * w for w in want])            # the entry ADDS
    calls, early = want[0], want[1]
    assert (calls[..., :n_classes].sum(axis=-1) == n).all()
    assert (early[..., 0] == early[..., 1] + early[..., 2] + early[..., 3]).all()


def test_rules_in_plain_numbers():
    """96-sample windows every 48: four steps, cap 240."""
    t = 0.5
    below = np.nextafter(t, 0.0)

    def host(best, margin, lengths=None, chunk=48, n_classes=13, labels=None, end=None, thresholds=(t,)):
        best = np.atleast_2d(np.asarray(best, np.int32))
        margin = np.atleast_2d(np.asarray(margin, np.float64))
        got = hip_backend.sweep_early_host((best, margin), end, list(thresholds), n_classes, labels,
                                           lengths, 96, chunk)
        same(got, ref.tally((best, margin), end, list(thresholds), n_classes, labels, lengths, 96,
                            chunk))
        return got

    # a margin equal to the threshold decides; one unit in the last place below does not; a NaN
    # leads nowhere
    _, early, windows, _ = host([3, 3, 3, 3], [t, 0, 0, 0])
    assert early[0, 0].tolist() == [1, 0, 0, 1, 0, 1, 0, 0] and windows[0, 0].tolist() == [1, 0, 0, 0]
    assert not early[1:].any()                               # from window 2 on: never decided
    _, early, _, _ = host([3, 3, 3, 3], [below, below, np.nan, below])
    assert not early.any()
    # best = n_classes and -1 lead like any barcode and count in no class; a label of -1 counts
    # nowhere
    calls, early, _, _ = host([[13, 13, 13, 13], [-1, -1, -1, -1], [2, 2, 2, 2]], [[0.9] * 4] * 3,
                              labels=np.array([13, 0, -1], np.int32))
    assert (early[:, 0, 0] == 3).all() and (early[:, 0, 1] == 3).all()
    assert (calls[:, 0, 0, :13].sum(axis=-1) == 1).all() and (calls[:, 0, 0, 2] == 1).all()
    assert calls[0, 0, 0, 13:].tolist() == [1, 1, 0]         # 13 == 13: right; -1 on label 0: wrong
    # decides class 3 at window 1 and ends on class 5: changed; ends on class 0: lost
    _, early, windows, pushes = host([[3, 3, 5, 5], [3, 0, 0, 0]], [[0.9] * 4] * 2,
                                     lengths=np.array([1000, 40], np.int64))
    assert early[0, 0].tolist() == [2, 0, 1, 1, 0, 2, 96 + 40, 1040]
    assert early[1, 0].tolist() == [1, 0, 1, 0, 0, 2, 144, 1000]      # m = 2: the second read never
    assert early[2, 0].tolist() == [1, 1, 0, 0, 0, 3, 192, 1000]      # m = 3: class 5, agrees
    assert pushes[0, 0].tolist() == [1, 1, 0, 0, 0]          # 40 samples: END in push 1; 96: push 2
    # m = steps: only the last window counts, and it is the final call
    assert early[3, 0].tolist() == [1, 1, 0, 0, 0, 4, 240, 1000] and windows[3, 0].tolist() == [0, 0, 0, 1]
    # late: the first lead behind m - 1
    _, early, _, _ = host([0, 0, 7, 7], [0.9] * 4)
    assert early[:, 0, 4].tolist() == [1, 1, 0, 0] and early[:, 0, 5].tolist() == [3, 3, 3, 4]
    # steps = 1; len = 0: one push, which carries END, and no sample
    best, margin = np.array([[4]], np.int32), np.array([[0.5]])
    got = hip_backend.sweep_early_host((best, margin), None, [0.5], 13, None,
                                       np.array([0], np.int64), 96, 1600)
    assert got[1][0, 0].tolist() == [1, 1, 0, 0, 0, 1, 0, 0] and got[3][0, 0].tolist() == [1]
    # len = 2^33 + 1 with c = 2^62: one push, all of the read; with c = 1 the window's own push
    long_read = np.array([(1 << 33) + 1] * 3, np.int64)
    _, early, _, pushes = host([[3] * 4] * 3, [[0.9] * 4] * 3, lengths=long_read, chunk=1 << 62)
    assert early[0, 0, 6] == 3 * ((1 << 33) + 1) == early[0, 0, 7] and pushes.shape == (4, 1, 1)
    _, early, _, pushes = host([[3] * 4] * 3, [[0.9] * 4] * 3, lengths=long_read, chunk=1)
    assert early[:, 0, 6].tolist() == [3 * 96, 3 * 144, 3 * 192, 3 * 240] and pushes[3, 0, 239] == 3
    # both sides: the pair session's read call under either, start, both
    end = (np.array([[0, 0, 0, 5]], np.int32), np.array([[0, 0, 0, 0.9]]))
    calls, _, _, _ = host([3, 3, 3, 3], [0.9] * 4, end=end)
    assert [int(np.argmax(calls[0, 0, j, :13])) for j in range(3)] == [0, 0, 0]
    calls, _, _, _ = host([0, 0, 0, 0], [0.9] * 4, end=end)
    assert [int(np.argmax(calls[0, 0, j, :13])) for j in range(3)] == [5, 0, 0]


def test_symbols_and_refusals_before_any_work():
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in hip_backend.EXPORTED_SYMBOLS, name
    assert hip_backend.sweep_early_pushes(1024, 6144, 1600) == 5
    assert hip_backend.sweep_early_pushes(96, 48, 1 << 62) == 1
    assert hip_backend.sweep_early_pushes(1024, 6144, 2) == 3328
    for bad in ((1024, 6144, 1), (1024, 6000, 1600), (1023, 6144, 1600), (0, 0, 1600),
                (1024, 6144, 0)):
        with pytest.raises(hip_backend.HipBackendError):
            hip_backend.sweep_early_pushes(*bad)
    best, margin = np.full((4, 3), 7, np.int32), np.full((4, 3), 0.25)
    labels, lengths = np.zeros(4, np.int32), np.full(4, 500, np.int64)
    thresholds = np.array([0.5])
    arrays = [np.full(shape, -1, np.int64) for shape in ((3, 1, 1, 8), (3, 1, 8), (3, 1, 3), (3, 1, 2))]
    p = lambda a: a.ctypes.data                                    # noqa: E731
    names = ['sb', 'sm', 'eb', 'em', 'labels', 'lengths', 'n', 'steps', 'classes', 'size', 'chunk',
             'thr', 'n_thr', 'calls', 'early', 'windows', 'pushes']
    good = [p(best), p(margin), None, None, p(labels), p(lengths), 4, 3, 5, 96, 100, p(thresholds), 1] + \
        [p(a) for a in arrays]

    def with_(**changed):
        args = list(good)
        for name, value in changed.items():
            args[names.index(name)] = value
        return args

    refused = [with_(sb=None), with_(sm=None), with_(eb=p(best)), with_(em=p(margin)), with_(n=-1),
               with_(steps=0), with_(classes=1), with_(classes=257), with_(size=95), with_(size=0),
               with_(size=-96), with_(chunk=0), with_(chunk=-5), with_(thr=None), with_(n_thr=0),
               with_(calls=None), with_(early=None), with_(windows=None), with_(pushes=None),
               with_(lengths=None)]
    for bad in refused:
        for entry in (lib.dbh_sweep_early_host, lib.dbh_sweep_early_tally):
            assert entry(*bad) == INVALID, bad
        assert lib.dbh_sweep_early_tally_dev(*bad, None) == INVALID, bad
    # P above 4096 (input 9000, 3 steps, chunk 4: cap 18000); a negative length on the host entries
    for entry in (lib.dbh_sweep_early_host, lib.dbh_sweep_early_tally):
        assert entry(*with_(size=9000, chunk=4)) == INVALID
        lengths[2] = -1
        assert entry(*good) == INVALID
        lengths[2] = 500
    assert lib.dbh_sweep_early_tally_dev(*with_(size=9000, chunk=4), None) == INVALID
    assert all((a == -1).all() for a in arrays) and (best == 7).all()
    for entry in (lib.dbh_sweep_early_host, lib.dbh_sweep_early_tally):
        assert entry(*with_(n=0)) == 0                               # nothing to count
    assert lib.dbh_sweep_early_tally_dev(*with_(n=0), None) == 0
    assert all((a == -1).all() for a in arrays)


def test_the_model_check_program_is_there():
    csrc = os.path.join(REPO, 'deepbinner_amd', 'csrc')
    text = open(os.path.join(csrc, 'Makefile')).read()
    assert 'early_asan:' in text and 'early_model_check.cpp' in text
    assert '-fsanitize=address,undefined' in text[text.index('early_asan:'):]
    source = open(os.path.join(csrc, 'early_model_check.cpp')).read()
    assert 'int main()' in source and 'dbh_early_core.h' in source
    kernels = open(os.path.join(csrc, 'dbh_sweep.hip')).read()
    assert 'dbh_early_core.h' in kernels and 'asm' not in kernels
    assert 'dbh_early_core.h' in open(os.path.join(csrc, 'dbh_api_sweep.hip')).read()


# ---- the command against a host stand-in ----------------------------------------------------------
def options(**given):
    base = dict(input=SINGLE, native=False, rapid=False, start_model=STARTS, end_model=None,
                max_scan_size=6144.0, score_diffs='0.5', labels=None, multi_read=False,
                batch_size=4, loader_procs=0, devices=0, live=True, chunk_samples=1600)
    base.update(given)
    return argparse.Namespace(**base)


def table(text):
    lines = text.strip('\n').split('\n')
    return lines[0].split('\t'), [line.split('\t') for line in lines[1:]]


LIVE_COLUMNS = ['min_windows', 'score_diff', 'mode', 'reads', 'decided', 'never', 'agree', 'changed',
                'lost', 'late', 'windows_sum', 'push_median', 'samples_sum', 'length_sum',
                'classified', 'none']


def test_command_says_what_replay_says(oracle_backend, gold, capsys):
    capsys.readouterr()
    sweep.sweep(options(), backend=ref.HostBackend())
    out = capsys.readouterr().out
    header, rows = table(out)
    assert header == LIVE_COLUMNS + [str(c) for c in range(1, 13)]
    assert [(int(r[0]), r[1], r[2]) for r in rows] == [(m, '0.5', '-') for m in range(1, 13)]
    assert all(all(v.lstrip('-').isdigit() for v in r[:1] + r[3:]) for r in rows)
    first = dict(zip(header, rows[0]))
    # replay's summary of the same reads (tests/test_live.py): 7 reads, 7 decided, 7 of 7 agree, 1
    # later than window 1, every one decided with its first 1600 samples
    replay_options = dict(vars(options()), scan_size=6144.0, score_diff=0.5, require_either=True,
                          require_start=False, require_both=False, min_windows=1,
                          stop_on_decision=False, channels=512)
    replay.replay(argparse.Namespace(**replay_options), backend=live_reference.HostBackend())
    replayed, err = capsys.readouterr()
    assert '7 reads, 7 decided' in err and 'agrees with the final call: 7 of 7' in err
    assert 'decided later than window 1: 1, never: 0' in err and 'median 1600, maximum 1600' in err
    assert [first[c] for c in ('reads', 'decided', 'never', 'agree', 'changed', 'lost', 'late')] == \
        ['7', '7', '0', '7', '0', '0', '1']
    assert first['push_median'] == '1' and first['samples_sum'] == str(7 * 1600)
    _, lines = table(replayed)
    assert first['windows_sum'] == str(sum(int(row[2]) for row in lines)) == '8'
    assert first['length_sum'] == str(sum(len(s) for s in gold['signals']))
    per_barcode = [sum(1 for row in lines if row[1] == str(c)) for c in range(1, 13)]
    assert [int(v) for v in rows[0][16:]] == per_barcode and first['classified'] == '7'
    # every min_windows against replay --stop_on_decision of that setting would be 12 replays: the
    # last row, where only the whole scan decides, is the final call
    last = dict(zip(header, rows[-1]))
    assert (last['decided'], last['agree'], last['late'], last['windows_sum']) == ('7', '7', '0', '84')
    assert rows[-1][16:] == rows[0][16:]


def test_command_with_labels_and_with_both_models(oracle_backend, gold, capsys, tmp_path):
    labels = tmp_path / 'labels.tsv'
    said = ['none', '3'] + ['0', '1', '1', '2', '12']
    labels.write_text('read_ID\tbarcode_call\n' + ''.join(
        '{}\t{}\n'.format(rid, label) for rid, label in zip(gold['read_ids'], said)))
    capsys.readouterr()
    backend = ref.HostBackend()
    sweep.sweep(options(end_model=ENDS, max_scan_size=1024.0, score_diffs='0.9,0.5',
                        labels=str(labels), chunk_samples=512), backend=backend)
    header, rows = table(capsys.readouterr().out)
    assert header == LIVE_COLUMNS + ['right', 'wrong', 'missed'] + [str(c) for c in range(1, 13)]
    assert [(r[0], r[1], r[2]) for r in rows] == [
        (str(m), t, mode) for m in (1, 2) for t in ('0.5', '0.9')
        for mode in ('either', 'start', 'both')]
    assert backend.batches == 2
    for r in rows:
        assert int(r[3]) == 7 == int(r[4]) + int(r[5]) and int(r[4]) == sum(int(v) for v in r[6:9])
        assert int(r[14]) + int(r[15]) == 7 and sum(int(v) for v in r[16:19]) == 6
    for a, b, c in zip(rows[0::3], rows[1::3], rows[2::3]):             # the start side repeats
        assert a[3:14] == b[3:14] == c[3:14]
        assert int(a[14]) >= int(b[14]) >= int(c[14])
    # the golden reads' start calls are 3 2 3 1 1 2 12: at 0.5 and m = 1, start rule, one label of
    # six is wrong (read 1: said 3, called 2) unless the end side disagrees
    start_rows = [r for r in rows if (r[0], r[1], r[2]) == ('1', '0.5', 'start')]
    assert len(start_rows) == 1 and int(start_rows[0][17]) <= 6


@pytest.mark.parametrize('given,message', [
    (dict(start_model=None, end_model=ENDS), 'replay needs a start model'),
    (dict(input=os.path.join(GOLD, 'training_data.txt')), 'cannot be swept with --live'),
    (dict(live=False), '--chunk_samples needs --live'),
    (dict(chunk_samples=0), '--chunk_samples must be at least 1'),
    (dict(chunk_samples=-3), '--chunk_samples must be at least 1'),
    (dict(chunk_samples=1), 'more than 4096 pushes'),
    (dict(devices=2), 'a sweep runs on one GPU'),
    (dict(score_diffs='0'), 'every --score_diffs value must be in the range (0, 1]'),
])
def test_command_refusals(oracle_backend, given, message):
    with pytest.raises(SystemExit) as e:
        sweep.sweep(options(**given), backend=ref.HostBackend())
    assert message in str(e.value) and '\n' not in str(e.value) and e.value.code != 0


def parent_table(counts, scan_sizes, thresholds, modes, reads, n_classes, labelled):
    """The table ``sweep`` printed before it had ``--live``, line by line."""
    columns = ['scan_size', 'score_diff', 'mode', 'reads', 'classified', 'none']
    if labelled:
        columns += ['right', 'wrong', 'missed']
    lines = ['\t'.join(columns + [str(c) for c in range(1, n_classes)])]
    for k, scan_size in enumerate(scan_sizes):
        for t, threshold in enumerate(thresholds):
            for j, mode in enumerate(modes):
                cell = [int(v) for v in counts[k, t, j]]
                row = [scan_size, repr(float(threshold)), mode, reads, sum(cell[1:n_classes]), cell[0]]
                if labelled:
                    row += cell[n_classes:n_classes + 3]
                lines.append('\t'.join(str(v) for v in row + cell[1:n_classes]))
    return '\n'.join(lines) + '\n'


def test_sweep_without_the_flag_prints_what_it_printed(oracle_backend, gold, capsys):
    class Recording(ref.HostBackend):
        def sweep_tally(self, start, end, thresholds, n_classes, labels=None, counts=None):
            self.counts = super().sweep_tally(start, end, thresholds, n_classes, labels, counts)
            return self.counts

        def sweep_early_tally(self, *args, **kwargs):
            raise AssertionError('the early tally ran without --live')

    for given in (dict(live=False, chunk_samples=None), dict()):
        backend = Recording()
        args = options(end_model=ENDS, max_scan_size=1024.0, score_diffs='0.5,0.9', **given)
        if not given:                          # the namespace of a caller that predates the flag
            del args.live, args.chunk_samples
        capsys.readouterr()
        sweep.sweep(args, backend=backend)
        out = capsys.readouterr().out
        assert out == parent_table(backend.counts, [512, 1024], [0.5, 0.9], sweep_reference.MODES, 7,
                                   13, False)


def test_command_line_entry(monkeypatch):
    seen = {}
    monkeypatch.setattr(sweep, 'sweep', lambda args: seen.update(vars(args)))
    cli.main(['sweep', '--native', 'some_dir'])
    assert seen['live'] is False and seen['chunk_samples'] is None
    cli.main(['sweep', '--native', '--live', 'some_dir'])
    assert seen['live'] is True and seen['chunk_samples'] is None            # (1600 in sweep())
    cli.main(['sweep', '-s', STARTS, '--live', '--chunk_samples', '512', 'some_dir'])
    assert seen['live'] is True and seen['chunk_samples'] == 512 and seen['end_model'] is None
    out = io.StringIO()
    with contextlib.redirect_stdout(out), pytest.raises(SystemExit):
        cli.main(['sweep', '--help'])
    assert '--live' in out.getvalue() and '--chunk_samples' in out.getvalue()
