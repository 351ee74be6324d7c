"""Live sessions without a GPU: the planning and decision rules on the host (``live_plan_host``, the
lines the kernels compile) against the NumPy restatement over every seam length, chunking and flag
order; the ``replay`` command - rows, summary, refusals - against a host stand-in for its session;
the new symbols and what the entries refuse before any device work."""
import argparse
import ctypes
import os

import numpy as np
import pytest

import live_reference as ref
import sweep_reference
from conftest import GOLD, MODEL_DIR, REPO
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import hip_backend, replay

SINGLE = os.path.join(GOLD, 'fast5', 'single')
STARTS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw')
ENDS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw')
NEW_SYMBOLS = ['dbh_live_create', 'dbh_live_destroy', 'dbh_live_push', 'dbh_live_track',
               'dbh_live_fold_dev', 'dbh_live_plan_host']
INVALID = 1


# ---- the rules on the host -------------------------------------------------------------------------
def chunk_plans(length, input_size, rng):
    """(lengths, flags) of one read delivered in every way the contract names."""
    h = input_size // 2
    plans = [([length], [ref.BEGIN | ref.END])]
    sizes = [h - 1, h, h + 1, 3 * h, 1600] + ([1] if input_size == 96 and length <= 700 else [])
    for size in sizes:
        parts = [min(size, length - a) for a in range(0, max(length, 1), size)]
        flags = [0] * len(parts)
        flags[0] |= ref.BEGIN
        flags[-1] |= ref.END
        plans.append((parts, flags))
        plans.append((parts + [0], [f & ~ref.END for f in flags] + [ref.END]))     # END alone
    cuts = np.sort(rng.integers(0, length + 1, 6))                 # random sizes, empty ones too
    parts = np.diff(np.concatenate([[0], cuts, [length]])).tolist()
    plans.append((parts, [ref.BEGIN] + [0] * (len(parts) - 2) + [ref.END]))
    # flags out of order: a chunk before any BEGIN, a chunk behind END, BEGIN in the middle of a read
    plans.append(([5, length, 7, length], [0, ref.BEGIN | ref.END, 0, ref.BEGIN]))
    plans.append(([length, length], [ref.BEGIN, ref.BEGIN | ref.END]))
    plans.append(([length], [ref.BEGIN]))                          # never ended
    return plans


@pytest.mark.parametrize('input_size,steps', [(96, 12), (1024, 4)])
def test_plan_host_against_the_restatement(input_size, steps):
    rng = np.random.default_rng(input_size)
    scan_size = steps * (input_size // 2)
    lengths = ref.seam_lengths(input_size, steps) + rng.integers(0, 2 * (scan_size + input_size), 12).tolist()
    checked = 0
    for length in lengths:
        for parts, flags in chunk_plans(int(length), input_size, rng):
            best = rng.integers(0, 4, steps).astype(np.int32)
            margin = rng.choice([0.25, 0.5, 0.75], steps)
            for options in (dict(), dict(min_windows=steps), dict(stop_on_decision=True),
                            dict(score_diff=0.75, min_windows=2, stop_on_decision=True)):
                got, got_new = hip_backend.live_plan_host(input_size, scan_size, parts, flags, best,
                                                          margin, **options)
                want, want_new = ref.plan(input_size, scan_size, parts, flags, best, margin, **options)
                assert got.dtype == want.dtype == hip_backend.LIVE_RESULT
                assert got.tobytes() == want.tobytes(), (length, parts, flags, options)
                assert np.array_equal(got_new, want_new), (length, parts, flags, options)
                checked += 1
    assert checked > 500


def test_plan_host_rules_in_plain_numbers():
    """96-sample windows every 48: four steps, cap 240."""
    plan = lambda lengths, flags, best, margin, **o: hip_backend.live_plan_host(  # noqa: E731
        96, 192, lengths, flags, best, margin, **o)
    best, margin = [0, 3, 3, 5], [0.9, 0.5, 0.7, 0.6]
    # windows become ready at 96, 144, 192, 240 samples; samples counts what is not kept too
    got, new = plan([95, 1, 47, 1, 1000], [ref.BEGIN, 0, 0, 0, 0], best, margin)
    assert new.tolist() == [0, 1, 0, 1, 2] and got['samples'].tolist() == [95, 96, 143, 144, 1144]
    assert got['status'].tolist() == [ref.PENDING, ref.PENDING, ref.PENDING, ref.DECIDED, ref.FINAL]
    # a margin equal to score_diff decides; the call stays when the maximum moves on
    assert got['call'].tolist() == [0, 0, 0, 3, 3] and got['final_call'].tolist() == [-1] * 4 + [5]
    assert got['decided_windows'][-1] == 2 and got['decided_samples'][-1] == 144
    # END makes every window ready: a short read's partial and empty windows
    got, new = plan([10, 0], [ref.BEGIN, ref.END], best, margin)
    assert new.tolist() == [0, 4] and got['status'].tolist() == [ref.PENDING, ref.FINAL]
    # min_windows never decides before window m, and decides at m when the rule already held
    for m in (1, 2, 3, 4):
        got, _ = plan([240], [ref.BEGIN], best, margin, min_windows=m)
        assert got['decided_windows'][0] == max(m, 2) and got['call'][0] == (5 if m == 4 else 3)
    # stop on decision: nothing runs behind the deciding window, later chunks report the same call
    got, new = plan([240, 50, 0], [ref.BEGIN, 0, ref.END], best, margin, stop_on_decision=True)
    assert new.tolist() == [2, 0, 0] and got['windows'].tolist() == [2, 2, 2]
    assert got['status'].tolist() == [ref.DECIDED] * 3 and got['call'].tolist() == [3, 3, 3]
    assert got['final_call'].tolist() == [-1] * 3 and got['samples'].tolist() == [240, 290, 290]
    # no read open: IDLE, and nothing changes
    got, new = plan([7, 9], [0, ref.END], best, margin)
    assert got['status'].tolist() == [ref.IDLE] * 2 and not got['samples'].any() and not new.any()


def test_plan_host_refuses_what_creation_refuses():
    lib = hip_backend.load_library()
    lengths, flags = np.array([10], np.int64), np.array([1], np.uint32)
    best, margin = np.zeros(12, np.int32), np.zeros(12)
    results = np.full(1, 7, hip_backend.LIVE_RESULT)
    p = lambda a: a.ctypes.data                                    # noqa: E731
    good = [96, 576, 0.5, 1, 0, p(lengths), p(flags), 1, p(best), p(margin), p(results), None]
    assert lib.dbh_live_plan_host(*good) == 0 and results['samples'][0] == 10
    results[:] = 7
    for at, bad in ((0, 97), (1, 500), (1, 0), (1, -48), (2, float('nan')), (3, 0), (3, 13), (4, 2),
                    (5, None), (6, None), (7, -1), (8, None), (9, None), (10, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_live_plan_host(*args) == INVALID, (at, bad)
    for bad_flags, bad_length in ((4, 10), (1, -1)):
        held = np.array([bad_length], np.int64), np.array([bad_flags], np.uint32)
        assert lib.dbh_live_plan_host(*(good[:5] + [p(held[0]), p(held[1])] + good[7:])) == INVALID
    assert (results['samples'] == 7).all()
    assert lib.dbh_live_plan_host(*(good[:7] + [0] + good[8:])) == 0            # no chunk


# ---- the C ABI without a device --------------------------------------------------------------------
def test_symbols_are_exported_and_listed():
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in hip_backend.EXPORTED_SYMBOLS, name
    header = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    section = header[header.index('---- live:'):header.index('---- compressed input')]
    for cite in ('classify.py:337-349', 'classify.py:368-374'):
        assert cite in section
    assert hip_backend.LIVE_RESULT == ref.RESULT and hip_backend.LIVE_RESULT.itemsize == 48
    assert (hip_backend.LIVE_IDLE, hip_backend.LIVE_PENDING, hip_backend.LIVE_DECIDED,
            hip_backend.LIVE_FINAL) == (ref.IDLE, ref.PENDING, ref.DECIDED, ref.FINAL)
    assert (hip_backend.LIVE_BEGIN, hip_backend.LIVE_END) == (ref.BEGIN, ref.END)
    from deepbinner_amd._cabi import Finalised, Owner, Scoped
    assert issubclass(hip_backend.LiveSession, (Owner,)) and \
        issubclass(hip_backend.LiveSession, Scoped) and issubclass(hip_backend.LiveSession, Finalised)


def test_bad_arguments_are_refused_before_any_device_work():
    lib = hip_backend.load_library()
    session = ctypes.c_void_p(7)
    # no model, no place for the session (1 stands for a pointer nobody may touch)
    assert lib.dbh_live_create(None, 4, 6144, 0.5, 1, 0, 0, ctypes.byref(session)) == INVALID
    assert lib.dbh_live_create(1, 4, 6144, 0.5, 1, 0, 0, None) == INVALID
    for channels in (0, -1, 16385):
        assert lib.dbh_live_create(1, channels, 6144, 0.5, 1, 0, 0, ctypes.byref(session)) == INVALID
    assert lib.dbh_live_create(1, 4, 6144, 0.5, 1, 0, -1, ctypes.byref(session)) == INVALID
    assert session.value == 7
    assert lib.dbh_live_destroy(None) == 0
    assert lib.dbh_live_push(None, 1, 1, 1, 1, 1, 1) == INVALID
    assert lib.dbh_live_push(None, 1, 1, 1, 1, 1, 0) == INVALID
    windows = ctypes.c_int32(-3)
    assert lib.dbh_live_track(None, 0, 1, 1, ctypes.byref(windows)) == INVALID and windows.value == -3
    assert lib.dbh_live_fold_dev(None, 1, 1, 4, 8, 4, 0.5, 1, 0, 1, 1, 1, 1, None) == INVALID


def test_the_model_check_program_is_there():
    text = open(os.path.join(REPO, 'deepbinner_amd', 'csrc', 'Makefile')).read()
    assert 'live_asan:' in text and 'live_model_check.cpp' in text and 'dbh_live.hip' in text
    assert '-fsanitize=address,undefined' in text[text.index('live_asan:'):]
    source = open(os.path.join(REPO, 'deepbinner_amd', 'csrc', 'live_model_check.cpp')).read()
    assert 'int main()' in source and 'dbh_live_core.h' in source
    kernels = open(os.path.join(REPO, 'deepbinner_amd', 'csrc', 'dbh_live.hip')).read()
    for shared in ('dbh_live_core.h', 'dbh_front.h', 'dbh_fold.h', 'dbh_wave.h'):
        assert shared in kernels or shared in open(
            os.path.join(REPO, 'deepbinner_amd', 'csrc', 'dbh_live.h')).read(), shared
    assert 'asm' not in kernels


# ---- the command against a host stand-in -----------------------------------------------------------
def options(**given):
    base = dict(input=SINGLE, native=False, rapid=False, start_model=STARTS, end_model=None,
                scan_size=6144.0, score_diff=0.5, require_either=True, require_start=False,
                require_both=False, min_windows=1, stop_on_decision=False, channels=512,
                chunk_samples=1600, multi_read=False, batch_size=4, loader_procs=0, devices=0)
    base.update(given)
    return argparse.Namespace(**base)


def table(text):
    lines = text.strip('\n').split('\n')
    return lines[0].split('\t'), [line.split('\t') for line in lines[1:]]


def predicted_rows(gold, chunk_samples, scan_size=6144, score_diff=0.5, min_windows=1, stop=False):
    """The table the restatement predicts: each read's windows through the oracle network and the
    sweep's fold as a whole, then the rules over the chunk lengths the command pushes."""
    from conftest import OracleModel
    from deepbinner_amd.model_format import ModelWeights
    model = OracleModel(ModelWeights.load(STARTS)[0])
    name = lambda c: 'none' if c == 0 else str(c)                  # noqa: E731
    rows = []
    for read_id, signal in zip(gold['read_ids'], gold['signals']):
        steps = scan_size // 512
        probs = model.predict(ref.front(signal[:scan_size + 512], 1024, steps)[:, :, None])
        best, margin = sweep_reference.sweep(np.asarray(probs, np.float32)[None])
        parts = [len(c) for c in ref.chunked(signal, chunk_samples)]
        flags = [0] * len(parts)
        flags[0] |= ref.BEGIN
        flags[-1] |= ref.END
        last = ref.plan(1024, scan_size, parts, flags, best[0], margin[0], score_diff=score_diff,
                        min_windows=min_windows, stop_on_decision=stop)[0][-1]
        decided, final = last['decided_windows'] > 0, last['status'] == ref.FINAL
        rows.append([read_id, name(last['call']) if decided else 'none',
                     str(last['decided_windows']) if decided else '-',
                     str(last['decided_samples']) if decided else '-',
                     name(last['final_call']) if final else '-', str(len(signal)),
                     ('yes' if last['call'] == last['final_call'] else 'no')
                     if decided and final else '-'])
    return rows


def test_command_prints_the_table_the_restatement_predicts(oracle_backend, gold, capsys):
    capsys.readouterr()
    replay.replay(options(), backend=ref.HostBackend())
    out, err = capsys.readouterr()
    header, lines = table(out)
    assert header == ['read_ID', 'live_call', 'decided_windows', 'decided_samples', 'final_call',
                      'samples', 'agree']
    order = [row[0] for row in lines]                      # the loaders' file order
    assert sorted(order) == sorted(gold['read_ids'])
    in_order = lambda rows: sorted(rows, key=lambda row: order.index(row[0]))      # noqa: E731
    want = in_order(predicted_rows(gold, 1600))
    assert lines == want
    # the golden reads: classify's start-side calls, each decided at its first or second window
    by_id = {row[0]: row for row in lines}
    assert [by_id[i][4] for i in gold['read_ids']] == ['3', '2', '3', '1', '1', '2', '12']
    assert [by_id[i][2] for i in gold['read_ids']] == ['1', '1', '2', '1', '1', '1', '1']
    assert [row[3] for row in lines] == ['1600', '1600', '1600', '1600', '1600', '1600', '1600']
    assert all(row[6] == 'yes' for row in lines)
    assert '7 reads, 7 decided' in err and 'median 1600, maximum 1600' in err
    assert 'agrees with the final call: 7 of 7' in err and 'decided later than window 1: 1, never: 0' in err
    # fewer channels than reads, other chunks, a late and a stopped decision: file order stays
    capsys.readouterr()
    replay.replay(options(channels=3, chunk_samples=512, min_windows=2, stop_on_decision=True),
                  backend=ref.HostBackend())
    out, err = capsys.readouterr()
    _, lines = table(out)
    assert lines == in_order(predicted_rows(gold, 512, min_windows=2, stop=True))
    assert [row[0] for row in lines] == order
    assert [row[1] for row in lines] == [row[4] for row in want]
    assert all(row[2] == '2' and row[3] == '1536' and row[4] == '-' and row[6] == '-' for row in lines)
    # an end model that comes with a preset is ignored
    capsys.readouterr()
    replay.replay(options(end_model=ENDS, channels=1), backend=ref.HostBackend())
    assert table(capsys.readouterr().out)[1] == want


@pytest.mark.parametrize('given,message', [
    (dict(start_model=None, end_model=ENDS), 'replay needs a start model'),
    (dict(devices=2), 'a replay runs on one GPU'),
    (dict(input=os.path.join(GOLD, 'training_data.txt')), 'cannot be replayed'),
    (dict(min_windows=0), '--min_windows must be at least 1'),
    (dict(min_windows=13), '--min_windows cannot be more than the 12 windows'),
    (dict(channels=0), '--channels must be from 1 to 16384'),
    (dict(channels=16385), '--channels must be from 1 to 16384'),
    (dict(chunk_samples=0), '--chunk_samples must be at least 1'),
    (dict(scan_size=6000.0), '--scan_size must be a multiple of half the model input size'),
])
def test_command_refusals(oracle_backend, given, message):
    with pytest.raises(SystemExit) as e:
        replay.replay(options(**given), backend=ref.HostBackend())
    assert message in str(e.value) and e.value.code != 0
    if 'input' in given:
        assert '\n' not in str(e.value)


def test_command_line_entry(monkeypatch):
    seen = {}
    monkeypatch.setattr(replay, 'replay', lambda args: seen.update(vars(args)))
    cli.main(['replay', '--native', 'some_dir'])
    assert seen['scan_size'] == 6144 and seen['score_diff'] == 0.5 and seen['min_windows'] == 1
    assert seen['channels'] == 512 and seen['chunk_samples'] == 1600
    assert not seen['stop_on_decision'] and not seen['multi_read'] and seen['devices'] == 0
    assert os.path.basename(seen['start_model']).startswith('EXP-NBD103_read_starts')
    cli.main(['replay', '-s', STARTS, '--channels', '3', '--chunk_samples', '512', '--min_windows',
              '2', '--stop_on_decision', '--multi_read', 'some_dir'])
    assert seen['channels'] == 3 and seen['chunk_samples'] == 512 and seen['min_windows'] == 2
    assert seen['stop_on_decision'] and seen['multi_read'] and seen['end_model'] is None
    with pytest.raises(SystemExit) as e:
        cli.main(['replay', 'some_dir'])
    assert 'you must provide at least one model' in str(e.value)
    for refused in ('prep', 'train'):
        with pytest.raises(SystemExit) as e:
            cli.main([refused])
        assert 'not part of this build' in str(e.value) and 'replay' in str(e.value)
