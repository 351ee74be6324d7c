"""Pair live sessions without a GPU: the tail ring and the end-window rules on the host
(``live_tail_plan_host``, the lines the kernels compile) against the NumPy restatement, as integers,
over every seam length and chunking, with the positions each end window reads checked against what
the plan stored; the combine rule's one text against the reference's truth table; the ``replay
--both_ends`` command - rows, summary, refusals - against a host stand-in; ``replay`` without the
flag unchanged."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import live_pair_reference as pair
import live_reference as ref
import test_live
from conftest import GOLD, REPO
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import hip_backend, replay
from oracle import classify_ref

CSRC = os.path.join(REPO, 'deepbinner_amd', 'csrc')
NEW_SYMBOLS = ['dbh_live_create_pair', 'dbh_live_push_pair', 'dbh_live_end_track',
               'dbh_live_tail_plan_host']
INVALID = 1
B, E = ref.BEGIN, ref.END


# ---- the ring and the end windows on the host ------------------------------------------------------
def deliveries(length, input_size, steps, rng):
    """(lengths, flags) of one read of ``length`` samples, delivered in every way the contract
    names; the read this test follows is the LAST one that ends in each list."""
    h = input_size // 2
    cap = steps * h + h
    cut = lambda sizes: [s for s in sizes]                           # noqa: E731

    def chunks_of(size):
        return [min(size, length - a) for a in range(0, max(length, 1), size)]

    def flagged(parts):
        flags = [0] * len(parts)
        flags[0] |= B
        flags[-1] |= E
        return cut(parts), flags

    plans = [flagged([length])]                                                  # whole
    sizes = [h - 1, h, h + 1] + ([1] if input_size == 96 else [])
    for size in sizes:
        plans.append(flagged(chunks_of(size)))
    for first in (cap, cap + 1, 2 * cap + 3):             # a single chunk of exactly that, the rest
        if length >= first:
            plans.append(flagged([first, length - first]))
    half = length // 2
    plans.append(flagged([0, half, 0, 0, length - half, 0]))                     # empty chunks
    plans.append(([length, 0], [B, E]))                                          # END alone
    plans.append(([length, 0, 0], [B, 0, E]))
    if length == 0:
        plans.append(([0], [B | E]))                                             # BEGIN|END, empty
    plans.append(([h + 3, length], [B, B | E]))                                  # BEGIN inside a read
    plans.append(([2 * cap + 5, 0, 7, length], [B, E, 0, B | E]))   # a short read after a long one
    plans.append(([3 * cap + 1, length // 3, length - length // 3], [B | E, B, E]))
    cuts = np.sort(rng.integers(0, length + 1, 5))
    parts = np.diff(np.concatenate([[0], cuts, [length]])).tolist()
    plans.append(flagged(parts))
    return plans


def follow(input_size, steps, lengths, flags, store, samples, ends, windows):
    """Plays the plan's stores into a ring (sample p of a read holds the value value_of(read, p))
    and checks, for every chunk that ended a read, that each end window's positions hold that
    read's samples [a, a + m).  -> the number of windows checked"""
    h = input_size // 2
    cap = steps * h + h
    ring = np.zeros(cap, np.int64)
    value_of = lambda read, p: 1000003 * read + p + 1                # noqa: E731
    read, n, is_open, checked = 0, 0, False, 0
    for i, (length, f) in enumerate(zip(lengths, flags)):
        if f & B:
            read, n, is_open = read + 1, 0, True
        elif not is_open:
            assert not store[i].any() and not ends[i]
            continue
        start, keep, at, head = (int(v) for v in store[i])
        assert 0 <= keep <= cap and start == length - keep and 0 <= at < cap
        assert head == min(keep, cap - at)
        values = value_of(read, n + start + np.arange(keep))
        ring[at:at + head] = values[:head]                            # two spans at the wrap
        ring[:keep - head] = values[head:]
        n += length
        assert samples[i] == n
        assert ends[i] == bool(f & E)
        if f & E:
            is_open = False
            for s in range(steps):
                a, m, pad, first = (int(v) for v in windows[i, s])
                assert 0 <= m <= input_size and pad == input_size - m and first == a % cap
                assert a >= max(n - cap, 0) and a + m <= n
                got = ring[(first + np.arange(m)) % cap]
                assert np.array_equal(got, value_of(read, a + np.arange(m))), (i, s, a, m)
                checked += 1
    return checked


@pytest.mark.parametrize('input_size,steps', [(96, 12), (1024, 4)])
def test_tail_plan_host_against_the_restatement(input_size, steps):
    rng = np.random.default_rng(input_size + 1)
    scan_size = steps * (input_size // 2)
    cap = scan_size + input_size // 2
    lengths = pair.read_lengths(input_size, steps) + rng.integers(0, 3 * cap, 10).tolist()
    plans = windows_checked = 0
    for length in lengths:
        for parts, flags in deliveries(int(length), input_size, steps, rng):
            got = hip_backend.live_tail_plan_host(input_size, scan_size, parts, flags)
            want = pair.tail_plan(input_size, scan_size, parts, flags)
            for g, w, what in zip(got, want, ('store', 'samples', 'ends', 'windows')):
                assert g.dtype == w.dtype and g.shape == w.shape, what
            ended = np.asarray(want[2], bool)
            assert np.array_equal(got[0], want[0]), (length, parts, flags)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert np.array_equal(got[3][ended], want[3][ended]), (length, parts, flags)
            assert not got[3][~ended].any()                           # left alone
            windows_checked += follow(input_size, steps, parts, flags, *got)
            plans += 1
    assert plans > 250 and windows_checked > 250 * steps


def test_tail_plan_rules_in_plain_numbers():
    """96-sample windows every 48, scan 192: four end windows, a ring of 240."""
    plan = lambda lengths, flags: hip_backend.live_tail_plan_host(96, 192, lengths, flags)  # noqa: E731
    store, samples, ends, windows = plan([100, 200, 50], [B, 0, E])
    assert store.tolist() == [[0, 100, 0, 100], [0, 200, 100, 140], [0, 50, 60, 50]]
    assert samples.tolist() == [100, 300, 350] and ends.tolist() == [0, 0, 1]
    # n = 350: [254, 350), [206, 302), [158, 254), [110, 206) - the last reaches back to n - cap
    assert windows[2].tolist() == [[254, 96, 0, 14], [206, 96, 0, 206], [158, 96, 0, 158],
                                   [110, 96, 0, 110]]
    # a chunk longer than the ring keeps its last 240; a read shorter than a window is padded in front
    store, samples, ends, windows = plan([500, 0, 30], [B, E, B | E])
    assert store.tolist() == [[260, 240, 20, 220], [0, 0, 20, 0], [0, 30, 0, 30]]
    assert windows[1, 0].tolist() == [404, 96, 0, 164] and windows[1, 3].tolist() == [260, 96, 0, 20]
    assert windows[2].tolist() == [[0, 30, 66, 0], [0, 0, 96, 0], [0, 0, 96, 0], [0, 0, 96, 0]]
    # no read open: nothing is stored, nothing ends
    store, samples, ends, _ = plan([7, 9], [0, E])
    assert not store.any() and not samples.any() and not ends.any()


def test_tail_plan_host_refuses_what_creation_refuses():
    lib = hip_backend.load_library()
    lengths, flags = np.array([10], np.int64), np.array([3], np.uint32)
    store, samples = np.full(4, 7, np.int64), np.full(1, 7, np.int64)
    ends, windows = np.full(1, 7, np.int32), np.full(12 * 4, 7, np.int64)
    p = lambda a: a.ctypes.data                                    # noqa: E731
    good = [96, 576, p(lengths), p(flags), 1, p(store), p(samples), p(ends), p(windows)]
    assert lib.dbh_live_tail_plan_host(*good) == 0 and samples[0] == 10 and ends[0] == 1
    samples[:] = 7
    for at, bad in ((0, 97), (0, 0), (1, 500), (1, 0), (1, -48), (2, None), (3, None), (4, -1),
                    (5, None), (6, None), (7, None), (8, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_live_tail_plan_host(*args) == INVALID, (at, bad)
    for bad_flags, bad_length in ((4, 10), (1, -1)):
        held = np.array([bad_length], np.int64), np.array([bad_flags], np.uint32)
        assert lib.dbh_live_tail_plan_host(*(good[:2] + [p(held[0]), p(held[1])] + good[4:])) == INVALID
    assert samples[0] == 7
    assert lib.dbh_live_tail_plan_host(*(good[:4] + [0] + good[5:])) == 0       # no chunk


# ---- the C ABI without a device --------------------------------------------------------------------
def test_symbols_are_exported_declared_and_listed():
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in hip_backend.EXPORTED_SYMBOLS, name
    header = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    section = header[header.index('---- live:'):header.index('---- compressed input')]
    for cite in ('classify.py:343-357', 'classify.py:298-322'):
        assert cite in section
    for name in NEW_SYMBOLS + ['dbh_live_end_result']:
        assert name in section, name
    assert hip_backend.LIVE_END_RESULT == pair.END_RESULT
    assert hip_backend.LIVE_END_RESULT.itemsize == 40


def test_bad_arguments_are_refused_before_any_device_work():
    lib = hip_backend.load_library()
    session = ctypes.c_void_p(7)
    by = ctypes.byref(session)
    # no start model, no end model, no place for the session (1: a pointer nobody may touch)
    assert lib.dbh_live_create_pair(None, 1, 4, 6144, 0.5, 1, 0, 0, 0, by) == INVALID
    assert lib.dbh_live_create_pair(1, None, 4, 6144, 0.5, 1, 0, 0, 0, by) == INVALID
    assert lib.dbh_live_create_pair(1, 1, 4, 6144, 0.5, 1, 0, 0, 0, None) == INVALID
    for channels in (0, -1, 16385):
        assert lib.dbh_live_create_pair(1, 1, channels, 6144, 0.5, 1, 0, 0, 0, by) == INVALID
    for mode in (-1, 3):
        assert lib.dbh_live_create_pair(1, 1, 4, 6144, 0.5, 1, 0, mode, 0, by) == INVALID
    assert lib.dbh_live_create_pair(1, 1, 4, 6144, 0.5, 1, 0, 0, -1, by) == INVALID
    assert session.value == 7
    assert lib.dbh_live_push_pair(None, 1, 1, 1, 1, 1, 1, 1) == INVALID
    assert lib.dbh_live_push_pair(None, 1, 1, 1, 1, 1, None, 0) == INVALID
    windows = ctypes.c_int32(-3)
    assert lib.dbh_live_end_track(None, 0, 1, 1, ctypes.byref(windows)) == INVALID
    assert windows.value == -3


# ---- the combine rule ------------------------------------------------------------------------------
def test_the_combine_rule_is_one_text_and_the_references_truth_table(gold, tmp_path):
    """dbh_combine.h - what dbh_combine_calls_dev's kernel, the live kernels and the model check
    compile - built for the host: 3 modes by the reference's 15 rows, and every pair of calls."""
    for source in ('dbh_kernels.hip', 'dbh_live_core.h'):
        assert '#include "dbh_combine.h"' in open(os.path.join(CSRC, source)).read(), source
    assert 'DBH_REQUIRE_BOTH' not in open(os.path.join(CSRC, 'dbh_kernels.hip')).read()
    assert 'DBH_REQUIRE_BOTH' not in open(os.path.join(CSRC, 'dbh_live.hip')).read()
    program = ('#include <cstdio>\n#include "dbh_combine.h"\nint main() {\n'
               '  for (int mode = 0; mode < 3; ++mode) for (int s = 0; s < 14; ++s)\n'
               '    for (int e = 0; e < 14; ++e) std::printf("%d %d %d %d\\n", mode, s, e, '
               'dbh::combine_calls(s, e, mode));\n  return 0; }\n')
    exe = str(tmp_path / 'combine')
    subprocess.run(['g++', '-std=c++17', '-I', CSRC, '-x', 'c++', '-', '-o', exe],
                   input=program.encode(), check=True)
    rows = [tuple(int(v) for v in line.split())
            for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split('\n')
            if line]
    got = {(mode, s, e): call for mode, s, e, call in rows}
    assert len(got) == 3 * 14 * 14
    number = lambda c: 0 if c == 'none' else int(c)                  # noqa: E731
    table = gold['calls']['combine_table']
    assert len(table) == 15
    for key, want in table.items():
        mode, s, e = key.split('|')
        assert got[pair.MODES.index(mode), number(s), number(e)] == number(want), key
    for (mode, s, e), call in got.items():
        assert call == pair.combine(s, e, pair.MODES[mode]), (mode, s, e)
    assert [hip_backend.COMBINE_MODES[m] for m in pair.MODES] == [0, 1, 2]


def test_the_model_check_program_covers_the_ring():
    text = open(os.path.join(CSRC, 'Makefile')).read()
    assert '-fsanitize=address,undefined' in text[text.index('live_asan:'):]
    source = open(os.path.join(CSRC, 'live_model_check.cpp')).read()
    for name in ('tail_store', 'end_window', 'end_record', 'plan_tail'):
        assert name in source and name in open(os.path.join(CSRC, 'dbh_live_core.h')).read(), name
    kernels = open(os.path.join(CSRC, 'dbh_live.hip')).read()
    for name in ('tail_store', 'end_window', 'end_record', 'dbh_front::window'):
        assert name in kernels, name
    assert 'atomic' not in kernels


# ---- the command against a host stand-in -----------------------------------------------------------
def options(**given):
    base = dict(both_ends=True, end_model=test_live.ENDS)
    base.update(given)
    return test_live.options(**base)


def predicted_rows(gold, mode, stop=False, min_windows=1, chunk_samples=1600):
    """The two columns the restatement predicts behind the start-only table's rows."""
    from conftest import OracleModel
    from deepbinner_amd.model_format import ModelWeights
    end_model = OracleModel(ModelWeights.load(test_live.ENDS)[0])
    name = lambda c: 'none' if c == 0 else str(c)                  # noqa: E731
    rows = test_live.predicted_rows(gold, chunk_samples, min_windows=min_windows, stop=stop)
    for row, signal in zip(rows, gold['signals']):
        x = pair.end_front(signal[-(6144 + 512):], len(signal), 1024, 12)
        best, margin = pair.sweep_reference.sweep(
            np.asarray(end_model.predict(x[:, :, None]), np.float32)[None])
        end_call = pair.end_call_of(best[0, -1], margin[0, -1], 0.5)
        start = row[4] if row[4] != '-' else row[1]              # the final call, or the early one
        start_call = 0 if start in ('none', '-') else int(start)
        row += [name(end_call), name(pair.combine(start_call, end_call, mode))]
    return rows


def test_command_prints_the_table_the_restatement_predicts(oracle_backend, gold, capsys):
    capsys.readouterr()
    replay.replay(options(), backend=pair.HostBackend())
    out, err = capsys.readouterr()
    header, lines = test_live.table(out)
    assert header == ['read_ID', 'live_call', 'decided_windows', 'decided_samples', 'final_call',
                      'samples', 'agree', 'end_call', 'read_call']
    order = [row[0] for row in lines]
    assert sorted(order) == sorted(gold['read_ids'])
    in_order = lambda rows: sorted(rows, key=lambda row: order.index(row[0]))      # noqa: E731
    want = in_order(predicted_rows(gold, 'require_either'))
    assert lines == want
    # the golden reads: the reference's own end-side and final calls (calls.json)
    by_id = {row[0]: row for row in lines}
    at = [gold['calls']['read_ids'].index(i) for i in gold['read_ids']]
    starts = [gold['calls']['EXP-NBD103_read_starts/start'][j] for j in at]
    ends = [gold['calls']['EXP-NBD103_read_ends/end'][j] for j in at]
    calls = {mode: {i: classify_ref.combine_calls(s, e, mode)
                    for i, s, e in zip(gold['read_ids'], starts, ends)} for mode in pair.MODES}
    assert [by_id[i][4] for i in gold['read_ids']] == starts
    assert [by_id[i][7] for i in gold['read_ids']] == ends
    assert [by_id[i][8] for i in gold['read_ids']] == \
        [calls['require_either'][i] for i in gold['read_ids']]
    counted = {'start only': 0, 'end only': 0, 'both agree': 0, 'both disagree': 0}
    for row in lines:
        s, e = row[4], row[7]
        if s != 'none' and e != 'none':
            counted['both agree' if s == e else 'both disagree'] += 1
        elif s != 'none' or e != 'none':
            counted['start only' if s != 'none' else 'end only'] += 1
    summary = '  barcode on: ' + ', '.join('{} {}'.format(k, v) for k, v in counted.items())
    assert err.rstrip('\n').split('\n')[-1] == summary
    assert '7 reads, 7 decided' in err
    # the other two rules; fewer channels than reads and other chunks
    for flag, mode in (('require_start', 'require_start'), ('require_both', 'require_both')):
        capsys.readouterr()
        replay.replay(options(require_either=False, channels=3, chunk_samples=512, **{flag: True}),
                      backend=pair.HostBackend())
        _, lines = test_live.table(capsys.readouterr().out)
        assert lines == in_order(predicted_rows(gold, mode, chunk_samples=512))
        assert [by_id[row[0]][7] for row in lines] == [row[7] for row in lines]
        assert [row[8] for row in lines] == [calls[mode][row[0]] for row in lines]
    # stopped on a decision: read_call is combined from the early start call
    capsys.readouterr()
    replay.replay(options(stop_on_decision=True, min_windows=2, chunk_samples=512),
                  backend=pair.HostBackend())
    _, lines = test_live.table(capsys.readouterr().out)
    assert lines == in_order(predicted_rows(gold, 'require_either', stop=True, min_windows=2,
                                            chunk_samples=512))
    assert all(row[4] == '-' and row[7] == by_id[row[0]][7] for row in lines)


@pytest.mark.parametrize('given,message', [
    (dict(end_model=None), 'replay --both_ends needs a start model and an end model'),
    (dict(start_model=None), 'replay --both_ends needs a start model and an end model'),
    (dict(input=os.path.join(GOLD, 'training_data.txt')), 'cannot be replayed'),
    (dict(devices=2), 'a replay runs on one GPU'),
])
def test_command_refusals(oracle_backend, given, message):
    with pytest.raises(SystemExit) as e:
        replay.replay(options(**given), backend=pair.HostBackend())
    assert message in str(e.value) and e.value.code != 0 and '\n' not in str(e.value)


def test_replay_without_the_flag_is_unchanged(oracle_backend, gold, capsys):
    """The same bytes beside the existing stand-in, with and without an end model at hand, through
    the backend of this file and through the one of the start-only tests."""
    seen = []
    for given, backend in ((dict(), ref.HostBackend()), (dict(), pair.HostBackend()),
                           (dict(end_model=test_live.ENDS), pair.HostBackend()),
                           (dict(end_model=test_live.ENDS, require_either=False, require_both=True),
                            pair.HostBackend())):
        capsys.readouterr()
        replay.replay(test_live.options(**given), backend=backend)
        seen.append(capsys.readouterr())
    assert all(s.out == seen[0].out and s.err == seen[0].err for s in seen)
    header, lines = test_live.table(seen[0].out)
    assert header == replay.HEADER and len(header) == 7 and 'barcode on' not in seen[0].err
    assert sorted(lines) == sorted(test_live.predicted_rows(gold, 1600))


def test_command_line_entry(monkeypatch):
    seen = {}
    monkeypatch.setattr(replay, 'replay', lambda args: seen.update(vars(args)))
    cli.main(['replay', '--native', 'some_dir'])
    assert seen['both_ends'] is False
    cli.main(['replay', '--native', '--both_ends', '--require_start', 'some_dir'])
    assert seen['both_ends'] is True and seen['require_start'] and not seen['require_either']
    assert os.path.basename(seen['end_model']).startswith('EXP-NBD103_read_ends')
