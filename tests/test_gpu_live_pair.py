"""Pair live sessions on the GPU: a channel's end track under every chunking against the chain of
existing entries on the whole read, bit for bit, and its three calls against the restatement; the
start side's records byte for byte those of a start-only session; the ring going on behind a stop;
the calls against ``classify_pair`` in all three combine modes; channels, rounds and LDS state; what
creation and a push refuse; ``replay --native --both_ends`` beside its host stand-in and beside
``classify --native``."""
import ctypes
import os

import numpy as np
import pytest

import general_fixtures
import live_pair_reference as pair
import live_reference as ref
import test_gpu_live as live
from conftest import GOLD

pytestmark = pytest.mark.gpu

SINGLE = os.path.join(GOLD, 'fast5', 'single')
STARTS, ENDS = 'EXP-NBD103_read_starts', 'EXP-NBD103_read_ends'
INVALID = 1
# name -> ((start input size, end input size), class count, scan size): the live tests' own shapes,
# the two sides with different weights; `mixed` a persistent start model and a general end model
PAIRS = {'persistent-13': ((1024, 1024), 13, 2048), 'general-2': ((96, 96), 2, 576),
         'general-33': ((96, 96), 33, 576), 'mixed-13': ((1024, 96), 13, 1536)}
bits, same_track = live.bits, live.same_track


def tail_reads(end_size, steps, seed, real, n_random=12):
    """Reads of every seam length of the end side and random ones up to 3 cap, so that the ring
    wraps more than once; every third one has a golden read's END spliced at the tail."""
    rng = np.random.default_rng(seed)
    cap = steps * (end_size // 2) + end_size // 2
    lengths = pair.read_lengths(end_size, steps) + rng.integers(0, 3 * cap, n_random).tolist()
    reads = []
    for i, length in enumerate(lengths):
        part = rng.integers(200, 900, int(length)).astype(np.int16)
        if i % 3 == 0:
            signal = real[i % len(real)]
            back = min(int(length), len(signal))
            part[len(part) - back:] = signal[len(signal) - back:]
        reads.append(part)
    return reads


def end_chain(hip, end_model, reads, scan_size):
    """The chain of existing entries on whole reads: the restated end windows of the last cap
    samples, ``model.predict``, ``hip.sweep_windows`` -> (best, margin) [N, steps_e]."""
    size = end_model.input_size
    steps = scan_size // (size // 2)
    cap = scan_size + size // 2
    x = np.concatenate([pair.end_front(read[-cap:] if len(read) else read, len(read), size, steps)
                        for read in reads])
    probs = end_model.predict(x).reshape(len(reads), steps, end_model.n_classes)
    return hip.sweep_windows(end_model, probs)


def expected_calls(start_track, end_track, mode, score_diff=0.5):
    """(end_call, start_call, read_call) per read from the last entries of the two tracks."""
    out = []
    for sb, sm, eb, em in zip(start_track[0], start_track[1], end_track[0], end_track[1]):
        start_call = pair.end_call_of(sb[-1], sm[-1], score_diff)
        end_call = pair.end_call_of(eb[-1], em[-1], score_diff)
        out.append((end_call, start_call, pair.combine(start_call, end_call, mode)))
    return out


@pytest.fixture(scope='module')
def cases(hip, all_signals):
    """name -> (start model, end model, scan size, reads, start tracks, end tracks), made once."""
    made = {}
    for name, ((size, end_size), n_classes, scan_size) in PAIRS.items():
        start = hip.HipModel(general_fixtures.geometry(size, n_classes), device=0)
        end = hip.HipModel(general_fixtures.geometry(end_size, n_classes, name=ENDS, seed=5), device=0)
        reads = tail_reads(end_size, scan_size // (end_size // 2), 11 + n_classes, all_signals)
        made[name] = (start, end, scan_size, reads, live.chain(hip, start, reads, scan_size),
                      end_chain(hip, end, reads, scan_size))
    assert made['mixed-13'][0].kind == hip.KIND_PERSISTENT and made['mixed-13'][1].kind == hip.KIND_GENERAL
    yield made
    for start, end, _, _, _, _ in made.values():
        start.close()
        end.close()


def deliver(session, pieces):
    """Every read on a channel of its own, all at once: round r pushes piece r of every read that
    still has one, END with its last piece.  -> (the last start record, the last end record) of
    every read, and the bytes of every push's start records"""
    last, seen = [None] * len(pieces), []
    for r in range(max(len(p) for p in pieces)):
        channels = [ch for ch, parts in enumerate(pieces) if r < len(parts)]
        results, ends = session.push_pair(channels, [pieces[ch][r] for ch in channels], begin=r == 0,
                                          end=[r == len(pieces[ch]) - 1 for ch in channels])
        seen.append(results.tobytes())
        for ch, result, end in zip(channels, results, ends):
            last[ch] = (result, end)
    return last, seen


# ---- 1: the end track and the calls under every chunking -------------------------------------------
@pytest.mark.parametrize('name', list(PAIRS))
def test_end_track_is_the_chain_of_existing_entries_under_every_chunking(hip, cases, name):
    start, end, scan_size, reads, start_track, (want_best, want_margin) = cases[name]
    end_size = end.input_size
    steps = scan_size // (end_size // 2)
    want = expected_calls(start_track, (want_best, want_margin), 'require_either')
    rng = np.random.default_rng(3)
    per_read = [pair.chunkings(read, end_size, steps, rng) for read in reads]
    names = list(dict.fromkeys(k for c in per_read for k in c))   # (a read too short for one: whole)
    called = 0
    with hip.LiveSession(start, len(reads), scan_size=scan_size, end_model=end) as session:
        assert session.end_steps == steps
        for chunking in names:
            pieces = [c.get(chunking, c['whole']) for c in per_read]
            last, _ = deliver(session, pieces)
            for ch, read in enumerate(reads):
                where = (name, chunking, ch, len(read))
                record, ended = last[ch]
                assert same_track(session.end_track(ch), (want_best[ch], want_margin[ch])), where
                assert ended['status'] == hip.LIVE_FINAL and ended['end_windows'] == steps, where
                assert ended['samples'] == len(read) == record['samples'], where
                assert ended['end_best'] == want_best[ch, -1], where
                assert bits(ended['end_margin']) == bits(want_margin[ch, -1]), where
                assert (ended['end_call'], ended['start_call'], ended['read_call']) == want[ch], where
                assert record['status'] == hip.LIVE_FINAL and record['final_call'] == want[ch][1], where
            called += sum(int(e['end_call']) != 0 for _, e in last)
        # a read that has begun again and not ended: PENDING, no call, no end track
        results, ends = session.push_pair([0, 1], [reads[-1][:100], reads[-2]], begin=True)
        assert (ends['status'] == hip.LIVE_PENDING).all() and (ends['end_call'] == -1).all()
        assert (ends['read_call'] == -1).all() and (ends['end_windows'] == 0).all()
        assert ends['samples'].tolist() == results['samples'].tolist()
        assert len(session.end_track(0)[0]) == 0
        # a chunk for a channel with no read open: IDLE, the record as it stands
        results, ends = session.push_pair([2], [reads[-1]])
        assert ends['status'][0] == hip.LIVE_IDLE and results['status'][0] == hip.LIVE_IDLE
        assert (ends['end_call'][0], ends['start_call'][0], ends['read_call'][0]) == want[2]
        assert same_track(session.end_track(2), (want_best[2], want_margin[2]))
    if name == 'persistent-13':                        # the shipped weights on the spliced ends
        assert called > 0


# ---- 2: the start side is untouched ----------------------------------------------------------------
@pytest.mark.parametrize('stop', [False, True], ids=['run on', 'stop on decision'])
def test_start_records_are_those_of_a_start_only_session(hip, cases, stop):
    for name in ('persistent-13', 'general-33'):
        start, end, scan_size, reads, _, _ = cases[name]
        half = start.input_size // 2
        for size in (1600, half + 1):
            pieces = [ref.chunked(read, size) for read in reads]
            with hip.LiveSession(start, len(reads), scan_size=scan_size, stop_on_decision=stop,
                                 end_model=end) as both, \
                    hip.LiveSession(start, len(reads), scan_size=scan_size,
                                    stop_on_decision=stop) as alone:
                _, seen = deliver(both, pieces)
                for r, got in enumerate(seen):
                    channels = [ch for ch, parts in enumerate(pieces) if r < len(parts)]
                    want = alone.push(channels, [pieces[ch][r] for ch in channels], begin=r == 0,
                                      end=[r == len(pieces[ch]) - 1 for ch in channels])
                    assert got == want.tobytes(), (name, size, r)
                for ch in range(len(reads)):
                    assert same_track(both.track(ch), alone.track(ch)), (name, size, ch)
                # push on a pair session is push_pair without the end records: the end side ran
                again = both.push(list(range(len(reads))), reads, begin=True, end=True)
                want = alone.push(list(range(len(reads))), reads, begin=True, end=True)
                assert again.tobytes() == want.tobytes()
                assert all(len(both.end_track(ch)[0]) == both.end_steps for ch in range(len(reads)))


# ---- 3: the ring goes on behind a stop -------------------------------------------------------------
def test_the_ring_goes_on_behind_a_stop(hip, hip_models, gold):
    start, end = hip_models[STARTS], hip_models[ENDS]
    cap = 6144 + 512
    # a golden read's first cap samples, its middle over again up to 2 cap, then its own last cap
    reads = [np.concatenate([s[:cap], np.resize(s[1000:-1000], 3 * cap - 2 * min(cap, len(s))),
                             s[-cap:]]) for s in gold['signals']]
    assert all(len(read) == 3 * cap for read in reads)
    _, end_calls = end.classify_signals(reads, 'end', 6144, 0.5)
    assert np.count_nonzero(end_calls) >= 3
    with hip.LiveSession(start, 7, stop_on_decision=True, end_model=end) as session:
        last, seen = deliver(session, [ref.chunked(read, 1600) for read in reads])
        first = np.frombuffer(seen[0], dtype=hip.LIVE_RESULT)
        # every read is decided within its first chunk (test_gpu_live: at window 1, 1, 2, 1, 1, 1, 1)
        assert (first['status'] == hip.LIVE_DECIDED).all()
        assert first['windows'].tolist() == [1, 1, 2, 1, 1, 1, 1]
        for ch, (record, ended) in enumerate(last):
            assert record['status'] == hip.LIVE_DECIDED and record['windows'] == first[ch]['windows']
            assert record['final_call'] == -1 and record['samples'] == len(reads[ch])
            assert ended['status'] == hip.LIVE_FINAL and ended['end_call'] == end_calls[ch]
            assert ended['start_call'] == record['call'] == first[ch]['call'] != 0
            assert ended['read_call'] == pair.combine(record['call'], end_calls[ch], 'require_either')
            assert len(session.end_track(ch)[0]) == 12


# ---- 4: against classify ---------------------------------------------------------------------------
def pack(signals):
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
    return np.concatenate(signals).astype(np.int16), offsets


@pytest.mark.parametrize('mode', pair.MODES)
def test_calls_are_classifys_on_the_golden_reads(hip, hip_models, gold, mode):
    start, end, signals = hip_models[STARTS], hip_models[ENDS], gold['signals']
    calls, (start_calls, end_calls), _ = hip.classify_pair(start, end, *pack(signals), 6144, 0.5,
                                                            mode=mode, want_sides=True)
    at = [gold['calls']['read_ids'].index(i) for i in gold['read_ids']]
    number = lambda c: 0 if c == 'none' else int(c)                # noqa: E731
    assert end_calls.tolist() == [number(gold['calls']['EXP-NBD103_read_ends/end'][j]) for j in at]
    with hip.LiveSession(start, 7, end_model=end, combine=mode) as session:
        last, _ = deliver(session, [ref.chunked(s, 1600) for s in signals])
    assert [int(e['end_call']) for _, e in last] == end_calls.tolist()
    assert [int(e['start_call']) for _, e in last] == start_calls.tolist()
    assert [int(e['read_call']) for _, e in last] == calls.tolist()
    tiled = [signals[i % 7] for i in range(64)]
    with hip.LiveSession(start, 64, end_model=end, combine=mode[len('require_'):]) as session:
        last, _ = deliver(session, [[s] for s in tiled])
    assert [int(e['end_call']) for _, e in last] == [end_calls[i % 7] for i in range(64)]
    assert [int(e['read_call']) for _, e in last] == [calls[i % 7] for i in range(64)]


def test_calls_depend_on_neither_channel_nor_what_it_held_before(hip, cases, all_signals):
    start, end, scan_size, _, _, _ = cases['persistent-13']
    reads = tail_reads(1024, scan_size // 512, 21, all_signals, n_random=287)
    assert len(reads) == 300
    by_length = np.argsort([-len(r) for r in reads], kind='stable')
    # three turns through 100 of 3,000 channels: the longest reads, then the shortest ones on the
    # same channels - the ring still holds the long read's tail -, then the ones between
    turns = [by_length[:100], by_length[200:], by_length[100:200]]
    rotating, tracks = {}, {}
    with hip.LiveSession(start, 3000, scan_size=scan_size, end_model=end) as session:
        channels = [(29 * j + 5) % 3000 for j in range(100)]
        for turn in turns:
            mine = [reads[i] for i in turn]
            session.push(channels, [r[:len(r) // 2] for r in mine], begin=True)
            _, ends = session.push_pair(channels, [r[len(r) // 2:] for r in mine], end=True)
            for j, i in enumerate(turn):
                rotating[int(i)], tracks[int(i)] = ends[j].copy(), session.end_track(channels[j])
    with hip.LiveSession(start, 1, scan_size=scan_size, end_model=end) as session:
        for i, read in enumerate(reads):
            _, ends = session.push_pair([0], [read], begin=True, end=True)
            assert ends[0].tobytes() == rotating[i].tobytes(), (i, len(read))
            assert same_track(session.end_track(0), tracks[i]), (i, len(read))
    assert sum(int(e['end_call']) != 0 for e in rotating.values()) > 0


# ---- 5: rounds and LDS state -----------------------------------------------------------------------
@pytest.mark.parametrize('name', ['persistent-13', 'general-33', 'mixed-13'])
def test_forward_rounds_of_any_size_and_any_prior_lds_state_give_the_same(hip, cases, name):
    start, end, scan_size, reads, _, (want_best, want_margin) = cases[name]
    seen = []
    for max_round_windows, pattern in ((1, 0xFFFFFFFF), (5, 0x7FC00000), (0, 0xFFFFFFFF)):
        with hip.LiveSession(start, len(reads), scan_size=scan_size, end_model=end,
                             max_round_windows=max_round_windows) as session:
            filled, total = hip.fill_lds(pattern)
            assert filled == total
            # END flushes every window of both sides in one push: rounds end inside a channel
            results, ends = session.push_pair(list(range(len(reads))), reads, begin=True, end=True)
            for ch in range(len(reads)):
                assert same_track(session.end_track(ch), (want_best[ch], want_margin[ch])), (name, ch)
            seen.append(results.tobytes() + ends.tobytes())
    assert seen[0] == seen[1] == seen[2]


# ---- 6: what is refused ----------------------------------------------------------------------------
def test_a_refused_call_changes_nothing(hip, cases):
    start, end, scan_size, reads, _, (want_best, want_margin) = cases['general-33']
    other = cases['general-2'][1]                                   # another class count
    lib = hip.load_library()
    handle = ctypes.c_void_p(7)
    by = ctypes.byref(handle)
    create = lambda *a: lib.dbh_live_create_pair(*a)               # noqa: E731
    assert create(start.handle, other.handle, 4, scan_size, 0.5, 1, 0, 0, 0, by) == INVALID
    assert create(start.handle, None, 4, scan_size, 0.5, 1, 0, 0, 0, by) == INVALID
    assert create(None, end.handle, 4, scan_size, 0.5, 1, 0, 0, 0, by) == INVALID
    for mode in (-1, 3):
        assert create(start.handle, end.handle, 4, scan_size, 0.5, 1, 0, mode, 0, by) == INVALID
    for scan in (scan_size + 1, 0, -48):
        assert create(start.handle, end.handle, 4, scan, 0.5, 1, 0, 0, 0, by) == INVALID
    # a scan size that the start side takes and the end side does not: h = 512, h_e = 48
    mixed_start, mixed_end = cases['mixed-13'][0], cases['mixed-13'][1]
    assert create(mixed_start.handle, mixed_end.handle, 4, 2048, 0.5, 1, 0, 0, 0, by) == INVALID
    assert create(mixed_end.handle, mixed_start.handle, 4, 48 * 31, 0.5, 1, 0, 0, 0, by) == INVALID
    assert handle.value == 7
    n = 8
    mine = reads[-n:]
    p = lambda a: a.ctypes.data                                    # noqa: E731
    channels = np.arange(4, dtype=np.int32)
    offsets = np.array([0, 100, 200, 300, 400], np.int64)
    samples = np.full(400, 500, np.int16)
    flags = np.full(4, 2, np.uint32)
    results = np.full(4, 9, hip.LIVE_RESULT)
    ends = np.full(4, 9, hip.LIVE_END_RESULT)
    with hip.LiveSession(start, n, scan_size=scan_size) as alone:      # a start-only session
        alone.push(list(range(n)), [r[:len(r) // 2] for r in mine], begin=True)
        before = [alone.track(ch) for ch in range(n)]
        args = [alone.handle, p(channels), p(offsets), p(samples), p(flags), p(results), p(ends), 4]
        assert lib.dbh_live_push_pair(*args) == INVALID
        windows = ctypes.c_int32(-3)
        assert lib.dbh_live_end_track(alone.handle, 0, p(results), p(results),
                                      ctypes.byref(windows)) == INVALID and windows.value == -3
        assert (results['samples'] == 9).all() and (ends['samples'] == 9).all()
        assert all(same_track(alone.track(ch), before[ch]) for ch in range(n))
        last = alone.push(list(range(n)), [r[len(r) // 2:] for r in mine], end=True)
        assert (last['samples'] == [len(r) for r in mine]).all()
    with hip.LiveSession(start, n, scan_size=scan_size, end_model=end) as session:
        session.push(list(range(n)), [r[:len(r) // 2] for r in mine], begin=True)
        before = [session.track(ch) for ch in range(n)]
        good = [session.handle, p(channels), p(offsets), p(samples), p(flags), p(results), p(ends), 4]
        bad_pushes = [(at, None) for at in range(6)] + [(7, -1)]
        for held in (np.array([0, 1, 2, 8], np.int32), np.array([0, -1, 2, 3], np.int32),
                     np.array([0, 1, 2, 1], np.int32)):            # outside the session, twice
            bad_pushes.append((1, held))
        bad_pushes.append((2, np.array([0, 100, 50, 300, 400], np.int64)))      # backwards
        bad_pushes.append((4, np.array([0, 4, 0, 0], np.uint32)))               # an unknown bit
        for at, bad in bad_pushes:
            args = list(good)
            args[at] = p(bad) if isinstance(bad, np.ndarray) else bad
            assert lib.dbh_live_push_pair(*args) == INVALID, (at, bad)
            assert (results['samples'] == 9).all() and (ends['samples'] == 9).all()
            for ch in range(n):
                assert same_track(session.track(ch), before[ch]), (at, bad, ch)
                assert len(session.end_track(ch)[0]) == 0
        assert lib.dbh_live_push_pair(*(good[:7] + [0])) == 0                   # no chunk
        windows = ctypes.c_int32(-3)
        for channel in (-1, n):
            assert lib.dbh_live_end_track(session.handle, channel, p(results), p(results),
                                          ctypes.byref(windows)) == INVALID
        assert windows.value == -3
        # ... and the session goes on as if nothing had been: the reads' other halves, to the bit
        _, ended = session.push_pair(list(range(n)), [r[len(r) // 2:] for r in mine], end=True)
        for ch in range(n):
            i = len(reads) - n + ch
            assert same_track(session.end_track(ch), (want_best[i], want_margin[i]))
            assert ended[ch]['status'] == hip.LIVE_FINAL and ended[ch]['samples'] == len(mine[ch])


# ---- 7: the command --------------------------------------------------------------------------------
def test_replay_both_ends_prints_what_its_host_stand_in_and_classify_print(hip, capsys, monkeypatch):
    import test_live
    import test_live_pair
    from conftest import OracleModel
    from deepbinner_amd import classify, replay
    from deepbinner_amd import deepbinner as cli
    capsys.readouterr()
    cli.main(['replay', '--native', '--both_ends', SINGLE])
    on_device = capsys.readouterr()
    with monkeypatch.context() as patch:
        patch.setattr(classify, 'build_model', lambda w: OracleModel(w))
        replay.replay(test_live_pair.options(), backend=pair.HostBackend())
    on_host = capsys.readouterr()
    assert on_device.out == on_host.out and len(on_host.out.strip().split('\n')) == 8
    assert on_device.err.strip().split('\n')[-1] == on_host.err.strip().split('\n')[-1]
    assert on_device.err.strip().split('\n')[-1].startswith('  barcode on: start only')
    for rule in ('--require_either', '--require_start', '--require_both'):
        cli.main(['replay', '--native', '--both_ends', rule, '--channels', '3', SINGLE])
        _, rows = test_live.table(capsys.readouterr().out)
        cli.main(['classify', '--native', rule, SINGLE])
        header, classified = test_live.table(capsys.readouterr().out)
        assert header == ['read_ID', 'barcode_call']
        assert {row[0]: row[8] for row in rows} == {row[0]: row[1] for row in classified}, rule
