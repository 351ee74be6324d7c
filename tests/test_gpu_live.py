"""Live sessions on the GPU: a channel's track under every chunking against the chain of existing
entries on the whole read, bit for bit; the resumable fold alone, split at every point; the final
calls against ``classify``; channels, rounds, LDS state, STOP_ON_DECISION, what a push refuses; the
``replay`` command beside its host stand-in."""
import ctypes
import os

import numpy as np
import pytest

import general_fixtures
import live_reference as ref
import sweep_reference
from conftest import GOLD

pytestmark = pytest.mark.gpu

SINGLE = os.path.join(GOLD, 'fast5', 'single')
STARTS = 'EXP-NBD103_read_starts'
INVALID = 1
# (kind, class count) -> (input size, scan size): the sweep tests' models
MODELS = {('persistent', 2): (1024, 2048), ('persistent', 13): (1024, 2048),
          ('persistent', 32): (1024, 2048), ('general', 2): (96, 576), ('general', 33): (96, 576),
          ('general', 256): (96, 576)}
MODEL_IDS = ['{}-{}'.format(*key) for key in MODELS]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_track(got, want, windows=None):
    """(best, margin) equal, the margins as bits; ``windows``: that many entries, a prefix of want"""
    n = len(want[0]) if windows is None else windows
    return (len(got[0]) == len(got[1]) == n and np.array_equal(got[0], want[0][:n]) and
            np.array_equal(bits(got[1]), bits(want[1][:n])))


def seam_reads(input_size, steps, seed, real, n_random=30):
    """Reads of every seam length and a few dozen random ones below 2 cap; every third one has a
    golden read's start spliced in front (as test_gpu_sweep.random_reads), so barcodes are called."""
    rng = np.random.default_rng(seed)
    cap = steps * (input_size // 2) + input_size // 2
    lengths = ref.seam_lengths(input_size, steps) + rng.integers(0, 2 * cap, n_random).tolist()
    reads = []
    for i, length in enumerate(lengths):
        part = rng.integers(200, 900, int(length)).astype(np.int16)
        if i % 3 == 0:
            signal = real[i % len(real)]
            front = min(int(length), len(signal))
            part[:front] = signal[:front]
        reads.append(part)
    return reads


def chain(hip, model, reads, scan_size):
    """The chain of existing entries on whole reads: the steps windows of the scan's front rule
    (empty ones all zero), ``model.predict``, ``hip.sweep_windows`` -> (best, margin) [N, steps]."""
    size = model.input_size
    steps = scan_size // (size // 2)
    x = np.concatenate([ref.front(read[:scan_size + size // 2], size, steps) for read in reads])
    probs = model.predict(x).reshape(len(reads), steps, model.n_classes)
    return hip.sweep_windows(model, probs)


@pytest.fixture(scope='module')
def cases(hip, all_signals):
    """(kind, class count) -> (model, scan size, reads, the chain's tracks), made once."""
    made = {}
    for (kind, n_classes), (size, scan_size) in MODELS.items():
        model = hip.HipModel(general_fixtures.geometry(size, n_classes), device=0)
        assert model.kind == (hip.KIND_PERSISTENT if kind == 'persistent' else hip.KIND_GENERAL)
        reads = seam_reads(size, scan_size // (size // 2), 7 + n_classes, all_signals)
        made[kind, n_classes] = (model, scan_size, reads, chain(hip, model, reads, scan_size))
    yield made
    for model, _, _, _ in made.values():
        model.close()


def deliver(session, reads, pieces, end=True, end_alone=False):
    """Every read on a channel of its own, all at once: round r pushes piece r of every read that
    still has one.  -> the last record of every read"""
    last = [None] * len(reads)
    for r in range(max(len(p) for p in pieces) + (1 if end_alone else 0)):
        channels, chunks, begin, ends = [], [], [], []
        for ch, parts in enumerate(pieces):
            final = r == len(parts) - 1
            if r < len(parts):
                chunks.append(parts[r])
                ends.append(end and final and not end_alone)
            elif r == len(parts) and end_alone and end:
                chunks.append(np.zeros(0, np.int16))
                ends.append(True)
            else:
                continue
            channels.append(ch)
            begin.append(r == 0)
        results = session.push(channels, chunks, begin=begin, end=ends)
        for ch, result in zip(channels, results):
            last[ch] = result
    return last


def random_pieces(read, rng):
    cuts = np.sort(rng.integers(0, len(read) + 1, 5))
    cuts = np.concatenate([[0], cuts, [cuts[-1]], [len(read)]])          # (an empty piece among them)
    return [read[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


# ---- 1: chunking invariance and parity -------------------------------------------------------------
@pytest.mark.parametrize('key', list(MODELS), ids=MODEL_IDS)
def test_track_is_the_chain_of_existing_entries_under_every_chunking(hip, cases, key):
    model, scan_size, reads, (want_best, want_margin) = cases[key]
    size, half = model.input_size, model.input_size // 2
    steps = scan_size // half
    rng = np.random.default_rng(3)
    chunkings = {'whole': [[read] for read in reads]}
    for step in [half - 1, half, half + 1, 3 * half, 1600] + ([1] if size == 96 else []):
        chunkings[step] = [ref.chunked(read, step) for read in reads]
    chunkings['random'] = [random_pieces(read, rng) for read in reads]
    called = 0
    with hip.LiveSession(model, len(reads), scan_size=scan_size) as session:
        for name, pieces in chunkings.items():
            for end_alone in ((False, True) if name in ('whole', half, 'random') else (False,)):
                last = deliver(session, reads, pieces, end_alone=end_alone)
                for ch, read in enumerate(reads):
                    where = (key, name, end_alone, ch, len(read))
                    assert same_track(session.track(ch), (want_best[ch], want_margin[ch])), where
                    assert last[ch]['status'] == hip.LIVE_FINAL and last[ch]['windows'] == steps, where
                    assert last[ch]['samples'] == len(read), where
                    assert last[ch]['best'] == want_best[ch, -1], where
                    assert bits(last[ch]['margin']) == bits(want_margin[ch, -1]), where
                called += sum(int(r['call']) != 0 for r in last)
        # a read that is never ended: the windows that are complete, the same bits
        deliver(session, reads, chunkings[1600], end=False)
        for ch, read in enumerate(reads):
            windows = min(steps, max(0, (len(read) - size) // half + 1))
            assert same_track(session.track(ch), (want_best[ch], want_margin[ch]), windows), (key, ch)
    if key == ('persistent', 13):                      # the shipped model on the spliced starts
        assert called > 0


# ---- 2: the fold alone -----------------------------------------------------------------------------
@pytest.mark.parametrize('key', list(MODELS), ids=MODEL_IDS)
def test_fold_resumes_at_every_split_point(hip, cases, key):
    model, scan_size = cases[key][0], cases[key][1]
    K, C = scan_size // (model.input_size // 2), model.n_classes
    probs = sweep_reference.hand_made(C, K, seed=5)                 # [12, K, C]
    n = len(probs)
    want_best, want_margin = sweep_reference.sweep(probs)
    _, one_state, one_best, one_margin = hip.live_fold(model, probs.reshape(-1, C), [K] * n, K)
    assert np.array_equal(one_best, want_best)
    # 256 fp64 additions of values <= 1, a division and a product: far inside 1e-12 (the sweep's bound)
    assert np.abs(one_margin - want_margin).max() <= 1e-12
    assert (one_state['windows'] == K).all() and (one_state['status'] == hip.LIVE_FINAL).all()
    splits = [[j] * n for j in range(K + 1)] + [[(3 * i + 1) % (K + 1) for i in range(n)]]
    for first in splits:
        head = np.concatenate([probs[i, :first[i]] for i in range(n)])
        tail = np.concatenate([probs[i, first[i]:] for i in range(n)])
        merged, state, best_a, margin_a = hip.live_fold(model, head, first, K)
        assert state['windows'].tolist() == first
        _, state, best_b, margin_b = hip.live_fold(model, tail, [K - j for j in first], K,
                                                   merged=merged, state=state)
        for i in range(n):
            best = np.concatenate([best_a[i, :first[i]], best_b[i, first[i]:]])
            margin = np.concatenate([margin_a[i, :first[i]], margin_b[i, first[i]:]])
            assert same_track((best, margin), (one_best[i], one_margin[i])), (key, first[i], i)
        assert state.tobytes() == one_state.tobytes(), (key, first)
    # the decision: the records the restatement makes of the device's own track
    moving = 4                                          # the row whose maximum moves on
    threshold = float(min(one_margin[moving, 0], one_margin[moving, -1]))
    for options in (dict(score_diff=0.5), dict(score_diff=threshold),
                    dict(score_diff=threshold, min_windows=2),
                    dict(score_diff=threshold, min_windows=K),
                    dict(score_diff=threshold, stop_on_decision=True)):
        state = hip.live_fold(model, probs.reshape(-1, C), [K] * n, K, **options)[1]
        for i in range(n):
            want = ref.plan(model.input_size, scan_size, [0], [ref.BEGIN | ref.END], one_best[i],
                            one_margin[i], **options)[0][0]
            for field in ('call', 'final_call', 'windows', 'decided_windows', 'best'):
                assert state[i][field] == want[field], (key, options, i, field)
            assert bits(state[i]['margin']) == bits(want['margin'])
            assert state[i]['status'] == want['status'], (key, options, i)
        m = options.get('min_windows', 1)
        # min_windows = m never decides before window m, and decides at m when the rule already held
        assert (state['decided_windows'][state['decided_windows'] > 0] >= m).all()
        if ('stop_on_decision' not in options and options['score_diff'] == threshold and
                (one_best[moving] != 0).all()):    # (256 classes: class 0 leads the later prefixes)
            assert state[moving]['decided_windows'] == m
            assert state[moving]['call'] == one_best[moving, m - 1]
            assert state[moving]['final_call'] == one_best[moving, -1]
    # the maximum moves on: the call stays the first class, the final call is the later one
    state = hip.live_fold(model, probs.reshape(-1, C), [K] * n, K, score_diff=threshold)[1]
    assert state[moving]['call'] == 1 and state[moving]['decided_windows'] == 1
    if C > 2:
        assert state[moving]['final_call'] == one_best[moving, -1] != 1
    # a margin exactly equal to score_diff decides, the next double above it does not
    at = float(one_margin[moving, 0])
    state = hip.live_fold(model, probs.reshape(-1, C), [K] * n, K, score_diff=at)[1]
    assert state[moving]['decided_windows'] == 1
    state = hip.live_fold(model, probs.reshape(-1, C), [K] * n, K,
                          score_diff=float(np.nextafter(at, np.inf)))[1]
    assert state[moving]['decided_windows'] != 1


# ---- 3: against classify ---------------------------------------------------------------------------
def test_final_calls_are_classifys_on_the_golden_reads(hip, hip_models, gold):
    model, signals = hip_models[STARTS], gold['signals']
    _, calls = model.classify_signals(signals, 'start', 6144, 0.5)
    assert calls.tolist() == [3, 2, 3, 1, 1, 2, 12]
    with hip.LiveSession(model, 7) as session:
        last = deliver(session, signals, [ref.chunked(s, 1600) for s in signals])
    assert [int(r['final_call']) for r in last] == calls.tolist()
    assert [int(r['call']) for r in last] == calls.tolist()
    assert [int(r['decided_windows']) for r in last] == [1, 1, 2, 1, 1, 1, 1]
    assert all(r['decided_samples'] == 1600 for r in last)
    tiled = [signals[i % 7] for i in range(64)]
    with hip.LiveSession(model, 64) as session:
        last = deliver(session, tiled, [[s] for s in tiled])
    assert [int(r['final_call']) for r in last] == [calls[i % 7] for i in range(64)]
    assert [int(r['decided_windows']) for r in last] == [[1, 1, 2, 1, 1, 1, 1][i % 7] for i in range(64)]


# ---- 4: channels -----------------------------------------------------------------------------------
def test_tracks_depend_on_neither_channel_nor_what_it_held_before(hip, cases, all_signals):
    model, scan_size, _, _ = cases['persistent', 13]
    size, steps = 1024, scan_size // 512
    reads = seam_reads(size, steps, 21, all_signals, n_random=288)
    assert len(reads) == 300
    want_best, want_margin = chain(hip, model, reads, scan_size)
    tracks = {}
    # 3,000 channels, the reads rotating through 100 of them in three turns, each in two pushes
    with hip.LiveSession(model, 3000, scan_size=scan_size) as session:
        channels = [(29 * j + 5) % 3000 for j in range(100)]
        for turn in range(3):
            mine = reads[100 * turn:100 * turn + 100]
            session.push(channels, [r[:len(r) // 2] for r in mine], begin=True)
            session.push(channels, [r[len(r) // 2:] for r in mine], end=True)
            for j, ch in enumerate(channels):
                tracks['rotating', 100 * turn + j] = session.track(ch)
        # one push with zero new windows everywhere, one with three new windows per channel
        long = [r for r in reads if len(r) >= size + 2 * 512][:50]
        channels = list(range(2000, 2000 + len(long)))
        first = session.push(channels, [r[:size - 1] for r in long], begin=True)
        assert (first['windows'] == 0).all() and (first['status'] == hip.LIVE_PENDING).all()
        second = session.push(channels, [r[size - 1:size + 2 * 512] for r in long])
        assert (second['windows'] == 3).all() and (second['samples'] == size + 1024).all()
        for ch, read in zip(channels, long):
            i = next(i for i, r in enumerate(reads) if r is read)
            assert same_track(session.track(ch), (want_best[i], want_margin[i]), 3)
    # another session, the reads in another channel order, whole
    with hip.LiveSession(model, 300, scan_size=scan_size) as session:
        order = list(range(299, -1, -1))
        session.push(order, reads, begin=True, end=True)
        for ch, i in zip(order, range(300)):
            tracks['reversed', i] = session.track(ch)
    # one channel, one read after the other
    with hip.LiveSession(model, 1, scan_size=scan_size) as session:
        for i, read in enumerate(reads):
            session.push([0], [read], begin=True, end=True)
            tracks['alone', i] = session.track(0)
    for i in range(300):
        for case in ('rotating', 'reversed', 'alone'):
            assert same_track(tracks[case, i], (want_best[i], want_margin[i])), (case, i, len(reads[i]))


# ---- 5: rounds -------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', list(MODELS), ids=MODEL_IDS)
def test_forward_rounds_of_any_size_give_the_same(hip, cases, key):
    model, scan_size, reads, (want_best, want_margin) = cases[key]
    seen = []
    for max_round_windows in (1, 5, 0):
        with hip.LiveSession(model, len(reads), scan_size=scan_size,
                             max_round_windows=max_round_windows) as session:
            # END flushes every window of every read in one push: rounds end inside a channel
            results = session.push(list(range(len(reads))), reads, begin=True, end=True)
            for ch in range(len(reads)):
                assert same_track(session.track(ch), (want_best[ch], want_margin[ch])), (key, ch)
            seen.append(results.tobytes())
    assert seen[0] == seen[1] == seen[2]


# ---- 6: LDS state ----------------------------------------------------------------------------------
@pytest.mark.parametrize('key', [('persistent', 13), ('general', 33)], ids=['persistent-13', 'general-33'])
def test_tracks_hold_to_any_prior_lds_state(hip, cases, key):
    model, scan_size, reads, (want_best, want_margin) = cases[key]
    for pattern in (0xFFFFFFFF, 0x7FC00000):
        with hip.LiveSession(model, len(reads), scan_size=scan_size) as session:
            seen, total = hip.fill_lds(pattern)
            assert seen == total
            session.push(list(range(len(reads))), reads, begin=True, end=True)
            for ch in range(len(reads)):
                assert same_track(session.track(ch), (want_best[ch], want_margin[ch])), (key, pattern, ch)


# ---- 7: STOP_ON_DECISION ---------------------------------------------------------------------------
def test_stop_on_decision_runs_nothing_behind_the_decision(hip, hip_models, gold):
    model, signals = hip_models[STARTS], gold['signals']
    pieces = [ref.chunked(s[:8000], 512) for s in signals]
    with hip.LiveSession(model, 7, stop_on_decision=True) as stopping, \
            hip.LiveSession(model, 7) as running:
        decided = {}
        for r in range(max(len(p) for p in pieces)):
            channels = [ch for ch in range(7) if r < len(pieces[ch])]
            chunks = [pieces[ch][r] for ch in channels]
            ends = [r == len(pieces[ch]) - 1 for ch in channels]
            got = stopping.push(channels, chunks, begin=r == 0, end=ends)
            ran = running.push(channels, chunks, begin=r == 0, end=ends)
            for ch, a, b in zip(channels, got, ran):
                assert a['samples'] == b['samples']
                if ch in decided:          # later chunks: DECIDED, the same call, nothing grows
                    first, track = decided[ch]
                    assert a['status'] == hip.LIVE_DECIDED and a['call'] == first['call']
                    assert a['windows'] == first['windows'] == first['decided_windows']
                    assert a['decided_samples'] == first['decided_samples'] and a['final_call'] == -1
                    assert same_track(stopping.track(ch), track)
                elif a['status'] == hip.LIVE_DECIDED:
                    decided[ch] = (a.copy(), stopping.track(ch))
                    assert a['call'] == b['call'] and a['decided_windows'] == b['decided_windows']
                    assert a['decided_samples'] == b['decided_samples'] == a['samples']
                else:
                    assert a['status'] == hip.LIVE_PENDING and a.tobytes() == b.tobytes()
                if ends[channels.index(ch)]:           # without the flag the same inputs reach FINAL
                    assert b['status'] == hip.LIVE_FINAL and b['windows'] == 12
                    assert b['call'] == a['call']
        assert sorted(decided) == list(range(7))
        assert [int(decided[ch][0]['windows']) for ch in range(7)] == [1, 1, 2, 1, 1, 1, 1]


# ---- 8: argument checks ----------------------------------------------------------------------------
def test_a_refused_push_changes_nothing(hip, cases):
    model, scan_size, reads, (want_best, want_margin) = cases['general', 33]
    lib = hip.load_library()
    handle = ctypes.c_void_p(7)
    for channels, scan, min_windows, flags in ((0, scan_size, 1, 0), (16385, scan_size, 1, 0),
                                               (4, scan_size + 1, 1, 0), (4, 0, 1, 0), (4, -48, 1, 0),
                                               (4, scan_size, 0, 0), (4, scan_size, 13, 0),
                                               (4, scan_size, 1, 2)):
        assert lib.dbh_live_create(model.handle, channels, scan, 0.5, min_windows, flags, 0,
                                   ctypes.byref(handle)) == INVALID
    assert lib.dbh_live_create(None, 4, scan_size, 0.5, 1, 0, 0, ctypes.byref(handle)) == INVALID
    assert lib.dbh_live_create(model.handle, 4, scan_size, 0.5, 1, 0, 0, None) == INVALID
    assert handle.value == 7
    n = 8
    with hip.LiveSession(model, n, scan_size=scan_size) as session:
        session.push(list(range(n)), [r[:len(r) // 2] for r in reads[-n:]], begin=True)
        before = [session.track(ch) for ch in range(n)]
        channels = np.arange(4, dtype=np.int32)
        offsets = np.array([0, 100, 200, 300, 400], np.int64)
        samples = np.full(400, 500, np.int16)
        flags = np.zeros(4, np.uint32)
        results = np.full(4, 9, hip.LIVE_RESULT)
        p = lambda a: a.ctypes.data                                # noqa: E731
        good = [session.handle, p(channels), p(offsets), p(samples), p(flags), p(results), 4]
        bad_pushes = [(at, None) for at in range(6)] + [(6, -1)]
        for held in (np.array([0, 1, 2, 8], np.int32), np.array([0, -1, 2, 3], np.int32),
                     np.array([0, 1, 2, 1], np.int32)):            # outside the session, twice
            bad_pushes.append((1, held))
        bad_pushes.append((2, np.array([0, 100, 50, 300, 400], np.int64)))      # backwards
        bad_pushes.append((4, np.array([0, 4, 0, 0], np.uint32)))               # an unknown bit
        for at, bad in bad_pushes:
            args = list(good)
            args[at] = p(bad) if isinstance(bad, np.ndarray) else bad
            assert lib.dbh_live_push(*args) == INVALID, (at, bad)
            assert (results['samples'] == 9).all()
            for ch in range(n):                                    # the tracks of all channels
                assert same_track(session.track(ch), before[ch]), (at, bad, ch)
        assert lib.dbh_live_push(*(good[:6] + [0])) == 0                        # no chunk
        for ch in range(n):
            assert same_track(session.track(ch), before[ch])
        # ... and the session goes on as if nothing had been: the reads' other halves, to the bit
        session.push(list(range(n)), [r[len(r) // 2:] for r in reads[-n:]], end=True)
        for ch in range(n):
            i = len(reads) - n + ch
            assert same_track(session.track(ch), (want_best[i], want_margin[i]))
        windows = ctypes.c_int32(-3)
        for channel in (-1, n):
            assert lib.dbh_live_track(session.handle, channel, p(results), p(results),
                                      ctypes.byref(windows)) == INVALID
        assert lib.dbh_live_track(session.handle, 0, None, p(results), ctypes.byref(windows)) == INVALID
        assert windows.value == -3


# ---- 9: the command --------------------------------------------------------------------------------
def test_replay_prints_what_its_host_stand_in_prints(hip, capsys, monkeypatch):
    import test_live
    from conftest import OracleModel
    from deepbinner_amd import classify, replay
    from deepbinner_amd import deepbinner as cli
    capsys.readouterr()
    cli.main(['replay', '--native', SINGLE])
    on_device = capsys.readouterr().out
    cli.main(['replay', '--native', '--chunk_samples', '512', '--channels', '3', SINGLE])
    other = capsys.readouterr().out
    with monkeypatch.context() as patch:
        patch.setattr(classify, 'build_model', lambda w: OracleModel(w))
        replay.replay(test_live.options(), backend=ref.HostBackend())
    on_host = capsys.readouterr().out
    assert on_device == on_host and len(on_host.strip().split('\n')) == 8
    columns = lambda text: [[row[i] for i in (0, 1, 2, 4)]         # noqa: E731
                            for row in test_live.table(text)[1]]
    assert columns(other) == columns(on_device)
