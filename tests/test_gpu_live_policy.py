"""Yield policies of live sessions on the GPU: the two policy kernels alone against the NumPy
restatement at every chunk and class count at which their loops and reductions change, actions as
bytes and yields as integers; sessions of both model kinds and pair sessions under three policies -
actions and yields the restatement's on the session's own records, records and tracks byte for byte
those of a session without a policy; the action read with the next push; seeded yields; what is
refused; the golden reads; ``replay --native`` with a policy beside its host stand-in."""
import os

import numpy as np
import pytest

import general_fixtures
import live_policy_reference as pol
import live_reference as ref
import test_gpu_live as live
from conftest import GOLD

pytestmark = pytest.mark.gpu

SINGLE = os.path.join(GOLD, 'fast5', 'single')
STARTS, ENDS = 'EXP-NBD103_read_starts', 'EXP-NBD103_read_ends'
INVALID = 1
BIG = (1 << 45) + 3
CHUNK_COUNTS = [1, 255, 256, 257, 1023, 1024, 1025, 2049, 16384]
CLASS_COUNTS = [2, 13, 33, 64, 65, 256]
# name -> (input size, class count, scan size): models the live tests already use
MODELS = {'general-2': (96, 2, 576), 'general-33': (96, 33, 576), 'persistent-13': (1024, 13, 2048)}
same_track = live.same_track


# ---- 1: the two kernels alone ----------------------------------------------------------------------
def random_weights(rng, n_classes):
    weights = rng.choice([-1, 0, 1, 2, 7, 1 << 20], n_classes).astype(np.int32)
    weights[0] = -1
    weights[-1] = 3                                                # (one balanced class at least)
    return weights


def random_push(rng, n, n_classes, n_channels, ending=None, klass=None):
    """(channels, flags, records) of one push as a session reports it."""
    records = np.zeros(n, dtype=ref.RESULT)
    records['status'] = rng.integers(0, 4, n)
    call = rng.integers(0, n_classes, n) if klass is None else np.full(n, klass)
    if klass is not None:
        records['status'] = np.maximum(records['status'], ref.DECIDED)
    records['call'] = np.where(records['status'] == ref.PENDING, 0, call)
    records['decided_windows'] = records['call'] != 0
    records['final_call'] = -1
    records['samples'] = rng.integers(0, 1 << 34, n)
    flags = rng.integers(0, 4, n).astype(np.uint32)
    if ending is not None:
        flags = (flags & ref.BEGIN) | (ref.END if ending else 0)
    return rng.permutation(n_channels)[:n].astype(np.int32), flags.astype(np.uint32), records


def on_device_and_restated(hip, pushes, weights, n_channels, **options):
    """Every push through ``live_policy_dev`` - yields and standing actions handed on from push to
    push - and through the restatement: actions as bytes, yields and standing actions as integers.
    -> the device's actions per push"""
    seed = {k: options.pop(k) for k in ('yield_samples', 'yield_reads') if k in options}
    want = pol.Policy(weights, n_channels, **options, **seed)
    samples, reads = want.yields()
    standing = np.zeros(n_channels, np.int32)
    out = []
    for p, (channels, flags, records) in enumerate(pushes):
        actions, samples, reads, standing = hip.live_policy_dev(
            records, flags, channels, weights, yield_samples=samples, yield_reads=reads,
            channel_action=standing, **options)
        restated = want.push(channels, flags, records)
        assert actions.dtype == hip.LIVE_ACTION == pol.ACTION
        assert actions.tobytes() == restated.tobytes(), (p, len(channels), len(weights))
        assert samples.tolist() == want.samples and reads.tolist() == want.reads, (p, len(weights))
        assert standing.tolist() == want.action, p
        out.append(actions)
    return out


@pytest.mark.parametrize('n_chunks', CHUNK_COUNTS)
def test_kernels_alone_at_every_chunk_and_class_count(hip, n_chunks):
    rng = np.random.default_rng(n_chunks)
    n_channels = n_chunks + 7
    reasons = set()
    for n_classes in CLASS_COUNTS:
        weights = random_weights(rng, n_classes)
        pushes = [random_push(rng, n_chunks, n_classes, n_channels) for _ in range(2)]
        options = dict(slack_samples=int(rng.choice([0, 1 << 20])),
                       undecided=str(rng.choice(['keep', 'eject'])),
                       yield_samples=rng.choice([0, 1 << 33, BIG], n_classes))
        for actions in on_device_and_restated(hip, pushes, weights, n_channels, **options):
            reasons |= set(actions['reason'].tolist())
    if n_chunks >= 255:
        assert reasons == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize('n_chunks,n_classes', [(16384, 256), (1025, 13), (257, 2)])
def test_kernels_alone_one_class_all_ending_none_ending_and_beyond_32_bits(hip, n_chunks, n_classes):
    rng = np.random.default_rng(n_classes)
    weights = np.full(n_classes, 1, np.int32)
    weights[0] = -1
    top = n_classes - 1
    seeded = dict(yield_samples=np.full(n_classes, BIG), yield_reads=np.full(n_classes, BIG))
    # every chunk the same class, every one ending: one workgroup's sum holds them all
    push = random_push(rng, n_chunks, n_classes, n_chunks, ending=True, klass=top)
    total = int(push[2]['samples'].astype(object).sum())
    assert total > 1 << 32 or n_chunks < 16
    for options in (dict(), seeded):
        actions, = on_device_and_restated(hip, [push], weights, n_chunks, **options)
        base = BIG if options else 0
        # (two classes: the one balanced class is its own floor)
        reason, floor = (pol.OVER_LEVEL, base) if n_classes > 2 else (pol.BALANCED, base + total)
        assert (actions['reason'] == reason).all() and (actions['klass'] == top).all()
        assert (actions['level'] == base + total).all() and (actions['floor'] == floor).all()
    # every chunk ending, of every class; none ending: the yields stay what they were
    on_device_and_restated(hip, [random_push(rng, n_chunks, n_classes, n_chunks, ending=True)],
                           weights, n_chunks, **seeded)
    none = random_push(rng, n_chunks, n_classes, n_chunks, ending=False)
    _, samples, reads, _ = hip.live_policy_dev(none[2], none[1], none[0], weights, **seeded)
    assert samples.tolist() == [BIG] * n_classes and reads.tolist() == [BIG] * n_classes
    on_device_and_restated(hip, [none], weights, n_chunks, **seeded)


def test_kernels_alone_the_chunk_table_in_two_orders(hip):
    rng = np.random.default_rng(2)
    n, n_classes = 2049, 33
    weights = random_weights(rng, n_classes)
    channels, flags, records = random_push(rng, n, n_classes, n)
    seen = []
    for order in (np.arange(n), rng.permutation(n)):
        actions, samples, reads, standing = hip.live_policy_dev(
            records[order], flags[order], channels[order], weights, slack_samples=5,
            yield_samples=np.full(n_classes, 1 << 33))
        by_channel = np.zeros(n, hip.LIVE_ACTION)
        by_channel[channels[order]] = actions
        seen.append((by_channel.tobytes(), samples.tolist(), reads.tolist(), standing.tolist()))
    assert seen[0] == seen[1]


# ---- 2: sessions -----------------------------------------------------------------------------------
def policies(n_classes):
    """Three policies: every barcode balanced; every kind of weight with slack, undecided ejected;
    no balanced class at all."""
    balanced = np.full(n_classes, 1, np.int32)
    mixed = np.resize(np.array([7, 0, -1, 1 << 20, 1], np.int32), n_classes)
    unbalanced = np.resize(np.array([0, -1], np.int32), n_classes)
    for weights in (balanced, mixed, unbalanced):
        weights[0] = -1
    return [dict(weights=balanced), dict(weights=mixed, slack_samples=1000, undecided='eject'),
            dict(weights=unbalanced, undecided='eject')]


def rotation(reads, rng):
    """Pushes of 300 reads through 100 of 3,000 channels: three turns, each read in two halves -
    BEGIN, then END -, the channels of a push in random order."""
    channels = np.array([(29 * j + 5) % 3000 for j in range(100)])
    pushes = []
    for turn in range(3):
        mine = reads[100 * turn:100 * turn + 100]
        for half in (0, 1):
            order = rng.permutation(100)
            cut = lambda r: r[:len(r) // 2] if half == 0 else r[len(r) // 2:]      # noqa: E731
            pushes.append((channels[order].tolist(), [cut(mine[j]) for j in order],
                           half == 0, half == 1))
    return pushes


@pytest.fixture(scope='module')
def models(hip):
    made = {name: hip.HipModel(general_fixtures.geometry(size, n_classes), device=0)
            for name, (size, n_classes, _) in MODELS.items()}
    made['end-13'] = hip.HipModel(general_fixtures.geometry(1024, 13, name=ENDS, seed=5), device=0)
    yield made
    for model in made.values():
        model.close()


def flags_of(n, begin, end):
    return np.full(n, ref.BEGIN * bool(begin) + ref.END * bool(end), np.uint32)


def run_policies(hip, model, scan_size, reads, end_model=None):
    """The rotation through a session without a policy, then through one per policy: records (and
    end records) byte for byte, tracks equal, actions and yields the restatement's on the session's
    own records.  -> the reasons seen"""
    pushes = rotation(reads, np.random.default_rng(9))
    pair = dict(end_model=end_model) if end_model is not None else {}
    plain, tracks = [], []
    with hip.LiveSession(model, 3000, scan_size=scan_size, **pair) as session:
        for channels, chunks, begin, end in pushes:
            if end_model is not None:
                results, ends = session.push_pair(channels, chunks, begin=begin, end=end)
                plain.append(results.tobytes() + ends.tobytes())
            else:
                plain.append(session.push(channels, chunks, begin=begin, end=end).tobytes())
            tracks.append([session.track(ch) for ch in channels[:5]])
    reasons = set()
    for policy in policies(model.n_classes):
        want = pol.Policy(n_channels=3000, **policy)
        with hip.LiveSession(model, 3000, scan_size=scan_size, policy=policy, **pair) as session:
            for p, (channels, chunks, begin, end) in enumerate(pushes):
                results, ends, actions = session.push_policy(channels, chunks, begin=begin, end=end)
                both = results.tobytes() + (ends.tobytes() if end_model is not None else b'')
                assert (ends is None) == (end_model is None)
                assert both == plain[p], p
                restated = want.push(channels, flags_of(len(channels), begin, end), results)
                assert actions.tobytes() == restated.tobytes(), p
                samples, counts = session.yields()
                assert samples.tolist() == want.samples and counts.tolist() == want.reads, p
                for ch, track in zip(channels[:5], tracks[p]):
                    assert same_track(session.track(ch), track), (p, ch)
                reasons |= set(actions['reason'].tolist())
            assert sum(want.reads) == 300 and sum(want.samples) == sum(len(r) for r in reads)
    return reasons


@pytest.mark.parametrize('name', list(MODELS))
def test_sessions_under_three_policies(hip, models, all_signals, name):
    size, n_classes, scan_size = MODELS[name]
    reads = live.seam_reads(size, scan_size // (size // 2), 31 + n_classes, all_signals, n_random=288)
    assert len(reads) == 300
    reasons = run_policies(hip, models[name], scan_size, reads)
    assert 0 in reasons
    if name == 'persistent-13':                                    # the shipped weights call barcodes
        assert reasons - {0, pol.UNDECIDED}, reasons


def test_pair_session_under_three_policies(hip, models, all_signals):
    reads = live.seam_reads(1024, 4, 44, all_signals, n_random=288)
    reasons = run_policies(hip, models['persistent-13'], 2048, reads, end_model=models['end-13'])
    assert reasons - {0, pol.UNDECIDED}, reasons


def test_the_action_arrives_with_the_next_push_and_seeded_yields_count(hip, hip_models, gold):
    model, signals = hip_models[STARTS], gold['signals']
    calls = [3, 2, 3, 1, 1, 2, 12]
    weights = np.full(13, -1, np.int32)
    weights[[1, 2, 3, 12]] = 1
    channels = list(range(7))
    with hip.LiveSession(model, 7, policy=dict(weights=weights)) as session:
        seed = np.zeros(13, np.int64)
        seed[[1, 2, 3, 12]] = [BIG, BIG + 1, BIG, BIG]
        session.set_yields(seed, np.arange(13))
        want = pol.Policy(weights, 7, yield_samples=seed, yield_reads=np.arange(13))
        # push runs the policy; its actions are read with the channels' next push
        results = session.push(channels, [s[:1600] for s in signals], begin=True)
        restated = want.push(channels, flags_of(7, True, False), results)
        assert results['call'].tolist() == calls
        assert restated['action'].tolist() == [1, 2, 1, 1, 1, 2, 1]       # barcode 2 is one ahead
        assert restated['level'].tolist() == [BIG, BIG + 1, BIG, BIG, BIG, BIG + 1, BIG]
        empty = [np.zeros(0, np.int16)] * 7
        results, ends, actions = session.push_policy(channels, empty)
        assert ends is None
        standing = want.push(channels, flags_of(7, False, False), results)
        assert actions.tobytes() == standing.tobytes()
        assert actions['action'].tolist() == restated['action'].tolist() and not actions['reason'].any()
        # END: the yields grow from the seed by what arrived
        results, _, actions = session.push_policy(channels, empty, end=True)
        assert actions.tobytes() == want.push(channels, flags_of(7, False, True), results).tobytes()
        samples, reads = session.yields()
        assert samples.tolist() == want.samples and reads.tolist() == want.reads
        assert samples[3] == BIG + 3200 and reads[3] == 3 + 2 and samples[2] == BIG + 1 + 3200
        # an IDLE chunk reports what stands; BEGIN clears it
        results, _, actions = session.push_policy([1], [signals[1][:10]])
        assert results['status'][0] == hip.LIVE_IDLE and actions[0].tolist() == (2, 0, 0, 0, 0, 0)
        results, _, actions = session.push_policy([1], [signals[1][:10]], begin=True)
        assert actions[0].tolist() == (0, 0, 0, 0, 0, 0)


# ---- 3: what is refused ----------------------------------------------------------------------------
def test_a_refused_call_changes_nothing(hip, models):
    model, other = models['general-33'], models['general-2']
    lib = hip.load_library()
    p = lambda a: a.ctypes.data                                    # noqa: E731
    weights = policies(33)[0]['weights']
    reads = [np.full(600, 500 + 10 * i, np.int16) for i in range(4)]
    channels = np.arange(4, dtype=np.int32)
    offsets = np.array([0, 100, 200, 300, 400], np.int64)
    samples = np.full(400, 500, np.int16)
    flags = np.full(4, 2, np.uint32)
    results = np.full(4, 9, hip.LIVE_RESULT)
    ends = np.full(4, 9, hip.LIVE_END_RESULT)
    actions = np.full(4, 9, hip.LIVE_ACTION)
    with hip.LiveSession(model, 4, scan_size=576) as plain:        # a session without a policy
        args = [plain.handle, p(channels), p(offsets), p(samples), p(flags), p(results), None, p(actions), 4]
        assert lib.dbh_live_push_policy(*args) == INVALID
        assert lib.dbh_live_yield(plain.handle, p(offsets), p(offsets)) == INVALID
        assert lib.dbh_live_set_yield(plain.handle, p(offsets), p(offsets)) == INVALID
        # what set_policy refuses leaves the session without one
        for bad in (np.r_[0, weights[1:]], np.r_[weights[:-1], -2], np.r_[weights[:-1], (1 << 20) + 1]):
            held = np.ascontiguousarray(bad, dtype=np.int32)
            assert lib.dbh_live_set_policy(plain.handle, p(held), 33, 0, 1) == INVALID
        assert lib.dbh_live_set_policy(plain.handle, p(weights), 32, 0, 1) == INVALID
        assert lib.dbh_live_set_policy(plain.handle, p(weights), 33, -1, 1) == INVALID
        assert lib.dbh_live_set_policy(plain.handle, p(weights), 33, 0, 0) == INVALID
        assert lib.dbh_live_set_policy(plain.handle, None, 33, 0, 1) == INVALID
        assert lib.dbh_live_push_policy(*args) == INVALID and (actions['level'] == 9).all()
        plain.push([0], [reads[0]], begin=True)
        assert lib.dbh_live_set_policy(plain.handle, p(weights), 33, 0, 1) == INVALID   # after a push
        assert (results['samples'] == 9).all()
    with pytest.raises(hip.HipBackendError):
        hip.LiveSession(other, 4, scan_size=576, policy=dict(weights=weights))          # 33 weights, 2 classes
    with hip.LiveSession(model, 4, scan_size=576, policy=dict(weights=weights)) as session:
        assert lib.dbh_live_set_policy(session.handle, p(weights), 33, 0, 1) == INVALID  # once
        session.set_yields(np.arange(33) * 1000, np.arange(33))
        _, _, before = session.push_policy(list(range(4)), reads, begin=True)
        good = [session.handle, p(channels), p(offsets), p(samples), p(flags), p(results), None,
                p(actions), 4]
        bad_pushes = [(at, None) for at in (0, 1, 2, 3, 4, 5, 7)] + [(6, p(ends)), (8, -1), (8, 5)]
        bad_pushes += [(1, np.array([0, 1, 2, 4], np.int32)), (1, np.array([0, 1, 1, 2], np.int32)),
                       (2, np.array([0, 100, 50, 300, 400], np.int64)),
                       (4, np.array([0, 4, 0, 0], np.uint32))]
        negative = np.arange(33, dtype=np.int64)
        negative[5] = -1
        positive = np.abs(negative)
        for at, bad in bad_pushes:
            args = list(good)
            args[at] = p(bad) if isinstance(bad, np.ndarray) else bad
            assert lib.dbh_live_push_policy(*args) == INVALID, (at, bad)
        assert lib.dbh_live_set_yield(session.handle, p(negative), p(offsets)) == INVALID
        assert lib.dbh_live_set_yield(session.handle, p(positive), p(negative)) == INVALID
        assert lib.dbh_live_set_yield(session.handle, None, p(negative)) == INVALID
        assert (results['samples'] == 9).all() and (actions['level'] == 9).all()
        samples_now, reads_now = session.yields()
        assert samples_now.tolist() == (np.arange(33) * 1000).tolist()
        assert reads_now.tolist() == list(range(33))
        assert lib.dbh_live_push_policy(*(good[:8] + [0])) == 0                      # no chunk
        # the session goes on as if nothing had been: the standing actions, then the ENDs
        _, _, standing = session.push_policy(list(range(4)), [r[:0] for r in reads])
        assert standing['action'].tolist() == before['action'].tolist()
        results_end, _, _ = session.push_policy(list(range(4)), [r[:0] for r in reads], end=True)
        assert results_end['samples'].tolist() == [600] * 4
        assert int(session.yields()[1].sum()) == sum(range(33)) + 4


# ---- 4: the golden reads and the command -----------------------------------------------------------
def test_golden_reads_on_64_channels(hip, hip_models, gold):
    model, signals = hip_models[STARTS], gold['signals']
    calls = [3, 2, 3, 1, 1, 2, 12]
    tiled = [signals[i % 7] for i in range(64)]
    for policy in (dict(weights=np.r_[-1, 0, 0, -1, [0] * 9].astype(np.int32)),         # --keep 3
                   dict(weights=np.r_[-1, 1, 1, 1, [-1] * 8, 1].astype(np.int32), slack_samples=40000)):
        seed = np.zeros(13, np.int64)
        seed[1] = 50000                     # barcode 1 is ahead by more than the second policy's slack
        want = pol.Policy(n_channels=64, yield_samples=seed, **policy)
        with hip.LiveSession(model, 64, policy=policy) as session:
            session.set_yields(seed, np.zeros(13, np.int64))
            channels = list(range(64))
            for r in range(max(-(-len(s) // 4000) for s in signals)):
                live_now = [ch for ch in channels if r * 4000 < len(tiled[ch])]
                end = [(r + 1) * 4000 >= len(tiled[ch]) for ch in live_now]
                results, _, actions = session.push_policy(
                    live_now, [tiled[ch][r * 4000:(r + 1) * 4000] for ch in live_now],
                    begin=r == 0, end=end)
                # the restatement on the known calls: each read decided in its first push
                known = np.array([pol.record(ref.DECIDED, calls[ch % 7],
                                             min((r + 1) * 4000, len(tiled[ch])))
                                  for ch in live_now], dtype=ref.RESULT)
                flags = ref.BEGIN * (r == 0) + ref.END * np.array(end)
                restated = want.push(live_now, flags, known)
                assert results['call'].tolist() == known['call'].tolist()
                assert actions.tobytes() == restated.tobytes(), r
            samples, reads = session.yields()
            assert samples.tolist() == want.samples and reads.tolist() == want.reads
            assert int(reads.sum()) == 64 and int(samples.sum()) == 50000 + sum(len(s) for s in tiled)


def test_replay_with_a_policy_prints_what_its_host_stand_in_prints(hip, capsys, monkeypatch):
    import test_live_policy
    from conftest import OracleModel
    from deepbinner_amd import classify, replay
    from deepbinner_amd import deepbinner as cli
    for flags, given in ((['--keep', '3'], dict(keep='3')),
                         (['--balance', '1,2,3,12', '--channels', '1'],
                          dict(balance='1,2,3,12', channels=1))):
        capsys.readouterr()
        cli.main(['replay', '--native'] + flags + [SINGLE])
        on_device = capsys.readouterr()
        with monkeypatch.context() as patch:
            patch.setattr(classify, 'build_model', lambda w: OracleModel(w))
            replay.replay(test_live_policy.options(**given), backend=pol.HostBackend())
        on_host = capsys.readouterr()
        assert on_device.out == on_host.out and len(on_host.out.strip().split('\n')) == 8
        table = lambda err: err[err.index('  barcode\treads'):]        # noqa: E731
        assert table(on_device.err) == table(on_host.err)
        assert 'eject' in on_device.out and 'keep' in on_device.out
