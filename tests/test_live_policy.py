"""Yield policies of live sessions without a GPU: the rules on the host (``live_policy_plan_host``,
the lines the kernels compile) against the NumPy restatement, as integers, case by case and over
random push sequences; the records of a session with a policy against those of one without; the
``replay`` command's simulated ejections - rows, yield table, refusals - against a host stand-in;
``replay`` without a policy flag unchanged; the new symbols and what they refuse."""
import os

import numpy as np
import pytest

import live_policy_reference as pol
import live_reference as ref
import test_live
from conftest import REPO
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import hip_backend, replay

CSRC = os.path.join(REPO, 'deepbinner_amd', 'csrc')
NEW_SYMBOLS = ['dbh_live_set_policy', 'dbh_live_push_policy', 'dbh_live_yield', 'dbh_live_set_yield',
               'dbh_live_policy_dev', 'dbh_live_policy_plan_host']
INVALID = 1
B, E = ref.BEGIN, ref.END
BIG = (1 << 45) + 3                     # a yield that a 32-bit sum or product truncates
GOLDEN_CALLS = ['3', '2', '3', '1', '1', '2', '12']


def records(*rows):
    return np.array([pol.record(*row) if isinstance(row, tuple) else pol.record(**row)
                     for row in rows], dtype=ref.RESULT)


def push(channels, flags, *rows):
    return (list(channels), list(flags), records(*rows))


def both(pushes, weights, n_channels, **options):
    """The host entry and the restatement over the same pushes, equal as integers.
    -> (the actions per push, the yield trace [pushes, 2, C])"""
    got, trace, standing = hip_backend.live_policy_plan_host(pushes, weights, n_channels, **options)
    want = pol.Policy(weights, n_channels, **options)
    for p, (channels, flags, recs) in enumerate(pushes):
        actions = want.push(channels, flags, recs)
        assert got[p].dtype == hip_backend.LIVE_ACTION == pol.ACTION
        assert got[p].tobytes() == actions.tobytes(), (p, got[p], actions)
        assert trace[p, 0].tolist() == want.samples and trace[p, 1].tolist() == want.reads, p
    assert standing.tolist() == want.action
    return got, trace


def decided(call, samples=1600):
    return dict(status=ref.DECIDED, call=call, samples=samples)


def ended(call, samples):
    return dict(status=ref.FINAL, call=call, samples=samples, decided=call != 0)


# ---- the rules, case by case -----------------------------------------------------------------------
def test_every_kind_of_weight():
    weights = [-1, -1, 0, 1, 7, 1 << 20]
    seed = [0, 0, 0, 70, 69, BIG]
    got, _ = both([push(range(5), [B] * 5, decided(1), decided(2), decided(3), decided(4), decided(5))],
                  weights, 5, yield_samples=seed)
    a = got[0]
    assert a['action'].tolist() == [pol.KEEP, pol.EJECT, pol.EJECT, pol.KEEP, pol.EJECT]
    assert a['reason'].tolist() == [pol.WEIGHT_KEEP, pol.WEIGHT_EJECT, pol.OVER_LEVEL, pol.BALANCED,
                                    pol.OVER_LEVEL]
    assert a['klass'].tolist() == [1, 2, 3, 4, 5]
    assert a['level'].tolist() == [0, 0, 70, 69 // 7, BIG >> 20] and (a['floor'] == 9).all()
    assert (a['reserved'] == 0).all()


@pytest.mark.parametrize('slack', [0, 5, 1 << 40])
def test_a_level_at_floor_plus_slack_is_kept_and_one_above_is_ejected(slack):
    for floor in (0, 17, BIG):
        for over, action, reason in ((0, pol.KEEP, pol.BALANCED), (1, pol.EJECT, pol.OVER_LEVEL)):
            seed = [0, floor * 3 + 2, (floor + slack + over) * 5 + 4]
            got, _ = both([push([0], [B], decided(2))], [-1, 3, 5], 1, slack_samples=slack,
                          yield_samples=seed)
            assert (got[0]['action'][0], got[0]['reason'][0]) == (action, reason), (slack, floor, over)
            assert got[0]['level'][0] == floor + slack + over and got[0]['floor'][0] == floor


def test_seeded_yields_beyond_32_bits_add_and_divide_as_int64():
    seed = [0, BIG, BIG]
    pushes = [push([0, 1], [B | E, B | E], ended(1, (1 << 33) + 1), ended(2, 5)),
              push([2], [B], decided(1))]
    got, trace = both(pushes, [-1, 1, 1], 3, yield_samples=seed, yield_reads=[0, BIG, 7])
    assert trace[0, 0].tolist() == [0, BIG + (1 << 33) + 1, BIG + 5]
    assert trace[0, 1].tolist() == [0, BIG + 1, 8]
    assert got[1]['level'][0] == BIG + (1 << 33) + 1 and got[1]['floor'][0] == BIG + 5
    assert got[1]['reason'][0] == pol.OVER_LEVEL


def test_a_read_that_begins_and_ends_in_one_chunk_sees_its_own_yield():
    got, trace = both([push([0], [B | E], ended(1, 1000))], [-1, 1, 1], 1)
    assert trace[0, 0].tolist() == [0, 1000, 0] and trace[0, 1].tolist() == [0, 1, 0]
    assert (got[0]['action'][0], got[0]['reason'][0], got[0]['level'][0], got[0]['floor'][0]) == \
        (pol.EJECT, pol.OVER_LEVEL, 1000, 0)


def test_two_channels_deciding_one_barcode_in_one_push_get_the_same_action():
    for seed, action in (([0, 10, 10], pol.KEEP), ([0, 11, 10], pol.EJECT)):
        got, _ = both([push([3, 1], [B, B], decided(1), decided(1))], [-1, 1, 1], 4,
                      yield_samples=seed)
        assert got[0]['action'].tolist() == [action, action]
        assert got[0][0].tobytes() == got[0][1].tobytes()


def test_an_end_counts_before_any_action_of_its_push_in_either_chunk_order():
    """Channel 0 ends a read of barcode 2 with 500 samples in the push in which channel 1 decides
    barcode 1, which stands at 400: behind the END the floor is 400 and the read is kept; an action
    taken in front of it would see a floor of 0 and eject."""
    rows = {0: (E, ended(2, 500)), 1: (0, decided(1))}
    seen = []
    for order in ((0, 1), (1, 0)):
        opened = push(order, [B, B], dict(samples=10), dict(samples=10))
        second = push(order, [rows[ch][0] for ch in order], *[rows[ch][1] for ch in order])
        got, trace = both([opened, second], [-1, 1, 1], 2, yield_samples=[0, 400, 0])
        assert trace[1, 0].tolist() == [0, 400, 500]
        seen.append({ch: got[1][i].tobytes() for i, ch in enumerate(order)})
    assert seen[0] == seen[1]
    kept = np.frombuffer(seen[0][1], pol.ACTION)[0]
    assert kept.tolist() == (pol.KEEP, pol.BALANCED, 1, 0, 400, 400)
    assert np.frombuffer(seen[0][0], pol.ACTION)[0].tolist() == (pol.EJECT, pol.OVER_LEVEL, 2, 0, 500, 400)


def test_the_floor_without_a_balanced_class_and_with_one_never_seen():
    got, _ = both([push([0, 1], [B, B], decided(1), decided(2))], [-1, -1, 0], 2,
                  yield_samples=[9, 9, 9])
    assert got[0]['floor'].tolist() == [0, 0] and got[0]['level'].tolist() == [0, 0]
    assert got[0]['action'].tolist() == [pol.KEEP, pol.EJECT]
    got, _ = both([push([0], [B], decided(1))], [-1, 1, 1, 1], 1, yield_samples=[0, 1, 50, 0])
    assert got[0]['floor'][0] == 0 and got[0]['action'][0] == pol.EJECT      # barcode 3 holds it at 0


@pytest.mark.parametrize('undecided,action', [('keep', pol.KEEP), ('eject', pol.EJECT)])
def test_a_read_that_ends_undecided(undecided, action):
    got, trace = both([push([0, 1], [B, B | E], dict(status=ref.PENDING, samples=10), ended(0, 77))],
                      [-1, 1], 2, undecided=undecided, yield_samples=[0, 5])
    assert got[0]['action'].tolist() == [pol.NONE, action]
    assert got[0][1].tolist() == (action, pol.UNDECIDED, 0, 0, 0, 5)
    assert got[0][0].tolist() == (0, 0, 0, 0, 0, 0)
    assert trace[0, 0].tolist() == [77, 5] and trace[0, 1].tolist() == [1, 0]


def test_an_action_stands_until_begin_and_an_idle_chunk_reports_it():
    idle = dict(status=ref.IDLE, call=1, samples=900)
    pushes = [push([0], [B], decided(1)),                          # keep: level 0, floor 0
              push([0, 1], [0, B | E], decided(1, 3200), ended(1, 100)),       # barcode 1 grows
              push([0], [E], ended(1, 4800)),
              push([0], [E], idle),                                # nothing open: IDLE, no yield
              push([0], [B], decided(1)),                          # a new read: decided afresh
              push([0], [0], idle)]
    got, trace = both(pushes, [-1, 1, 1], 2)
    assert [a['action'][0] for a in got] == [pol.KEEP, pol.KEEP, pol.KEEP, pol.KEEP, pol.EJECT, pol.EJECT]
    assert [a['reason'][0] for a in got] == [pol.BALANCED, 0, 0, 0, pol.OVER_LEVEL, 0]
    assert got[1][1]['action'] == pol.EJECT                        # (its own 100 against a floor of 0)
    assert trace[:, 0, 1].tolist() == [0, 100, 4900, 4900, 4900, 4900]
    assert got[4]['level'][0] == 4900 and got[5].tolist() == [(pol.EJECT, 0, 0, 0, 0, 0)]


def test_random_push_sequences():
    rng = np.random.default_rng(34)
    checked = 0
    for trial in range(40):
        n_classes = int(rng.integers(2, 40))
        n_channels = int(rng.integers(1, 60))
        weights = rng.choice([-1, 0, 1, 2, 7, 1 << 20], n_classes).astype(np.int32)
        weights[0] = -1
        options = dict(slack_samples=int(rng.choice([0, 3, 1 << 40])),
                       undecided=str(rng.choice(['keep', 'eject'])),
                       yield_samples=rng.choice([0, 5, BIG], n_classes),
                       yield_reads=rng.integers(0, 3, n_classes))
        pushes = []
        for _ in range(int(rng.integers(1, 12))):
            channels = rng.permutation(n_channels)[:rng.integers(0, n_channels + 1)]
            rows = []
            for _ in channels:
                status = int(rng.integers(0, 4))
                call = int(rng.integers(0, n_classes)) if status != ref.PENDING else 0
                rows.append(dict(status=status, call=call, samples=int(rng.integers(0, 1 << 34)),
                                 decided=call != 0))
            pushes.append(push(channels, rng.integers(0, 4, len(channels)), *rows))
            checked += len(channels)
        both(pushes, weights, n_channels, **options)
    assert checked > 2000


# ---- the C ABI without a device --------------------------------------------------------------------
def test_symbols_are_exported_declared_and_listed():
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in hip_backend.EXPORTED_SYMBOLS, name
    header = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    section = header[header.index('---- live:'):header.index('---- compressed input')]
    for name in NEW_SYMBOLS + ['dbh_live_action', 'DBH_LIVE_ACTION_EJECT', 'DBH_LIVE_REASON_OVER_LEVEL']:
        assert name in section, name
    assert hip_backend.LIVE_ACTION == pol.ACTION and hip_backend.LIVE_ACTION.itemsize == 32
    assert (hip_backend.LIVE_NO_ACTION, hip_backend.LIVE_KEEP, hip_backend.LIVE_EJECT) == \
        (pol.NONE, pol.KEEP, pol.EJECT)
    assert hip_backend.LIVE_REASONS.index('over_level') == pol.OVER_LEVEL
    assert hip_backend.LIVE_REASONS.index('undecided') == pol.UNDECIDED


def test_the_rules_are_one_text():
    core = open(os.path.join(CSRC, 'dbh_live_core.h')).read()
    kernels = open(os.path.join(CSRC, 'dbh_live.hip')).read()
    check = open(os.path.join(CSRC, 'live_model_check.cpp')).read()
    for name in ('policy_ok', 'yield_class', 'level_of', 'action_of'):
        assert 'DBLIVE_FN' in core and name in core and name in check, name
    for name in ('yield_class', 'level_of', 'action_of', 'yield_kernel', 'action_kernel'):
        assert name in kernels, name
    assert 'asm' not in kernels and 'atomic' not in kernels
    api = open(os.path.join(CSRC, 'dbh_api_live.hip')).read()
    assert 'plan_policy_push' in api and 'policy_ok' in api


def test_bad_arguments_are_refused_before_any_device_work():
    lib = hip_backend.load_library()
    weights = np.array([-1, 1], np.int32)
    p = lambda a: a.ctypes.data                                    # noqa: E731
    assert lib.dbh_live_set_policy(None, p(weights), 2, 0, pol.KEEP) == INVALID
    assert lib.dbh_live_push_policy(None, 1, 1, 1, 1, 1, None, 1, 1) == INVALID
    assert lib.dbh_live_push_policy(None, 1, 1, 1, 1, 1, None, 1, 0) == INVALID
    assert lib.dbh_live_yield(None, 1, 1) == INVALID and lib.dbh_live_set_yield(None, 1, 1) == INVALID
    # the kernels alone: counts and the policy's own numbers, before any pointer is touched
    dev = [1, 1, 1, 4, 1, 2, 0, pol.KEEP, 1, 1, 1, 1, None]
    for at, bad in ((3, -1), (3, 16385), (5, 0), (5, 257), (6, -1), (7, 0), (7, 3), (0, None),
                    (1, None), (2, None), (4, None), (8, None), (9, None), (10, None), (11, None)):
        args = list(dev)
        args[at] = bad
        assert lib.dbh_live_policy_dev(*args) == INVALID, (at, bad)
    assert lib.dbh_live_policy_dev(*(dev[:3] + [0] + dev[4:])) == 0          # no chunk


def test_plan_host_refuses_a_bad_policy_and_bad_tables_and_changes_nothing():
    lib = hip_backend.load_library()
    p = lambda a: a.ctypes.data                                    # noqa: E731
    weights = np.array([-1, 1, 0], np.int32)
    offsets = np.array([0, 2], np.int64)
    channels, flags = np.array([0, 1], np.int32), np.array([B, B | E], np.uint32)
    recs = records(decided(1), ended(1, 50))
    standing, samples, reads = np.full(2, 7, np.int32), np.full(3, 7, np.int64), np.full(3, 7, np.int64)
    actions = np.full(2, 9, hip_backend.LIVE_ACTION)
    good = [p(weights), 3, 0, pol.KEEP, p(offsets), 1, p(channels), p(flags), p(recs), 2,
            p(standing), p(samples), p(reads), p(actions), None]
    bad_calls = [(0, None), (1, 0), (1, 257), (2, -1), (3, 0), (3, 3), (4, None), (5, -1), (6, None),
                 (7, None), (8, None), (9, 0), (9, 16385), (9, 1), (10, None), (11, None), (12, None),
                 (13, None)]
    for held in ([0, 1, 0], [-1, -2, 0], [-1, (1 << 20) + 1, 0]):                  # weights
        bad_calls.append((0, np.array(held, np.int32)))
    bad_calls.append((4, np.array([1, 2], np.int64)))                              # not from 0
    bad_calls.append((4, np.array([0, -1], np.int64)))                             # backwards
    bad_calls.append((6, np.array([0, 0], np.int32)))                              # twice
    bad_calls.append((6, np.array([0, 2], np.int32)))                              # outside
    bad_calls.append((7, np.array([B, 4], np.uint32)))                             # an unknown bit
    bad_calls.append((11, np.array([0, -1, 0], np.int64)))                         # a negative yield
    for at, bad in bad_calls:
        args = list(good)
        args[at] = p(bad) if isinstance(bad, np.ndarray) else bad
        assert lib.dbh_live_policy_plan_host(*args) == INVALID, (at, bad)
        assert (standing == 7).all() and (reads == 7).all() and (actions['level'] == 9).all()
        assert (samples == 7).all() or at == 11
    assert lib.dbh_live_policy_plan_host(*(good[:5] + [0] + good[6:])) == 0        # no push
    assert (standing == 7).all() and (samples == 7).all()
    standing[:] = 0
    assert lib.dbh_live_policy_plan_host(*good) == 0
    assert samples.tolist() == [7, 57, 7] and reads.tolist() == [7, 8, 7]
    assert actions['action'].tolist() == [pol.KEEP, pol.KEEP] and standing.tolist() == [1, 1]
    assert actions['level'].tolist() == [57, 57] and actions['floor'].tolist() == [57, 57]


def test_the_model_check_program_covers_the_policy():
    text = open(os.path.join(CSRC, 'Makefile')).read()
    assert '-fsanitize=address,undefined' in text[text.index('live_asan:'):]
    source = open(os.path.join(CSRC, 'live_model_check.cpp')).read()
    for name in ('plan_policy_push', 'action_of', 'floor_of', '1LL << 50'):
        assert name in source, name


# ---- the stand-in: the action changes nothing else -------------------------------------------------
class CountingModel:
    """A model whose answer is a function of the window's first value: enough for the records."""
    def __init__(self, input_size=96, n_classes=5):
        from deepbinner_amd.hip_backend import _TensorSpec
        self.inputs = [_TensorSpec((None, input_size, 1))]
        self.outputs = [_TensorSpec((None, n_classes))]
        self.n_classes = n_classes

    def predict(self, x, batch_size=None):
        x = np.asarray(x, np.float32)[:, :, 0]
        out = np.full((len(x), self.n_classes), 0.02, np.float32)
        top = (np.abs(x[:, 0] * 1000).astype(np.int64) % self.n_classes)
        out[np.arange(len(x)), top] = 1 - 0.02 * (self.n_classes - 1)
        return out


@pytest.mark.parametrize('with_end', [False, True], ids=['start only', 'pair'])
def test_records_with_a_policy_are_those_without_byte_for_byte(with_end):
    rng = np.random.default_rng(5)
    model, end_model = CountingModel(), CountingModel() if with_end else None
    weights = [-1, 1, 0, 2, -1]
    backend = pol.HostBackend()
    plain = backend.LiveSession(model, 6, end_model=end_model, scan_size=576)
    ruled = backend.LiveSession(model, 6, end_model=end_model, scan_size=576,
                                policy=dict(weights=weights, undecided='eject'))
    restated = pol.Policy(weights, 6, undecided='eject')
    taken = set()
    for r in range(30):
        channels = rng.permutation(6)[:rng.integers(1, 7)].tolist()
        chunks = [rng.integers(200, 900, rng.integers(0, 300)).astype(np.int16) for _ in channels]
        begin, end = rng.random(len(channels)) < 0.3, rng.random(len(channels)) < 0.3
        results, ends, actions = ruled.push_policy(channels, chunks, begin=begin, end=end)
        if with_end:
            want, want_ends = plain.push_pair(channels, chunks, begin=begin, end=end)
            assert ends.tobytes() == want_ends.tobytes()
        else:
            want = plain.push(channels, chunks, begin=begin, end=end)
            assert ends is None
        assert results.tobytes() == want.tobytes(), r
        flags = begin * B + end * E
        assert actions.tobytes() == restated.push(channels, flags, results).tobytes()
        assert [y.tolist() for y in ruled.yields()] == [restated.samples, restated.reads]
        for ch in channels:
            assert [t.tolist() for t in ruled.track(ch)] == [t.tolist() for t in plain.track(ch)]
        taken |= set(actions['reason'].tolist())
    assert taken >= {0, pol.WEIGHT_KEEP, pol.WEIGHT_EJECT, pol.BALANCED}


# ---- the command against the stand-in --------------------------------------------------------------
def options(**given):
    base = dict(balance=None, deplete=None, keep=None, slack_samples=0, eject_undecided=False,
                eject_samples=None)
    base.update(given)
    return test_live.options(**base)


def run(capsys, **given):
    capsys.readouterr()
    replay.replay(options(**given), backend=pol.HostBackend())
    out, err = capsys.readouterr()
    header, rows = test_live.table(out)
    return header, rows, err


def yield_table(err):
    lines = err.rstrip('\n').split('\n')
    at = lines.index('  barcode\treads\tejected\tdelivered\trecorded')
    assert lines[-1].startswith('  rounds: ')
    return {row.split('\t')[0].strip(): [int(v) for v in row.split('\t')[1:]]
            for row in lines[at + 1:-1]}, int(lines[-1].split(': ')[1])


def test_keep_ejects_exactly_the_other_reads(oracle_backend, gold, capsys):
    calls = dict(zip(gold['read_ids'], GOLDEN_CALLS))
    for eject_samples, E in ((None, 1600), (0, 0), (700, 700), (1 << 30, 1 << 30)):
        header, rows, err = run(capsys, keep='3', eject_samples=eject_samples)
        assert header == replay.HEADER + ['action', 'delivered'] and len(rows) == 7
        table = {}
        for row in rows:
            call, samples = calls[row[0]], int(row[5])
            assert row[1] == call and row[3] == '1600'             # decided in its first push
            assert samples == len(gold['signals'][gold['read_ids'].index(row[0])])
            assert row[7] == ('keep' if call == '3' else 'eject'), row
            want = samples if call == '3' else min(samples, min(samples, 1600) + E)
            assert int(row[8]) == want, (row, E)
            t = table.setdefault(call, [0, 0, 0, 0])
            t[0], t[1], t[2], t[3] = t[0] + 1, t[1] + (call != '3'), t[2] + want, t[3] + samples
        assert sum(row[7] == 'eject' for row in rows) == 5
        got, rounds = yield_table(err)
        assert got == table
        assert rounds == max(max(1, -(-int(row[8]) // 1600)) +
                             (E == 0 and row[7] == 'eject' and int(row[5]) > 1600) for row in rows)


def test_balance_on_one_channel_keeps_first_reads_and_ejects_repeats(oracle_backend, gold, capsys):
    header, rows, err = run(capsys, balance='1,2,3,12', channels=1)
    yields, seen_actions = {1: 0, 2: 0, 3: 0, 12: 0}, []
    for row in rows:                                               # file order: one read at a time
        call, samples = int(row[1]), int(row[5])
        level, floor = yields[call], min(yields.values())
        want = 'eject' if level > floor else 'keep'
        delivered = samples if want == 'keep' else min(samples, min(samples, 1600) + 1600)
        assert (row[7], int(row[8])) == (want, delivered), row
        if yields[call] == 0:
            assert want == 'keep'                                  # the first read of a barcode
        elif min(yields.values()) == 0:
            assert want == 'eject'                                 # a repeat while another is at 0
        yields[call] += delivered
        seen_actions.append(want)
    assert 'keep' in seen_actions and 'eject' in seen_actions
    got, _ = yield_table(err)
    assert {int(k): v[2] for k, v in got.items()} == yields
    # shares and slack: with shares of a million no level leaves 0; with slack beyond any read too
    for given in (dict(balance='1:1000000,2:1000000,3:1000000,12:1000000'),
                  dict(balance='1,2,3,12', slack_samples=1 << 40)):
        _, rows, _ = run(capsys, channels=1, **given)
        assert all(row[7] == 'keep' and row[8] == row[5] for row in rows)
    # depleted barcodes beside balanced ones
    _, rows, _ = run(capsys, balance='1,2', deplete='12', channels=1)
    assert all((row[7] == 'eject') == (row[1] == '12') or row[1] in ('1', '2') for row in rows)
    assert all(row[7] == 'keep' for row in rows if row[1] == '3')


def test_reads_that_end_undecided(oracle_backend, gold, capsys):
    for flag, action in ((False, 'keep'), (True, 'eject')):
        _, rows, err = run(capsys, keep='3', eject_undecided=flag, score_diff=1.5, channels=2)
        assert all(row[1] == 'none' and row[4] == 'none' for row in rows)
        # undecided is known when the read is FINAL: at END, or with the push that brings the
        # scan's last window (6144 + 512 samples: the fifth chunk)
        for row in rows:
            samples = int(row[5])
            want = min(samples, 8000 + 1600) if flag else samples
            assert (row[7], int(row[8])) == (action, want), row
        assert any(int(row[8]) < int(row[5]) for row in rows) == flag
        got, _ = yield_table(err)
        assert list(got) == ['none'] and got['none'][0] == 7 and got['none'][1] == 7 * flag
    _, rows, _ = run(capsys, eject_undecided=True, channels=2)     # a policy of its own
    assert all(row[7] == 'keep' and row[1] != 'none' for row in rows)


def test_both_ends_with_a_policy(oracle_backend, gold, capsys):
    header, rows, _ = run(capsys, keep='3', both_ends=True, end_model=test_live.ENDS, eject_samples=1 << 30)
    assert header == replay.PAIR_HEADER + ['action', 'delivered']
    _, plain, _ = run(capsys, both_ends=True, end_model=test_live.ENDS)
    assert [row[:9] for row in rows] == plain                      # nobody left early: the same calls
    assert [row[9] for row in rows] == ['keep' if row[1] == '3' else 'eject' for row in rows]


@pytest.mark.parametrize('given,message', [
    (dict(balance='1,1'), '--balance names barcode 1 twice'),
    (dict(balance='1', deplete='1'), 'barcode 1 is named by --balance and by --deplete'),
    (dict(keep='2', deplete='2'), 'barcode 2 is named by --deplete and by --keep'),
    (dict(keep='2', balance='2:3'), 'barcode 2 is named by --balance and by --keep'),
    (dict(balance='13'), 'the model has barcodes 1 to 12'),
    (dict(deplete='0'), 'the model has barcodes 1 to 12'),
    (dict(balance='1:0'), 'share of barcode 1 must be from 1 to 1048576'),
    (dict(balance='1:1048577'), 'share of barcode 1 must be from 1 to 1048576'),
    (dict(balance=''), '--balance takes barcode numbers'),
    (dict(keep='1:2'), '--keep takes barcode numbers'),
    (dict(balance='1:'), '--balance takes barcode numbers'),
    (dict(deplete='x'), '--deplete takes barcode numbers'),
    (dict(slack_samples=5), 'need a policy'),
    (dict(eject_samples=5), 'need a policy'),
    (dict(keep='1', slack_samples=5), '--slack_samples needs --balance'),
    (dict(balance='1', slack_samples=-1), '--slack_samples cannot be negative'),
    (dict(keep='1', eject_samples=-1), '--eject_samples cannot be negative'),
])
def test_command_refusals(oracle_backend, given, message):
    with pytest.raises(SystemExit) as e:
        replay.replay(options(**given), backend=pol.HostBackend())
    assert message in str(e.value) and e.value.code != 0 and '\n' not in str(e.value)


def test_replay_without_a_policy_flag_is_unchanged(oracle_backend, gold, capsys):
    """Byte for byte what the start-only and the pair tests hold it to, through this file's backend
    and with the policy options present but unset."""
    seen = []
    for args, backend in ((test_live.options(), ref.HostBackend()), (options(), pol.HostBackend()),
                          (test_live.options(), pol.HostBackend())):
        capsys.readouterr()
        replay.replay(args, backend=backend)
        seen.append(capsys.readouterr())
    assert all(s.out == seen[0].out and s.err == seen[0].err for s in seen)
    header, lines = test_live.table(seen[0].out)
    assert header == replay.HEADER and 'rounds' not in seen[0].err and 'ejected' not in seen[0].err
    assert sorted(lines) == sorted(test_live.predicted_rows(gold, 1600))


def test_command_line_entry(monkeypatch):
    seen = {}
    monkeypatch.setattr(replay, 'replay', lambda args: seen.update(vars(args)))
    cli.main(['replay', '--native', 'some_dir'])
    assert seen['balance'] is None and seen['deplete'] is None and seen['keep'] is None
    assert seen['slack_samples'] == 0 and not seen['eject_undecided'] and seen['eject_samples'] is None
    cli.main(['replay', '--native', '--balance', '1:2,2:1', '--deplete', '5', '--slack_samples', '9',
              '--eject_undecided', '--eject_samples', '0', 'some_dir'])
    assert seen['balance'] == '1:2,2:1' and seen['deplete'] == '5' and seen['slack_samples'] == 9
    assert seen['eject_undecided'] and seen['eject_samples'] == 0
    weights = replay.parse_policy(options(balance='1:2,2:1', deplete='5'), 13)[0]['weights']
    assert weights.tolist() == [-1, 2, 1, -1, -1, 0] + [-1] * 7
    weights = replay.parse_policy(options(keep='3', balance='4'), 13)[0]['weights']
    assert weights.tolist() == [-1, 0, 0, -1, 1] + [0] * 8
