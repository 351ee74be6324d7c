"""The resident trainer on the device (include/deepbinner_hip.h, "a resident trainer"; DESIGN.md
section 18) against tests/train_step_reference.py (pinned in tests/test_train_step_reference.py).

Nothing here has a tolerance of its own making.  The noise is held to one fp32 unit in the last
place of the fp64 reference's rounded value (log, cos and sqrt of two libraries are a few fp64 units
apart, the sum is rounded once).  The update is IEEE double operation for operation on both sides:
equal bit for bit.  A trainer's step is replayed on the host from the library's stateless pieces -
dbh_train_noise, dbh_gradients (the same call gives the same bits: section 17), the NumPy update
with dbh_nadam_schedule's coefficients - and must equal it bit for bit after every step, which pins
the wiring: the step seed, noise once and in front of the statistics, the loss of the batch before
the update, the gradient blob's zeros leaving the moving slots to the average, one advance of
iterations and m_schedule per step.  The learning test's lines are twice the fp64 reference's own
loss bound and four windows (profiles/train_step/learning.txt).
"""
import ctypes
import os

import numpy as np
import pytest

import train_reference as tr
import train_step_reference as ts
from deepbinner_amd.model_format import BN_CHANNELS, ModelWeights, param_count

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    differ = np.flatnonzero(bits(got) != bits(want))
    assert differ.size == 0, '{}: {} of {} differ, first at {}: {!r} against {!r}'.format(
        what, differ.size, np.size(want), differ[0], np.ravel(got)[differ[0]], np.ravel(want)[differ[0]])


# ---- noise ---------------------------------------------------------------------------------------
# (input size, windows, seed): 64 window numbers through the hash; the largest positions; a seed
# whose upper half takes part
NOISE_CASES = [(96, 64, tr.SEED), (16384, 2, tr.SEED), (130, 5, tr.HIGH_SEED)]


@pytest.mark.parametrize('size,n,seed', NOISE_CASES, ids=lambda v: str(v))
def test_noise_within_one_ulp_of_the_fp64_reference(hip, size, n, seed):
    x = np.random.default_rng([size, n]).standard_normal((n, size)).astype(np.float32)
    got = hip.train_noise(x, 0.02, seed)
    want = ts.add_noise(x, 0.02, seed)
    ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got)))
    off = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print('L{} N{}: {} of {} values differ from the reference, worst {:.2f} ulp'.format(
        size, n, int((got != want).sum()), got.size, float((off / ulp).max())))
    assert (off <= ulp).all()
    noise = got.astype(np.float64) - x
    assert 0.019 < noise.std() < 0.021 and np.abs(noise).max() <= 0.02 * ts.Z_MAX + 1e-6
    same_bits(hip.train_noise(x, 0.02, seed), got, 'the same call twice')
    assert (hip.train_noise(x, 0.02, ts.step_seed(seed, 1)) != got).mean() > 0.99


def test_noise_of_nothing_returns_the_input(hip):
    x = np.random.default_rng(5).standard_normal((3, 130)).astype(np.float32)
    x[0, :4] = [-0.0, 0.0, np.float32(1e-40), -np.float32(1e-40)]
    same_bits(hip.train_noise(x, 0.0, tr.HIGH_SEED), x, 'noise_std 0')
    assert np.signbit(hip.train_noise(x, 0.0, 1)[0, 0])


# ---- update --------------------------------------------------------------------------------------
def update_inputs(classes):
    n = param_count(classes)
    rng = np.random.default_rng([classes, n])
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * np.exp(2 * rng.standard_normal(n))).astype(np.float32)
    m = np.maximum(rng.standard_normal(n), -1.0).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * np.exp(2 * rng.standard_normal(n))).astype(np.float32)
    blob, _ = ts.moving_index(classes)
    g[blob] = m[blob] = v[blob] = 0                 # as dbh_gradients and a trainer leave them
    stats = rng.standard_normal(960).astype(np.float32)     # distinct per channel and layer
    assert np.unique(stats).size == 960
    trainable = np.setdiff1d(np.arange(n), blob)
    flat = rng.choice(trainable, 64, replace=False)
    flat = np.concatenate([flat, [0, trainable[-1], blob[0] - 1]])   # both ends, the last bias
    g[flat[:40]] = 0
    v[flat[:40]] = 0                                # the update is exactly -lr mu_t1 m' / epsilon
    g[flat[40:52]] = np.float32(1e-40)              # a denormal gradient
    v[flat[46:52]] = 0
    return p, g, m, v, stats, blob, flat


@pytest.mark.parametrize('t0', [0, 7])
@pytest.mark.parametrize('classes', [2, 13, 33, 256])
def test_update_equals_the_numpy_update_bit_for_bit(hip, classes, t0):
    p, g, m, v, stats, blob, flat = update_inputs(classes)
    schedule = 1.0
    for t in range(t0):
        schedule = hip.nadam_schedule(t, schedule)['sched_new']
    k = hip.nadam_schedule(t0, schedule)
    want = ts.nadam_update(p, g, m, v, stats, classes, k)
    got = hip.nadam_update(p, g, m, v, stats, classes, k)
    for name, a, b in zip(('p', 'm', 'v'), got, want):
        same_bits(a, b, '{} at C = {}, t0 = {}'.format(name, classes, t0))
    gp, gm, gv = got
    assert not gm[blob].any() and not gv[blob].any()
    assert (gp[blob] != p[blob]).mean() > 0.99
    # batch normalisation 5's 192 channels, from the header's layout alone
    start = param_count(classes) - 4 * sum(BN_CHANNELS) + 4 * sum(BN_CHANNELS[:4])
    for quarter, first in ((2, 2 * sum(BN_CHANNELS[:4])), (3, 2 * sum(BN_CHANNELS[:4]) + 192)):
        old = p[start + quarter * 192:start + (quarter + 1) * 192].astype(np.float64)
        batch = stats[first:first + 192].astype(np.float64)
        same_bits(gp[start + quarter * 192:start + (quarter + 1) * 192],
                  (old - (old - batch) * (1.0 - k['bn_momentum'])).astype(np.float32), 'BN5')
    # g = 0 and v = 0: exactly -lr * mu_t1 * m' / epsilon
    zero = flat[:40]
    m_new = k['beta_1'] * m[zero].astype(np.float64)
    move = (k['lr'] * (k['mu_t1'] * (m_new / (1.0 - k['sched_next'])))) / k['epsilon']
    same_bits(gp[zero], (p[zero].astype(np.float64) - move).astype(np.float32), 'g = 0, v = 0')
    assert (gp[flat] != p[flat]).sum() >= flat.size - 2
    # the trainable elements do not read the statistics
    other = hip.nadam_update(p, g, m, v, stats[::-1].copy(), classes, k)
    trainable = np.setdiff1d(np.arange(p.size), blob)
    same_bits(other[0][trainable], gp[trainable], 'trainable elements under other statistics')
    assert (other[0][blob] != gp[blob]).mean() > 0.99


# ---- trainer: replay -----------------------------------------------------------------------------
def batch(size, n, classes, draw):
    weights, x, labels = tr.case_inputs(size, n, classes, draw=draw)
    return weights, x, np.roll(labels, draw)


def replay_step(hip, state, x, labels, **options):
    return ts.full_step(state, x, labels, schedule=hip.nadam_schedule, noise=hip.train_noise,
                        gradients=hip.loss_and_gradients, **options)


def check_state(trainer, state, what):
    same_bits(trainer.weights().flat(), state.flat, what + ': weights')
    got = trainer.state()
    same_bits(got['m'], state.m, what + ': m')
    same_bits(got['v'], state.v, what + ': v')
    assert got['iterations'] == trainer.iterations == state.iterations, what
    assert got['m_schedule'] == state.m_schedule, what


REPLAY = [(96, 3, 2), (130, 5, 13), (200, 2, 33), (1024, 4, 13)]


@pytest.mark.parametrize('size,n,classes', REPLAY, ids=lambda v: str(v))
def test_trainer_steps_replay_from_the_stateless_pieces(hip, size, n, classes):
    weights = batch(size, n, classes, 0)[0]
    state = ts.State(weights)
    blob, _ = ts.moving_index(classes)
    with hip.Trainer(weights, n, seed=tr.HIGH_SEED) as trainer:
        check_state(trainer, state, 'before any step')
        for step in range(4):
            _, x, labels = batch(size, n, classes, step)
            got = trainer.step(x, labels)
            before = state.flat.copy()
            want = replay_step(hip, state, x, labels, seed=tr.HIGH_SEED)
            assert got == want, (step, got, want)
            check_state(trainer, state, 'step {}'.format(step))
            assert (state.flat[blob] != before[blob]).mean() > 0.9      # the averages moved
            assert not state.m[blob].any() and not state.v[blob].any()
        assert state.iterations == 4 and 0 < state.m_schedule < 0.05

        # the queued entry: four steps without a host synchronisation in between, then one
        queued = hip.Trainer(weights, n, seed=tr.HIGH_SEED)
        stream = hip.Stream()
        xs = [hip.DeviceBuffer.from_array(batch(size, n, classes, s)[1]) for s in range(4)]
        ls = [hip.DeviceBuffer.from_array(batch(size, n, classes, s)[2]) for s in range(4)]
        losses, counts = hip.DeviceBuffer(4 * 8), hip.DeviceBuffer(4 * 8)
        for s in range(4):
            queued.step_dev(xs[s].ptr, ls[s].ptr, n, losses.ptr + 8 * s, counts.ptr + 8 * s, stream.ptr)
        stream.synchronize()
        check_state(queued, state, 'four queued steps')
        same_bits(xs[0].download((n, size), np.float32), batch(size, n, classes, 0)[1], 'x_dev')
        queued.close()
        stream.close()
    # the loss of the queued steps: those of a second replay
    again = ts.State(weights)
    want = [replay_step(hip, again, *batch(size, n, classes, s)[1:], seed=tr.HIGH_SEED) for s in range(4)]
    assert list(losses.download(4, np.float64)) == [w[0] for w in want]
    assert list(counts.download(4, np.int64)) == [w[1] for w in want]


def test_a_smaller_batch_in_a_larger_trainer(hip):
    """max_windows 8: a step at 8 windows, then one at 3.  The statistics are per call; nothing of
    the first batch's rows reaches the second step."""
    size, classes = 130, 13
    weights, x8, l8 = batch(size, 8, classes, 0)
    _, x3, l3 = batch(size, 3, classes, 1)
    state = ts.State(weights)
    with hip.Trainer(weights, 8, seed=tr.SEED) as trainer:
        for x, labels in ((x8, l8), (x3, l3)):
            got = trainer.step(x, labels)
            assert got == replay_step(hip, state, x, labels, seed=tr.SEED)
            check_state(trainer, state, '{} windows'.format(len(labels)))


def test_trainer_refuses_before_it_works(hip):
    size, classes = 96, 2
    weights, x, labels = batch(size, 3, classes, 0)
    lib = hip.load_library()
    loss, count = ctypes.c_double(7.0), ctypes.c_int64(7)
    with hip.Trainer(weights, 3) as trainer:
        def step(n, lab=labels):
            big = np.zeros((4, size), dtype=np.float32)
            lab = np.ascontiguousarray(lab, dtype=np.int32)
            return lib.dbh_trainer_step(trainer._handle, big.ctypes.data, lab.ctypes.data, n,
                                        ctypes.byref(loss), ctypes.byref(count))
        assert step(4, np.zeros(4)) == UNSUPPORTED
        assert step(0) == INVALID
        assert step(3, [0, 2, 1]) == INVALID and step(3, [0, -1, 1]) == INVALID
        assert lib.dbh_trainer_step_dev(trainer._handle, None, None, 3, None, None, None) == INVALID
        flat = np.zeros(param_count(classes) + 1, dtype=np.float32)
        assert lib.dbh_trainer_get_weights(trainer._handle, flat, flat.size) == 4
        assert (loss.value, count.value) == (7.0, 7) and trainer.iterations == 0
        same_bits(trainer.weights().flat(), weights.flat(), 'weights after refused steps')
        with pytest.raises(ValueError):
            trainer.load_state({'m': flat, 'v': flat, 'iterations': 0, 'm_schedule': 1.0})


# ---- resume --------------------------------------------------------------------------------------
def test_resume_continues_bit_for_bit(hip, tmp_path):
    size, n, classes = 130, 5, 13
    weights = batch(size, n, classes, 0)[0]
    batches = [batch(size, n, classes, s)[1:] for s in range(6)]
    options = {'seed': tr.HIGH_SEED, 'bn_momentum': 0.9, 'lr': 0.004}
    with hip.Trainer(weights, n, **options) as straight:
        results = [straight.step(x, labels) for x, labels in batches]
        want_w, want = straight.weights().flat(), straight.state()
    assert want['iterations'] == 6

    path = str(tmp_path / 'model.dbw')
    with hip.Trainer(weights, n, **options) as first:
        assert [first.step(x, labels) for x, labels in batches[:3]] == results[:3]
        half_w, half = first.weights(), first.state()
        first.save_checkpoint(path)
    assert half['iterations'] == 3
    loaded, shape = ModelWeights.load(path)                # the model file `classify` loads
    assert shape == [None, size, 1] and loaded.n_classes == classes
    same_bits(loaded.flat(), half_w.flat(), 'the checkpoint\'s weights')
    assert os.path.isfile(hip.Trainer.state_path(path))

    resumed = hip.Trainer(half_w, n, **options)
    resumed.load_state(half)
    from_files = hip.Trainer.from_checkpoint(path, n)       # its options come from the checkpoint
    assert from_files.options['lr'] == 0.004 and from_files.options['seed'] == tr.HIGH_SEED
    for name, trainer in (('state and weights', resumed), ('checkpoint files', from_files)):
        with trainer:
            assert trainer.iterations == 3
            assert [trainer.step(x, labels) for x, labels in batches[3:]] == results[3:], name
            same_bits(trainer.weights().flat(), want_w, name + ': weights')
            got = trainer.state()
            same_bits(got['m'], want['m'], name + ': m')
            same_bits(got['v'], want['v'], name + ': v')
            assert (got['iterations'], got['m_schedule']) == (6, want['m_schedule'])
    # a fresh trainer that skips the state does not get there
    with hip.Trainer(half_w, n, **options) as cold:
        assert cold.step(*batches[3]) != results[3]


# ---- learning ------------------------------------------------------------------------------------
def test_it_learns_and_the_model_object_can_use_the_result(hip):
    """The task, the step count and the reference's own figures: profiles/train_step/learning.txt
    (tools/train_step_learning.py; the fp64 reference ends at a last-10 loss of 0.0397, under a
    quarter of ln 3 = 0.2747, and 64 of 64).  The device gets twice the loss and four windows:
    trajectories of two roundings part over 300 steps, and the point is that weights and moving
    averages together are a model the inference path can use."""
    train, (held_x, held_labels) = ts.learning_batches()
    assert len(train) == ts.LEARN_STEPS and train[0][0].shape == (16, ts.LEARN_INPUT)
    with hip.Trainer(ts.learning_weights(), ts.LEARN_BATCH, **ts.LEARN_OPTIONS) as trainer:
        losses = [trainer.step(x, labels)[0] for x, labels in train]
        trained = trainer.weights()
    last = float(np.mean(losses[-10:]))
    model = hip.HipModel(trained, device=0)
    probs = model.predict(held_x[:, :, None])
    model.close()
    right = int((probs.argmax(axis=1) == held_labels).sum())
    print('first 10 steps: mean loss {:.4f}; last 10: {:.4f} (line {:.4f}); held-out {} of 64'.format(
        float(np.mean(losses[:10])), last, np.log(3) / 2, right))
    assert last < np.log(3) / 2
    assert right >= 60
