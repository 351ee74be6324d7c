"""Fine-tuning behind frozen blocks on the device (include/deepbinner_hip.h, "FROZEN BLOCKS";
DESIGN.md section 38).

Every check is an equality of bits against code that is already held to the fp64 reference: the
same call at frozen_blocks = 0 (tests/test_gpu_gradients.py), dbh_nadam_update
(tests/test_gpu_trainer.py), and a trainer's step replayed from its stateless pieces.  No tolerance
is introduced here.  The one inequality - the head alone learns - takes its step count from the
fp64 reference (HEAD_STEPS below).
"""
import ctypes
import os

import numpy as np
import pytest

import finetune_cases as fc
import train_reference as tr
import train_step_reference as ts
from conftest import GOLD, MODEL_DIR
from deepbinner_amd import deepbinner as cli
from deepbinner_amd.model_format import ModelWeights, param_count

pytestmark = pytest.mark.gpu

INVALID = 1


def guarded(size, n, classes, rate):
    """(weights, x, labels, seed) of the train_reference.GUARDED case of that shape and rate."""
    case = next(c for c in tr.GUARDED if c[:4] == (size, n, classes, rate) and c[4] == tr.SEED)
    return tr.case_inputs(size, n, classes, case[5]) + (case[4],)


# (input size, windows, classes, dropout rate, windows after tiling or None)
#   (96, 3, 2): the minimum length, BN7 over three elements;  (96, 1, 2): one window
#   (130, 5, 13): odd lengths;  (2050, 3, 13): an odd length at the first pool
#   (1024, 4, 13): the shipped geometry;  (96, 64, 5): 64 window numbers through the hash
#   (96, 64, 5) tiled to 700 windows: 33,600 rows at conv1d_1 - 254 parts of 132 rows per weight
#   gradient and a last one of 72 (tests/test_gpu_gradients.py repeats guarded batches the same way)
CASES = [(96, 3, 2, 0.15, None), (96, 1, 2, 0.0, None), (130, 5, 13, 0.15, None),
         (2050, 3, 13, 0.15, None),
         (1024, 4, 13, 0.0, None), (96, 64, 5, 0.15, None), (96, 64, 5, 0.0, 700)]


def case_inputs(case):
    size, n, classes, rate, tiled = case
    weights, x, labels, seed = guarded(size, n, classes, rate)
    if tiled:               # (96, 700, 5, 0.0): the guarded 64 windows, repeated and cut at 700
        times = -(-tiled // n)
        x, labels = np.tile(x, (times, 1))[:tiled], np.tile(labels, times)[:tiled]
    return weights, x, labels, rate, seed


def run_dev(hip, weights, x, labels, rate, seed, f):
    """dbh_gradients_frozen_dev with the gradient buffer all ones (0xFF bytes) beforehand"""
    flat = weights.flat()
    n = x.shape[0]
    work = hip.gradients_workspace_bytes(weights.n_classes, weights.input_size, n)
    filled = np.full(flat.size, 0xFFFFFFFF, dtype=np.uint32)
    with hip.device_arrays(flat, x, labels, 8, 8, filled, 960 * 4, work) as (
            w, xd, ld, loss, correct, grads, stats, ws):
        hip.gradients_dev(w.ptr, flat.size, weights.n_classes, weights.input_size, xd.ptr, ld.ptr, n,
                          rate, seed, loss.ptr, correct.ptr, grads.ptr, stats.ptr, ws.ptr,
                          frozen_blocks=f)
        hip.synchronize()
        return (float(loss.download((1,), np.float64)[0]), int(correct.download((1,), np.int64)[0]),
                grads.download((flat.size,), np.float32), stats.download((960,), np.float32))


def check_frozen_gradients(got, full, classes, f, what):
    slices, moving = tr.tensor_slices(classes)
    frozen, trainable = fc.tensor_names(f)
    assert np.float64(got[0]).tobytes() == np.float64(full[0]).tobytes(), what
    assert got[1] == full[1], what
    fc.same_bits(got[3], full[3], what + ': batch statistics')
    for name in trainable:
        fc.same_bits(got[2][slices[name]], full[2][slices[name]], '{}: {}'.format(what, name))
    for name in frozen:
        assert not fc.bits(got[2][slices[name]]).any(), '{}: {} is not +0.0'.format(what, name)
    for sl in moving:
        assert not fc.bits(got[2][sl]).any(), what + ': a moving slot is not +0.0'


# ---- 1. gradients ----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'L{}-N{}-C{}-rate{}-tiled{}'.format(*c))
def test_frozen_gradients_are_the_full_call_s_bits(hip, case):
    weights, x, labels, rate, seed = case_inputs(case)
    classes = weights.n_classes
    assert x.shape[0] == (case[4] or case[1])
    full = hip.loss_and_gradients(weights, x, labels, dropout_rate=rate, seed=seed)
    slices, _ = tr.tensor_slices(classes)
    if case[0] >= 130:      # (at 96 BN7 sees few elements; with one, most gradients are exactly 0)
        assert all(full[2][sl].any() for sl in slices.values())
    for f in range(fc.MAX_FROZEN + 1):
        what = 'f = {}'.format(f)
        got = hip.loss_and_gradients(weights, x, labels, dropout_rate=rate, seed=seed, frozen_blocks=f)
        check_frozen_gradients(got, full, classes, f, what)
        check_frozen_gradients(run_dev(hip, weights, x, labels, rate, seed, f), full, classes, f,
                               what + ' through the device entry')


def test_frozen_blocks_outside_the_range_are_refused(hip):
    weights, x, labels, seed = guarded(96, 3, 2, 0.15)
    lib = hip.load_library()
    flat = weights.flat()
    grads = np.full(flat.size, 7.0, dtype=np.float32)
    stats = np.full(960, 7.0, dtype=np.float32)
    loss, correct = ctypes.c_double(7.0), ctypes.c_int64(7)
    for f in (-1, 8):
        assert lib.dbh_gradients_frozen(flat, flat.size, 2, 96, x, labels, 3, 0.15, seed,
                                        ctypes.byref(loss), ctypes.byref(correct), grads, stats,
                                        f) == INVALID
        # (pointers of 16: aligned and not null, so nothing but frozen_blocks is left to refuse)
        assert lib.dbh_gradients_frozen_dev(16, flat.size, 2, 96, 16, 16, 3, 0.15, seed, 16, 16, 16,
                                            16, 16, None, f) == INVALID
        k = hip.NadamCoefficients(**hip.nadam_schedule(0))
        assert lib.dbh_nadam_update_frozen(16, 16, 16, 16, 16, flat.size, 2, ctypes.byref(k),
                                           f) == INVALID
        assert lib.dbh_nadam_update_frozen_dev(16, 16, 16, 16, 16, flat.size, 2, ctypes.byref(k),
                                               None, f) == INVALID
    assert (grads == 7.0).all() and (stats == 7.0).all() and (loss.value, correct.value) == (7.0, 7)
    with hip.Trainer(weights, 3) as trainer:
        for f in (-1, 8):
            assert lib.dbh_trainer_set_frozen(trainer._handle, f) == INVALID
        assert trainer.frozen_blocks == 0
        trainer.frozen_blocks = 5
        assert trainer.frozen_blocks == 5
        assert lib.dbh_trainer_get_frozen(trainer._handle, None) == INVALID
    for f in (-1, 8):                                   # refused before anything is allocated
        with pytest.raises(ValueError):
            hip.Trainer(weights, 3, frozen_blocks=f)


# ---- 2. f = 0 through the new entries is the old entries -------------------------------------------
def test_no_frozen_blocks_is_the_old_entries_bit_for_bit(hip):
    weights, x, labels, seed = guarded(130, 5, 13, 0.15)
    lib = hip.load_library()
    flat = weights.flat()
    grads = np.zeros(flat.size, dtype=np.float32)
    stats = np.zeros(960, dtype=np.float32)
    loss, correct = ctypes.c_double(0), ctypes.c_int64(0)
    assert lib.dbh_gradients(flat, flat.size, 13, 130, x, labels, 5, 0.15, seed, ctypes.byref(loss),
                             ctypes.byref(correct), grads, stats) == 0
    new = hip.loss_and_gradients(weights, x, labels, dropout_rate=0.15, seed=seed, frozen_blocks=0)
    assert np.float64(new[0]).tobytes() == np.float64(loss.value).tobytes() and new[1] == correct.value
    fc.same_bits(new[2], grads, 'gradients')
    fc.same_bits(new[3], stats, 'batch statistics')

    p, m, v = update_state(13)
    k = hip.nadam_schedule(3, 0.5)
    old = [np.array(a) for a in (p, m, v)]
    coefficients = hip.NadamCoefficients(**k)
    assert lib.dbh_nadam_update(old[0].ctypes.data, grads.ctypes.data, old[1].ctypes.data,
                                old[2].ctypes.data, stats.ctypes.data, p.size, 13,
                                ctypes.byref(coefficients)) == 0
    for name, a, b in zip('pmv', hip.nadam_update(p, grads, m, v, stats, 13, k, frozen_blocks=0), old):
        fc.same_bits(a, b, name)
    assert fc.bits(old[0]).tobytes() != fc.bits(p).tobytes()


# ---- 3. the update ---------------------------------------------------------------------------------
def update_state(classes):
    """p and non-zero m and v EVERYWHERE, the moving slots included: nothing frozen may rely on zeros"""
    n = param_count(classes)
    rng = np.random.default_rng([classes, 37])
    p = rng.standard_normal(n).astype(np.float32)
    m = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 + 1e-3).astype(np.float32)
    assert m.all() and v.all()
    return p, m, v


@pytest.mark.parametrize('f', [1, 4, 7])
def test_update_leaves_frozen_elements_alone(hip, f):
    weights, x, labels, seed = guarded(130, 5, 13, 0.15)
    _, _, grads, stats = hip.loss_and_gradients(weights, x, labels, dropout_rate=0.15, seed=seed)
    p, m, v = update_state(13)
    k = hip.nadam_schedule(2, 0.7)
    mask = fc.frozen_mask(13, f)
    assert 0 < mask.sum() < mask.size
    plain = hip.nadam_update(p, grads, m, v, stats, 13, k)
    got = hip.nadam_update(p, grads, m, v, stats, 13, k, frozen_blocks=f)
    for name, new, old, free in zip('pmv', got, (p, m, v), plain):
        fc.same_bits(new[mask], old[mask], '{}: frozen elements at f = {}'.format(name, f))
        fc.same_bits(new[~mask], free[~mask], '{}: the other elements at f = {}'.format(name, f))
    # the unfrozen call moves what the frozen one leaves: the check above is not empty
    assert (fc.bits(plain[0])[mask] != fc.bits(p)[mask]).mean() > 0.9
    for name, new, want in zip('pmv', got, fc.frozen_update(p, grads, m, v, stats, 13, k, f)):
        fc.same_bits(new, want, name + ': the NumPy restatement')


# ---- 4. the trainer --------------------------------------------------------------------------------
OPTIONS = {'seed': tr.HIGH_SEED, 'dropout_rate': 0.15, 'noise_std': 0.02}


def batch(draw):
    weights, x, labels = tr.case_inputs(130, 5, 13, draw=draw)
    return weights, x, np.roll(labels, draw)


def replay_step(hip, state, x, labels, f):
    """One step on ``state`` from the library's stateless pieces, as the header lists them."""
    seed = ts.step_seed(OPTIONS['seed'], state.iterations)
    noisy = hip.train_noise(x, OPTIONS['noise_std'], seed)
    loss, n_correct, grads, stats = hip.loss_and_gradients(
        state.weights(), noisy, labels, dropout_rate=OPTIONS['dropout_rate'], seed=seed, frozen_blocks=f)
    k = hip.nadam_schedule(state.iterations, state.m_schedule, **OPTIONS)
    state.flat, state.m, state.v = hip.nadam_update(state.flat, grads, state.m, state.v, stats,
                                                    state.n_classes, k, frozen_blocks=f)
    state.iterations += 1
    state.m_schedule = k['sched_new']
    return loss, n_correct


def check_state(trainer, state, what):
    fc.same_bits(trainer.weights().flat(), state.flat, what + ': weights')
    got = trainer.state()
    fc.same_bits(got['m'], state.m, what + ': m')
    fc.same_bits(got['v'], state.v, what + ': v')
    assert (got['iterations'], got['m_schedule']) == (state.iterations, state.m_schedule), what


@pytest.mark.parametrize('f', [2, 4, 7])
def test_trainer_steps_leave_the_frozen_blocks_alone_and_replay(hip, f):
    weights = batch(0)[0]
    start = weights.flat()
    state = ts.State(weights)
    mask = fc.frozen_mask(13, f)
    frozen_moving, live_moving = fc.moving_masks(13, f)
    with hip.Trainer(weights, 5, frozen_blocks=f, **OPTIONS) as trainer:
        assert trainer.frozen_blocks == f
        for step in range(3):
            _, x, labels = batch(step)
            before = state.flat.copy()
            got = trainer.step(x, labels)
            assert got == replay_step(hip, state, x, labels, f), step
            what = 'f = {}, step {}'.format(f, step)
            check_state(trainer, state, what)
            now, moments = trainer.weights().flat(), trainer.state()
            fc.same_bits(now[mask], start[mask], what + ': frozen weights and moving statistics')
            assert not fc.bits(moments['m'])[mask].any() and not fc.bits(moments['v'])[mask].any()
            assert frozen_moving.sum() == 2 * sum(fc.BN_CHANNELS[:f])
            if live_moving.any():                           # (f = 7 leaves none behind it)
                assert (now[live_moving] != before[live_moving]).mean() > 0.9
            assert (now[~mask] != before[~mask]).any()

        # a state with non-zero moments on the frozen tensors: they stay, and so do the weights
        rng = np.random.default_rng(f)
        loaded = {'m': (0.1 * rng.standard_normal(start.size)).astype(np.float32),
                  'v': (rng.standard_normal(start.size) ** 2 + 1e-3).astype(np.float32),
                  'iterations': state.iterations, 'm_schedule': state.m_schedule}
        trainer.load_state(loaded)
        state.m, state.v = loaded['m'].copy(), loaded['v'].copy()
        assert trainer.frozen_blocks == f                   # not part of a state
        _, x, labels = batch(3)
        assert trainer.step(x, labels) == replay_step(hip, state, x, labels, f)
        check_state(trainer, state, 'f = {} after load_state'.format(f))
        now, moments = trainer.weights().flat(), trainer.state()
        fc.same_bits(now[mask], start[mask], 'frozen weights under loaded moments')
        fc.same_bits(moments['m'][mask], loaded['m'][mask], 'frozen m under loaded moments')
        fc.same_bits(moments['v'][mask], loaded['v'][mask], 'frozen v under loaded moments')


def test_set_frozen_between_steps_takes_effect_at_the_next(hip):
    weights = batch(0)[0]
    state = ts.State(weights)
    plan = [0, 0, 6]
    with hip.Trainer(weights, 5, **OPTIONS) as trainer:
        for step, f in enumerate(plan):
            if trainer.frozen_blocks != f:
                trainer.frozen_blocks = f
            _, x, labels = batch(step)
            before = trainer.weights().flat()
            assert trainer.step(x, labels) == replay_step(hip, state, x, labels, f)
            check_state(trainer, state, 'step {} at f = {}'.format(step, f))
            moved = fc.bits(trainer.weights().flat()) != fc.bits(before)
            mask = fc.frozen_mask(13, 6)
            assert (not moved[mask].any()) if f else moved[mask].mean() > 0.5


def test_queued_dataset_steps_use_the_frozen_blocks(hip):
    """The data-set entries and an epoch queued whole: the same trainer state as the same steps
    one by one, and the frozen blocks as they began."""
    weights = batch(0)[0]
    rng = np.random.default_rng(5)
    samples = rng.integers(-400, 400, size=(12, 130)).astype(np.int16)
    labels = rng.integers(13, size=12).astype(np.int32)
    order = rng.permutation(12)
    mask = fc.frozen_mask(13, 4)
    with hip.Dataset(samples, labels, 13) as data, \
            hip.Trainer(weights, 4, frozen_blocks=4, **OPTIONS) as epoch, \
            hip.Trainer(weights, 4, frozen_blocks=4, **OPTIONS) as single:
        losses, counts = epoch.run_epoch(data, order, 4, 2.0)
        want = [single.step_dataset(data, order[4 * t:4 * t + 4], 2.0) for t in range(3)]
        assert [(float(a), int(b)) for a, b in zip(losses, counts)] == want
        fc.same_bits(epoch.weights().flat(), single.weights().flat(), 'weights')
        fc.same_bits(epoch.weights().flat()[mask], weights.flat()[mask], 'frozen blocks')
        assert (epoch.weights().flat()[~mask] != weights.flat()[~mask]).mean() > 0.5


# ---- 5. it learns ----------------------------------------------------------------------------------
def test_the_head_alone_learns_behind_a_frozen_front(hip):
    """finetune_cases says how the task and the step count were chosen on the fp64 reference: its
    loss falls from 0.953 at the first head-only step to 0.250 at step HEAD_STEPS = 75
    (tests/test_finetune.py asserts the halving).  The device trains its own five-class source,
    re-draws the head for three classes and has to end below where it began."""
    train, _ = ts.learning_batches()
    pre, steps = fc.HEAD_PRETRAIN_STEPS, fc.HEAD_STEPS
    source = ModelWeights.fresh(fc.HEAD_SOURCE_CLASSES, ts.LEARN_INPUT, seed=ts.LEARN_WEIGHT_SEED)
    with hip.Trainer(source, ts.LEARN_BATCH, **ts.LEARN_OPTIONS) as trainer:
        for x, labels in train[:pre]:
            trainer.step(x, labels)
        source = trainer.weights()
    start = source.with_fresh_head(ts.LEARN_CLASSES, seed=fc.HEAD_SEED)
    mask = fc.frozen_mask(ts.LEARN_CLASSES, fc.MAX_FROZEN)
    with hip.Trainer(start, ts.LEARN_BATCH, frozen_blocks=fc.MAX_FROZEN, **ts.LEARN_OPTIONS) as trainer:
        losses = [trainer.step(x, labels)[0] for x, labels in train[pre:pre + steps]]
        trained = trainer.weights().flat()
    print('head only: first loss {:.4f}, loss of step {} {:.4f}, mean of the last five {:.4f}'.format(
        losses[0], steps, losses[-1], float(np.mean(losses[-5:]))))
    assert len(losses) == steps and losses[-1] < losses[0]
    fc.same_bits(trained[mask], start.flat()[mask], 'the frozen front')
    head = tr.tensor_slices(ts.LEARN_CLASSES)[0]
    for name in ('conv1d_20/kernel', 'conv1d_20/bias'):
        assert (trained[head[name]] != start.flat()[head[name]]).all(), name


# ---- 6. fit, end to end ----------------------------------------------------------------------------
def training_file(path, fold=None):
    """26 windows of 1,024 samples cut from the golden training text's five signals at six offsets,
    labelled 0 .. 12 in turn (``fold``: label % fold)."""
    with open(os.path.join(GOLD, 'training_data.txt')) as f:
        signals = [line.rstrip('\n').split('\t')[1].split(',') for line in f]
    cuts = [signal[at:at + 1024] for at in range(0, 1501, 300) for signal in signals][:26]
    with open(path, 'w') as f:
        for i, cut in enumerate(cuts):
            f.write('{}\t{}\n'.format(i % 13 if fold is None else i % 13 % fold, ','.join(cut)))
    return str(path)


def run_fit(tmp_path, capsys, name, extra, fold=None):
    data = training_file(tmp_path / (name + '.txt'), fold)
    out = str(tmp_path / (name + '.dbw'))
    start = os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw')
    cli.main(['fit', '--train', data, '--val', data, '--model_out', out, '--model_in', start,
              '--epochs', '1', '--batch_size', '13', '--batches_per_epoch', '2', '--seed', '3'] + extra)
    return ModelWeights.load(start)[0], out, capsys.readouterr().out


def test_fit_with_frozen_blocks_writes_a_model_classify_loads(hip, tmp_path, capsys):
    import deepbinner_amd.classify as classify
    start, out, text = run_fit(tmp_path, capsys, 'frozen', ['--freeze', '6'])
    assert 'Frozen blocks: 6 of 7 - training 14,653 of 107,197 parameters' in text
    assert 'Epoch 1/1' in text
    model, input_size, output_size = classify.load_trained_model(out)
    model.close()
    assert (input_size, output_size) == (1024, 13)
    written = ModelWeights.load(out)[0].flat()
    mask = fc.frozen_mask(13, 6)
    assert written[mask].tobytes() == start.flat()[mask].tobytes()
    slices, moving = tr.tensor_slices(13)
    for name in fc.tensor_names(6)[1]:
        assert written[slices[name]].tobytes() != start.flat()[slices[name]].tobytes(), name
    assert written[moving[6]].tobytes() != start.flat()[moving[6]].tobytes()


def test_fit_with_a_fresh_head_takes_another_class_count(hip, tmp_path, capsys):
    start, out, text = run_fit(tmp_path, capsys, 'folded', ['--fresh_head', '--freeze', '7'], fold=4)
    assert 'Number of possible barcode classifications = 4' in text
    assert 'Frozen blocks: 7 of 7 - training 196 of 106,756 parameters' in text
    written = ModelWeights.load(out)[0]
    assert written.n_classes == 4 and written.input_size == 1024
    for (kernel, bias), (k0, b0) in zip(written.convs[:-1], start.convs[:-1]):
        assert kernel.tobytes() == k0.tobytes() and bias.tobytes() == b0.tobytes()
    for got, want in zip(written.bns, start.bns):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    head = start.with_fresh_head(4, seed=3).convs[-1]
    assert written.convs[-1][0].tobytes() != head[0].tobytes()          # and the head has trained
