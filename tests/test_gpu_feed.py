"""Device-fed batches, validation and the fit command on the device (include/deepbinner_hip.h,
"device-fed batches, validation") against tests/feed_reference.py (pinned in
tests/test_feed_reference.py).

A batch is integer work up to one fp64 expression per value, correctly rounded on both sides: equal
bit for bit.  A data-set step is replayed from the stateless pieces (Dataset.batch with the step
seed, then Trainer.step): equal bit for bit.  evaluate is held to section 17's first rule: per case
e32 = max |loss32 - loss64| / max |loss64| of the fp32 NumPy run, and every window of the device
within max(4 e32, 1e-6) of the fp64 loss, relative to max |loss64|
(profiles/fit/evaluate_gpu.txt).  The learning test's lines are section 18's: twice the fp64
restatement's own loss bound and four windows (profiles/fit/learning.txt; the restatement's run is
asserted in tests/test_fit_cli.py).
"""
import ctypes
import os

import numpy as np
import pytest

import feed_reference as fr
import train_reference as tr
import train_step_reference as ts
from deepbinner_amd.model_format import ModelWeights

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    differ = np.flatnonzero(bits(got) != bits(want))
    assert differ.size == 0, '{}: {} of {} differ, first at {}: {!r} against {!r}'.format(
        what, differ.size, np.size(want), differ[0], np.ravel(got)[differ[0]], np.ravel(want)[differ[0]])


def signal_windows(length, n, classes):
    """n int16 windows: signal-like draws, then the constant window, the alternating extremes, a
    full-range draw and the odd-sum extremes (tests/test_feed_reference.py's special windows)."""
    rng = np.random.default_rng([2, length])
    level = rng.integers(300, 700, size=(n - 4, 1))
    spread = rng.integers(5, 120, size=(n - 4, 1))
    x = np.rint(level + spread * rng.standard_normal((n - 4, length))).astype(np.int16)
    labels = rng.integers(classes, size=n).astype(np.int32)
    return np.concatenate([x, fr.special_windows(length)]), labels


# ---- Dataset.batch ---------------------------------------------------------------------------------
# (input size, slots, augmentation, seed).  96 .. 130: half = 24, 24, 26, 32 (L / 4 rounds both ways);
# 1024: one position per thread; 16384: sixteen.  The last two hold a key tie across a rank
# boundary in an augmented slot (tests/test_feed_reference.py::test_equal_keys_rank_by_index).
BATCH_CASES = [(96, 8, 1.0, 1), (96, 64, 2.0, tr.SEED), (98, 9, 1e9, 2), (102, 11, 2.0, tr.HIGH_SEED),
               (130, 16, 1e9, 3), (1024, 33, 2.0, 4), (16384, 8, 2.0, 5),
               (1024, 40, 1e9, 24), (16384, 30, 1e9, 7)]
# Sizes between 1024 and 16384, where a thread holds `per` = 2 .. 16 positions and the last busy
# thread fewer: 1026 (per 2, 513 threads busy), 2050 (per 3, thread 683 holds one), 5000 (per 5,
# 1,000 busy), 16382 (per 16, the last thread holds 14).  Then each size again with a key tie
# across a rank boundary in an augmented slot (tests/test_feed_reference.py, PARTIAL_TIES).
BATCH_CASES += [(1026, 10, 1e9, 11), (2050, 10, 2.0, 12), (5000, 10, 1e9, 13), (16382, 10, 1e9, 14),
                (1026, 40, 1e9, 24), (2050, 16, 1e9, 10), (5000, 14, 1e9, 1), (16382, 30, 1e9, 8)]
# (input size, seed, slot) of the key ties
TIES = [(16384, 7, 29), (1024, 24, 36), (1026, 24, 36), (2050, 10, 14), (5000, 1, 13), (16382, 8, 29)]


@pytest.mark.parametrize('length,slots,aug,seed', BATCH_CASES, ids=str)
def test_batch_equals_the_numpy_restatement_bit_for_bit(hip, length, slots, aug, seed):
    n, classes = 12, 5
    samples, labels = signal_windows(length, n, classes)
    rng = np.random.default_rng([length, slots])
    indices = rng.integers(n, size=slots)
    indices[:6] = [0, n - 1, n - 4, n - 3, n - 2, n - 1]      # both ends, a repeat, the special windows
    indices[-1] = 0
    for tie_length, tie_seed, tie_slot in TIES:
        if (length, seed) == (tie_length, tie_seed):
            assert slots > tie_slot and fr.slot_is_augmented(seed, tie_slot, fr.augment_threshold(aug))
    want_x, want_labels = fr.batch(samples, labels, indices, aug, seed)
    with hip.Dataset.from_arrays(samples, labels, classes) as data:
        assert len(data) == n
        x, got_labels = data.batch(indices, aug, seed)
        same_bits(x, want_x, 'batch')
        assert (got_labels == want_labels).all()
        same_bits(data.batch(indices, aug, seed)[0], x, 'the same call twice')
        # the queued form on device arrays
        on_device = hip.DeviceBuffer.from_array(indices.astype(np.int64))
        x_dev, labels_dev = hip.DeviceBuffer(x.nbytes), hip.DeviceBuffer(4 * slots)
        data.batch_dev(on_device.ptr, slots, aug, seed, x_dev.ptr, labels_dev.ptr)
        hip.synchronize()
        same_bits(x_dev.download(x.shape, np.float32), want_x, 'batch_dev')
        assert (labels_dev.download(slots, np.int32) == want_labels).all()
    augmented = [fr.slot_is_augmented(seed, w, fr.augment_threshold(aug)) for w in range(slots)]
    plain = fr.normalise(samples[indices])
    if aug == 1.0:
        assert not any(augmented)
        same_bits(x, plain, 'aug = 1 copies')
    else:
        assert any(augmented)
        changed = (bits(x) != bits(plain)).any(axis=1)
        constant = indices == n - 4
        assert (changed == (np.array(augmented) & ~constant)).all()


def test_windows_past_the_stats_grid(hip):
    """65,536 + 40 windows of 96: window_stats runs 65,536 workgroups, so the last 40 windows are
    their workgroups' second, and their mean, deviation and label lie past index 65,535.  The last
    40 are signal_windows' draws and special windows."""
    classes, grid = 5, 65536
    rng = np.random.default_rng(96)
    tail, tail_labels = signal_windows(96, 40, classes)
    level = rng.integers(300, 700, size=(grid, 1))
    front = (level + rng.integers(-200, 201, size=(grid, 96))).astype(np.int16)
    samples = np.concatenate([front, tail])
    labels = np.concatenate([rng.integers(classes, size=grid).astype(np.int32), tail_labels])
    n = grid + 40
    indices = np.array([0, grid - 1, grid, n - 1, n - 4, n - 3, n - 2, grid + 1, grid + 17, 1, n - 1])
    aug, seed = 2.0, 6
    picked = samples[indices]
    want_x, want_labels = fr.batch(picked, labels[indices], np.arange(indices.size), aug, seed)
    augmented = [fr.slot_is_augmented(seed, w, fr.augment_threshold(aug)) for w in range(indices.size)]
    assert any(augmented) and not all(augmented)
    with hip.Dataset.from_arrays(samples, labels, classes) as data:
        assert len(data) == n
        x, got_labels = data.batch(indices, aug, seed)
        same_bits(x, want_x, 'batch')
        assert (got_labels == want_labels).all()
        x, got_labels = data.batch(indices, 1.0)
        same_bits(x, fr.normalise(picked), 'aug = 1')
        assert (got_labels == labels[indices]).all()
        # every window's statistics, through batches of all of them in turn
        plain = fr.normalise(samples)
        for first in range(0, n, 8192):
            some = np.arange(first, min(first + 8192, n))
            same_bits(data.batch(some, 1.0)[0], plain[some], 'windows from {}'.format(first))


def test_batch_refuses_before_it_works(hip):
    samples, labels = signal_windows(96, 6, 3)
    lib = hip.load_library()
    with hip.Dataset.from_arrays(samples, labels, 3) as data:
        x = np.full((2, 96), 7, dtype=np.float32)
        out_labels = np.full(2, 7, dtype=np.int32)

        def call(indices, aug=2.0, n=2):
            indices = np.asarray(indices, dtype=np.int64)
            return lib.dbh_dataset_batch(data.handle, indices.ctypes.data, n, aug, 0, x.ctypes.data,
                                         out_labels.ctypes.data)
        assert call([0, 6]) == INVALID and call([-1, 0]) == INVALID
        assert call([0, 1], aug=0.5) == INVALID and call([0, 1], aug=float('nan')) == INVALID
        assert call([0, 1], n=0) == INVALID
        assert call([0, 1], n=2 ** 20 // 96 + 1) == UNSUPPORTED
        assert (x == 7).all() and (out_labels == 7).all()
        assert call([0, 5]) == 0 and (out_labels == labels[[0, 5]]).all()
        # the queued entry cannot check device indices: NaN and the label -1, nothing read outside
        on_device = hip.DeviceBuffer.from_array(np.array([6, -1, 2], dtype=np.int64))
        x_dev, labels_dev = hip.DeviceBuffer(3 * 96 * 4), hip.DeviceBuffer(12)
        data.batch_dev(on_device.ptr, 3, 2.0, 0, x_dev.ptr, labels_dev.ptr)
        hip.synchronize()
        got = x_dev.download((3, 96), np.float32)
        assert np.isnan(got[:2]).all() and np.isfinite(got[2]).all()
        assert list(labels_dev.download(3, np.int32)) == [-1, -1, labels[2]]
        # a trainer of another geometry
        with hip.Trainer(ModelWeights.fresh(4, 96), 4) as other:
            loss, right = ctypes.c_double(7.0), ctypes.c_int64(7)
            indices = np.zeros(2, dtype=np.int64)
            assert lib.dbh_trainer_step_dataset(other._handle, data.handle, indices.ctypes.data, 2,
                                                2.0, ctypes.byref(loss), ctypes.byref(right)) == UNSUPPORTED
            assert lib.dbh_trainer_evaluate_dataset(other._handle, data.handle, 0, 2, ctypes.byref(loss),
                                                    ctypes.byref(right), None) == UNSUPPORTED
        with hip.Trainer(ModelWeights.fresh(3, 96), 4) as trainer:
            def step(indices, aug=2.0, n=2):
                indices = np.asarray(indices, dtype=np.int64)
                return lib.dbh_trainer_step_dataset(trainer._handle, data.handle, indices.ctypes.data,
                                                    n, aug, ctypes.byref(loss), ctypes.byref(right))
            assert step([0, 6]) == INVALID and step([0, 1], aug=0.99) == INVALID
            assert step([0, 1, 2, 3, 4], n=5) == UNSUPPORTED and step([0, 1], n=0) == INVALID
            assert lib.dbh_trainer_evaluate_dataset(trainer._handle, data.handle, 3, 4, ctypes.byref(loss),
                                                    ctypes.byref(right), None) == INVALID
            assert (loss.value, right.value) == (7.0, 7) and trainer.iterations == 0


# ---- evaluate --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fr.EVAL_CASES, ids=str)
def test_evaluate_against_the_fp64_reference(hip, case):
    ref = fr.eval_case(case)
    assert (ref['gap'] > fr.EVAL_GAP).all()
    loss_sum, right, losses = hip.evaluate(ref['weights'], ref['x'], ref['labels'])
    scale = np.abs(ref['loss64']).max()
    e32 = np.abs(ref['loss32'] - ref['loss64']).max() / scale
    bound = max(4 * e32, 1e-6)
    ratios = np.abs(losses - ref['loss64']) / scale / bound
    print('evaluate L{} N{} C{}: e32 {:.3e}, bound {:.3e}, device error / bound per window {}'.format(
        *case, e32, bound, ' '.join('{:.3f}'.format(r) for r in ratios)))
    assert (ratios <= 1.0).all()
    assert right == int((ref['best64'] == ref['labels']).sum())
    total = 0.0
    for value in losses:
        total += float(value)
    assert loss_sum == total                                    # added in window order, fp64
    again = hip.evaluate(ref['weights'], ref['x'], ref['labels'])
    assert again[0] == loss_sum and (again[2] == losses).all()


def test_evaluate_on_a_fresh_model_agrees_with_the_inference_path(hip):
    """Moving mean 0 and moving variance 1: evaluate's calls are those of the general forward path
    (HipModel(general=True).predict) on the same windows."""
    size, n, classes = 130, 8, 13
    weights = ModelWeights.fresh(classes, size, seed=3)
    # A fresh model's logits are a few 1e-3 and close together.  Both device paths are fp32
    # arithmetic, so the windows are the 8 of 32 draws on which the fp64 reference's call is
    # clearest, and that gap must be 64 times the fp32 NumPy run's own largest logit error.
    pool = np.random.default_rng(9).standard_normal((32, size)).astype(np.float32)
    _, _, logits = fr.evaluate(weights, pool, np.zeros(32, dtype=np.int32))
    _, _, logits32 = fr.evaluate(weights, pool, np.zeros(32, dtype=np.int32), np.float32)
    top = np.sort(logits, axis=1)
    clearest = np.sort(np.argsort(top[:, -1] - top[:, -2])[-n:])
    assert ((top[:, -1] - top[:, -2])[clearest] > 64 * np.abs(logits32 - logits).max()).all()
    x, best = pool[clearest], logits[clearest].argmax(axis=1)
    model = hip.HipModel(weights, device=0, general=True)
    probs = model.predict(x[:, :, None])
    model.close()
    calls = probs.argmax(axis=1)
    assert (calls == best).all()
    labels = calls.astype(np.int32)
    labels[::3] = (labels[::3] + 1) % classes
    loss_sum, right, losses = hip.evaluate(weights, x, labels)
    assert right == int((calls == labels).sum()) == n - len(labels[::3])
    assert np.isfinite(losses).all() and loss_sum > 0
    # window by window: a hit with predict's call as the label, a miss with any other
    for w in range(n):
        assert hip.evaluate(weights, x[w:w + 1], [calls[w]])[1] == 1, w
        assert hip.evaluate(weights, x[w:w + 1], [(calls[w] + 1 + w) % classes])[1] == 0, w


def small_set(size, classes, n=7):
    samples, labels = signal_windows(size, max(n, 5), classes)
    return samples[:n], labels[:n]


def trainer_bits(trainer):
    state = trainer.state()
    return (bits(trainer.weights().flat()).copy(), bits(state['m']).copy(), bits(state['v']).copy(),
            state['iterations'], state['m_schedule'])


def assert_same_trainer(a, b, what):
    for name, x, y in zip(('weights', 'm', 'v'), a[:3], b[:3]):
        assert (x == y).all(), '{}: {}'.format(what, name)
    assert a[3:] == b[3:], what


def test_trainer_evaluate_in_chunks_and_without_a_trace(hip):
    size, classes = 130, 13
    samples, labels = small_set(size, classes)
    weights = tr.case_inputs(size, 5, classes, draw=0)[0]
    with hip.Dataset.from_arrays(samples, labels, classes) as data, \
            hip.Trainer(weights, 3, seed=tr.SEED) as chunked, \
            hip.Trainer(weights, 7, seed=tr.SEED) as whole, \
            hip.Trainer(weights, 3, seed=tr.SEED) as twin:
        before = trainer_bits(chunked)
        a = chunked.evaluate(data, window_losses=True)           # 3 + 3 + 1
        b = whole.evaluate(data, window_losses=True)
        assert a[0] == b[0] and a[1] == b[1] and (a[2] == b[2]).all()
        x, batch_labels = data.batch(np.arange(7))
        direct = hip.evaluate(weights, x, batch_labels)
        assert direct[0] == a[0] and direct[1] == a[1] and (direct[2] == a[2]).all()
        part = chunked.evaluate(data, first=2, count=4, window_losses=True)
        assert (part[2] == a[2][2:6]).all()
        assert_same_trainer(trainer_bits(chunked), before, 'after evaluate')
        # the workspace is shared: the next step is that of a twin which did not evaluate
        got = chunked.step_dataset(data, [0, 6, 3], 2.0)
        want = twin.step_dataset(data, [0, 6, 3], 2.0)
        assert got == want
        assert_same_trainer(trainer_bits(chunked), trainer_bits(twin), 'the step after evaluate')
        assert chunked.evaluate(data) != a[:2]                  # and the weights moved


# ---- data-set steps --------------------------------------------------------------------------------
@pytest.mark.parametrize('size,classes', [(96, 3), (1024, 13)], ids=str)
def test_dataset_steps_replay_from_batch_and_step(hip, size, classes):
    n, batch, aug = 12, 4, 2.0
    samples, labels = signal_windows(size, n, classes)
    weights = tr.case_inputs(size, batch, classes, draw=0)[0]
    picks = [np.random.default_rng([size, t]).integers(n, size=batch) for t in range(4)]
    with hip.Dataset.from_arrays(samples, labels, classes) as data:
        with hip.Trainer(weights, batch, seed=tr.HIGH_SEED) as fed, \
                hip.Trainer(weights, batch, seed=tr.HIGH_SEED) as replay:
            results = []
            for t in range(3):
                got = fed.step_dataset(data, picks[t], aug)
                x, batch_labels = data.batch(picks[t], aug, ts.step_seed(tr.HIGH_SEED, t))
                assert got == replay.step(x, batch_labels), t
                assert_same_trainer(trainer_bits(fed), trainer_bits(replay), 'step {}'.format(t))
                results.append(got)
            got = fed.step_dataset(data, picks[3], aug)
            x, batch_labels = data.batch(picks[3], aug, ts.step_seed(tr.HIGH_SEED, 3))
            assert got == replay.step(x, batch_labels)
            results.append(got)
            final = trainer_bits(fed)
        # the queued form: four steps on device indices, one synchronisation
        with hip.Trainer(weights, batch, seed=tr.HIGH_SEED) as queued:
            stream = hip.Stream()
            on_device = hip.DeviceBuffer.from_array(np.concatenate(picks).astype(np.int64))
            losses, counts = hip.DeviceBuffer(4 * 8), hip.DeviceBuffer(4 * 8)
            for t in range(4):
                queued.step_dataset_dev(data, on_device.ptr + 8 * batch * t, batch, aug,
                                        losses.ptr + 8 * t, counts.ptr + 8 * t, stream.ptr)
            stream.synchronize()
            assert_same_trainer(trainer_bits(queued), final, 'four queued steps')
            assert list(losses.download(4, np.float64)) == [r[0] for r in results]
            assert list(counts.download(4, np.int64)) == [r[1] for r in results]
            stream.close()
        # and run_epoch, which fit uses
        with hip.Trainer(weights, batch, seed=tr.HIGH_SEED) as epoch:
            got_losses, got_counts = epoch.run_epoch(data, np.concatenate(picks), batch, aug)
            assert list(got_losses) == [r[0] for r in results]
            assert list(got_counts) == [r[1] for r in results]
            assert_same_trainer(trainer_bits(epoch), final, 'run_epoch')


def test_a_smaller_batch_leaves_nothing_of_the_one_before(hip):
    size, classes = 130, 13
    samples, labels = signal_windows(size, 12, classes)
    weights = tr.case_inputs(size, 8, classes, draw=0)[0]
    with hip.Dataset.from_arrays(samples, labels, classes) as data, \
            hip.Trainer(weights, 8, seed=tr.SEED) as fed, hip.Trainer(weights, 8, seed=tr.SEED) as replay:
        for t, picks in enumerate(([0, 1, 2, 3, 4, 5, 6, 7], [11, 9, 10])):
            got = fed.step_dataset(data, picks, 2.0)
            x, batch_labels = data.batch(picks, 2.0, ts.step_seed(tr.SEED, t))
            assert got == replay.step(x, batch_labels)
            assert_same_trainer(trainer_bits(fed), trainer_bits(replay), '{} windows'.format(len(picks)))


# ---- fit, end to end -------------------------------------------------------------------------------
def test_fit_learns_and_the_same_command_gives_the_same_files(hip, tmp_path, capsys):
    """The task, the step count and the restatement's own figures: tests/feed_reference.py and
    profiles/fit/learning.txt (the fp64 restatement ends its last epoch at a training loss of
    0.1824, under a quarter of ln 4 = 0.3466, and calls 64 of 64 with the saved model:
    tests/test_fit_cli.py).  The device gets twice the loss and four windows."""
    from deepbinner_amd import deepbinner as cli
    (train_x, train_l), (val_x, val_l) = fr.fit_sets()
    train, val = str(tmp_path / 'train.txt'), str(tmp_path / 'val.txt')
    fr.write_training_file(train, train_x, train_l)
    fr.write_training_file(val, val_x, val_l)
    outs = [str(tmp_path / name) for name in ('first.dbw', 'second.dbw')]
    texts = []
    for out in outs:
        capsys.readouterr()
        cli.main(['fit', '--train', train, '--val', val, '--model_out', out, '--batch_size',
                  str(fr.FIT_BATCH), '--epochs', str(fr.FIT_EPOCHS), '--aug', '2', '--seed',
                  str(fr.FIT_SEED)])
        texts.append(capsys.readouterr().out)
    epochs = [fr.EPOCH_LINE.match(line) for line in texts[0].splitlines() if line.startswith('Epoch ')]
    assert len(epochs) == fr.FIT_EPOCHS and all(epochs)
    for m in epochs:
        print(m.group(0).replace(str(tmp_path), '<WORK>'))
    assert float(epochs[-1].group(3)) < np.log(4) / 2
    weights, _ = ModelWeights.load(outs[0])
    model = hip.HipModel(weights, device=0)
    probs = model.predict(fr.normalise(val_x)[:, :, None])
    model.close()
    right = int((probs.argmax(axis=1) == val_l).sum())
    print('the saved model calls {} of 64 validation windows right'.format(right))
    assert right >= 60
    assert texts[0].replace(outs[0], '') == texts[1].replace(outs[1], '')
    for suffix in ('', '.state.npz'):
        with open(outs[0] + suffix, 'rb') as a, open(outs[1] + suffix, 'rb') as b:
            assert a.read() == b.read(), suffix or 'model file'
    assert os.path.getsize(outs[0] + '.state.npz') > 0
