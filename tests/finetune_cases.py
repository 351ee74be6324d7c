"""A helper, not a test: frozen blocks (include/deepbinner_hip.h, "FROZEN BLOCKS"; DESIGN.md
section 38) restated from the header's table alone, for tests/test_finetune.py and
tests/test_gpu_finetune.py - which tensors and which moving statistics f frozen blocks cover, the
update with those left alone, and the learning task of the head-only test.

Nothing here has a tolerance: a frozen call is held to the same call at f = 0, bit for bit.
"""
import numpy as np

import train_reference as tr
import train_step_reference as ts
from deepbinner_amd.model_format import BN_CHANNELS, ModelWeights

MAX_FROZEN = 7
# f -> the last frozen convolution, conv1d_<that>; batch_normalization_1 .. f are frozen with them
LAST_FROZEN_CONV = {0: 0, 1: 1, 2: 4, 3: 7, 4: 9, 5: 16, 6: 17, 7: 19}


def tensor_names(f):
    """(frozen, trainable): the names of train_reference.tensor_slices, split at f blocks."""
    frozen = ['conv1d_%d/%s' % (i, part) for i in range(1, LAST_FROZEN_CONV[f] + 1)
              for part in ('kernel', 'bias')]
    frozen += ['bn_%d/%s' % (j, part) for j in range(1, f + 1) for part in ('gamma', 'beta')]
    slices, _ = tr.tensor_slices(2)
    return frozen, [name for name in slices if name not in frozen]


def frozen_mask(n_classes, f):
    """bool [param_count]: the elements a step with f frozen blocks must leave alone in p, m and v
    - the frozen tensors and the moving statistics of batch_normalization_1 .. f."""
    slices, moving = tr.tensor_slices(n_classes)
    mask = np.zeros(moving[-1].stop, dtype=bool)
    for name in tensor_names(f)[0]:
        mask[slices[name]] = True
    for sl in moving[:f]:
        mask[sl] = True
    return mask


def moving_masks(n_classes, f):
    """(frozen, live): bool masks of the moving statistics of bn_1 .. f and of bn_f+1 .. 7."""
    _, moving = tr.tensor_slices(n_classes)
    frozen = np.zeros(moving[-1].stop, dtype=bool)
    live = np.zeros_like(frozen)
    for j, sl in enumerate(moving):
        (frozen if j < f else live)[sl] = True
    return frozen, live


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    differ = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert differ.size == 0, '{}: {} of {} differ, first at {}: {!r} against {!r}'.format(
        what, differ.size, np.size(want), differ[0], np.ravel(got)[differ[0]], np.ravel(want)[differ[0]])


def frozen_update(params, grads, m, v, batch_stats, n_classes, k, f):
    """dbh_nadam_update_frozen in NumPy: train_step_reference's update, the frozen elements put
    back as they were."""
    out = ts.nadam_update(params, grads, m, v, batch_stats, n_classes, k)
    mask = frozen_mask(n_classes, f)
    for new, old in zip(out, (params, m, v)):
        new[mask] = np.asarray(old, dtype=np.float32)[mask]
    return out


# ---- the head-only learning test -----------------------------------------------------------------
# train_step_reference's three-motif task.  The source is a model of FIVE classes trained on the
# task's first HEAD_PRETRAIN_STEPS batches with nothing frozen (a head behind an untrained front
# learns nothing: 300 steps leave the fp64 reference's loss at 1.0 to 1.3).  Its head is then re-drawn
# for the task's three classes and trained alone, f = 7, on the HEAD_STEPS batches that follow.
# HEAD_STEPS is chosen on the fp64 reference alone (head_only_reference): a step count at which
# both the loss of the last step and the mean of the last five are at most half of the first step's
# loss - 0.953 at first; step 75 has 0.250, the last five a mean of 0.285 (a step's loss is that of
# 16 windows under dropout and moves by 0.2 from one to the next; step 36 is the first to meet both).
HEAD_SOURCE_CLASSES = 5
HEAD_SEED = 11
HEAD_PRETRAIN_STEPS = 150
HEAD_STEPS = 75


def head_only_reference():
    """The fp64 reference's losses of the HEAD_STEPS head-only steps, from its own source model."""
    train, _ = ts.learning_batches()
    source = ts.State(ModelWeights.fresh(HEAD_SOURCE_CLASSES, ts.LEARN_INPUT, seed=ts.LEARN_WEIGHT_SEED))
    for x, labels in train[:HEAD_PRETRAIN_STEPS]:
        ts.full_step(source, x, labels, **ts.LEARN_OPTIONS)
    state = ts.State(source.weights().with_fresh_head(ts.LEARN_CLASSES, seed=HEAD_SEED))
    return [ts.full_step(state, x, labels, gradients=head_only_gradients, **ts.LEARN_OPTIONS)[0]
            for x, labels in train[HEAD_PRETRAIN_STEPS:HEAD_PRETRAIN_STEPS + HEAD_STEPS]]


def head_only_gradients(weights, x, labels, rate, seed):
    """train_reference's fp64 gradients with every slot but conv1d_20's zeroed: what
    train_step_reference.full_step takes as ``gradients`` for a step at f = 7."""
    r = tr.loss_and_gradients(weights, x, labels, rate=rate, seed=seed)
    grads = np.array(r.grads)
    grads[frozen_mask(weights.n_classes, MAX_FROZEN)] = 0
    return r.loss, r.n_correct, grads, r.stats
