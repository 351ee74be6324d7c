"""The learning task of tests/test_gpu_trainer.py on the fp64 NumPy reference
(tests/train_step_reference.full_step: same hash, same noise, same update), on the CPU: the task and
the step count are chosen so that THIS run ends with its mean training loss over the last 10 steps
under a quarter of ln 3 and a held-out batch of 64 fully right through the inference forward pass
(oracle/network_ref.forward, moving statistics).  The GPU test asserts twice that loss and 60 of 64.

    python tools/train_step_learning.py > profiles/train_step/learning.txt
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import train_step_reference as ts                                # noqa: E402
from oracle import network_ref                                   # noqa: E402


def main():
    train, (held_x, held_labels) = ts.learning_batches()
    state = ts.State(ts.learning_weights())
    print('# fp64 NumPy reference, no GPU: {} classes, input size {}, a motif of {} samples x {} at a '
          'random offset in N(0, 1); fresh weights (seed {}), batches of {}, options {}, the rest '
          'the defaults'.format(ts.LEARN_CLASSES, ts.LEARN_INPUT, ts.MOTIF_LENGTH, ts.MOTIF_SCALE,
                                ts.LEARN_WEIGHT_SEED, ts.LEARN_BATCH, ts.LEARN_OPTIONS))
    losses = []
    for i, (x, labels) in enumerate(train, start=1):
        loss, _ = ts.full_step(state, x, labels, **ts.LEARN_OPTIONS)
        losses.append(loss)
        if i % 25 == 0:
            probs = network_ref.forward(state.weights(), held_x, dtype=np.float64)
            print('step {:4d}  mean loss of the last 10 steps {:.4f}  held-out right {:2d} of 64'
                  .format(i, np.mean(losses[-10:]), int((probs.argmax(axis=1) == held_labels).sum())))
    last = float(np.mean(losses[-10:]))
    probs = network_ref.forward(state.weights(), held_x, dtype=np.float64)
    right = int((probs.argmax(axis=1) == held_labels).sum())
    print('after {} steps: mean loss of the last 10 steps {:.4f} (a quarter of ln 3: {:.4f}), '
          'held-out {} of 64'.format(len(train), last, np.log(3) / 4, right))
    assert last < np.log(3) / 4 and right == 64


if __name__ == '__main__':
    main()
