"""What feeding a step from a resident data set costs: 200 queued dbh_trainer_step_dataset_dev calls
at augmentation 2 against 200 queued dbh_trainer_step_dev calls on windows already on the device -
at (1024, 13) for batches of 20 (the reference's default, deepbinner.py:265) and 256, and at
(16384, 13) for 20, where the selection runs over the most positions.  Then the assemble kernel
alone, 200 queued calls, at augmentation 2, at 1 (no slot augmented: gather and normalise only) and
at 1e9 (every slot runs the selection).  Host clock around queued work that ends in a synchronise;
the two steps alternate, five runs each after a warm-up run, so the plain step's own run-to-run
spread is beside the difference.  Last, one epoch of 100 steps through Trainer.run_epoch (what `fit`
does) against a host-fed loop over the same indices: Dataset.batch, then Trainer.step.  A first
measurement: no threshold.

    python tools/fit_rate.py > profiles/fit/steps_gpu.txt
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from deepbinner_amd import hip_backend as hip                     # noqa: E402
from deepbinner_amd.model_format import ModelWeights             # noqa: E402

CALLS, RUNS, SAMPLES, AUG = 200, 5, 4096, 2.0


def measure(size, n):
    weights = ModelWeights.fresh(13, size, seed=1)
    rng = np.random.default_rng([size, n])
    samples = np.rint(500 + 60 * rng.standard_normal((SAMPLES, size))).astype(np.int16)
    labels = rng.integers(13, size=SAMPLES).astype(np.int32)
    data = hip.Dataset.from_arrays(samples, labels, 13)
    picks = rng.integers(SAMPLES, size=(CALLS, n)).astype(np.int64)
    indices = hip.DeviceBuffer.from_array(picks)
    first_x, first_labels = data.batch(picks[0])
    x, x_labels = hip.DeviceBuffer.from_array(first_x), hip.DeviceBuffer.from_array(first_labels)
    loss, correct = hip.DeviceBuffer(8), hip.DeviceBuffer(8)
    plain = hip.Trainer(weights, n, seed=1)
    fed = hip.Trainer(weights, n, seed=1)
    stream = hip.Stream()

    def step():
        for _ in range(CALLS):
            plain.step_dev(x.ptr, x_labels.ptr, n, loss.ptr, correct.ptr, stream.ptr)

    def step_dataset():
        for t in range(CALLS):
            fed.step_dataset_dev(data, indices.ptr + 8 * n * t, n, AUG, loss.ptr, correct.ptr,
                                 stream.ptr)

    def assemble(aug=AUG):
        for t in range(CALLS):
            data.batch_dev(indices.ptr + 8 * n * t, n, aug, t, x.ptr, x_labels.ptr, stream.ptr)

    def copy_only():            # augmentation 1: no slot is augmented, the kernel gathers and normalises
        assemble(1.0)

    def all_augmented():        # every slot runs the selection
        assemble(1e9)

    def run(fn):
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) / CALLS

    run(step), run(step_dataset)
    times = {'step': [], 'step_dataset': []}
    for _ in range(RUNS):
        times['step'].append(run(step))
        times['step_dataset'].append(run(step_dataset))
    for name, fn in (('assemble', assemble), ('assemble aug 1', copy_only),
                     ('assemble aug 1e9', all_augmented)):
        run(fn)
        times[name] = [run(fn) for _ in range(RUNS)]
    for name in ('step', 'step_dataset', 'assemble', 'assemble aug 1', 'assemble aug 1e9'):
        t = times[name]
        print('L {:5d} batch {:3d}  {:16s} ms per call: {}   median {:.4f}'.format(
            size, n, name, '  '.join('{:.4f}'.format(v * 1e3) for v in t), np.median(t) * 1e3))
    s, d = np.median(times['step']), np.median(times['step_dataset'])
    spread = (max(times['step']) - min(times['step'])) / s
    print('L {:5d} batch {:3d}  step_dataset / step = {:.4f}; the plain step\'s own spread over its '
          'runs: {:.4f} of its median; assemble alone / step = {:.4f}'.format(
              size, n, d / s, spread, np.median(times['assemble']) / s))
    for thing in (plain, fed, stream, data):
        thing.close()


def epoch(size=1024, n=20, steps=100):
    weights = ModelWeights.fresh(13, size, seed=1)
    rng = np.random.default_rng(7)
    samples = np.rint(500 + 60 * rng.standard_normal((SAMPLES, size))).astype(np.int16)
    labels = rng.integers(13, size=SAMPLES).astype(np.int32)
    order = hip.epoch_order(1, 0, SAMPLES)[:steps * n]
    with hip.Dataset.from_arrays(samples, labels, 13) as data:
        for name in ('queued', 'host-fed', 'queued', 'host-fed'):
            with hip.Trainer(weights, n, seed=1) as trainer:
                t0 = time.perf_counter()
                if name == 'queued':
                    losses, _ = trainer.run_epoch(data, order, n, AUG)
                else:
                    losses = []
                    for t in range(steps):
                        x, batch_labels = data.batch(order[t * n:(t + 1) * n], AUG,
                                                     hip.step_seed(1, t))
                        losses.append(trainer.step(x, batch_labels)[0])
                seconds = time.perf_counter() - t0
            print('L {} batch {}  one epoch of {} steps, {:8s}: {:.1f} ms ({:.3f} ms per step), last '
                  'loss {!r}'.format(size, n, steps, name, seconds * 1e3, seconds * 1e3 / steps,
                                     float(losses[-1])))


def main():
    print('# C = 13, fresh weights, dropout 0.15, noise 0.02, augmentation {}; {} samples resident; one '
          'MI355X ({}), one session; {} queued calls per run, then one synchronise; {} alternating runs '
          'after one warm-up run each'.format(AUG, SAMPLES, hip.device_name(0), CALLS, RUNS))
    for size, n in ((1024, 20), (1024, 256), (16384, 20)):
        measure(size, n)
    epoch()


if __name__ == '__main__':
    main()
