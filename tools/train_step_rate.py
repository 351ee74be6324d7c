"""200 queued dbh_trainer_step_dev calls against 200 queued dbh_gradients_dev calls at (1024, 13)
for batches of 20 (the reference's default, deepbinner.py:265) and 256: what noise and update add
to the gradient pass.  Host clock around queued work that ends in a synchronise; the two alternate,
five runs each after a warm-up run, so the gradient call's own run-to-run spread is beside the
difference.  A first measurement: no threshold.

    python tools/train_step_rate.py > profiles/train_step/steps_gpu.txt
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from deepbinner_amd import hip_backend as hip                     # noqa: E402
from deepbinner_amd.model_format import ModelWeights             # noqa: E402

CALLS, RUNS = 200, 5


def main():
    weights, _ = ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models',
                                                'EXP-NBD103_read_starts.dbw'))
    flat = weights.flat()
    print('# L = 1024, C = 13, dropout 0.15, noise 0.02; one MI355X ({}), one session; {} queued calls '
          'per run, then one synchronise; {} alternating runs after one warm-up run each'.format(
              hip.device_name(0), CALLS, RUNS))
    for n in (20, 256):
        rng = np.random.default_rng(n)
        x = hip.DeviceBuffer.from_array(rng.standard_normal((n, 1024)).astype(np.float32))
        labels = hip.DeviceBuffer.from_array(rng.integers(13, size=n).astype(np.int32))
        w = hip.DeviceBuffer.from_array(flat)
        loss, correct = hip.DeviceBuffer(8), hip.DeviceBuffer(8)
        grads, stats = hip.DeviceBuffer(flat.nbytes), hip.DeviceBuffer(960 * 4)
        work = hip.DeviceBuffer(hip.gradients_workspace_bytes(13, 1024, n))
        trainer = hip.Trainer(weights, n, seed=1)
        stream = hip.Stream()

        def gradients():
            hip.gradients_dev(w.ptr, flat.size, 13, 1024, x.ptr, labels.ptr, n, 0.15, 1, loss.ptr,
                              correct.ptr, grads.ptr, stats.ptr, work.ptr, stream.ptr)

        def step():
            trainer.step_dev(x.ptr, labels.ptr, n, loss.ptr, correct.ptr, stream.ptr)

        def run(fn):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            stream.synchronize()
            return (time.perf_counter() - t0) / CALLS

        run(gradients), run(step)
        times = {'gradients': [], 'step': []}
        for _ in range(RUNS):
            times['gradients'].append(run(gradients))
            times['step'].append(run(step))
        for name in ('gradients', 'step'):
            t = times[name]
            print('batch {:3d}  {:9s} ms per call: {}   median {:.3f}  ({:.1f} calls/s, {:.0f} windows/s)'
                  .format(n, name, '  '.join('{:.3f}'.format(v * 1e3) for v in t),
                          np.median(t) * 1e3, 1 / np.median(t), n / np.median(t)))
        g, s = np.median(times['gradients']), np.median(times['step'])
        spread = (max(times['gradients']) - min(times['gradients'])) / g
        print('batch {:3d}  step / gradients = {:.4f}; the gradient call\'s own spread over its runs: '
              '{:.4f} of its median'.format(n, s / g, spread))
        final = float(loss.download(1, np.float64)[0])
        print('batch {:3d}  loss of the last step {:.4f} after {} steps on one batch'.format(
            n, final, trainer.iterations))
        trainer.close()
        stream.close()


if __name__ == '__main__':
    main()
