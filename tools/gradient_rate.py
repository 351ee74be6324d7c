"""Milliseconds per dbh_gradients_dev call at (1024, 13) for batches of 20 (the reference's default,
deepbinner.py:265) and 256, three runs each, with the general path's forward-only time at the same
shape beside it for scale.  A first measurement: no parent figure and no bar.

    python tools/gradient_rate.py > profiles/train_gradients/rate.txt
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from deepbinner_amd import hip_backend as hip                     # noqa: E402
from deepbinner_amd.model_format import ModelWeights             # noqa: E402

CALLS = 20


def main():
    weights, _ = ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models',
                                                'EXP-NBD103_read_starts.dbw'))
    flat = weights.flat()
    print('# dbh_gradients_dev, L = 1024, C = 13, dropout 0.15; one MI355X ({}), one session, '
          '{} calls per run after 3 warm-up calls'.format(hip.device_name(0), CALLS))
    general = hip.HipModel(weights, device=0, general=True)
    for n in (20, 256):
        rng = np.random.default_rng(n)
        x = rng.standard_normal((n, 1024)).astype(np.float32)
        labels = rng.integers(13, size=n).astype(np.int32)
        bufs = [hip.DeviceBuffer.from_array(a) for a in (flat, x, labels)]
        loss, correct = hip.DeviceBuffer(8), hip.DeviceBuffer(8)
        grads, stats = hip.DeviceBuffer(flat.nbytes), hip.DeviceBuffer(960 * 4)
        probs = hip.DeviceBuffer(n * 13 * 4)
        work = hip.DeviceBuffer(hip.gradients_workspace_bytes(13, 1024, n))

        def step():
            hip.gradients_dev(bufs[0].ptr, flat.size, 13, 1024, bufs[1].ptr, bufs[2].ptr, n, 0.15,
                              1, loss.ptr, correct.ptr, grads.ptr, stats.ptr, work.ptr)

        def forward():
            general.predict_dev(bufs[1].ptr, n, probs.ptr)

        for name, fn in (('loss and gradients', step), ('general forward only', forward)):
            for _ in range(3):
                fn()
            hip.synchronize()
            runs = []
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    fn()
                hip.synchronize()
                runs.append((time.perf_counter() - t0) * 1e3 / CALLS)
            print('batch {:3d}  {:22s} ms per call: {}'.format(
                n, name, '  '.join('{:.3f}'.format(r) for r in runs)))


if __name__ == '__main__':
    main()
