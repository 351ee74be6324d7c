#!/usr/bin/env python3
"""What the evidence costs, in one process on one GPU: `--reads` reads
(10,000) of 6,656 samples - seeded squiggle-like int16 signals, tools/sweep_rate.py's law - through
ONE general-kind model of the shipped start geometry at scan size 6144, side start:

  classify   HipModel.classify_signals: slice, forward, merge and call
  locate     HipModel.locate_signals: the same with the head storing the evidence of every window
             (416 B beside about 244 KB of activations), in groups of one chunk of the layer chain,
             then the rule's kernel and the locations copied back

After a warm-up of each, `--rounds` (5) alternating rounds; medians and spreads.  A record, not a
bound.

    python tools/locate_rate.py [--reads 10000] [--rounds 5] [--out profiles/locate/rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))


def spread(values):
    values = sorted(values)
    return {'median': values[len(values) // 2], 'min': values[0], 'max': values[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--reads', type=int, default=10000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--length', type=int, default=6656)
    ap.add_argument('--out', type=str, default=None)
    opts = ap.parse_args()
    from sweep_rate import squiggles
    from deepbinner_amd import hip_backend as hb
    from deepbinner_amd.model_format import ModelWeights
    assert hb.device_count() >= 1, 'no HIP device visible'
    weights = ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models',
                                             'EXP-NBD103_read_starts.dbw'))[0]
    model = hb.HipModel(weights, device=0, general=True)
    n, length = opts.reads, opts.length
    signals = [s for first in range(0, n, 100)
               for s in squiggles(min(100, n - first), length, 1 + first)]

    def walled(run):
        t0 = time.perf_counter()
        out = run()
        return time.perf_counter() - t0, out

    def classify():
        return model.classify_signals(signals, 'start', 6144, 0.5)

    def locate():
        return model.locate_signals(signals, 'start', 6144, 0.5)

    (_, (c_probs, c_calls)), (_, (probs, calls, locations)) = walled(classify), walled(locate)
    assert np.array_equal(c_probs, probs) and np.array_equal(c_calls, calls)
    seconds = {'classify': [], 'locate': []}
    for _ in range(opts.rounds):
        seconds['classify'].append(walled(classify)[0])
        seconds['locate'].append(walled(locate)[0])
    medians = {name: spread(s)['median'] for name, s in seconds.items()}
    record = {
        'device': hb.device_name(0), 'reads': n, 'samples_per_read': length, 'scan_size': 6144,
        'windows': 12 * n, 'rounds': opts.rounds, 'model': 'EXP-NBD103_read_starts, general-kind',
        'located': int((locations['cls'] != 0).sum()),
        'workspace_bytes_per_group': hb.locate_workspace_bytes(model, n, 6144),
        'seconds': {name: spread(s) for name, s in seconds.items()},
        'classify_reads_per_s': n / medians['classify'],
        'locate_reads_per_s': n / medians['locate'],
        'locate_over_classify': medians['locate'] / medians['classify'],
    }
    text = json.dumps(record, indent=1)
    print(text, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
