#!/usr/bin/env python3
"""What a sweep costs beside the classify calls it replaces, in one process
on one GPU: 10,000 reads of the kind bench.py's configs[1] classifies (seeded squiggle-like int16
signals), each cut to its two ends of max_scan_size + 512 samples as the loaders cut a long read,
in pinned memory, through the two --native models with max_scan_size 12288 (K = 24 scan sizes):

  sweep         one hip_backend.sweep_pair + one sweep_tally of nine thresholds:
                24 windows per read end
  classify_max  (a) one hip_backend.classify_pair at scan size 12288: the same 24 windows per read
                end, one setting's calls
  classify_all  (b) the 24 classify_pair calls, scan sizes 512 .. 12288, that give what the sweep
                gives at ONE threshold: 300 windows per read end

After a warm-up of each - in which the sweep's calls at score difference 0.5 are compared with
(b)'s per-side calls, read by read - the three alternate `--rounds` times; medians and spreads of
the wall time around calls that end synchronised.  A record, not a bound.

    python tools/sweep_rate.py [--reads 10000] [--rounds 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
MAX_SCAN_SIZE, HALF = 12288, 512
THRESHOLDS = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]


def squiggles(n, length, seed):
    """bench.py's synthetic_reads law at another length: 70 % levels N(450, 80) held 8 samples +
    N(0, 8) noise, 25 % Gaussian, 5 % flat; clipped to [0, 2047]."""
    rng = np.random.default_rng(seed)
    kind = rng.random(n)
    levels = np.repeat(rng.normal(450, 80, (n, length // 8)), 8, axis=1) + rng.normal(0, 8, (n, length))
    gauss = rng.normal(450, 60, (n, length))
    flat = np.repeat(rng.integers(300, 700, (n, 1)), length, axis=1)
    sig = np.where(kind[:, None] < 0.70, levels, np.where(kind[:, None] < 0.95, gauss, flat))
    return np.clip(np.rint(sig), 0, 2047).astype(np.int16)


def spread(values):
    values = sorted(values)
    return {'median': values[len(values) // 2], 'min': values[0], 'max': values[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--reads', type=int, default=10000)
    ap.add_argument('--rounds', type=int, default=3)
    opts = ap.parse_args()
    from deepbinner_amd import hip_backend as hb
    from deepbinner_amd.model_format import ModelWeights
    assert hb.device_count() >= 1, 'no HIP device visible'
    lib = hb.load_library()
    models = [hb.HipModel(ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models', name + '.dbw'))[0],
                          device=0) for name in ('EXP-NBD103_read_starts', 'EXP-NBD103_read_ends')]
    n, length = opts.reads, 2 * (MAX_SCAN_SIZE + HALF)         # both kept ends, back to back
    steps = MAX_SCAN_SIZE // HALF
    ptr = ctypes.c_void_p()
    hb.check(lib.dbh_malloc_host(ctypes.byref(ptr), n * length * 2), 'dbh_malloc_host')
    samples = np.ctypeslib.as_array(ctypes.cast(ptr.value, ctypes.POINTER(ctypes.c_int16)), shape=(n * length,))
    for first in range(0, n, 500):
        count = min(500, n - first)
        samples[first * length:(first + count) * length] = squiggles(count, length, 1 + first // 500).reshape(-1)
    offsets = np.arange(n + 1, dtype=np.int64) * length

    def sweep():
        start, end = hb.sweep_pair(models[0], models[1], samples, offsets, MAX_SCAN_SIZE)
        return start, end, hb.sweep_tally(start, end, THRESHOLDS, 13)

    def classify_max():
        return hb.classify_pair(models[0], models[1], samples, offsets, MAX_SCAN_SIZE, 0.5)

    def classify_all():
        return [hb.classify_pair(models[0], models[1], samples, offsets, k * HALF, 0.5, want_sides=True)
                for k in range(1, steps + 1)]

    # warm-up, and the same calls: the sweep at 0.5 beside every one of (b)'s 24 runs
    start, end, counts = sweep()
    classify_max()
    for k, (final, sides, _) in enumerate(classify_all()):
        for (best, margin), calls in zip((start, end), sides):
            assert np.array_equal(np.where((best[:, k] != 0) & (margin[:, k] >= 0.5), best[:, k], 0), calls), k
        assert np.array_equal(np.bincount(final, minlength=13), counts[k, THRESHOLDS.index(0.5), 0, :13]), k
    routes = {'sweep': sweep, 'classify_max': classify_max, 'classify_all': classify_all}
    seconds = {name: [] for name in routes}
    for _ in range(opts.rounds):
        for name, run in routes.items():
            t0 = time.perf_counter()
            run()
            seconds[name].append(time.perf_counter() - t0)
    per_end = {'sweep': steps, 'classify_max': steps, 'classify_all': steps * (steps + 1) // 2}
    print(json.dumps({
        'device': hb.device_name(0), 'reads': n, 'samples_per_read': length, 'pinned': True,
        'max_scan_size': MAX_SCAN_SIZE, 'scan_sizes': steps, 'thresholds': len(THRESHOLDS),
        'rounds': opts.rounds, 'windows_per_read_end': per_end,
        'seconds': {name: spread(s) for name, s in seconds.items()},
        'sweep_over_classify_max_median': spread(seconds['sweep'])['median'] / spread(seconds['classify_max'])['median'],
        'classify_all_over_sweep_median': spread(seconds['classify_all'])['median'] / spread(seconds['sweep'])['median'],
        'same_calls_as_classify_all_at_0.5': True}, indent=1), flush=True)
    hb.check(lib.dbh_free_host(ptr), 'dbh_free_host')


if __name__ == '__main__':
    main()
