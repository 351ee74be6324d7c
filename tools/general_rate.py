#!/usr/bin/env python3
"""Throughput of the general forward path (models of any input size / class count), one GPU:

    python tools/general_rate.py [--windows 16384] [--reps 5] [--reads 20000] [--out FILE]

  - windows/s of dbh_predict_dev (fp32 windows already on the device, HIP events around the
    launches) for the general path at (L, C) = (1024, 13), (2048, 13), (1024, 97), (4096, 25) and
    for the persistent kernel at (1024, 13), in the same process;
  - end-to-end reads/s of dbh_classify_pair_i16 (host int16 reads in, calls out) with a (1024, 97)
    start + end pair, scan size 6144.
Models are the shipped EXP-NBD103 weights reloaded / widened as tests/general_fixtures.py does.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def windows_per_second(hb, model, n, reps):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((n, model.input_size)).astype(np.float32)
    d_x = hb.DeviceBuffer.from_array(x)
    d_p = hb.DeviceBuffer(n * model.n_classes * 4)
    model.predict_dev(d_x.ptr, n, d_p.ptr)           # warm-up (and workspace growth)
    hb.synchronize()
    a, b = hb.Event(), hb.Event()
    a.record()
    for _ in range(reps):
        model.predict_dev(d_x.ptr, n, d_p.ptr)
    b.record()
    b.synchronize()
    return n * reps / (a.elapsed_ms(b) / 1e3)


def pair_reads_per_second(hb, start, end, n_reads, reps):
    rng = np.random.default_rng(2)
    lengths = np.clip(rng.lognormal(np.log(20000), 0.5, n_reads), 2000, 200000).astype(np.int64)
    keep = np.minimum(lengths, 2 * (6144 + 512))      # the scanned ends, as the loaders keep them
    offsets = np.zeros(n_reads + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(keep)
    samples = np.clip(rng.normal(450, 80, int(offsets[-1])), 0, 2047).astype(np.int16)
    hb.classify_pair(start, end, samples, offsets, 6144, 0.5)     # warm-up
    t = time.perf_counter()
    for _ in range(reps):
        hb.classify_pair(start, end, samples, offsets, 6144, 0.5)
    return n_reads * reps / (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--windows', type=int, default=16384)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--reads', type=int, default=20000)
    ap.add_argument('--out')
    args = ap.parse_args()
    from deepbinner_amd import hip_backend as hb
    from general_fixtures import ENDS, geometry
    rows = []
    for (L, C, general) in [(1024, 13, False), (1024, 13, True), (2048, 13, False),
                            (1024, 97, False), (4096, 25, False)]:
        model = hb.HipModel(geometry(L, C), device=0, general=general)
        n = max(256, args.windows * 1024 // L)
        rate = windows_per_second(hb, model, n, args.reps)
        rows.append({'input_size': L, 'n_classes': C,
                     'path': 'general' if model.kind == 1 else 'persistent',
                     'windows': n, 'windows_per_s': round(rate)})
        print('L={:5d} C={:3d} {:10s} {:>12,.0f} windows/s'.format(L, C, rows[-1]['path'], rate),
              flush=True)
        model.close()
    start = hb.HipModel(geometry(1024, 97), device=0)
    end = hb.HipModel(geometry(1024, 97, name=ENDS), device=0)
    reads = pair_reads_per_second(hb, start, end, args.reads, args.reps)
    print('classify_pair_i16 (1024, 97) start + end, scan 6144: {:,.0f} reads/s'.format(reads))
    result = {'device': hb.device_name(0), 'forward': rows,
              'pair_1024_97_reads_per_s': round(reads), 'pair_reads': args.reads}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
