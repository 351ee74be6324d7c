"""Reads per second of prep's adapter scan, two ways on the same synthetic reads, alternating:

  resident   prep_signal.locate_adapters: one dtw_locate_batch call for the batch
  host loop  what there was before it: trim and normalise on the host, then one
             semi_global_dtw_with_rescaling_batch call per window index over the reads that have
             not hit yet (two blocking passes, alignments to the host, lstsq per pair)

  python tools/prep_signal_rate.py [--reads 2000] [--samples 20000] [--query 400] [--side start]
                                   [--repeats 5] [--out FILE]

Prints one JSON line (and writes it to --out).  Both ways start from the raw int16 reads and end
with the adapter positions; the wall clock runs around the whole call, which ends in a device
synchronise.  Most reads carry the adapter in window 0, as real reads do; the resident way still
computes every window of every read (no early exit), the host loop drops a read once it has hit.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from deepbinner_amd import dtw_semi_global as dtw      # noqa: E402
from deepbinner_amd import prep_signal                 # noqa: E402
from deepbinner_amd.trim_signal import normalise       # noqa: E402


def squiggle(rng, n_samples):
    levels = rng.normal(0.0, 1.0, size=n_samples // 5 + 2)
    return np.repeat(levels, rng.integers(5, 12, size=len(levels)))[:n_samples]


def make_reads(n_reads, n_samples, n_query, seed=1):
    rng = np.random.default_rng(seed)
    adapter = squiggle(rng, n_query)
    reads = []
    for r in range(n_reads):
        signal = squiggle(rng, n_samples)
        kind = r % 10
        if kind < 8:
            at = int(rng.integers(50, 1000))                   # window 0
        elif kind == 8:
            at = int(rng.integers(1600, 14000))                # a later window
        else:
            at = None                                          # nowhere
        if at is not None:
            signal[at:at + n_query] = adapter + rng.normal(0, 0.1, n_query)
        raw = np.round(signal * 80.0 + 500.0).astype(np.int16)
        reads.append(np.concatenate([np.full(60, 520, dtype=np.int16), raw]))
    return reads, 1.1 * adapter + 0.2


def host_loop(reads, adapter, side):
    """The adapter scan as it could be written before dtw_locate_batch."""
    signals = []
    for read in reads:
        trimmed = prep_signal.trim_signal(read, out=None)
        signals.append(None if trimmed is None else normalise(trimmed))
    positions = [(None, None)] * len(reads)
    open_reads = [r for r, s in enumerate(signals) if s is not None]
    windows = {r: prep_signal.adapter_windows(len(signals[r]), side) for r in open_reads}
    for index in range(30):
        todo = [r for r in open_reads
                if index < len(windows[r]) and windows[r][index][1] > windows[r][index][0]]
        if not todo:
            continue
        results = dtw.semi_global_dtw_with_rescaling_batch(
            [signals[r][windows[r][index][0]:windows[r][index][1]] for r in todo],
            [adapter] * len(todo))
        for r, (distance, start, end, _) in zip(todo, results):
            if distance <= prep_signal.THRESHOLD:
                at = windows[r][index][0]
                positions[r] = (int(start) + at, int(end) + at)
                open_reads.remove(r)
    return positions


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reads', type=int, default=2000)
    parser.add_argument('--samples', type=int, default=20000)
    parser.add_argument('--query', type=int, default=400)
    parser.add_argument('--side', default='start')
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--out')
    args = parser.parse_args()
    reads, adapter = make_reads(args.reads, args.samples, args.query)
    # warm-up of both ways at the sizes that are timed: code load, buffers
    prep_signal.locate_adapters(reads[:200], adapter, args.side)
    host_loop(reads[:200], adapter, args.side)
    seconds = {'resident': [], 'host_loop': []}
    kernel_ms, cells, answers = [], 0, {}
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        answers['resident'] = prep_signal.locate_adapters(reads, adapter, args.side)
        seconds['resident'].append(time.perf_counter() - t0)
        ms, cells = dtw.last_kernel_time()
        kernel_ms.append(ms)
        t0 = time.perf_counter()
        answers['host_loop'] = host_loop(reads, adapter, args.side)
        seconds['host_loop'].append(time.perf_counter() - t0)
    # where the resident call's time goes, in one more run: the trimming, the library call
    # (argument checks, plan, upload, kernels, download), and the rest of the Python around it
    spent = {'trim': 0.0, 'library_call': 0.0}

    def timed(name, function):
        def wrapper(*a, **kw):
            t = time.perf_counter()
            try:
                return function(*a, **kw)
            finally:
                spent[name] += time.perf_counter() - t
        return wrapper

    prep_signal._trim_all = timed('trim', prep_signal._trim_all)
    dtw.locate_batch = timed('library_call', dtw.locate_batch)
    t0 = time.perf_counter()
    prep_signal.locate_adapters(reads, adapter, args.side)
    spent['other_python'] = time.perf_counter() - t0 - spent['trim'] - spent['library_call']
    found = sum(1 for p in answers['resident'] if p[0] is not None)
    agree = sum(1 for a, b in zip(answers['resident'], answers['host_loop']) if a == b)
    line = {'reads': args.reads, 'samples': args.samples, 'query': args.query, 'side': args.side,
            'repeats': args.repeats, 'adapters_found': found, 'same_positions_both_ways': agree,
            'resident_kernel_ms': [round(ms, 3) for ms in kernel_ms], 'resident_cells': cells,
            'resident_seconds_by_stage': {k: round(v, 4) for k, v in spent.items()}}
    for way, times in seconds.items():
        line[way] = {'seconds': [round(t, 4) for t in times],
                     'reads_per_second_median': round(args.reads / float(np.median(times)), 1),
                     'reads_per_second_min_max': [round(args.reads / max(times), 1),
                                                  round(args.reads / min(times), 1)]}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
