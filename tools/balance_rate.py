#!/usr/bin/env python3
"""Signals per second of the random half of `balance` on three routes, in
one process, at section 22's two sizes - 10,000 signals of 1,024 values and 1,500 of 16,384:

  device   hip_backend.ResidentText, as balance runs it, in balance's chunks: generator and
           formatter on one stream, one synchronisation, only text downloaded
  host     the same two calls on the CPU models (host=True)
  python   a loop that restates the reference's per-value law (balance.py:164-193): one
           random.gauss and one str() per value; a sine stands in for noise.pnoise1, which is a C
           extension in the reference.  Minutes at full size, so it runs on `--python_share` of
           the signals and is reported per signal like the others.

After a warm-up of each the routes alternate `--rounds` times; medians and spreads are printed,
and for the device route the share of its chunks' time that the kernels take, by the route's own
device events.
Each size is measured by a child process under a time limit of its own.

    python tools/balance_rate.py [--rounds 5] [--python_share 0.02]
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SIZES = ((10000, 1024), (1500, 16384))


def python_signal(rng, size):
    import math
    kind = rng.choice(['flat', 'gaussian', 'multi_gaussian', 'perlin'])
    values = []
    if kind == 'flat':
        values = [rng.randint(0, 1000)] * size
    elif kind == 'gaussian':
        mean, stdev = rng.uniform(300, 600), rng.uniform(10, 500)
        values = [int(rng.gauss(mean, stdev)) for _ in range(size)]
    elif kind == 'multi_gaussian':
        while len(values) < size:
            length = rng.randint(100, 500)
            mean, stdev = rng.uniform(300, 600), rng.uniform(10, 500)
            values += [int(rng.gauss(mean, stdev)) for _ in range(length)]
    else:
        rng.randint(1, 4)
        step, start = rng.uniform(0.001, 0.04), rng.uniform(0.0, 1.0)
        factor, mean = rng.uniform(10, 300), rng.uniform(300, 600)
        values = [int(mean + factor * math.sin(start + i * step)) for i in range(size)]
    return '0\t' + ','.join(str(v) for v in values[:size]) + '\n'


def spread(values):
    values = sorted(values)
    return {'median': values[len(values) // 2], 'min': values[0], 'max': values[-1]}


def worker(n, size, rounds, python_share):
    import numpy as np
    from deepbinner_amd import balance, hip_backend as hb
    assert hb.device_count() >= 1, 'no HIP device visible'
    per_chunk = balance.chunk_signals(size)
    n_python = max(4, int(n * python_share))

    def chunks(count):
        return [(first, min(per_chunk, count - first)) for first in range(0, count, per_chunk)]

    resident = hb.ResidentText(min(per_chunk, n), size)       # as balance.add_random_signals keeps it
    chunk_ms = []

    def device():
        total = 0
        for first, count in chunks(n):
            t0 = time.perf_counter()
            signals = resident.random_signals(1, first, count)
            text = resident.format_training_text(np.zeros(count, dtype=np.int32), signals)
            total += len(text)
            del text
            chunk_ms.append((time.perf_counter() - t0) * 1e3)
            chunk_ms[-1] = (chunk_ms[-1],) + resident.last_ms
        return total

    def host():
        total = 0
        for first, count in chunks(n):
            signals = hb.random_signals(1, first, count, size, host=True)
            total += len(hb.format_training_text(np.zeros(count, dtype=np.int32), signals, host=True))
        return total

    def python():
        rng = random.Random(1)
        return sum(len(python_signal(rng, size)) for _ in range(n_python))

    # the two routes write the same bytes, at the size that is timed
    for first, count in chunks(n):
        labels = np.zeros(count, dtype=np.int32)
        text = resident.format_training_text(labels, resident.random_signals(1, first, count))
        assert text == hb.format_training_text(labels, hb.random_signals(1, first, count, size, host=True),
                                               host=True)
        del text

    routes = {'device': (device, n), 'host': (host, n), 'python': (python, n_python)}
    text_bytes = {name: run() for name, (run, _) in routes.items()}        # warm-up
    assert text_bytes['device'] == text_bytes['host']
    seconds = {name: [] for name in routes}
    for _ in range(rounds):
        for name, (run, _) in routes.items():
            t0 = time.perf_counter()
            run()
            seconds[name].append(time.perf_counter() - t0)
    rates = {name: spread([routes[name][1] / s for s in seconds[name]]) for name in routes}

    # the kernels' share of the device route, by the route's own events: the chunks of the timed runs
    timed = chunk_ms[-rounds * len(chunks(n)):]
    median = {name: sorted(c[k] for c in timed)[len(timed) // 2]
              for k, name in enumerate(('chunk_ms', 'generator_ms', 'formatter_ms'))}
    median['kernels_share_of_chunk'] = (median['generator_ms'] + median['formatter_ms']) / median['chunk_ms']
    resident.close()
    print(json.dumps({
        'signals': n, 'values_per_signal': size, 'text_bytes': text_bytes['device'],
        'chunks': len(chunks(n)), 'first_chunk_signals': chunks(n)[0][1], 'python_signals': n_python,
        'rounds': rounds, 'device': hb.device_name(0), 'signals_per_s': rates,
        'device_over_host_median': rates['device']['median'] / rates['host']['median'],
        'device_over_python_median': rates['device']['median'] / rates['python']['median'],
        'chunk_median': median}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--python_share', type=float, default=0.02)
    ap.add_argument('--scale', type=float, default=1.0, help='a share of the signals, for a rehearsal')
    ap.add_argument('--limit', type=int, default=240, help="seconds a size's measurement may take")
    ap.add_argument('--worker', nargs=2, type=int, help=argparse.SUPPRESS)
    opts = ap.parse_args()
    if opts.worker:
        return worker(opts.worker[0], opts.worker[1], opts.rounds, opts.python_share)
    for n, size in SIZES:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker',
                               str(max(4, int(n * opts.scale))), str(size), '--rounds', str(opts.rounds),
                               '--python_share', str(opts.python_share)], timeout=opts.limit)
        if done.returncode != 0:          # nothing more is started on the device after a failure
            sys.exit('the measurement of {} x {} ended with status {}'.format(n, size, done.returncode))


if __name__ == '__main__':
    main()
