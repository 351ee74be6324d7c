"""``prep_signal.trim_positions`` beside the loop of ``np.std`` it stands in for, on section 20's
workload (synthetic raw reads of 20,000 samples, host only):

  python tools/samples_rate.py [--reads 2000] [--samples 20000] [--repeats 5] [--out FILE]

Prints one JSON line (and writes it to --out): the seconds of each way, alternating, and on how
many reads they agree.  A record, not a bound.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from deepbinner_amd import prep_signal                  # noqa: E402
from prep_signal_rate import make_reads                 # noqa: E402


def std_loop(reads):
    return [prep_signal.trim_signal(read, out=None) for read in reads]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reads', type=int, default=2000)
    parser.add_argument('--samples', type=int, default=20000)
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--out')
    options = parser.parse_args()
    raws, _ = make_reads(options.reads, options.samples, 400)
    seconds = {'trim_positions': [], 'np_std_loop': []}
    for _ in range(options.repeats):
        t0 = time.perf_counter()
        positions = prep_signal.trim_positions(raws)
        seconds['trim_positions'].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        trimmed = std_loop(raws)
        seconds['np_std_loop'].append(time.perf_counter() - t0)
    same = sum(1 for raw, p, t in zip(raws, positions, trimmed)
               if (p < 0 and t is None) or (t is not None and len(raw) - len(t) == p))
    line = {'reads': options.reads, 'samples': options.samples, 'repeats': options.repeats,
            'same_positions': same}
    for way, times in seconds.items():
        line[way] = {'seconds': [round(t, 4) for t in times],
                     'median_ms': round(1000 * float(np.median(times)), 2)}
    text = json.dumps(line)
    print(text)
    if options.out:
        with open(options.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
