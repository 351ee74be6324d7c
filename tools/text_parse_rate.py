#!/usr/bin/env python3
"""Lines per second of hip_backend.read_training_data on both routes, parse='host' (the line-by-line
Python loop, the yardstick) and parse='gpu' (blocks parsed on the device), on
the same file in the same process: after a warm-up of each, the two alternate `--rounds` times.
For the GPU route also the time by stage.  Two seeded files: many lines of 1,024 values, and fewer
of 16,384.  Every file is measured by a child process under a time limit of its own.

    python tools/text_parse_rate.py [--lines 20000] [--long_lines 1500] [--rounds 5]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def write_file(path, n_lines, n_values, seed):
    """label 0..3, values as a sequencer's: three or four digits, now and then a sign or a zero"""
    import numpy as np
    rng = np.random.default_rng(seed)
    with open(path, 'wb') as out:
        for first in range(0, n_lines, 256):
            rows = rng.integers(350, 1200, size=(min(256, n_lines - first), n_values))
            rows[rng.random(rows.shape) < 0.01] *= -1
            for k, row in enumerate(rows):
                out.write(b'%d\t' % ((first + k) % 4) + ','.join(map(str, row.tolist())).encode() + b'\n')


def spread(rates):
    rates = sorted(rates)
    return {'median': rates[len(rates) // 2], 'min': rates[0], 'max': rates[-1]}


def worker(path, rounds):
    import numpy as np
    from deepbinner_amd import hip_backend as hb
    assert hb.device_count() >= 1, 'no HIP device visible'
    stages = []

    def staged(data, input_size):
        t0 = time.perf_counter()
        got = hb.parse_training_text(data, input_size)
        stages[-1]['parse_call'] += time.perf_counter() - t0
        for name, ms in zip(('upload', 'kernels', 'download'), hb.text_stage_ms()):
            stages[-1][name] += ms / 1e3
        return got

    def run(route):
        t0 = time.perf_counter()
        if route == 'gpu':
            stages.append(dict.fromkeys(('parse_call', 'upload', 'kernels', 'download'), 0.0))
            got = hb.read_training_data(path, parse='gpu', block_parser=staged)
            stages[-1]['total'] = time.perf_counter() - t0
        else:
            got = hb.read_training_data(path, parse='host')
        return got, time.perf_counter() - t0

    (host, _), (gpu, _) = run('host'), run('gpu')           # warm-up, and the same arrays
    assert np.array_equal(host[0], gpu[0]) and np.array_equal(host[1], gpu[1])
    assert host[0].dtype == gpu[0].dtype and host[1].dtype == gpu[1].dtype
    n = len(host[1])
    del stages[:]
    seconds = {'host': [], 'gpu': []}
    for _ in range(rounds):
        for route in ('host', 'gpu'):
            seconds[route].append(run(route)[1])
    # the stages in front of the parser, on their own: reading the file, cutting it into blocks
    t0 = time.perf_counter()
    with open(path, 'rb') as raw:
        while raw.read(hb.TEXT_BLOCK_BYTES):
            pass
    file_read = time.perf_counter() - t0
    t0 = time.perf_counter()
    n_blocks = sum(1 for _ in hb.training_text_blocks(path))
    cutting = time.perf_counter() - t0 - file_read
    t0 = time.perf_counter()
    with hb.Dataset(gpu[0], gpu[1], 4) as ds:
        assert len(ds) == n
    create = time.perf_counter() - t0
    median = {k: sorted(s[k] for s in stages)[len(stages) // 2] for k in stages[0]}
    print(json.dumps({
        'file_bytes': os.path.getsize(path), 'lines': n, 'values_per_line': int(host[0].shape[1]),
        'blocks': n_blocks, 'rounds': rounds, 'device': hb.device_name(0),
        'lines_per_s': {r: spread([n / s for s in seconds[r]]) for r in seconds},
        'gpu_over_host_median': spread([n / s for s in seconds['gpu']])['median']
        / spread([n / s for s in seconds['host']])['median'],
        'gpu_route_seconds_median': dict(median, file_read=file_read, cutting_blocks=max(cutting, 0.0),
                                         dbh_dataset_create=create)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--lines', type=int, default=20000)
    ap.add_argument('--long_lines', type=int, default=1500)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--limit', type=int, default=420, help='seconds a file\'s measurement may take')
    ap.add_argument('--worker', help=argparse.SUPPRESS)
    opts = ap.parse_args()
    if opts.worker:
        return worker(opts.worker, opts.rounds)
    with tempfile.TemporaryDirectory() as work:
        for name, n_lines, n_values in (('lines_1024', opts.lines, 1024),
                                        ('lines_16384', opts.long_lines, 16384)):
            path = os.path.join(work, name + '.txt')
            write_file(path, n_lines, n_values, seed=22)
            done = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', path,
                                   '--rounds', str(opts.rounds)], timeout=opts.limit)
            if done.returncode != 0:      # nothing more is started on the device after a failure
                sys.exit('the measurement of {} ended with status {}'.format(name, done.returncode))
            os.remove(path)


if __name__ == '__main__':
    main()
