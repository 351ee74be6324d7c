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

`--live` times instead what choosing `replay`'s --min_windows and --score_diff
costs: 10,000 reads of 6,000 to 20,000 samples - two in three with the start of a golden read in
front, so that barcodes lead - through the shipped start model at scan size 6144 (12 windows), in
chunks of 1,600 samples:

  sweep_live    what `sweep --live` does per batch: the reads clipped as its pack clips them,
                hip_backend.sweep_pair, then sweep_early_tally for min_windows 1 .. 12 and nine
                thresholds (108 settings); the two timed apart, and early_kernel's own time from an
                event pair around dbh_sweep_early_tally_dev on buffers already on the device
  sweep_tally   hip_backend.sweep_tally on the same tracks, for scale
  replay        the only route without it: the loop of `replay --stop_on_decision` (512 channels, one
                chunk per open read per round, a LiveSession) once per setting, for the SUBSET of
                settings in the output, at least twelve; `replay_108_scaled` is their median time
                per setting times 108 - scaled, not run

`--rounds` times over, alternating; medians and ranges.  A last pass with the forward kernel's
launch tally on counts the windows the sweep ran: one window pass per read is reads x 12.  For every
replayed setting the counts made from the session's records are compared with the tally's cell.
A record, not a bound.

    python tools/sweep_rate.py --live        (writes profiles/sweep/live_rate.json, or --out)
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


LIVE_SCAN_SIZE, LIVE_CHUNK, LIVE_CHANNELS = 6144, 1600, 512
# the replayed subset: the corners and the middle of the 12 x 9 grid
LIVE_SUBSET = [(1, 0.1), (1, 0.5), (1, 0.9), (2, 0.3), (2, 0.5), (3, 0.5), (4, 0.7), (6, 0.1), (6, 0.5),
               (6, 0.9), (9, 0.5), (12, 0.1), (12, 0.5), (12, 0.9)]


def live_reads(n, seed):
    golden = np.load(os.path.join(REPO, 'tests', 'golden', 'reads.npz'))
    real = [golden['samples'][golden['offsets'][i]:golden['offsets'][i + 1]] for i in range(7)]
    rng = np.random.default_rng(seed)
    lengths = rng.integers(6000, 20001, n)
    noise = squiggles(64, 20000, seed)
    reads = []
    for i, length in enumerate(lengths.tolist()):
        read = noise[i % 64, :length].copy()
        if i % 3:
            front = min(length, len(real[i % 7]), 8000)
            read[:front] = real[i % 7][:front]
        reads.append(read)
    return reads


def replay_once(hb, model, reads, m, t):
    """The loop of the replay command under --stop_on_decision -> the reads' last records."""
    last = [None] * len(reads)
    slots, nxt = [None] * LIVE_CHANNELS, 0
    with hb.LiveSession(model, LIVE_CHANNELS, scan_size=LIVE_SCAN_SIZE, score_diff=t, min_windows=m,
                        stop_on_decision=True) as session:
        while True:
            for ch in range(LIVE_CHANNELS):
                if slots[ch] is None and nxt < len(reads):
                    slots[ch], nxt = [nxt, 0], nxt + 1
            active = [ch for ch in range(LIVE_CHANNELS) if slots[ch] is not None]
            if not active:
                return last
            chunks, begin, end = [], [], []
            for ch in active:
                i, at = slots[ch]
                chunks.append(reads[i][at:at + LIVE_CHUNK])
                begin.append(at == 0)
                end.append(at + LIVE_CHUNK >= len(reads[i]))
                slots[ch][1] = at + LIVE_CHUNK
            results = session.push(active, chunks, begin=begin, end=end)
            for ch, result, done in zip(active, results, end):
                if done:
                    last[slots[ch][0]] = result.copy()
                    slots[ch] = None


def live(opts):
    from deepbinner_amd import classify, sweep
    from deepbinner_amd import hip_backend as hb
    from deepbinner_amd.model_format import ModelWeights
    assert hb.device_count() >= 1, 'no HIP device visible'
    model = hb.HipModel(ModelWeights.load(os.path.join(
        REPO, 'deepbinner_amd', 'models', 'EXP-NBD103_read_starts.dbw'))[0], device=0)
    steps = LIVE_SCAN_SIZE // HALF
    reads = live_reads(opts.reads, 1)
    lengths = np.array([len(r) for r in reads], dtype=np.int64)
    keep = classify.scanned_end_samples(LIVE_SCAN_SIZE, 2 * HALF)

    def sweep_pass():
        t0 = time.perf_counter()
        samples, offsets = sweep.pack(reads, keep)
        t1 = time.perf_counter()
        start, _ = hb.sweep_pair(model, None, samples, offsets, LIVE_SCAN_SIZE)
        t2 = time.perf_counter()
        counts = hb.sweep_early_tally(start, None, THRESHOLDS, 13, None, lengths, 2 * HALF, LIVE_CHUNK)
        t3 = time.perf_counter()
        hb.sweep_tally(start, None, THRESHOLDS, 13)
        t4 = time.perf_counter()
        return start, counts, {'pack': t1 - t0, 'sweep_pair': t2 - t1, 'early_tally': t3 - t2,
                               'sweep_live': t3 - t0, 'sweep_tally': t4 - t3}

    def kernel_ms(start):
        """early_kernel alone: an event pair around the device entry, buffers resident."""
        lib = hb.load_library()
        pushes = hb.sweep_early_pushes(2 * HALF, LIVE_SCAN_SIZE, LIVE_CHUNK)
        fresh = hb.sweep_early_counts(steps, len(THRESHOLDS), False, 13, pushes)
        bufs = [hb.DeviceBuffer.from_array(a) for a in
                (start[0], start[1], lengths, np.array(THRESHOLDS)) + tuple(fresh)]
        first, second = hb.Event(), hb.Event()
        try:
            hb.synchronize()
            first.record()
            hb.check(lib.dbh_sweep_early_tally_dev(
                bufs[0].ptr, bufs[1].ptr, None, None, None, bufs[2].ptr, len(lengths), steps, 13,
                2 * HALF, LIVE_CHUNK, bufs[3].ptr, len(THRESHOLDS), *[b.ptr for b in bufs[4:]], None),
                'dbh_sweep_early_tally_dev')
            second.record()
            second.synchronize()
            return first.elapsed_ms(second)
        finally:
            for b in bufs:
                b.free()

    start, counts, _ = sweep_pass()                            # warm-up
    replay_once(hb, model, reads[:2 * LIVE_CHANNELS], 1, 0.5)
    parts = {name: [] for name in ('pack', 'sweep_pair', 'early_tally', 'sweep_live', 'sweep_tally')}
    kernel, replay_seconds = [], {setting: [] for setting in LIVE_SUBSET}
    for _ in range(opts.rounds):
        start, counts, seconds = sweep_pass()
        for name, value in seconds.items():
            parts[name].append(value)
        kernel.append(kernel_ms(start))
        for m, t in LIVE_SUBSET:
            t0 = time.perf_counter()
            last = replay_once(hb, model, reads, m, t)
            replay_seconds[m, t].append(time.perf_counter() - t0)
            decided = [r for r in last if int(r['decided_windows']) > 0]
            cell = counts[1][m - 1, THRESHOLDS.index(t)]
            assert [len(decided), sum(int(r['decided_windows']) for r in decided),
                    sum(int(r['decided_samples']) for r in decided)] == \
                [int(cell[0]), int(cell[5]), int(cell[6])], (m, t)
    model.timing_enable(1)                                     # the windows the sweep's pass runs
    model.timing_read()
    sweep_pass()
    _, launches, windows = model.timing_read()
    model.timing_enable(0)
    per_setting = [spread(s)['median'] for s in replay_seconds.values()]
    per_setting_median = sorted(per_setting)[len(per_setting) // 2]
    sweep_live = spread(parts['sweep_live'])
    out = {
        'device': hb.device_name(0), 'reads': len(reads), 'samples': int(lengths.sum()),
        'scan_size': LIVE_SCAN_SIZE, 'chunk_samples': LIVE_CHUNK, 'min_windows': steps,
        'thresholds': len(THRESHOLDS), 'settings': steps * len(THRESHOLDS), 'rounds': opts.rounds,
        'seconds': {name: spread(s) for name, s in parts.items()},
        'early_kernel_ms': spread(kernel),
        'forward_launches_of_one_pass': launches, 'windows_of_one_pass': windows,
        'one_window_pass_per_read': windows == len(reads) * steps,
        'replay_channels': LIVE_CHANNELS,
        'replay_seconds_per_setting': {'{},{}'.format(m, t): spread(s)
                                       for (m, t), s in replay_seconds.items()},
        'replay_settings_run': len(LIVE_SUBSET),
        'replay_subset_seconds': spread([sum(s[i] for s in replay_seconds.values())
                                         for i in range(opts.rounds)]),
        'replay_108_scaled': {'seconds': per_setting_median * steps * len(THRESHOLDS),
                              'how': 'median seconds per replayed setting x 108; scaled, not run'},
        'replay_108_scaled_over_sweep_live': per_setting_median * steps * len(THRESHOLDS) / sweep_live['median'],
        'early_tally_over_sweep_tally': spread(parts['early_tally'])['median'] / spread(parts['sweep_tally'])['median'],
        'decided_at_1_0.5': int(counts[1][0, THRESHOLDS.index(0.5), 0]),
        'same_counts_as_replay': True}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')
    model.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--reads', type=int, default=10000)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--live', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'sweep', 'live_rate.json'),
                    help='with --live: where the record is written')
    opts = ap.parse_args()
    if opts.live:
        return live(opts)
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
