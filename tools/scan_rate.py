#!/usr/bin/env python3
"""What a scan costs, in one process on one GPU: `--reads` reads (2,000) of
20,000 and of 100,000 samples - seeded squiggle-like int16 signals, tools/sweep_rate.py's law -
through the two --native models:

  scan            HipModel.scan_packed of the start and of the end model: every window of every
                  read cut, through the network, folded, turned into events (threshold 0.5)
  front           dbh_scan_windows_dev alone over the same windows, 32,768 at a time, between events
  predict         dbh_predict_dev alone on as many windows (those of the last front chunk, again
                  and again): what the network itself takes on this window count
  events          dbh_scan_events_dev alone on the start model's track (it allocates its counts
                  and synchronises: wall time)
  classify_pair   hip_backend.classify_pair at scan size 6144 on the same reads, for scale: 12
                  windows per read end however long the read (this entry is the parent commit's)

After a warm-up of each, `--rounds` rounds; medians and spreads.  A record, not a bound.

    python tools/scan_rate.py [--reads 2000] [--rounds 3]
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
CHUNK = 32768


def spread(values):
    values = sorted(values)
    return {'median': values[len(values) // 2], 'min': values[0], 'max': values[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--reads', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--lengths', type=str, default='20000,100000')
    opts = ap.parse_args()
    from sweep_rate import squiggles
    from deepbinner_amd import hip_backend as hb
    from deepbinner_amd.model_format import ModelWeights
    assert hb.device_count() >= 1, 'no HIP device visible'
    lib = hb.load_library()
    models = [hb.HipModel(ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models', name + '.dbw'))[0],
                          device=0) for name in ('EXP-NBD103_read_starts', 'EXP-NBD103_read_ends')]
    record = {'device': hb.device_name(0), 'reads': opts.reads, 'rounds': opts.rounds, 'lengths': {}}
    for length in [int(v) for v in opts.lengths.split(',')]:
        n = opts.reads
        samples = np.concatenate([squiggles(min(100, n - first), length, 1 + first).reshape(-1)
                                  for first in range(0, n, 100)])
        offsets = np.arange(n + 1, dtype=np.int64) * length
        per_read = int(hb.scan_window_count(1024, length))
        windows = n * per_read

        def scan():
            return [m.scan_packed(samples, offsets, side, 0.5, 1, 12, track=(side == 'start'))
                    for m, side in zip(models, ('start', 'end'))]

        def classify_pair():
            return hb.classify_pair(models[0], models[1], samples, offsets, 6144, 0.5)

        (events, best, margin, window_offsets), end_events = scan()
        classify_pair()
        held = [hb.DeviceBuffer.from_array(samples), hb.DeviceBuffer.from_array(offsets),
                hb.DeviceBuffer(8 * (n + 1)), hb.DeviceBuffer(CHUNK * 1024 * 4),
                hb.DeviceBuffer(CHUNK * 13 * 4)]
        hb.check(lib.dbh_scan_window_offsets_dev(held[1].ptr, n, 1024, held[2].ptr, None))
        marks = [hb.Event() for _ in range(2)]

        def front():
            marks[0].record()
            for w0 in range(0, windows, CHUNK):
                hb.check(lib.dbh_scan_windows_dev(held[0].ptr, held[1].ptr, held[2].ptr, n, 1024, 0,
                                                  w0, min(CHUNK, windows - w0), held[3].ptr, None))
            marks[1].record()
            marks[1].synchronize()
            return marks[0].elapsed_ms(marks[1]) / 1e3

        def predict():
            marks[0].record()
            for w0 in range(0, windows, CHUNK):
                models[0].predict_dev(held[3].ptr, min(CHUNK, windows - w0), held[4].ptr)
            marks[1].record()
            marks[1].synchronize()
            return marks[0].elapsed_ms(marks[1]) / 1e3

        def event_pass():
            t0 = time.perf_counter()
            hb.scan_events(best, margin, window_offsets, 0.5, 1, 12)
            return time.perf_counter() - t0

        def walled(run):
            t0 = time.perf_counter()
            run()
            return time.perf_counter() - t0

        front(), predict(), event_pass()
        seconds = {name: [] for name in ('scan', 'front', 'predict', 'events', 'classify_pair')}
        for _ in range(opts.rounds):
            seconds['scan'].append(walled(scan))
            seconds['front'].append(front())
            seconds['predict'].append(predict())
            seconds['events'].append(event_pass())
            seconds['classify_pair'].append(walled(classify_pair))
        for buf in held:
            buf.free()
        medians = {name: spread(s)['median'] for name, s in seconds.items()}
        record['lengths'][str(length)] = {
            'windows_per_read_and_side': per_read, 'windows_per_side': windows,
            'events_start': len(events), 'events_end': len(end_events),
            'seconds': {name: spread(s) for name, s in seconds.items()},
            # both sides: 2 x windows through the network in `scan`
            'scan_windows_per_s': 2 * windows / medians['scan'],
            'front_windows_per_s': windows / medians['front'],
            'predict_dev_windows_per_s': windows / medians['predict'],
            'events_windows_per_s_host_copies_included': windows / medians['events'],
            'classify_pair_reads_per_s': n / medians['classify_pair'],
        }
    print(json.dumps(record, indent=1), flush=True)


if __name__ == '__main__':
    main()
