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

`--occlude` times, instead of classify against locate, locate against

  occluded   HipModel.locate_occluded_signals: locate, then every read called again with the located
             span blanked, with all but the span blanked and with a control stretch blanked - four
             passes of windows through the layer chain

in the same alternating rounds, and counts what the three variants did to the calls.  `--golden
PATH` also writes the table of the seven golden reads through the two shipped models at scan size
6144.

    python tools/locate_rate.py [--reads 10000] [--rounds 5] [--out profiles/locate/rate.json]
    python tools/locate_rate.py --occlude [--out profiles/locate/occlude_rate.json]
                                [--golden profiles/locate/occlude_golden.json]
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
    ap.add_argument('--occlude', action='store_true')
    ap.add_argument('--golden', type=str, default=None)
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

    if opts.occlude:
        return occlude_leg(opts, hb, model, signals, walled, locate)
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
    write(record, opts.out)


def write(record, path):
    text = json.dumps(record, indent=1)
    print(text, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write(text + '\n')


def tally(occlusions):
    """Among the located reads with a result: calls lost under out, kept under only and ctrl."""
    out = {}
    for v in ('out', 'only', 'ctrl'):
        has = (occlusions['cls'] != 0) & (occlusions[v + '_call'] >= 0)
        same = occlusions[v + '_call'][has] == occlusions['cls'][has]
        out[v] = {'results': int(has.sum()),
                  'lost' if v == 'out' else 'kept': int((~same).sum() if v == 'out' else same.sum()),
                  'median_p': float(np.median(occlusions[v + '_p'][has])) if has.any() else None}
    return out


def occlude_leg(opts, hb, model, signals, walled, locate):
    n = len(signals)

    def occluded():
        return model.locate_occluded_signals(signals, 'start', 6144, 0.5)

    (_, (probs, calls, locations)), (_, (o_probs, o_calls, o_locations, occlusions)) = \
        walled(locate), walled(occluded)
    assert np.array_equal(o_probs, probs) and np.array_equal(o_calls, calls)
    assert o_locations.tobytes() == locations.tobytes()
    seconds = {'locate': [], 'occluded': []}
    for _ in range(opts.rounds):
        seconds['locate'].append(walled(locate)[0])
        seconds['occluded'].append(walled(occluded)[0])
    medians = {name: spread(s)['median'] for name, s in seconds.items()}
    write({
        'device': hb.device_name(0), 'reads': n, 'samples_per_read': opts.length, 'scan_size': 6144,
        'windows': 12 * n, 'rounds': opts.rounds, 'model': 'EXP-NBD103_read_starts, general-kind',
        'located': int((locations['cls'] != 0).sum()), 'variants': tally(occlusions),
        'workspace_bytes_per_group': {'locate': hb.locate_workspace_bytes(model, n, 6144),
                                      'occluded': hb.locate_occluded_workspace_bytes(model, n, 6144)},
        'seconds': {name: spread(s) for name, s in seconds.items()},
        'locate_reads_per_s': n / medians['locate'],
        'occluded_reads_per_s': n / medians['occluded'],
        'occluded_over_locate': medians['occluded'] / medians['locate'],
    }, opts.out)
    if opts.golden:
        golden_table(hb, opts.golden)


def golden_table(hb, path):
    """The seven golden reads through the two shipped models at scan size 6144."""
    from deepbinner_amd.model_format import ModelWeights
    reads = np.load(os.path.join(REPO, 'tests', 'golden', 'reads.npz'))
    offsets = reads['offsets'].astype(np.int64)
    rows, totals = [], {}
    for side, name in (('start', 'EXP-NBD103_read_starts'), ('end', 'EXP-NBD103_read_ends')):
        weights = ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models', name + '.dbw'))[0]
        model = hb.HipModel(weights, device=0, general=True)
        _, _, locations, occlusions = model.locate_occluded_packed(reads['samples'], offsets, side,
                                                                   6144, 0.5)
        model.close()
        totals[side] = tally(occlusions)
        for r in range(len(offsets) - 1):
            loc, occ = locations[r], occlusions[r]
            row = {'side': side, 'read': r, 'samples': int(offsets[r + 1] - offsets[r]),
                   'cls': int(occ['cls'])}
            if occ['cls'] != 0:
                row.update(p=float(occ['p']), first=int(loc['first_sample']),
                           end=int(loc['end_sample']), share=float(loc['share']),
                           ctrl_first=int(occ['ctrl_first']), ctrl_end=int(occ['ctrl_end']))
                for v in ('out', 'only', 'ctrl'):
                    if occ[v + '_call'] >= 0:
                        row[v] = {'call': int(occ[v + '_call']), 'p': float(occ[v + '_p'])}
                    else:
                        row[v] = 'no samples in the span' if loc['end_sample'] == loc['first_sample'] \
                            else 'the control would overlap the span'
            rows.append(row)
    write({'device': hb.device_name(0), 'scan_size': 6144, 'score_diff': 0.5, 'totals': totals,
           'rows': rows}, path)


if __name__ == '__main__':
    main()
