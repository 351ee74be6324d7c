#!/usr/bin/env python3
"""What a live session's push costs, in one process on one GPU: the shipped
start model (persistent kind), `--channels` channels (512, then 3,000) each playing reads cut from
the seven golden reads plus noise, 1,600 samples (0.4 s at 4 kHz) per channel and round; a read of
6,000 to 20,000 samples ends with END and the channel begins the next one.

  push          LiveSession.push_packed: staging, append, window list, front, forward rounds, fold,
                results, one synchronise - the wall time of the call
  reclassify    the only alternative without a session: HipModel.classify_packed over every open
                channel's accumulated prefix, at the largest scan size (a multiple of half the input
                size, at most 6,144) not above the prefix; one call per scan size.  Channels whose
                prefix already covered scan size + half a window a round earlier are left out (their
                call cannot change any more), and the packing of the prefixes is not timed.

Both are timed in the same loop, alternating, on the same reads: `--pushes` (200) rounds after a
warm-up of `--warmup` (40) rounds, which is longer than the longest read and so covers every shape;
`--repeats` (3) times over.  Per repeat the median and the 99th percentile of a push's wall time,
the windows per push, the kernel launches per push as counted from the code (append, list and
results once; front, forward and fold per forward round; two copies beside them), and the same for
the alternative.  A record, not a bound.

    python tools/live_rate.py [--channels 512,3000] [--pushes 200] [--out profiles/live/rate.json]

`--pair` times instead, in the same loop on the same pushes, alternating:

  start_only    the start-only session's push, as above
  pair          a pair session's push (LiveSession with the shipped end model, push_pair_packed):
                the ring store in every push, and in a push that ends reads their end windows, the
                end model's forward rounds, the fold and combine_calls.  Reads end at their natural
                rate: every read of 6,000 to 20,000 samples once
  alternative   what there is without a pair session: the start-only push plus one classify_pair
                call (end model only) per push on the tails - the last scan size + half a window
                samples, kept by the caller - of the reads that ended in it; the keeping and packing
                of the tails is not timed

and, apart, pushes in which no read ends, for the cost of the ring store alone.  Median, 99th
percentile, launches per push; over `--repeats` the median and the range of the medians.

    python tools/live_rate.py --pair --out profiles/live/pair_rate.json

`--policy` times instead, in the same loop on identical chunks, alternating:

  start_only    the start-only session's push, as above
  policy        the push of a session with a yield policy (barcodes 1, 2, 3 and 12 balanced, the
                others kept; push_policy_packed): the two policy kernels behind the results kernel
                and the download of the action records

Median and 99th percentile per repeat, over `--repeats` the median and the range of the medians, the
kernel launches per push as counted from the code (the policy push: two more), the copies (one
more) and the synchronises (one each).  The start records of the two pushes are compared as bytes.

    python tools/live_rate.py --policy --out profiles/live/policy_rate.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CHUNK, SCAN, SIZE = 1600, 6144, 1024
CAP = SCAN + SIZE // 2


def percentiles(seconds):
    s = np.sort(np.asarray(seconds))
    return {'median_ms': 1e3 * float(s[len(s) // 2]),
            'p99_ms': 1e3 * float(s[min(len(s) - 1, int(np.ceil(0.99 * len(s))) - 1)]),
            'max_ms': 1e3 * float(s[-1])}


class Player:
    """The channels' reads: each one a golden read's start, carried on by its own samples again,
    plus a little noise; lengths 6,000 .. 20,000."""

    def __init__(self, golden, n_channels, seed, keep_whole=False):
        self.rng = np.random.default_rng(seed)
        self.bases = [np.resize(g, 20000 + CHUNK).astype(np.int16) for g in golden]
        self.noise = self.rng.integers(-3, 4, 1 << 22).astype(np.int16)
        self.n = n_channels
        self.base = np.zeros(n_channels, np.int64)
        self.length = np.zeros(n_channels, np.int64)
        self.at = np.zeros(n_channels, np.int64)
        for ch in range(n_channels):
            self.begin(ch)
            self.at[ch] = -int(self.rng.integers(0, 8)) * CHUNK      # the channels out of step
        self.prefix = np.zeros((n_channels, CAP), np.int16)
        # --pair: every read whole, for the alternative's tails
        self.whole = np.zeros((n_channels, 20000 + CHUNK), np.int16) if keep_whole else None

    def begin(self, ch):
        self.base[ch] = self.rng.integers(0, len(self.bases))
        self.length[ch] = self.rng.integers(6000, 20001)
        self.at[ch] = 0

    def round(self):
        """-> (channels, offsets, samples, flags) of the next push; keeps every prefix up to date"""
        channels, parts, flags = [], [], []
        for ch in range(self.n):
            at = int(self.at[ch])
            if at < 0:                                  # this channel has not begun yet
                self.at[ch] = at + CHUNK
                continue
            end = min(at + CHUNK, int(self.length[ch]))
            shift = int(self.rng.integers(0, len(self.noise) - CHUNK))
            part = self.bases[self.base[ch]][at:end] + self.noise[shift:shift + end - at]
            if at < CAP:
                self.prefix[ch, at:min(end, CAP)] = part[:max(0, min(end, CAP) - at)]
            if self.whole is not None:
                self.whole[ch, at:end] = part
            channels.append(ch)
            parts.append(part)
            flags.append((1 if at == 0 else 0) | (2 if end == self.length[ch] else 0))
            self.at[ch] = end
        offsets = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=offsets[1:])
        return (np.array(channels, np.int32), offsets, np.concatenate(parts),
                np.array(flags, np.uint32))

    def finish(self, channels, flags):
        for ch, f in zip(channels, flags):
            if f & 2:
                self.begin(int(ch))

    def tails(self, channels, flags):
        """(samples, offsets) of the last CAP samples of the reads that ended with this push"""
        parts = [self.whole[ch, max(0, int(self.at[ch]) - CAP):int(self.at[ch])]
                 for ch, f in zip(channels, flags) if f & 2]
        offsets = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=offsets[1:])
        return (np.concatenate(parts) if parts else np.zeros(0, np.int16)), offsets

    def prefixes(self, channels):
        """The alternative's work this round: {scan size: (samples, offsets)} over the channels
        whose prefix holds half a window at least and had not covered CAP a round earlier."""
        groups = {}
        for ch in channels:
            n = int(self.at[ch])
            if n < SIZE // 2 or n - CHUNK >= CAP:
                continue
            scan = min(SCAN, n // (SIZE // 2) * (SIZE // 2))
            groups.setdefault(scan, []).append(self.prefix[ch, :min(n, CAP)])
        packed = {}
        for scan, parts in groups.items():
            offsets = np.zeros(len(parts) + 1, np.int64)
            np.cumsum([len(p) for p in parts], out=offsets[1:])
            packed[scan] = (np.concatenate(parts), offsets)
        return packed


def measure(hb, model, golden, n_channels, opts, seed):
    player = Player(golden, n_channels, seed)
    push_s, alt_s, windows, rounds, alt_windows, alt_calls = [], [], [], [], [], []
    with hb.LiveSession(model, n_channels, scan_size=SCAN) as session:
        round_windows = min(n_channels * 12, (64 << 20) // (SIZE * 4))
        before = np.zeros(n_channels, np.int64)
        for r in range(opts.warmup + opts.pushes):
            channels, offsets, samples, flags = player.round()
            t0 = time.perf_counter()
            results = session.push_packed(channels, offsets, samples, flags)
            t1 = time.perf_counter()
            packed = player.prefixes(channels)
            t2 = time.perf_counter()
            for scan, (s, o) in packed.items():
                model.classify_packed(s, o, 'start', scan, 0.5)
            t3 = time.perf_counter()
            new = int((results['windows'] - np.where(flags & 1, 0, before[channels])).sum())
            before[channels] = results['windows']
            player.finish(channels, flags)
            if r >= opts.warmup:
                push_s.append(t1 - t0)
                alt_s.append(t3 - t2)
                windows.append(new)
                rounds.append(-(-new // round_windows))
                alt_windows.append(sum((len(o) - 1) * (scan // (SIZE // 2))
                                       for scan, (_, o) in packed.items()))
                alt_calls.append(len(packed))
    return {
        'pushes': len(push_s), 'push': percentiles(push_s), 'reclassify': percentiles(alt_s),
        'windows_per_push': {'mean': float(np.mean(windows)), 'max': int(np.max(windows))},
        'kernel_launches_per_push': {'mean': float(np.mean([3 + 3 * k for k in rounds])),
                                     'max': int(max(3 + 3 * k for k in rounds)), 'copies': 2},
        'reclassify_windows_per_round': {'mean': float(np.mean(alt_windows)),
                                         'max': int(np.max(alt_windows))},
        'reclassify_calls_per_round': float(np.mean(alt_calls)),
    }


def measure_pair(hb, model, end_model, golden, n_channels, opts, seed):
    player = Player(golden, n_channels, seed, keep_whole=True)
    start_s, pair_s, alt_s = [], [], []
    ended, launches_start, launches_pair = [], [], []
    round_windows = min(n_channels * 12, (64 << 20) // (SIZE * 4))
    with hb.LiveSession(model, n_channels, scan_size=SCAN) as alone, \
            hb.LiveSession(model, n_channels, scan_size=SCAN, end_model=end_model) as both:
        before = np.zeros(n_channels, np.int64)
        for r in range(opts.warmup + opts.pushes):
            channels, offsets, samples, flags = player.round()
            t0 = time.perf_counter()
            results = alone.push_packed(channels, offsets, samples, flags)
            t1 = time.perf_counter()
            got, ends = both.push_pair_packed(channels, offsets, samples, flags)
            t2 = time.perf_counter()
            tails, tail_offsets = player.tails(channels, flags)
            n_ended = len(tail_offsets) - 1
            t3 = time.perf_counter()
            if n_ended:
                end_calls = hb.classify_pair(None, end_model, tails, tail_offsets, SCAN, 0.5)
            t4 = time.perf_counter()
            assert got.tobytes() == results.tobytes()
            if n_ended:
                assert np.array_equal(ends['end_call'][(flags & 2) != 0], end_calls)
            new = int((results['windows'] - np.where(flags & 1, 0, before[channels])).sum())
            before[channels] = results['windows']
            player.finish(channels, flags)
            if r >= opts.warmup:
                start_s.append(t1 - t0)
                pair_s.append(t2 - t1)
                alt_s.append((t1 - t0) + (t4 - t3))
                ended.append(n_ended)
                k = -(-new // round_windows)
                launches_start.append(3 + 3 * k)
                launches_pair.append(3 + 3 * k + 3 * -(-(n_ended * 12) // round_windows))
        # pushes in which no read ends: every channel begins a 20,000-sample read at once, twelve
        # chunks of it, three times over (BEGIN inside a read starts anew).  The first five chunks
        # of a read complete start windows; behind cap the start side stores nothing, and a pair
        # push is the ring store alone
        channels = np.arange(n_channels, dtype=np.int32)
        offsets = np.arange(n_channels + 1, dtype=np.int64) * CHUNK
        early_start, early_pair, late_start, late_pair = [], [], [], []
        for r in range(36):
            samples = np.concatenate([player.bases[(ch + r) % len(player.bases)][
                (r % 12) * CHUNK:(r % 12 + 1) * CHUNK] for ch in range(n_channels)])
            flags = np.full(n_channels, 1 if r % 12 == 0 else 0, np.uint32)
            t0 = time.perf_counter()
            results = alone.push_packed(channels, offsets, samples, flags)
            t1 = time.perf_counter()
            got, _ = both.push_pair_packed(channels, offsets, samples, flags)
            t2 = time.perf_counter()
            assert got.tobytes() == results.tobytes()
            if r >= 12:                                 # (the first read: warm-up of these shapes)
                (early_start if r % 12 < 5 else late_start).append(t1 - t0)
                (early_pair if r % 12 < 5 else late_pair).append(t2 - t1)
    quiet = {'start_only_with_windows': percentiles(early_start),
             'pair_with_windows': percentiles(early_pair),
             'start_only_behind_cap': percentiles(late_start),
             'pair_behind_cap': percentiles(late_pair), 'kernel_launches_per_push': 'the same: '
             '6 with new windows, 3 behind cap', 'pushes': len(early_start) + len(late_start)}
    out = {
        'pushes': len(start_s), 'start_only': percentiles(start_s), 'pair': percentiles(pair_s),
        'no_read_ends': quiet,
        'alternative': percentiles(alt_s),
        'reads_ended_per_push': {'mean': float(np.mean(ended)), 'max': int(np.max(ended))},
        'kernel_launches_per_push': {
            'start_only': {'mean': float(np.mean(launches_start)), 'max': int(max(launches_start)),
                           'copies': 2},
            'pair': {'mean': float(np.mean(launches_pair)), 'max': int(max(launches_pair)),
                     'copies': 3}},
    }
    return out


def measure_policy(hb, model, golden, n_channels, opts, seed):
    player = Player(golden, n_channels, seed)
    weights = np.full(13, -1, np.int32)
    weights[[1, 2, 3, 12]] = 1
    start_s, policy_s, launches, ejected, decided = [], [], [], 0, 0
    round_windows = min(n_channels * 12, (64 << 20) // (SIZE * 4))
    with hb.LiveSession(model, n_channels, scan_size=SCAN) as alone, \
            hb.LiveSession(model, n_channels, scan_size=SCAN, policy=dict(weights=weights)) as ruled:
        before = np.zeros(n_channels, np.int64)
        for r in range(opts.warmup + opts.pushes):
            channels, offsets, samples, flags = player.round()
            order = (alone, ruled) if r % 2 == 0 else (ruled, alone)       # who goes first alternates
            taken = {}
            for session in order:
                t0 = time.perf_counter()
                if session is alone:
                    results = session.push_packed(channels, offsets, samples, flags)
                else:
                    got, _, actions = session.push_policy_packed(channels, offsets, samples, flags)
                taken[session is alone] = time.perf_counter() - t0
            assert got.tobytes() == results.tobytes()
            new = int((results['windows'] - np.where(flags & 1, 0, before[channels])).sum())
            before[channels] = results['windows']
            player.finish(channels, flags)
            if r >= opts.warmup:
                start_s.append(taken[True])
                policy_s.append(taken[False])
                launches.append(3 + 3 * -(-new // round_windows))
                took = actions[actions['reason'] != 0]
                decided += len(took)
                ejected += int((took['action'] == hb.LIVE_EJECT).sum())
        yield_samples, yield_reads = ruled.yields()
    return {
        'pushes': len(start_s), 'start_only': percentiles(start_s), 'policy': percentiles(policy_s),
        'kernel_launches_per_push': {
            'start_only': {'mean': float(np.mean(launches)), 'max': int(max(launches)), 'copies': 2,
                           'synchronises': 1},
            'policy': {'mean': float(np.mean(launches)) + 2, 'max': int(max(launches)) + 2,
                       'copies': 3, 'synchronises': 1}},
        'actions_taken': decided, 'of_them_eject': ejected,
        'yield_reads': int(yield_reads.sum()), 'yield_samples': int(yield_samples.sum()),
    }


def main_policy(hb, model, golden, opts, record):
    record['policy'] = 'barcodes 1, 2, 3, 12 balanced with share 1, slack 0, the others kept'
    for n_channels in [int(v) for v in opts.channels.split(',')]:
        repeats = [measure_policy(hb, model, golden, n_channels, opts, seed=100 * n_channels + k)
                   for k in range(opts.repeats)]
        entry = {'repeats': repeats}
        for key in ('start_only', 'policy'):
            entry[key + '_median_ms'] = spread([rep[key]['median_ms'] for rep in repeats])
            entry[key + '_p99_ms'] = spread([rep[key]['p99_ms'] for rep in repeats])
        entry['policy_minus_start_only_median_ms'] = spread(
            [rep['policy']['median_ms'] - rep['start_only']['median_ms'] for rep in repeats])
        entry['policy_share_of_chunk_period'] = entry['policy_median_ms']['median'] / 400.0
        record['channels'][str(n_channels)] = entry


def spread(values):
    values = sorted(values)
    return {'median': values[len(values) // 2], 'min': values[0], 'max': values[-1]}


def main_pair(hb, model, golden, opts, record):
    from deepbinner_amd.model_format import ModelWeights
    end_model = hb.HipModel(ModelWeights.load(os.path.join(
        REPO, 'deepbinner_amd', 'models', 'EXP-NBD103_read_ends.dbw'))[0], device=0)
    record['end_model'] = 'EXP-NBD103_read_ends, persistent kind'
    for n_channels in [int(v) for v in opts.channels.split(',')]:
        repeats = [measure_pair(hb, model, end_model, golden, n_channels, opts,
                                seed=100 * n_channels + k) for k in range(opts.repeats)]
        entry = {'repeats': repeats}
        for key in ('start_only', 'pair', 'alternative'):
            entry[key + '_median_ms'] = spread([rep[key]['median_ms'] for rep in repeats])
            entry[key + '_p99_ms'] = spread([rep[key]['p99_ms'] for rep in repeats])
        for key in ('start_only_with_windows', 'pair_with_windows', 'start_only_behind_cap',
                    'pair_behind_cap'):
            entry['no_read_ends_' + key + '_median_ms'] = spread(
                [rep['no_read_ends'][key]['median_ms'] for rep in repeats])
        entry['pair_share_of_chunk_period'] = entry['pair_median_ms']['median'] / 400.0
        record['channels'][str(n_channels)] = entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--channels', type=str, default='512,3000')
    ap.add_argument('--pushes', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--pair', action='store_true',
                    help='time a pair session beside the start-only one and the alternative')
    ap.add_argument('--policy', action='store_true',
                    help='time the push of a session with a yield policy beside the start-only one')
    opts = ap.parse_args()
    from deepbinner_amd import hip_backend as hb
    from deepbinner_amd.model_format import ModelWeights
    assert hb.device_count() >= 1, 'no HIP device visible'
    weights = ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models',
                                             'EXP-NBD103_read_starts.dbw'))[0]
    model = hb.HipModel(weights, device=0)
    reads = np.load(os.path.join(REPO, 'tests', 'golden', 'reads.npz'))
    golden = [reads['samples'][reads['offsets'][i]:reads['offsets'][i + 1]] for i in range(7)]
    record = {'device': hb.device_name(0), 'model': 'EXP-NBD103_read_starts, persistent kind',
              'chunk_samples': CHUNK, 'chunk_period_ms': 400.0, 'scan_size': SCAN,
              'warmup_pushes': opts.warmup, 'channels': {}}
    if opts.pair:
        main_pair(hb, model, golden, opts, record)
    if opts.policy:
        main_policy(hb, model, golden, opts, record)
    for n_channels in [] if opts.pair or opts.policy else [int(v) for v in opts.channels.split(',')]:
        repeats = [measure(hb, model, golden, n_channels, opts, seed=100 * n_channels + k)
                   for k in range(opts.repeats)]
        medians = sorted(rep['push']['median_ms'] for rep in repeats)
        alt = sorted(rep['reclassify']['median_ms'] for rep in repeats)
        record['channels'][str(n_channels)] = {
            'repeats': repeats,
            'push_median_ms': {'median': medians[len(medians) // 2], 'min': medians[0],
                               'max': medians[-1]},
            'reclassify_median_ms': {'median': alt[len(alt) // 2], 'min': alt[0], 'max': alt[-1]},
            'reclassify_over_push': alt[len(alt) // 2] / medians[len(medians) // 2],
            'push_share_of_chunk_period': medians[len(medians) // 2] / 400.0,
        }
    text = json.dumps(record, indent=1)
    print(text, flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
