"""A helper, not a test: the early tally's rule (include/deepbinner_hip.h, "early tally") restated in
plain Python integers, per read - what a live session with ``min_windows`` = m and ``score_diff`` = t
decides on a read whose start track is (best[k], margin[k]) and which a replay delivers in chunks of
``chunk`` samples - and the four arrays counted from it.  Nothing here is shared with
csrc/dbh_early_core.h; tests/test_sweep_live.py holds it to tests/live_reference.py's ``plan``, the
live contract itself.  Also the host stand-in for ``sweep --live``'s backend."""
import numpy as np

import sweep_reference

DECIDED, AGREE, CHANGED, LOST, LATE, WINDOWS, SAMPLES, LENGTH = range(8)
MAX_PUSHES = 4096


def ceil_div(a, b):
    return -(-a // b)


def leads(best, margin, t):
    return int(best) != 0 and float(margin) >= t          # (NaN >= t is False)


def pushes_bound(input_size, scan_size, chunk):
    return ceil_div(scan_size + input_size // 2, chunk)


def crossings(best, margin, t):
    """first[k]: the smallest k' >= k whose window leads at t, None if there is none - one walk from
    the last window down."""
    first, nxt = [None] * len(best), None
    for k in range(len(best) - 1, -1, -1):
        if leads(best[k], margin[k], t):
            nxt = k
        first[k] = nxt
    return first


def decision(best, margin, d, t, length, input_size, chunk):
    """The record of a read decided at window d (None: never)."""
    steps, h = len(best), input_size // 2
    final = int(best[steps - 1]) if leads(best[steps - 1], margin[steps - 1], t) else 0
    if d is None:
        return dict(call=0, decided_windows=0, decided_samples=0, push=0, final_call=final)
    out = dict(call=int(best[d]), decided_windows=d + 1, final_call=final, push=0, decided_samples=0)
    if length is not None:
        length, chunk = int(length), int(chunk)
        last = max(1, ceil_div(length, chunk))           # the push that carries END
        out['push'] = min(ceil_div(d * h + input_size, chunk), last)
        out['decided_samples'] = min(out['push'] * chunk, length)
    return out


def outcome(best, margin, m, t, length, input_size, chunk):
    """One read, one setting: call, decided_windows, decided_samples, push (from 1) and final_call."""
    d = next((k for k in range(m - 1, len(best)) if leads(best[k], margin[k], t)), None)
    return decision(best, margin, d, t, length, input_size, chunk)


def combine(s, e, mode):
    """classify.py:298-322 on call numbers; mode 0 either, 1 start, 2 both."""
    if s == e:
        return s
    if mode == 2:
        return 0
    if e == 0:
        return s
    if mode == 1:
        return 0
    return e if s == 0 else 0


def tally(start, end, thresholds, n_classes, labels=None, lengths=None, input_size=1024,
          chunk=1600):
    """-> (calls [K, T, modes, C + 3], early [K, T, 8], windows [K, T, K], pushes [K, T, P] or None),
    all int64 (object sums first: a sum of lengths may pass 2^63 nowhere a test goes, but it is
    Python's integers that add)."""
    best, margin = np.asarray(start[0]), np.asarray(start[1])
    n, steps = best.shape
    both = end is not None and end[0] is not None
    modes, T, C = (3 if both else 1), len(thresholds), n_classes
    P = None if lengths is None else pushes_bound(input_size, steps * (input_size // 2), chunk)
    calls = np.zeros((steps, T, modes, C + 3), dtype=object)
    early = np.zeros((steps, T, 8), dtype=object)
    windows = np.zeros((steps, T, steps), dtype=object)
    pushes = None if P is None else np.zeros((steps, T, P), dtype=object)
    for i in range(n):
        b, g = best[i].tolist(), margin[i].tolist()
        label = -1 if labels is None else int(labels[i])
        length = None if lengths is None else int(lengths[i])
        for t, threshold in enumerate(thresholds):
            end_call = 0
            if both and leads(end[0][i][steps - 1], end[1][i][steps - 1], threshold):
                end_call = int(end[0][i][steps - 1])
            first = crossings(b, g, threshold)
            known = {}
            for m in range(1, steps + 1):
                d = first[m - 1]
                if d not in known:
                    known[d] = decision(b, g, d, threshold, length, input_size, chunk)
                o = known[d]
                for mode in range(modes):
                    call = combine(o['call'], end_call, mode) if both else o['call']
                    if 0 <= call < C:
                        calls[m - 1, t, mode, call] += 1
                    if label >= 0:
                        calls[m - 1, t, mode,
                              C if call == label else (C + 1 if call != 0 else C + 2)] += 1
                if d is None:
                    continue
                row = early[m - 1, t]
                row[DECIDED] += 1
                row[AGREE] += o['call'] == o['final_call']
                row[CHANGED] += o['final_call'] not in (0, o['call'])
                row[LOST] += o['final_call'] == 0
                row[LATE] += o['decided_windows'] > m
                row[WINDOWS] += o['decided_windows']
                windows[m - 1, t, d] += 1
                if length is not None:
                    row[SAMPLES] += o['decided_samples']
                    row[LENGTH] += length
                    pushes[m - 1, t, o['push'] - 1] += 1
    as_int = lambda a: None if a is None else a.astype(np.int64)          # noqa: E731
    return as_int(calls), as_int(early), as_int(windows), as_int(pushes)


class HostBackend(sweep_reference.HostBackend):
    """What ``sweep.sweep`` with ``--live`` asks of ``hip_backend`` beyond the sweep's own entries,
    on the host and by this file's rule."""

    @staticmethod
    def sweep_early_pushes(input_size, scan_size, chunk_samples):
        pushes = pushes_bound(input_size, scan_size, chunk_samples)
        assert pushes <= MAX_PUSHES
        return pushes

    @staticmethod
    def sweep_early_counts(steps, n_thresholds, both, n_classes, pushes=None):
        zeros = lambda *shape: np.zeros(shape, dtype=np.int64)            # noqa: E731
        return (zeros(steps, n_thresholds, 3 if both else 1, n_classes + 3),
                zeros(steps, n_thresholds, 8), zeros(steps, n_thresholds, steps),
                None if pushes is None else zeros(steps, n_thresholds, pushes))

    def sweep_early_tally(self, start, end, thresholds, n_classes, labels=None, lengths=None,
                          input_size=1024, chunk_samples=1600, counts=None):
        got = tally(start, end, list(thresholds), n_classes, labels, lengths, input_size,
                    chunk_samples)
        if counts is None:
            return got
        for mine, more in zip(counts, got):
            if mine is not None:
                mine += more
        return counts
