"""A helper, not a test: the scan's contract (include/deepbinner_hip.h, "scan") restated in NumPy, as
simply as it can be said - how many windows a read has and which samples each one holds, the
normalising (tests/feed_reference.py's rule, over the samples present), the track (the sweep's fold
at one step: tests/sweep_reference.py) and the event rule as a plain loop over windows.  Also a host
stand-in for the command's backend (``HostBackend``), which drives a model that only has ``predict``
- the oracle of the conftest - through these windows."""
import numpy as np

import feed_reference
import sweep_reference

EVENT = np.dtype([('read', np.int64), ('cls', np.int32), ('first', np.int32), ('last', np.int32),
                  ('reserved', np.int32), ('peak', np.float64)])


def lengths_around(input_size):
    """The read lengths at which the window count or a window's padding changes."""
    L, h = input_size, input_size // 2
    return [0, 1, h - 1, h, L - 1, L, L + 1, L + h - 1, L + h, L + h + 1, 10 * h + 7]


def window_count(n, input_size):
    """W(n) = 1 for n <= L, else ceil((n - L) / h) + 1."""
    half = input_size // 2
    return 1 if n <= input_size else -((input_size - n) // half) + 1


def window_bounds(n, k, input_size, side):
    """[a, b) of window k of a read of n samples."""
    half = input_size // 2
    if side == 'start':
        return min(k * half, n), min(k * half + input_size, n)
    assert side == 'end'
    return max(n - k * half - input_size, 0), max(n - k * half, 0)


def window_offsets(lengths, input_size):
    counts = [window_count(int(n), input_size) for n in lengths]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def windows(signal, input_size, side):
    """float32 [W, L]: every window of one read, normalised over the samples present and padded
    behind (start) or in front (end); an empty window is zeros."""
    signal = np.asarray(signal, dtype=np.int16)
    n = len(signal)
    out = np.zeros((window_count(n, input_size), input_size), dtype=np.float32)
    for k in range(len(out)):
        a, b = window_bounds(n, k, input_size, side)
        if b == a:
            continue
        values = feed_reference.normalise(signal[None, a:b])[0]
        if side == 'start':
            out[k, :b - a] = values
        else:
            out[k, input_size - (b - a):] = values
    return out


def batch_windows(signals, input_size, side):
    """float32 [sum of W, L]: the windows of a batch in global window order."""
    return np.concatenate([windows(s, input_size, side) for s in signals])


def track(window_probs):
    """[W, C] per-window probabilities -> (best int32 [W], margin float64 [W]): the sweep's fold at
    steps = 1 with every window as its own read."""
    best, margin = sweep_reference.sweep(np.asarray(window_probs, dtype=np.float32)[:, None, :])
    return best[:, 0], margin[:, 0]


def events(best, margin, offsets, threshold, min_windows=1, skip_windows=0, max_events=None):
    """-> (events EVENT array - the first ``max_events`` - , the true total, interior events per
    read): maximal runs of consecutive windows of one read that fire one class, window by window."""
    found, interior = [], np.zeros(len(offsets) - 1, dtype=np.int32)
    for read in range(len(offsets) - 1):
        run = None                                      # [class, first, last, peak]
        runs = []
        for k in range(int(offsets[read + 1] - offsets[read])):
            at = int(offsets[read]) + k
            cls = int(best[at]) if best[at] != 0 and margin[at] >= threshold else 0
            if run is not None and cls == run[0]:
                run[2], run[3] = k, max(run[3], float(margin[at]))
                continue
            if run is not None:
                runs.append(run)
            run = [cls, k, k, float(margin[at])] if cls != 0 else None
        if run is not None:
            runs.append(run)
        for cls, first, last, peak in runs:
            if last - first + 1 >= min_windows:
                found.append((read, cls, first, last, 0, peak))
                interior[read] += first >= skip_windows
    kept = found if max_events is None else found[:max_events]
    return np.array(kept, dtype=EVENT), len(found), interior


def random_track(rng, lengths, density, n_classes=13):
    """A track over reads of ``lengths`` windows: a window fires (a barcode best, margin at least
    0.5) with probability ``density``, in runs - a firing window repeats the class before it half
    the time - and the others are class 0 with a large margin or a barcode with a small one."""
    total = int(np.sum(lengths))
    fires = rng.random(total) < density
    cls = rng.integers(1, n_classes, total)
    repeat = rng.random(total) < 0.5
    for i in range(1, total):
        if repeat[i]:
            cls[i] = cls[i - 1]
    best = np.where(fires, cls, np.where(rng.random(total) < 0.5, 0, cls)).astype(np.int32)
    margin = np.where(fires, rng.choice([0.5, 0.625, 0.75, 0.875, 1.0], total),
                      np.where(best == 0, 0.9375, rng.choice([0.0, 0.125, 0.25, 0.375], total)))
    return best, margin.astype(np.float64), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


class HostBackend:
    """What ``scan.scan`` asks of ``hip_backend`` - ``classify_pair`` and ``scan_packed`` - on the
    host, for models with ``predict`` and ``inputs`` (the conftest's OracleModel)."""

    def __init__(self):
        self.batches = 0

    @staticmethod
    def _signals(samples, offsets):
        return [samples[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]

    def classify_pair(self, start_model, end_model, samples, offsets, scan_size, score_diff,
                      mode='require_either'):
        from oracle import classify_ref
        self.batches += 1
        signals = self._signals(samples, offsets)
        calls = []
        for model, side in ((start_model, 'start'), (end_model, 'end')):
            if model is None:
                continue
            size = int(model.inputs[0].shape[1])
            calls.append(classify_ref.call_batch(lambda w: model.predict(w[:, :, None]), signals,
                                                 size, scan_size, score_diff, side)[0])
        final = calls[0] if len(calls) == 1 else [
            classify_ref.combine_calls(s, e, mode) for s, e in zip(*calls)]
        return np.array([0 if c == 'none' else int(c) for c in final], dtype=np.int32)

    def scan_packed(self, model, samples, offsets, side, threshold, min_windows=1, skip_windows=0):
        signals = self._signals(samples, offsets)
        size = int(model.inputs[0].shape[1])
        x = batch_windows(signals, size, side)
        best, margin = track(model.predict(x[:, :, None]))
        return events(best, margin, window_offsets([len(s) for s in signals], size), threshold,
                      min_windows, skip_windows)[0]
