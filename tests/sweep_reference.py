"""The sweep's contract (include/deepbinner_hip.h, "sweep") restated in NumPy, as simply as it can be
said: the fold over prefixes of a read's windows, make_sum_to_one in float64 with class 0 kept, the
best class with the lowest index among equals, its margin over the runner-up, the call at a
threshold, the three combine rules and the tally.  Also a host stand-in for the command's backend
(``HostBackend``), which drives a model that only has ``predict`` - the oracle of the conftest -
through the windows of tests' ``oracle/classify_ref.py``."""
import numpy as np

MODES = ('either', 'start', 'both')


def fold(window_probs):
    """window_probs [N, K, C] float32 -> merged [N, K, C] float32: row k - 1 is the merge of
    windows 0 .. k - 1 (class 0 the minimum, the barcodes the maximum; classify.py:368-374)."""
    p = np.asarray(window_probs, dtype=np.float32)
    merged = p.copy()
    for k in range(1, p.shape[1]):
        merged[:, k, 0] = np.minimum(merged[:, k - 1, 0], p[:, k, 0])
        merged[:, k, 1:] = np.maximum(merged[:, k - 1, 1:], p[:, k, 1:])
    return merged


def renormalise(merged):
    """make_sum_to_one (classify.py:387-393) in float64 over the last axis, class 0 kept; barcodes
    that are all zero stay zero."""
    p = np.asarray(merged, dtype=np.float64).copy()
    rest = p[..., 1:].sum(axis=-1)
    safe = np.where(rest > 0, rest, 1.0)
    factor = np.where(rest > 0, (1.0 - p[..., 0]) / safe, 0.0)
    p[..., 1:] = p[..., 1:] * factor[..., None]
    return p


def best_and_margin(probs):
    """probs [..., C] float64 -> (best int32 [...], margin float64 [...]): the highest value's
    class, the lowest index among equals (classify.py:285-295: a stable sort, reversed), and its
    lead over the highest of the others."""
    probs = np.asarray(probs, dtype=np.float64)
    best = np.argmax(probs, axis=-1)                  # (the first of equals)
    top = np.take_along_axis(probs, best[..., None], axis=-1)[..., 0]
    others = probs.copy()
    np.put_along_axis(others, best[..., None], -np.inf, axis=-1)
    return best.astype(np.int32), top - others.max(axis=-1)


def sweep(window_probs):
    """[N, K, C] per-window probabilities -> (best [N, K], margin [N, K])"""
    return best_and_margin(renormalise(fold(window_probs)))


def calls_at(best, margin, threshold):
    return np.where((best != 0) & (margin >= threshold), best, 0).astype(np.int32)


def combine(start, end, mode):
    """classify.py:298-322 on call numbers (0 = none), elementwise."""
    start, end = np.asarray(start), np.asarray(end)
    if mode == 'both':
        other = np.zeros_like(start)
    elif mode == 'start':
        other = np.where(end == 0, start, 0)
    else:
        assert mode == 'either'
        other = np.where(end == 0, start, np.where(start == 0, end, 0))
    return np.where(start == end, start, other)


def tally(start, end, thresholds, n_classes, labels=None):
    """start / end: (best, margin) [N, K] or None -> counts int64 [K, T, modes, C + 3]: per final
    class, then right / wrong / missed of the reads with a label >= 0."""
    sides = [s for s in (start, end) if s is not None]
    n, steps = sides[0][0].shape
    modes = MODES if len(sides) == 2 else ('-',)
    counts = np.zeros((steps, len(thresholds), len(modes), n_classes + 3), dtype=np.int64)
    known = None if labels is None else np.asarray(labels) >= 0
    for k in range(steps):
        for t, threshold in enumerate(thresholds):
            per_side = [calls_at(b[:, k], m[:, k], threshold) for b, m in sides]
            for j, mode in enumerate(modes):
                final = per_side[0] if len(sides) == 1 else combine(per_side[0], per_side[1], mode)
                inside = final[(final >= 0) & (final < n_classes)]
                counts[k, t, j, :n_classes] = np.bincount(inside, minlength=n_classes)
                if known is not None:
                    call, label = final[known], np.asarray(labels)[known]
                    counts[k, t, j, n_classes] = np.sum(call == label)
                    counts[k, t, j, n_classes + 1] = np.sum((call != label) & (call != 0))
                    counts[k, t, j, n_classes + 2] = np.sum((call == 0) & (label != 0))
    return counts


def hand_made(n_classes, steps, seed, n_reads=12):
    """Per-window probabilities [N, K, C] float32 with the rows a fold can get wrong; every value a
    multiple of 2^-9, so that sums are exact in any order and no barcode ties with class 0 by
    rounding."""
    rng = np.random.default_rng(seed)
    unit = np.float32(2.0 ** -9)
    rows = []
    tie = np.zeros((steps, n_classes), np.float32)          # two barcodes tie exactly
    tie[:, 0] = 64 * unit
    tie[:, 1:] = unit
    tie[:, [1, n_classes - 1]] = 200 * unit
    rows.append(tie)
    rows.append(np.full((steps, n_classes), unit, np.float32))       # all classes equal
    zero_best = np.full((steps, n_classes), unit, np.float32)        # class 0 best
    zero_best[:, 0] = 400 * unit
    rows.append(zero_best)
    only_zero = np.zeros((steps, n_classes), np.float32)             # p0 == 1, barcodes zero
    only_zero[:, 0] = 1.0
    rows.append(only_zero)
    moving = np.full((steps, n_classes), unit, np.float32)           # the maximum moves on
    moving[:, 0] = 100 * unit
    for s in range(steps):
        moving[s, 1 + s % (n_classes - 1)] = (150 + 10 * s) * unit
    rows.append(moving)
    late = only_zero.copy()                                          # a barcode appears late
    late[steps - 1, 0] = 10 * unit
    late[steps - 1, n_classes - 1] = 300 * unit
    rows.append(late)
    while len(rows) < n_reads:                                       # random rows on the grid
        r = rng.integers(1, 60, (steps, n_classes)).astype(np.float32) * unit
        r[:, 0] = rng.integers(1, 400, steps).astype(np.float32) * unit
        rows.append(r)
    return np.stack(rows[:n_reads])


def window_probs_of(predict, signals, input_size, max_scan_size, side):
    """Per-window probabilities [N, K, C] float32 of a model that only predicts, on the windows
    oracle/classify_ref.py cuts (classify.py:337-357)."""
    from oracle import classify_ref
    windows = classify_ref.make_windows(signals, input_size, max_scan_size, side)
    per_step = [np.asarray(predict(windows[s]), dtype=np.float32) for s in range(len(windows))]
    return np.stack(per_step, axis=1)


class HostBackend:
    """What ``sweep.sweep`` asks of ``hip_backend`` - ``sweep_pair``, ``sweep_tally``,
    ``sweep_counts`` - on the host, for models with ``predict``, ``input_size``, ``n_classes``."""
    SWEEP_MODES = MODES

    def __init__(self):
        self.batches = 0

    @staticmethod
    def sweep_counts(steps, n_thresholds, both, n_classes):
        return np.zeros((steps, n_thresholds, 3 if both else 1, n_classes + 3), dtype=np.int64)

    def sweep_pair(self, start_model, end_model, samples, offsets, max_scan_size):
        self.batches += 1
        signals = [samples[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
        out = []
        for model, side in ((start_model, 'start'), (end_model, 'end')):
            if model is None:
                out.append((None, None))
                continue
            size = int(model.inputs[0].shape[1])
            probs = window_probs_of(lambda w: model.predict(w[:, :, None]), signals, size,
                                    max_scan_size, side)
            out.append(sweep(probs))
        return tuple(out)

    def sweep_tally(self, start, end, thresholds, n_classes, labels=None, counts=None):
        start = start if start is not None and start[0] is not None else None
        end = end if end is not None and end[0] is not None else None
        got = tally(start, end, list(thresholds), n_classes, labels)
        if counts is None:
            return got
        counts += got
        return counts
