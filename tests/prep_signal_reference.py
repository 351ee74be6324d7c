"""NumPy restatement of the contract of ``dtw_rescaled_batch`` and ``dtw_locate_batch``
(include/deepbinner_dtw.h, "prep's signal stage"), with ``oracle.dtw_ref`` for the DTW itself: the
bits the device has to give.  Beside it, the reference's own method (``lstsq`` fit, ``np.mean`` /
``np.std`` normalise) and its two adapter loops replayed in plain Python, to hold the restatement
and the window construction against."""
import math

import numpy as np

from oracle import dtw_ref

LANES = 64
SLOPE_RANGE = (0.75, 1.333)
INF = float('inf')


def squiggle(rng, n_levels, dwell=8):
    """tests/test_dtw.py::squiggle"""
    levels = rng.normal(0.0, 1.0, size=n_levels)
    return np.repeat(levels, rng.integers(max(1, dwell - 3), dwell + 4, size=n_levels))


def lane_sum(values):
    """The header's summation order: partial l takes entries l, l + 64, ... in order, from +0.0;
    the total takes the 64 partials in lane order, from +0.0.  (Padding with +0.0 changes no
    partial: none of them is ever -0.0.)"""
    padded = np.zeros(-(-max(len(values), 1) // LANES) * LANES, dtype=np.float64)
    padded[:len(values)] = values
    partial = np.zeros(LANES, dtype=np.float64)
    for row in padded.reshape(-1, LANES):
        partial = partial + row
    total = np.float64(0.0)
    for value in partial:
        total = total + value
    return total


def fit(ref, query, pairs):
    """(m, b), or None where no line can be fitted.  ``pairs``: pass 1's alignment from start to
    end, as dtw_ref returns it; the stored order the sums run in is the reverse."""
    stored = np.array(pairs, dtype=np.int64).reshape(-1, 2)[::-1]
    x, y = query[stored[:, 1]], ref[stored[:, 0]]
    n = np.float64(len(x))
    sx, sy, sxx, sxy = lane_sum(x), lane_sum(y), lane_sum(x * x), lane_sum(x * y)
    with np.errstate(all='ignore'):
        denominator = n * sxx - sx * sx
        if denominator == 0.0 or not np.isfinite(denominator):
            return None
        m = (n * sxy - sx * sy) / denominator
        b = (sy - m * sx) / n
    return m, b


def rescaled(ref, query):
    """(distance, ref_start, ref_end, slope, pairs, query') as the contract has them."""
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    query = np.ascontiguousarray(query, dtype=np.float64)
    _, _, _, pairs = dtw_ref.semi_global_dtw(ref, query)
    line = fit(ref, query, pairs)
    if line is None:
        moved, slope = query.copy(), float('nan')
    else:
        with np.errstate(all='ignore'):
            moved, slope = line[0] * query + line[1], float(line[0])
    distance, start, end, pairs = dtw_ref.semi_global_dtw(ref, moved)
    if line is None or slope < SLOPE_RANGE[0] or slope > SLOPE_RANGE[1]:
        distance = INF
    return distance, start, end, slope, np.array(pairs, dtype=np.int32).reshape(-1, 2), moved


def queries_beside_a_slope_bound(ref, query, bound):
    """(inside, outside): two multiples c * query, neighbours in c, whose fitted slopes lie on
    either side of ``bound`` (0.75 or 1.333): c walks away from 1 until the slope has crossed the
    bound, then bisection on c with this restatement, so the slopes are as close to the bound as
    a change of c in its last bits makes them."""
    def outside(c):
        slope = rescaled(ref, c * query)[3]
        return slope < bound if bound < 1.0 else slope > bound
    good, bad = 1.0, 1.0
    while not outside(bad):
        good, bad = bad, bad + (0.03 if bound < 1.0 else -0.03)
        assert 0.5 < bad < 2.0
    for _ in range(60):
        middle = 0.5 * (good + bad)
        if outside(middle):
            bad = middle
        else:
            good = middle
    return good * query, bad * query


def moments(signal):
    length = len(signal)
    s = sum(int(v) for v in signal)
    q = sum(int(v) * int(v) for v in signal)
    return s / length, math.sqrt(length * q - s * s) / length


def normalised(samples, mean, std):
    centred = np.asarray(samples, dtype=np.float64) - mean
    return centred / std if std > 0.0 else centred


def first_hit(distances, threshold):
    for k, d in enumerate(distances):
        if d <= threshold and d < INF:
            return k
    return -1


def locate(regions, mean_std, queries, jobs, group_offsets, threshold):
    """``regions[r]``: int16 array; jobs: (read, from, to, query).  Returns distances,
    positions[n, 2], slopes, hits as the contract has them."""
    signals = [normalised(region, *mean_std[r]) for r, region in enumerate(regions)]
    distances, positions, slopes = [], [], []
    for read, first, last, query in jobs:
        if first == last:
            distances.append(INF)
            positions.append((-1, -1))
            slopes.append(float('nan'))
            continue
        d, s, e, m, _, _ = rescaled(signals[read][first:last], queries[query])
        distances.append(d)
        positions.append((s, e))
        slopes.append(m)
    hits = []
    for g in range(len(group_offsets) - 1):
        hit = first_hit(distances[group_offsets[g]:group_offsets[g + 1]], threshold)
        hits.append(-1 if hit < 0 else group_offsets[g] + hit)
    return (np.array(distances), np.array(positions, dtype=np.int32).reshape(-1, 2),
            np.array(slopes), np.array(hits, dtype=np.int32))


# ------------------------------------------------------------------ the reference's own method
def reference_rescaled(ref, query):
    """dtw_semi_global.py:61-95 with the oracle's DTW: lstsq fit, two iterations."""
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    query = np.array(query, dtype=np.float64)
    _, _, _, pairs = dtw_ref.semi_global_dtw(ref, query)
    x = [query[j] for _, j in pairs]
    y = [ref[i] for i, _ in pairs]
    m, b = np.linalg.lstsq(np.vstack([x, np.ones(len(x))]).T, y, rcond=None)[0]
    query = m * query + b
    distance, start, end, pairs = dtw_ref.semi_global_dtw(ref, query)
    if m < SLOPE_RANGE[0] or m > SLOPE_RANGE[1]:
        distance = INF
    return distance, start, end, m, np.array(pairs, dtype=np.int32).reshape(-1, 2), query


def reference_normalise(signal):
    """trim_signal.py:61-69"""
    if len(signal) == 0:
        return signal
    mean = np.mean(signal)
    stdev = np.std(signal)
    if stdev > 0.0:
        return (signal - mean) / stdev
    return signal - mean


def reference_start_windows(length):
    """prep_native_start.py:115-118 on a signal of that length: the slices a DTW is run on."""
    signal = range(length)
    windows = []
    for range_start in range(0, 15000, 500):
        range_end = range_start + 1500
        search = signal[range_start:range_end]
        if len(search) > 0:
            windows.append((search[0], search[-1] + 1))
    return windows


def reference_end_windows(length):
    """prep_native_end.py:115-121"""
    signal = range(length)
    windows = []
    for i in range(0, 15000, 500):
        range_end = len(signal) - i
        range_start = range_end - 1500
        if range_start < 0:
            continue
        search = signal[range_start:range_end]
        if len(search) > 0:
            windows.append((search[0], search[-1] + 1))
    return windows
