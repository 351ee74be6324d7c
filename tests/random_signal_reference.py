"""A helper, not a test: the random signals of ``balance`` restated in NumPy - the contract of
``include/deepbinner_hip.h``, "random signals" (DESIGN.md section 23).  Every operation is written
as the header lists it, in float64, so flat and perlin values are held bit for bit; the Gaussian
kinds go through ``log`` and ``cos`` of another library, which can move a truncated value (by one)
only where the value before truncation lies on an integer - ``signals`` returns each value's
distance from the nearest integer so that a test can demand that its cases stay clear of that.
"""
import functools

import numpy as np

import train_reference as tr

M32 = 0xFFFFFFFF
FLAT, GAUSSIAN, MULTI_GAUSSIAN, PERLIN = 0, 1, 2, 3
LAYER_SIGNAL, LAYER_SEGMENT, LAYER_DRAW, LAYER_GRADIENT = 11, 12, 13, 14
GUARD = 2.0 ** -30


def bits(seed, layer, signal, position, channel):
    """24 bits as uint64; signal, position and channel broadcast against each other"""
    seed = int(seed) & (2 ** 64 - 1)
    lo, hi = seed & M32, seed >> 32
    m = np.uint64(M32)
    h = tr._mix(np.uint64((lo + layer * 0x9e3779b9) & M32))
    h = tr._mix(h ^ np.uint64(hi))
    h = tr._mix((h + np.asarray(signal, dtype=np.uint64)) & m)
    counter = (np.asarray(position, dtype=np.uint64) * np.uint64(256)
               + np.asarray(channel, dtype=np.uint64)) & m
    return tr._mix(h ^ counter) >> np.uint64(8)


def unit(b):
    return b.astype(np.float64) / 16777216.0


def parameters(seed, s):
    b = [bits(seed, LAYER_SIGNAL, s, 0, c) for c in range(8)]
    return {'kind': int(b[0] % np.uint64(4)), 'level': int(b[1] % np.uint64(1001)),
            'mean': float(300.0 + 300.0 * unit(b[2])), 'stdev': float(10.0 + 490.0 * unit(b[3])),
            'octaves': 1 + int(b[4] % np.uint64(4)), 'step': float(0.001 + 0.039 * unit(b[5])),
            'start': float(unit(b[6])), 'factor': float(10.0 + 290.0 * unit(b[7]))}


def normal(seed, s, size):
    i = np.arange(size)
    u1 = (bits(seed, LAYER_DRAW, s, i, 0).astype(np.float64) + 1.0) / 16777216.0
    u2 = bits(seed, LAYER_DRAW, s, i, 1).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def segments(seed, s, size):
    """per value: the mean and the stdev of the segment it lies in, and the number of segments"""
    mean, stdev = np.empty(size), np.empty(size)
    at, k = 0, 0
    while at < size:
        length = 100 + int(bits(seed, LAYER_SEGMENT, s, k, 0) % np.uint64(401))
        mean[at:at + length] = 300.0 + 300.0 * unit(bits(seed, LAYER_SEGMENT, s, k, 1))
        stdev[at:at + length] = 10.0 + 490.0 * unit(bits(seed, LAYER_SEGMENT, s, k, 2))
        at, k = at + length, k + 1
    return mean, stdev, k


def perlin(seed, s, p, size):
    x = p['start'] + np.arange(size).astype(np.float64) * p['step']
    total, weights = np.zeros(size), 0.0
    for k in range(p['octaves']):
        amp = 0.5 ** k
        xk = x * (2.0 ** k)
        j = np.floor(xk)
        t = xk - j
        f = t * t * t * (t * (t * 6.0 - 15.0) + 10.0)
        a = (2.0 * unit(bits(seed, LAYER_GRADIENT, s, j.astype(np.uint64), k)) - 1.0) * t
        b = (2.0 * unit(bits(seed, LAYER_GRADIENT, s, j.astype(np.uint64) + np.uint64(1), k)) - 1.0) * (t - 1.0)
        n = a + f * (b - a)
        total = total + amp * 2.0 * n
        weights = weights + amp
    return p['mean'] + p['factor'] * (total / weights)


def signal(seed, s, size):
    """-> (int16 values, kind, the smallest distance of an untruncated Gaussian value from an
    integer - inf for the exact kinds)"""
    p = parameters(seed, s)
    if p['kind'] == FLAT:
        return np.full(size, p['level'], dtype=np.int16), FLAT, np.inf
    if p['kind'] == PERLIN:
        return np.trunc(perlin(seed, s, p, size)).astype(np.int16), PERLIN, np.inf
    if p['kind'] == GAUSSIAN:
        raw = p['mean'] + p['stdev'] * normal(seed, s, size)
    else:
        mean, stdev, _ = segments(seed, s, size)
        raw = mean + stdev * normal(seed, s, size)
    return np.trunc(raw).astype(np.int16), p['kind'], float(np.abs(raw - np.rint(raw)).min())


def signals(seed, first, n, size):
    """-> (int16 [n, size], kinds [n], the smallest distance from an integer over all of them)"""
    rows, kinds, nearest = [], [], np.inf
    for s in range(first, first + n):
        row, kind, near = signal(seed, s, size)
        rows.append(row)
        kinds.append(kind)
        nearest = min(nearest, near)
    return np.stack(rows), np.array(kinds), nearest


# Rows past one chunk of 256 multi_gaussian segments (256 * 500 = 128,000 values), and the longest
# row the entries take: 8 signals each, seed 3 + size, first signal 0.  Both hold all four kinds,
# every multi_gaussian one has more than 256 segments, and the guard holds (test_random_signals.py).
LONG_SIZES = [131072, 2 ** 20]
LONG_SIGNALS = 8
# More signals than the grid has workgroups (65,536), of 102 values - the smallest row with two
# segments.  The guard over all 6.7 million values holds at seed 8, the first seed tried.
MANY_SEED, MANY_SIGNALS, MANY_SIZE = 8, 65536 + 64, 102


@functools.lru_cache(maxsize=None)
def long_case(size):
    """signals() of a LONG_SIZES case, computed once; the rows are read-only"""
    rows, kinds, nearest = signals(3 + size, 0, LONG_SIGNALS, size)
    rows.setflags(write=False)
    return rows, kinds, nearest


@functools.lru_cache(maxsize=None)
def many_case_nearest():
    return nearest_of_many(MANY_SEED, 0, MANY_SIGNALS, MANY_SIZE)


def nearest_of_many(seed, first, n, size):
    """signals()' third result for n short signals, without a loop over the signals: the draws are
    hashed for every (signal, position) at once, and only the multi_gaussian signals walk their
    segments, all of them together, segment number by segment number"""
    s = np.arange(first, first + n, dtype=np.uint64)
    kind = bits(seed, LAYER_SIGNAL, s, 0, 0) % np.uint64(4)
    drawn = np.flatnonzero((kind == GAUSSIAN) | (kind == MULTI_GAUSSIAN))
    if not drawn.size:
        return np.inf
    multi = kind[drawn] == MULTI_GAUSSIAN
    column, i = s[drawn][:, None], np.arange(size, dtype=np.uint64)[None, :]
    u1 = (bits(seed, LAYER_DRAW, column, i, 0).astype(np.float64) + 1.0) / 16777216.0
    u2 = bits(seed, LAYER_DRAW, column, i, 1).astype(np.float64) / 16777216.0
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    mean = np.broadcast_to((300.0 + 300.0 * unit(bits(seed, LAYER_SIGNAL, column, 0, 2))), z.shape).copy()
    stdev = np.broadcast_to((10.0 + 490.0 * unit(bits(seed, LAYER_SIGNAL, column, 0, 3))), z.shape).copy()
    walkers = s[drawn][multi]
    seg_mean, seg_stdev = np.empty((walkers.size, size)), np.empty((walkers.size, size))
    at, k, places = np.zeros(walkers.size, dtype=np.int64), 0, np.arange(size)[None, :]
    while (at < size).any():
        length = 100 + (bits(seed, LAYER_SEGMENT, walkers, k, 0) % np.uint64(401)).astype(np.int64)
        inside = (places >= at[:, None]) & (places < (at + length)[:, None])
        seg_mean = np.where(inside, (300.0 + 300.0 * unit(bits(seed, LAYER_SEGMENT, walkers, k, 1)))[:, None], seg_mean)
        seg_stdev = np.where(inside, (10.0 + 490.0 * unit(bits(seed, LAYER_SEGMENT, walkers, k, 2)))[:, None], seg_stdev)
        at, k = at + length, k + 1
    mean[multi], stdev[multi] = seg_mean, seg_stdev
    raw = mean + stdev * z
    return float(np.abs(raw - np.rint(raw)).min())


def nearest_at_size_one(seed, first, n):
    """signals()' third result for n signals of ONE value, without a loop over the signals"""
    s = np.arange(first, first + n, dtype=np.uint64)
    kind = bits(seed, LAYER_SIGNAL, s, 0, 0) % np.uint64(4)
    u1 = (bits(seed, LAYER_DRAW, s, 0, 0).astype(np.float64) + 1.0) / 16777216.0
    u2 = bits(seed, LAYER_DRAW, s, 0, 1).astype(np.float64) / 16777216.0
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    one = (300.0 + 300.0 * unit(bits(seed, LAYER_SIGNAL, s, 0, 2))) + (10.0 + 490.0 * unit(bits(seed, LAYER_SIGNAL, s, 0, 3))) * z
    many = (300.0 + 300.0 * unit(bits(seed, LAYER_SEGMENT, s, 0, 1))) + (10.0 + 490.0 * unit(bits(seed, LAYER_SEGMENT, s, 0, 2))) * z
    raw = np.where(kind == GAUSSIAN, one, many)[(kind == GAUSSIAN) | (kind == MULTI_GAUSSIAN)]
    return float(np.abs(raw - np.rint(raw)).min()) if raw.size else np.inf
