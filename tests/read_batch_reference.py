"""NumPy restatement of what a read batch resident on the device has to compute (DESIGN.md
section 21): the trim rule decided in integers, the moments from exact integer sums, and the
windows of the adapter scan.  The bits a device implementation has to give."""
import math

import numpy as np

SKIP, STEP, AHEAD, NEEDED, BOUND = 10, 25, 5, 4, 250000
SHORTEST_TRIMMABLE = SKIP + AHEAD * STEP
WINDOW, EVERY, WINDOWS = 1500, 500, 30


def n_full(length):
    return 0 if length < SKIP + STEP else (length - SKIP) // STEP


def window_margins(signal):
    """25 Q_k - S_k^2 of every full window of a raw read, as int64 (at most 6.8e11)."""
    n = n_full(len(signal))
    x = np.asarray(signal[SKIP:SKIP + STEP * n], dtype=np.int64).reshape(n, STEP)
    s, q = x.sum(axis=1), (x * x).sum(axis=1)
    return STEP * q - s * s


def trim_position(signal):
    """The trim position of a raw int16 read, or -1 where it cannot be trimmed."""
    high = window_margins(signal) > BOUND
    n = len(high)
    k = 0
    while True:
        if k >= n:                                        # (a)
            return -1
        if high[k]:
            if k + AHEAD - 1 >= n:                        # (b)
                return -1
            if int(high[k:k + AHEAD].sum()) >= NEEDED:    # (c)
                return SKIP + STEP * k
        k += 1


def sums(signal):
    """(S, Q) of a signal as Python integers."""
    x = np.asarray(signal, dtype=np.int64)
    return int(x.sum()), int((x * x).sum())


def moments(signal):
    """(mean, std) of a trimmed read: D = n Q - S^2 as an exact integer, its conversion to a
    double correctly rounded (Python's), one square root, one division.  Empty: 0.0, 0.0."""
    n = len(signal)
    if n == 0:
        return 0.0, 0.0
    s, q = sums(signal)
    return s / n, math.sqrt(n * q - s * s) / n


def adapter_windows(length, side):
    """The scan's windows [a, b) of a trimmed read of that length, in the order of the
    reference's loops."""
    windows = []
    for i in range(0, EVERY * WINDOWS, EVERY):
        if side == 'start':
            windows.append((min(i, length), min(i + WINDOW, length)))
        elif length - i - WINDOW >= 0:
            windows.append((length - i - WINDOW, length - i))
    return windows
