"""Restatements for ``deepbinner_amd.samples``: the cutting rules of the reference's ``prep``
replayed with a generator passed in, and its two spacing verdicts; and the synthetic raw reads
``prep_signal.trim_positions`` is tried on."""
import numpy as np

import prep_signal_reference as P


def synthetic_raw(rng):
    """quiet open pore of random length with isolated noisy windows, then signal"""
    quiet = rng.integers(0, 3000)
    pore = 520 + rng.integers(-3, 4, size=quiet)
    for at in rng.integers(0, max(quiet, 1), size=rng.integers(0, 6)):
        pore[at:at + rng.integers(5, 60)] += rng.integers(-200, 200)
    signal = np.round(P.squiggle(rng, rng.integers(1, 120)) * 80 + 500)
    return np.concatenate([pore, signal]).astype(np.int16)


# ---- the reference's cutting rules, on a generator passed in -----------------------------------
# (prep_functions.py:156-233; each returns the slice that the reference prints, or None)
def reference_around(rng, signal, include_start, include_end, size):
    low = max(0, include_end - size)
    if low > include_start:
        return None                        # randint raises: the sample is dropped
    start = rng.randint(low, include_start)
    end = start + size
    if end > len(signal):
        start, end = len(signal) - size, len(signal)
    sample = signal[start:end]
    return sample if len(sample) == size else None


def reference_middle(rng, signal, size):
    high = len(signal) - 25000 - size
    if high < 25000:
        return None
    start = rng.randint(25000, high)
    return signal[start:start + size]


def reference_before(rng, signal, before_point, size):
    if before_point - size < 0:
        return None
    start = rng.randint(0, before_point - size)
    sample = signal[start:start + size]
    return sample if len(sample) == size else None


def reference_after(rng, signal, after_point, size):
    if after_point + size > len(signal):
        return None
    end = rng.randint(after_point + size, len(signal))
    sample = signal[end - size:end]
    return sample if len(sample) == size else None


def reference_oddly_spaced(side, adapter, barcode, size):
    """prep_native_start.py:152-166 / prep_native_end.py:155-169 -> None, 'long' or 'gap'"""
    if barcode[1] - barcode[0] >= size:
        return 'long'
    if side == 'start':
        gap = barcode[0] - adapter[1]
        return 'gap' if gap < 15 or gap > 90 else None
    gap = adapter[0] - barcode[1]
    return 'gap' if gap < -100 or gap > -20 else None
