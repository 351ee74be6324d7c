"""
The signal stage of the reference's ``prep``: where are the adapter and the barcode in a read's
raw signal?  The reference's names (``prep_functions.py``, ``prep_native_start.py``,
``prep_native_end.py``) on top of ``dtw_locate_batch`` (``include/deepbinner_dtw.h``), and the
batch forms that give the device something to do:

  ``trim_signal(signal)``                                   prep_functions.py:78-88
  ``align_adapter_to_read_start_dtw(signal, adapter)``      prep_native_start.py:114-131
  ``align_adapter_to_read_end_dtw(signal, adapter)``        prep_native_end.py:114-134
  ``align_barcode_to_read_dtw(search, start, name, table)`` prep_functions.py:138-153
  ``locate_adapters(signals, adapter, side)``               all reads of a batch in one call
  ``locate_barcodes(signals, adapter_positions, barcodes, side)``

and two host pieces beside them:

  ``trim_positions(signals)``                               section 21's integer trim rule
  ``read_squiggles(path)``, ``write_squiggles(path, table)``

The expected squiggles of adapters and barcodes are not part of this package: the caller passes
them.  The sequence stage of ``prep`` (mappy, edlib) does not exist here and ``prep`` as a command
stays refused.

Positions index the TRIMMED signal, as the reference's functions return them.

What is uploaded.  The adapter scan looks at windows of 1,500 samples every 500, 30 of them: the
first (start) or last (end) 14,500 + 1,500 = 16,000 trimmed samples, and ``locate_adapters`` uploads
those as int16.  The barcode scan looks at [adapter_end - 100, adapter_end + 1,000) at the start -
no further than sample 16,998, so 16,999 samples from the front - and at
[adapter_start - 1,000, end of read) at the end - no further back than 17,000 samples from the
end; ``locate_barcodes`` uploads each read's search window alone.  Mean and standard deviation
are the whole trimmed read's (``signal_moments``), formed on the host from exact integer sums.
"""

import math
import sys

import numpy as np

from . import dtw_semi_global
from .trim_signal import CannotTrim, find_signal_start_pos

MAX_TRIM_AMOUNT = 2000             # prep_functions.py:29
THRESHOLD = 50.0                   # prep_native_start.py:124, prep_functions.py:149
WINDOW, STEP, SPAN = 1500, 500, 15000
ADAPTER_REACH = SPAN - STEP + WINDOW            # 16,000 samples from either end
START_BARCODE_BEFORE, START_BARCODE_AFTER = 100, 1000     # prep_native_start.py:90-92
END_BARCODE_BEFORE = 1000                                 # prep_native_end.py:91-92


def _say(out, text):
    if out is not None:
        print(text, file=sys.stderr if out is True else out)


def trim_signal(signal, out=True):
    """prep_functions.py:78-88, with its quirk: "excessive trimming" prints a verdict and the
    signal is trimmed and returned all the same.  ``None`` where trimming fails.  ``out``: where
    the reference's lines go - standard error, a file, or ``None`` for nowhere."""
    _say(out, '    untrimmed signal length: {}'.format(len(signal)))
    try:
        start_trim_pos = find_signal_start_pos(signal)
    except CannotTrim:
        _say(out, '  verdict: skipping due to failed signal trimming')
        return None
    _say(out, '    trim amount: {}'.format(start_trim_pos))
    if start_trim_pos > MAX_TRIM_AMOUNT:
        _say(out, '  verdict: skipping due to excessive trimming')
    return signal[start_trim_pos:]


def _as_int16(signal):
    signal = np.asarray(signal)
    if signal.dtype != np.int16:
        if signal.dtype.kind not in 'iu' or (len(signal) and (signal.min() < -32768 or
                                                              signal.max() > 32767)):
            raise ValueError('raw reads are int16 samples')
        signal = signal.astype(np.int16)
    return signal


def signal_moments(signal):
    """(mean, std) of an int16 signal as the header's contract has them: S = sum x and
    Q = sum x^2 as exact integers, D = L Q - S^2, mean = S / L, std = sqrt(D) / L."""
    length = len(signal)
    if length == 0:
        return 0.0, 0.0
    x = np.asarray(signal, dtype=np.int64)
    s, q = int(x.sum()), int((x * x).sum())
    d = length * q - s * s
    return s / length, math.sqrt(d) / length


def adapter_windows(length, side):
    """The windows [a, b) of a trimmed signal of ``length`` samples that the reference's loops
    look at, in their order.  Start (prep_native_start.py:115-118): slices that run off the end
    get shorter, then empty - the empty ones are listed, and skipped by the device as the
    reference's ``len(...) > 0`` skips them.  End (prep_native_end.py:115-121): counted from the
    back, those with ``range_start < 0`` left out."""
    windows = []
    for i in range(0, SPAN, STEP):
        if side == 'start':
            windows.append((min(i, length), min(i + WINDOW, length)))
        elif side == 'end':
            range_end = length - i
            if range_end - WINDOW < 0:
                continue
            windows.append((range_end - WINDOW, range_end))
        else:
            raise ValueError("side is 'start' or 'end'")
    return windows


def adapter_region(length, side):
    """The part [first, last) of a trimmed signal that ``adapter_windows`` can touch."""
    if side == 'start':
        return 0, min(length, ADAPTER_REACH)
    return max(0, length - ADAPTER_REACH), length


def barcode_window(length, adapter_position, side):
    """The barcode's search window [a, b) in a trimmed signal, or ``None`` where the reference
    refuses (``barcode_search_signal_start < 0``) or there is no adapter position."""
    if adapter_position is None or adapter_position[0] is None:
        return None
    adapter_start, adapter_end = adapter_position
    if side == 'start':
        first, last = adapter_end - START_BARCODE_BEFORE, adapter_end + START_BARCODE_AFTER
    elif side == 'end':
        first, last = adapter_start - END_BARCODE_BEFORE, length
    else:
        raise ValueError("side is 'start' or 'end'")
    if first < 0:
        return None
    return min(first, length), max(min(first, length), min(last, length))


class _Table:
    """The query table of a call: every distinct query signal once."""

    def __init__(self):
        self.arrays, self.index = [], {}

    def add(self, signal):
        if id(signal) not in self.index:
            self.index[id(signal)] = len(self.arrays)
            self.arrays.append(np.ascontiguousarray(signal, dtype=np.float64).ravel())
        return self.index[id(signal)]

    def packed(self):
        offsets = np.zeros(len(self.arrays) + 1, dtype=np.int64)
        np.cumsum([len(a) for a in self.arrays], out=offsets[1:])
        return np.concatenate(self.arrays), offsets


def locate(trimmed, regions, windows, threshold=THRESHOLD):
    """One ``dtw_locate_batch`` call.  ``trimmed[r]``: read r's trimmed int16 signal;
    ``regions[r] = (first, last)``: what of it is uploaded; ``windows[r]``: its group, a list of
    ``(a, b, query signal)`` in trimmed coordinates inside the region.  Returns a dict: per read
    ``positions`` ((start, end) in trimmed coordinates, or (None, None)), and the call's own
    ``distances``, ``job_positions`` (window-relative), ``slopes``, ``hits``, ``jobs``,
    ``group_offsets``."""
    table = _Table()
    pieces, mean_std, jobs, group_offsets = [], [], [], [0]
    for r, signal in enumerate(trimmed):
        first, last = regions[r]
        pieces.append(signal[first:last])
        mean_std.append(signal_moments(signal))
        for a, b, query in windows[r]:
            jobs.append((r, a - first, b - first, table.add(query)))
        group_offsets.append(len(jobs))
    if not jobs:
        return {'positions': [(None, None)] * len(trimmed), 'distances': np.zeros(0),
                'job_positions': np.zeros((0, 2), dtype=np.int32), 'slopes': np.zeros(0),
                'hits': np.full(len(trimmed), -1, dtype=np.int32), 'jobs': jobs,
                'group_offsets': group_offsets}
    region_offsets = np.zeros(len(pieces) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in pieces], out=region_offsets[1:])
    flat_queries, query_offsets = table.packed()
    distances, job_positions, slopes, hits = dtw_semi_global.locate_batch(
        np.concatenate(pieces), region_offsets, np.array(mean_std, dtype=np.float64),
        flat_queries, query_offsets, np.array(jobs, dtype=np.int64), group_offsets, threshold)
    positions = []
    for r, hit in enumerate(hits):
        if hit < 0:
            positions.append((None, None))
        else:
            at = jobs[hit][1] + regions[r][0]
            positions.append((int(job_positions[hit, 0]) + at, int(job_positions[hit, 1]) + at))
    return {'positions': positions, 'distances': distances, 'job_positions': job_positions,
            'slopes': slopes, 'hits': hits, 'jobs': jobs, 'group_offsets': group_offsets}


def _trim_all(signals):
    return [trim_signal(_as_int16(s), out=None) for s in signals]


def _scatter(n, kept, found):
    positions = [(None, None)] * n
    for r, position in zip(kept, found):
        positions[r] = position
    return positions


def locate_adapters(signals, adapter_signal, side):
    """The adapter scan of every read of a batch in one device call.  ``signals``: raw int16
    reads.  They are trimmed, the windows of ``adapter_windows`` are scanned for
    ``adapter_signal`` and the first with a distance <= 50.0 wins.  Returns per read
    ``(adapter_signal_start, adapter_signal_end)`` in the trimmed signal, or ``(None, None)``
    (no window hit, or the read could not be trimmed)."""
    trimmed = _trim_all(signals)
    kept = [r for r, t in enumerate(trimmed) if t is not None]
    chosen = [trimmed[r] for r in kept]
    result = locate(chosen, [adapter_region(len(t), side) for t in chosen],
                    [[(a, b, adapter_signal) for a, b in adapter_windows(len(t), side)]
                     for t in chosen])
    return _scatter(len(signals), kept, result['positions'])


def locate_barcodes(signals, adapter_positions, barcode_signals, side):
    """The barcode scan of every read of a batch in one device call.  ``adapter_positions``:
    what ``locate_adapters`` returned for these reads; ``barcode_signals[r]``: read r's expected
    barcode squiggle (the sequence stage names the barcode), or ``None`` for a read without one.
    Returns per read ``(barcode_signal_start, barcode_signal_end)`` in the trimmed signal, or
    ``(None, None)``: no barcode asked for, no adapter, a search window that would start before
    the signal, or a distance above 50.0."""
    if not len(signals) == len(adapter_positions) == len(barcode_signals):
        raise ValueError('one adapter position and one barcode signal (or None) per read, please')
    trimmed = _trim_all(signals)
    kept, regions = [], []
    for r, t in enumerate(trimmed):
        if t is None or barcode_signals[r] is None:
            continue
        window = barcode_window(len(t), adapter_positions[r], side)
        if window is not None:
            kept.append(r)
            regions.append(window)
    result = locate([trimmed[r] for r in kept], regions,
                    [[(a, b, barcode_signals[r])] for r, (a, b) in zip(kept, regions)])
    return _scatter(len(signals), kept, result['positions'])


def _is_raw(signal):
    return np.asarray(signal).dtype.kind in 'iu'


def _first_hit(signal, windows, query):
    """A normalised (floating-point) signal: the windows go to the device as they are, through
    ``dtw_rescaled_batch``, and the first hit is picked here."""
    signal = np.asarray(signal, dtype=np.float64)
    windows = [(a, b) for a, b in windows if b > a]
    results = dtw_semi_global.rescaled_batch([signal[a:b] for a, b in windows],
                                             [query] * len(windows), alignments=False)
    for (a, _), (distance, start, end, _, _, _) in zip(windows, results):
        if distance <= THRESHOLD:
            return start + a, end + a, distance
    return None, None, None


def _align_adapter(signal, adapter_signal, side):
    if _is_raw(signal):
        # taken as the trimmed read: normalised on the device with its own mean and std
        signal = _as_int16(signal)
        result = locate([signal], [adapter_region(len(signal), side)],
                        [[(a, b, adapter_signal) for a, b in adapter_windows(len(signal), side)]])
        start, end = result['positions'][0]
        distance = None if start is None else float(result['distances'][result['hits'][0]])
    else:
        start, end, distance = _first_hit(signal, adapter_windows(len(signal), side),
                                          adapter_signal)
    if start is None:
        print('  verdict: skipping due to high adapter DTW distance', file=sys.stderr)
        return None, None
    print('    adapter DTW: {}-{} ({:.2f})'.format(start, end, distance), file=sys.stderr)
    return start, end


def align_adapter_to_read_start_dtw(signal, adapter_signal):
    """prep_native_start.py:114-131.  ``signal``: the trimmed read, either normalised
    (floating point, as the reference passes it) or raw int16, which the device normalises."""
    return _align_adapter(signal, adapter_signal, 'start')


def align_adapter_to_read_end_dtw(signal, adapter_signal):
    """prep_native_end.py:114-134; ``signal`` as for the start."""
    return _align_adapter(signal, adapter_signal, 'end')


def align_barcode_to_read_dtw(barcode_search_signal, barcode_search_signal_start, barcode_name,
                              barcode_signals):
    """prep_functions.py:138-153: the refusal of a search window that would start before the
    signal, one rescaled DTW, the 50.0 verdict.  ``barcode_search_signal``: normalised."""
    if barcode_search_signal_start < 0:
        return None, None
    distance, start, end, _, _, _ = dtw_semi_global.rescaled_batch(
        [barcode_search_signal], [barcode_signals[barcode_name]], alignments=False)[0]
    start += barcode_search_signal_start
    end += barcode_search_signal_start
    print('    barcode{} DTW: {}-{} ({:.2f})'.format(barcode_name, start, end, distance),
          file=sys.stderr)
    if distance > THRESHOLD:
        print('  verdict: skipping due to high barcode DTW distance', file=sys.stderr)
        return None, None
    return start, end


# ------------------------------------------------------------------------------------------------
# Host pieces: the trim rule in integers for a list of reads, and the
# expected squiggles as a text file.
TRIM_SKIP, TRIM_STEP, TRIM_AHEAD, TRIM_NEEDED = 10, 25, 5, 4      # trim_signal.py:24-58
TRIM_BOUND = 250000            # 25 Q - S^2 above this: a population std above 20.0 (section 21)


TRIM_FIRST_LOOK = 16           # windows looked at first: most reads begin within 410 samples


def _trim_look(signals, windows):
    """The trim rule over the first ``windows`` windows of every read at once.  Returns an int64
    array: the position, -1 (CannotTrim), or -2 where the rule needs windows further on."""
    n = len(signals)
    n_full = np.array([0 if len(s) < TRIM_SKIP + TRIM_STEP else (len(s) - TRIM_SKIP) // TRIM_STEP
                       for s in signals], dtype=np.int64)
    seen = np.minimum(n_full, windows)
    block = np.zeros((n, windows * TRIM_STEP), dtype=np.int64)     # padding: windows that are not high
    for r, signal in enumerate(signals):
        take = int(seen[r]) * TRIM_STEP
        block[r, :take] = signal[TRIM_SKIP:TRIM_SKIP + take]
    x = block.reshape(n, windows, TRIM_STEP)
    s, q = x.sum(axis=2), (x * x).sum(axis=2)
    high = TRIM_STEP * q - s * s > TRIM_BOUND
    running = np.concatenate((np.zeros((n, 1), dtype=np.int64), np.cumsum(high, axis=1)), axis=1)
    ahead = np.zeros((n, windows), dtype=np.int64)                 # high among k .. k+4
    whole = windows - TRIM_AHEAD + 1
    ahead[:, :whole] = running[:, TRIM_AHEAD:] - running[:, :whole]
    last = np.arange(windows)[None, :] + TRIM_AHEAD - 1            # k + 4
    known = last < seen[:, None]               # all five windows are among those looked at
    beyond = last >= n_full[:, None]           # (b): the look-ahead leaves the read
    stop = high & known & (ahead >= TRIM_NEEDED)                   # (c)
    event = stop | (high & ~known)             # (c), (b), or a high window that needs more
    first = np.argmax(event, axis=1)
    rows = np.arange(n)
    out = np.where(stop[rows, first], TRIM_SKIP + TRIM_STEP * first,
                   np.where(beyond[rows, first], -1, -2))
    # no event: (a) at the end of the read, or quiet so far
    return np.where(event.any(axis=1), out, np.where(seen == n_full, -1, -2)).astype(np.int64)


def trim_positions(signals):
    """The trim position of every raw int16 read of a list, by the integer rule of DESIGN.md
    section 21, as an int64 array: what ``find_signal_start_pos`` returns, and -1 where it raises
    ``CannotTrim``.  The first 16 windows of all reads are decided in one set of NumPy operations;
    the reads whose rule needs windows further on are looked at again, eight times as far each
    time - in place of one ``np.std`` per window and read."""
    signals = [_as_int16(s) for s in signals]
    positions = np.full(len(signals), -1, dtype=np.int64)
    todo, windows = np.arange(len(signals)), TRIM_FIRST_LOOK
    while len(todo):
        found = _trim_look([signals[r] for r in todo], windows)
        positions[todo] = found
        todo = todo[found == -2]
        windows *= 8
    return positions


def _barcode_number(name):
    if not name.isdigit() or len(name) > 4:
        raise ValueError('a squiggle is named adapter or by its barcode number, not {!r}'
                         .format(name))
    return int(name)


def read_squiggles(path):
    """Expected squiggles from a text file, one per line: ``name<TAB>v1,v2,...``.  The name
    ``adapter`` is required; every other name is a barcode number (``01``, ``1``, ...).  Returns
    ``{'adapter': float64 array, 1: float64 array, ...}``.  ValueError, naming the line, for a
    duplicate name, a missing ``adapter``, and an empty, non-numeric or non-finite value."""
    table = {}
    with open(path, 'rt') as lines:
        for number, line in enumerate(lines, 1):
            line = line.rstrip('\r\n')
            if not line.strip():
                continue
            where = 'line {} of {}'.format(number, path)
            parts = line.split('\t')
            if len(parts) != 2:
                raise ValueError('{}: expected name<TAB>v1,v2,...'.format(where))
            name = parts[0].strip()
            try:
                key = name if name == 'adapter' else _barcode_number(name)
            except ValueError as e:
                raise ValueError('{}: {}'.format(where, e))
            if key in table:
                raise ValueError('{}: a second squiggle named {}'.format(where, name))
            try:
                values = np.array([float(v) for v in parts[1].split(',')], dtype=np.float64)
            except ValueError:
                raise ValueError('{}: an empty or non-numeric value'.format(where))
            if not np.isfinite(values).all():
                raise ValueError('{}: a value that is not finite'.format(where))
            table[key] = values
    if 'adapter' not in table:
        raise ValueError('{}: no squiggle named adapter'.format(path))
    return table


def write_squiggles(path, table):
    """The counterpart of ``read_squiggles``: ``adapter`` first, then the barcodes in ascending
    number, every value by ``repr`` so that it reads back to the same double."""
    if 'adapter' not in table:
        raise ValueError('no squiggle named adapter')
    names = ['adapter'] + sorted(k for k in table if k != 'adapter')
    with open(path, 'wt') as out:
        for key in names:
            values = np.asarray(table[key], dtype=np.float64).ravel()
            if not len(values) or not np.isfinite(values).all():
                raise ValueError('squiggle {} is empty or holds a value that is not finite'
                                 .format(key))
            name = key if key == 'adapter' else '{:02d}'.format(int(key))
            out.write('{}\t{}\n'.format(name, ','.join(repr(float(v)) for v in values)))
