"""The sweep: calls at every scan size from one window pass, and their tally ("sweep")."""

import ctypes

import numpy as np

from ._abi import _handle, _packed, _ptr, check, load_library
from ._device import device_arrays, synchronize


def sweep_steps(input_size, max_scan_size):
    """Scan sizes a sweep covers: input_size / 2 times 1 .. this many."""
    half = int(input_size) // 2
    steps = int(max_scan_size) // half if half else 0
    if steps < 1 or steps * half != int(max_scan_size):
        raise ValueError('max_scan_size must be a positive multiple of half the model input size')
    return steps


def sweep_pair(start_model, end_model, samples, offsets, max_scan_size):
    """One batch of packed reads (as ``classify_pair`` takes them) through the window pass of the
    start and the end model at ``max_scan_size`` and the fold over scan sizes, in ONE call of the
    C ABI (``dbh_sweep_pair_i16``) -> ((best_s, margin_s), (best_e, margin_e)): int32 and float64
    [N, K], column k - 1 for scan size k * input_size / 2.  The call at threshold t is
    ``np.where((best != 0) & (margin >= t), best, 0)``.  The pair of a model that is None is
    (None, None)."""
    lib = load_library()
    models = (start_model, end_model)
    first = next((m for m in models if m is not None), None)
    if first is None:
        raise ValueError('no model')
    if any(m is not None and m.input_size != first.input_size for m in models):
        raise ValueError('the two models of a sweep must have one input size')
    steps = sweep_steps(first.input_size, max_scan_size)
    samples, offsets, n = _packed(samples, offsets)
    best = [np.zeros((n, steps), dtype=np.int32) if m is not None else None for m in models]
    margin = [np.zeros((n, steps), dtype=np.float64) if m is not None else None for m in models]
    if n > 0:
        check(lib.dbh_sweep_pair_i16(
            _handle(start_model), _handle(end_model),
            samples.ctypes.data if samples.size else None, offsets.ctypes.data, n,
            int(max_scan_size), _ptr(best[0]), _ptr(margin[0]), _ptr(best[1]), _ptr(margin[1])),
            'dbh_sweep_pair_i16')
    return (best[0], margin[0]), (best[1], margin[1])


SWEEP_MODES = ('either', 'start', 'both')      # DBH_REQUIRE_EITHER, _START, _BOTH


def sweep_counts(steps, n_thresholds, both, n_classes):
    """The zeroed counts of ``sweep_tally``: int64 [K, T, modes, C + 3] - per final class, then
    right, wrong, missed - with three modes (SWEEP_MODES) for two sides and one for one."""
    return np.zeros((int(steps), int(n_thresholds), 3 if both else 1, int(n_classes) + 3),
                    dtype=np.int64)


def sweep_tally(start, end, thresholds, n_classes, labels=None, counts=None):
    """The outcomes of one batch, counted on the device (``dbh_sweep_tally``): ``start`` / ``end``
    are the (best, margin) pairs of ``sweep_pair`` (None or (None, None): that side is not there),
    ``labels`` int32 per read (0 = known to carry no barcode, negative = unknown) or None.  ADDS
    into ``counts`` (``sweep_counts``; made when None) and returns it."""
    sides = [side if side is not None and side[0] is not None else None for side in (start, end)]
    if sides[0] is None and sides[1] is None:
        raise ValueError('no side')
    shape = next(side[0].shape for side in sides if side is not None)
    n, steps = shape
    held = []
    for side in sides:
        if side is None:
            held.append((None, None))
            continue
        best = np.ascontiguousarray(side[0], dtype=np.int32)
        margin = np.ascontiguousarray(side[1], dtype=np.float64)
        if best.shape != shape or margin.shape != shape:
            raise ValueError('best and margin of both sides must be [N, K] alike')
        held.append((best, margin))
    thresholds = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.shape != (n,):
            raise ValueError('one label per read')
    fresh = sweep_counts(steps, len(thresholds), sides[0] is not None and sides[1] is not None,
                         n_classes)
    counts, want = fresh if counts is None else counts, fresh.shape
    if counts.shape != want or counts.dtype != np.int64 or not counts.flags['C_CONTIGUOUS']:
        raise ValueError('counts must be a C-contiguous int64 array of shape {}'.format(want))
    check(load_library().dbh_sweep_tally(
        _ptr(held[0][0]), _ptr(held[0][1]), _ptr(held[1][0]), _ptr(held[1][1]), _ptr(labels), n, steps,
        int(n_classes), thresholds.ctypes.data if thresholds.size else None, len(thresholds),
        counts.ctypes.data), 'dbh_sweep_tally')
    return counts


EARLY_COLUMNS = ('decided', 'agree', 'changed', 'lost', 'late', 'windows', 'samples', 'length')


def sweep_early_pushes(input_size, scan_size, chunk_samples):
    """P = ceil((scan_size + input_size / 2) / chunk_samples): the push by which a replay in chunks
    of ``chunk_samples`` has folded every window (``dbh_sweep_early_pushes``; above 4096: refused)."""
    pushes = ctypes.c_int(0)
    check(load_library().dbh_sweep_early_pushes(int(input_size), int(scan_size), int(chunk_samples),
                                                ctypes.byref(pushes)), 'dbh_sweep_early_pushes')
    return pushes.value


def sweep_early_counts(steps, n_thresholds, both, n_classes, pushes=None):
    """The zeroed arrays of ``sweep_early_tally``, all int64 with first axis min_windows - 1:
    calls [K, T, modes, C + 3] (``sweep_counts``), early [K, T, 8] (EARLY_COLUMNS), windows
    [K, T, K] and pushes [K, T, ``pushes``] (None without ``pushes``: no read lengths)."""
    k, t = int(steps), int(n_thresholds)
    return (sweep_counts(k, t, both, n_classes), np.zeros((k, t, 8), dtype=np.int64),
            np.zeros((k, t, k), dtype=np.int64),
            None if pushes is None else np.zeros((k, t, int(pushes)), dtype=np.int64))


def _early(entry, start, end, thresholds, n_classes, labels, lengths, input_size, chunk_samples,
           counts):
    best = np.ascontiguousarray(start[0], dtype=np.int32)
    (n, steps), held = best.shape, [best, np.ascontiguousarray(start[1], dtype=np.float64)]
    both = end is not None and end[0] is not None
    if both:
        held += [np.ascontiguousarray(end[0], dtype=np.int32),
                 np.ascontiguousarray(end[1], dtype=np.float64)]
    if any(a.shape != (n, steps) for a in held):
        raise ValueError('best and margin of both sides must be [N, K] alike')
    thresholds = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int32)
    if lengths is not None:
        lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    if any(a is not None and a.shape != (n,) for a in (labels, lengths)):
        raise ValueError('one label and one length per read')
    pushes = None if lengths is None else sweep_early_pushes(input_size, steps * (int(input_size) // 2),
                                                             chunk_samples)
    fresh = sweep_early_counts(steps, len(thresholds), both, n_classes, pushes)
    counts = fresh if counts is None else tuple(counts)
    for got, want in zip(counts, fresh):
        if (got is None) != (want is None) or (want is not None and (
                got.shape != want.shape or got.dtype != np.int64 or not got.flags['C_CONTIGUOUS'])):
            raise ValueError('counts must be the arrays of sweep_early_counts')
    check(getattr(load_library(), entry)(
        _ptr(held[0]), _ptr(held[1]), _ptr(held[2]) if both else None,
        _ptr(held[3]) if both else None, _ptr(labels), _ptr(lengths), n, steps, int(n_classes),
        int(input_size), int(chunk_samples), thresholds.ctypes.data if thresholds.size else None,
        len(thresholds), *[_ptr(a) for a in counts]), entry)
    return counts


def sweep_early_tally(start, end, thresholds, n_classes, labels=None, lengths=None, input_size=1024,
                      chunk_samples=1600, counts=None):
    """What a live session would have decided early at every ``min_windows`` 1 .. K and every
    threshold, counted on the device from the tracks of ``sweep_pair`` (``dbh_sweep_early_tally``):
    ``start`` is required, ``end`` (or None) makes the calls those of a pair session; ``lengths``
    int64 per read, taken before any clip (None: no pushes, samples or length).  ADDS into ``counts``
    (``sweep_early_counts``; made when None) and returns (calls, early, windows, pushes)."""
    return _early('dbh_sweep_early_tally', start, end, thresholds, n_classes, labels, lengths,
                  input_size, chunk_samples, counts)


def sweep_early_host(start, end, thresholds, n_classes, labels=None, lengths=None, input_size=1024,
                     chunk_samples=1600, counts=None):
    """``sweep_early_tally`` by the same rule on the host, no device (``dbh_sweep_early_host``)."""
    return _early('dbh_sweep_early_host', start, end, thresholds, n_classes, labels, lengths,
                  input_size, chunk_samples, counts)


def sweep_windows(model, window_probs):
    """The fold alone (``dbh_sweep_windows_dev``; parity tests): per-window probabilities float32
    [N, K, C] of ``model``'s class count -> (best int32 [N, K], margin float64 [N, K]), by the form
    of the fold that belongs to the model's kind."""
    window_probs = np.ascontiguousarray(window_probs, dtype=np.float32)
    n, steps, n_classes = window_probs.shape
    if n_classes != model.n_classes:
        raise ValueError('window_probs must have the model\'s {} classes'.format(model.n_classes))
    best = np.zeros((n, steps), dtype=np.int32)
    margin = np.zeros((n, steps), dtype=np.float64)
    if n == 0:
        return best, margin
    with device_arrays(window_probs, best.nbytes, margin.nbytes) as (d_probs, d_best, d_margin):
        check(load_library().dbh_sweep_windows_dev(model.handle, d_probs.ptr, n, steps, d_best.ptr,
                                                   d_margin.ptr, None), 'dbh_sweep_windows_dev')
        synchronize()
        return (d_best.download(best.shape, np.int32), d_margin.download(margin.shape, np.float64))
