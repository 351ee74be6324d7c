"""The scan: every window of a read through the network, and runs of windows that fire one class
as events (include/deepbinner_hip.h, "scan").  The whole pass is ``HipModel.scan_packed``; here are
its record, its window arithmetic and the parity-only entries of its parts."""

import ctypes

import numpy as np

from ._abi import _packed, _side, check, load_library
from ._device import device_arrays, synchronize

# dbh_scan_event: a run of windows of one read that fire one class (include/deepbinner_hip.h, "scan")
SCAN_EVENT = np.dtype([('read', np.int64), ('cls', np.int32), ('first', np.int32),
                       ('last', np.int32), ('reserved', np.int32), ('peak', np.float64)])
assert SCAN_EVENT.itemsize == 32


def scan_window_count(input_size, n_samples):
    """W(n): the windows a scan cuts from a read of ``n_samples`` samples (an integer, or an array
    of them -> int64 array): 1 up to ``input_size`` samples, then one more per half input size
    begun (``dbh_scan_window_count``)."""
    input_size = int(input_size)
    if input_size % 2 or not 96 <= input_size <= 16384:
        raise ValueError('input_size must be even and from 96 to 16,384')
    if np.ndim(n_samples):
        n = np.asarray(n_samples, dtype=np.int64)
        if (n < 0).any():
            raise ValueError('a read cannot have a negative length')
        half = input_size // 2
        return np.where(n <= input_size, 1, (n - input_size + half - 1) // half + 1).astype(np.int64)
    count = ctypes.c_int64(0)
    check(load_library().dbh_scan_window_count(input_size, int(n_samples), ctypes.byref(count)),
          'dbh_scan_window_count')
    return count.value


def host_window_offsets(input_size, offsets):
    """Sample offsets int64 [N + 1] of packed reads -> where each read's windows begin in global
    window order, int64 [N + 1], worked out on the host."""
    return np.concatenate(
        [[0], np.cumsum(scan_window_count(input_size, np.diff(offsets)))]).astype(np.int64)


def scan_packed(model, samples, offsets, side, threshold, min_windows=1, skip_windows=0):
    """``model.scan_packed`` as a function of the backend (what ``scan.scan`` calls)."""
    return model.scan_packed(samples, offsets, side, threshold, min_windows, skip_windows)


def scan_window_offsets(offsets, input_size):
    """``dbh_scan_window_offsets_dev`` alone (parity tests): sample offsets int64 [N + 1] ->
    window offsets int64 [N + 1]."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    with device_arrays(offsets, 8 * (n + 1)) as (d_offsets, d_out):
        check(load_library().dbh_scan_window_offsets_dev(d_offsets.ptr, n, int(input_size),
                                                         d_out.ptr, None),
              'dbh_scan_window_offsets_dev')
        synchronize()
        return d_out.download((n + 1,), np.int64)


def scan_windows(samples, offsets, input_size, side, first_window=0, n_windows=None):
    """The scan's front alone (``dbh_scan_windows_dev``; parity tests): global windows
    [first_window, first_window + n_windows) of the packed reads, cut, normalised and padded ->
    float32 [n_windows, input_size].  ``n_windows`` None: up to the batch's last."""
    samples, offsets, n = _packed(samples, offsets)
    lib = load_library()
    window_offsets = host_window_offsets(input_size, offsets)
    if n_windows is None:
        n_windows = int(window_offsets[-1]) - int(first_window)
    x = np.zeros((int(n_windows), int(input_size)), dtype=np.float32)
    if n == 0 or n_windows == 0:
        return x
    with device_arrays(samples, offsets, window_offsets.nbytes, x.nbytes) as \
            (d_samples, d_offsets, d_window_offsets, d_x):
        check(lib.dbh_scan_window_offsets_dev(d_offsets.ptr, n, int(input_size),
                                              d_window_offsets.ptr, None),
              'dbh_scan_window_offsets_dev')
        check(lib.dbh_scan_windows_dev(d_samples.ptr, d_offsets.ptr, d_window_offsets.ptr, n,
                                       int(input_size), _side(side), int(first_window),
                                       int(n_windows), d_x.ptr, None), 'dbh_scan_windows_dev')
        synchronize()
        return d_x.download(x.shape, np.float32)


def scan_events(best, margin, window_offsets, threshold, min_windows=1, skip_windows=0,
                max_events=None):
    """The event pass alone (``dbh_scan_events_dev``): a track in global window order (``best``
    int32, ``margin`` float64) and the reads' window offsets -> (events SCAN_EVENT array - the
    first ``max_events`` of them; None: room for all - , the true total, interior events per read
    int32 [N])."""
    best = np.ascontiguousarray(best, dtype=np.int32)
    margin = np.ascontiguousarray(margin, dtype=np.float64)
    window_offsets = np.ascontiguousarray(window_offsets, dtype=np.int64)
    n = len(window_offsets) - 1
    if best.shape != margin.shape or best.ndim != 1 or (n >= 0 and len(best) != window_offsets[-1]):
        raise ValueError('best and margin must hold one entry per window')
    capacity = len(best) if max_events is None else int(max_events)
    with device_arrays(best, margin, window_offsets, max(capacity, 1) * SCAN_EVENT.itemsize,
                       max(n, 1) * 4, 8) as \
            (d_best, d_margin, d_window_offsets, d_events, d_interior, d_total):
        check(load_library().dbh_scan_events_dev(
            d_best.ptr, d_margin.ptr, d_window_offsets.ptr, n, float(threshold), int(min_windows),
            int(skip_windows), d_events.ptr, capacity, d_interior.ptr, d_total.ptr, None),
            'dbh_scan_events_dev')
        synchronize()
        total = int(d_total.download((1,), np.int64)[0])
        events = d_events.download((min(total, capacity),), SCAN_EVENT)
        return events, total, d_interior.download((max(n, 0),), np.int32)
