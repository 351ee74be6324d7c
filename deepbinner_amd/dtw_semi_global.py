"""
Semi-global dynamic time warping on the GPU: the host side of ``libdeepbinner_dtw.so`` (C ABI
``include/deepbinner_dtw.h``, kernel ``csrc/dtw_kernel.hip``), with the call surface of the
reference's ``deepbinner/dtw_semi_global.py``:

  ``semi_global_dtw(ref, query)``                  (:44-59)  one alignment
  ``semi_global_dtw_with_rescaling(ref, query)``   (:62-95)  two passes with a linear re-fit of the
                                                             query in between

and, new, the batched forms that give the device something to do - ``semi_global_dtw_batch`` and
``semi_global_dtw_with_rescaling_batch`` take lists of signals and run every pair of a pass in one
launch.  Results per pair are exactly those of the one-pair functions.

``semi_global_dtw_with_rescaling_batch(..., resident=True)`` and ``rescaled_batch`` keep both passes
and the fit between them on the device (``dtw_rescaled_batch``), by the contract written in
``include/deepbinner_dtw.h``: normal equations with a fixed summation order in place of ``lstsq``.
``locate_batch`` is the binding of ``dtw_locate_batch``, which ``prep_signal`` builds on.

There is no CPU fallback: without the library or without a gfx950 device the calls raise.
"""

import ctypes
import os

import numpy as np
from numpy.ctypeslib import ndpointer

from . import _cabi

LIB_NAME = 'libdeepbinner_dtw.so'
_lib = None


def _signatures():
    c_int, c_i64, c_double, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    i16, i32, i64, f64 = (ndpointer(t, flags='C_CONTIGUOUS') for t in
                          (ctypes.c_int16, ctypes.c_int32, ctypes.c_int64, ctypes.c_double))
    return {
        'dtw_version': (ctypes.c_char_p, []),
        'dtw_status_string': (ctypes.c_char_p, [c_int]),
        'dtw_last_error': (ctypes.c_char_p, []),
        # exactly the reference's binding (dtw_semi_global.py:33-41)
        'semi_global_dtw': (c_double, [f64, f64, c_int, c_int, i32, i32, i32]),
        'dtw_semi_global_batch': (c_int, [f64, i64, f64, i64, c_i64, f64, i32, i32, c_void_p]),
        'dtw_rescaled_batch': (c_int, [f64, i64, f64, i64, c_i64, f64, i32, f64, c_void_p,
                                       c_void_p, c_void_p]),
        'dtw_locate_batch': (c_int, [i16, i64, f64, c_i64, f64, i64, c_i64, i64, c_i64, i64, c_i64,
                                     c_double, f64, i32, f64, i32]),
        'dtw_last_kernel_time': (c_int, [ctypes.POINTER(c_double), ctypes.POINTER(c_i64)]),
    }


# The ABI, once: {name: (restype, argtypes)}.  tests/test_dtw.py holds its names to the header.
SIGNATURES = _signatures()
EXPORTED_SYMBOLS = list(SIGNATURES)


def library_path():
    return os.environ.get('DEEPBINNER_DTW_LIB') or os.path.join(
        os.path.dirname(os.path.abspath(__file__)), LIB_NAME)


def available():
    return os.path.isfile(library_path())


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.isfile(path):
        raise RuntimeError('{} is not built (run `make -C deepbinner_amd/csrc`): the DTW has no '
                           'CPU fallback'.format(path))
    _lib = _cabi.bind(path, SIGNATURES)
    return _lib


def _failed(lib, what, status=None):
    text = lib.dtw_last_error().decode()
    if status is not None:
        text = '{} ({})'.format(lib.dtw_status_string(status).decode(), text)
    raise RuntimeError('{} failed: {}'.format(what, text))


def semi_global_dtw(ref, query):
    """(distance, ref_start, ref_end, [(ref_index, query_index), ...]) - the pairs from the start
    of the alignment to its end, as the reference returns them (:52-59)."""
    lib = load_library()
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    query = np.ascontiguousarray(query, dtype=np.float64)
    alignment = np.empty((len(ref) + len(query)) * 2, dtype=np.int32)
    positions = np.empty(2, dtype=np.int32)
    path_length = np.zeros(1, dtype=np.int32)
    distance = lib.semi_global_dtw(ref, query, len(ref), len(query), alignment, positions,
                                   path_length)
    if path_length[0] == 0:
        _failed(lib, 'semi_global_dtw')
    pairs = alignment[:2 * int(path_length[0])].reshape(-1, 2)[::-1]
    return distance, positions[0], positions[1], [(a, b) for a, b in pairs]


def _pack(signals):
    arrays = [np.ascontiguousarray(s, dtype=np.float64).ravel() for s in signals]
    offsets = np.zeros(len(arrays) + 1, dtype=np.int64)
    np.cumsum([len(a) for a in arrays], out=offsets[1:])
    flat = np.concatenate(arrays) if arrays else np.zeros(0, dtype=np.float64)
    return np.ascontiguousarray(flat), offsets


def semi_global_dtw_batch(refs, queries, alignments=True):
    """One launch for all pairs (refs[k], queries[k]).  Returns a list of
    ``(distance, ref_start, ref_end, pairs)`` with ``pairs`` an ``int32[n, 2]`` array of
    (ref_index, query_index) from start to end, or ``None`` when ``alignments`` is false."""
    if len(refs) != len(queries):
        raise ValueError('as many queries as references, please')
    lib = load_library()
    n = len(refs)
    if n == 0:
        return []
    flat_refs, ref_offsets = _pack(refs)
    flat_queries, query_offsets = _pack(queries)
    distances = np.empty(n, dtype=np.float64)
    positions = np.empty(2 * n, dtype=np.int32)
    lengths = np.empty(n, dtype=np.int32)
    alignment = np.empty(2 * int(ref_offsets[-1] + query_offsets[-1]), dtype=np.int32) \
        if alignments else None
    status = lib.dtw_semi_global_batch(
        flat_refs, ref_offsets, flat_queries, query_offsets, n, distances, positions, lengths,
        alignment.ctypes.data if alignments else None)
    if status != 0:
        _failed(lib, 'dtw_semi_global_batch', status)
    results = []
    for k in range(n):
        pairs = None
        if alignments:
            at = 2 * int(ref_offsets[k] + query_offsets[k])
            pairs = alignment[at:at + 2 * int(lengths[k])].reshape(-1, 2)[::-1]
        results.append((float(distances[k]), int(positions[2 * k]), int(positions[2 * k + 1]),
                        pairs))
    return results


def last_kernel_time():
    """(milliseconds, cells) of the kernels of the last call."""
    lib = load_library()
    ms, cells = ctypes.c_double(0.0), ctypes.c_int64(0)
    lib.dtw_last_kernel_time(ctypes.byref(ms), ctypes.byref(cells))
    return ms.value, cells.value


ITERATIONS = 2                       # reference :70
SLOPE_RANGE = (0.75, 1.333)          # reference :91-93


def _refit(ref, query, pairs):
    """Least-squares line through (query value, reference value) over the aligned pairs; the
    query moved onto it (reference :81-89)."""
    x = query[pairs[:, 1]]
    y = ref[pairs[:, 0]]
    design = np.vstack([x, np.ones(len(x))]).T
    slope, intercept = np.linalg.lstsq(design, y, rcond=None)[0]
    return slope * query + intercept, slope


def rescaled_batch(refs, queries, alignments=True):
    """The rescaled DTW of every pair (refs[k], queries[k]) with both passes and the fit between
    them on the device (``dtw_rescaled_batch``).  Returns a list of
    ``(distance, ref_start, ref_end, slope, pairs, rescaled_query)``: ``pairs`` as
    ``semi_global_dtw_batch`` gives them, of pass 2, or ``None`` when ``alignments`` is false."""
    if len(refs) != len(queries):
        raise ValueError('as many queries as references, please')
    lib = load_library()
    n = len(refs)
    if n == 0:
        return []
    flat_refs, ref_offsets = _pack(refs)
    flat_queries, query_offsets = _pack(queries)
    distances = np.empty(n, dtype=np.float64)
    positions = np.empty(2 * n, dtype=np.int32)
    slopes = np.empty(n, dtype=np.float64)
    rescaled = np.empty(len(flat_queries), dtype=np.float64)
    lengths = np.empty(n, dtype=np.int32)
    alignment = np.empty(2 * int(ref_offsets[-1] + query_offsets[-1]), dtype=np.int32) \
        if alignments else None
    status = lib.dtw_rescaled_batch(
        flat_refs, ref_offsets, flat_queries, query_offsets, n, distances, positions, slopes,
        rescaled.ctypes.data, lengths.ctypes.data, alignment.ctypes.data if alignments else None)
    if status != 0:
        _failed(lib, 'dtw_rescaled_batch', status)
    results = []
    for k in range(n):
        pairs = None
        if alignments:
            at = 2 * int(ref_offsets[k] + query_offsets[k])
            pairs = alignment[at:at + 2 * int(lengths[k])].reshape(-1, 2)[::-1]
        results.append((float(distances[k]), int(positions[2 * k]), int(positions[2 * k + 1]),
                        float(slopes[k]), pairs,
                        rescaled[int(query_offsets[k]):int(query_offsets[k + 1])]))
    return results


def locate_batch(samples, region_offsets, mean_std, queries, query_offsets, jobs, group_offsets,
                 threshold):
    """``dtw_locate_batch`` as the header has it: int16 regions of reads, (mean, std) per read,
    a table of query signals, jobs (read, from, to, query) in groups.  Returns
    ``(distances, positions[n_jobs, 2], slopes, hits)`` as arrays."""
    lib = load_library()
    samples = np.ascontiguousarray(samples, dtype=np.int16)
    region_offsets = np.ascontiguousarray(region_offsets, dtype=np.int64)
    mean_std = np.ascontiguousarray(mean_std, dtype=np.float64).reshape(-1)
    queries = np.ascontiguousarray(queries, dtype=np.float64)
    query_offsets = np.ascontiguousarray(query_offsets, dtype=np.int64)
    jobs = np.ascontiguousarray(jobs, dtype=np.int64).reshape(-1)
    group_offsets = np.ascontiguousarray(group_offsets, dtype=np.int64)
    n_reads, n_queries = len(region_offsets) - 1, len(query_offsets) - 1
    n_jobs, n_groups = len(jobs) // 4, len(group_offsets) - 1
    if n_reads < 0 or n_queries < 0 or n_groups < 0 or len(jobs) % 4 or \
            len(mean_std) != 2 * max(n_reads, 0):
        raise ValueError('offset arrays have one entry more than there are reads, queries and '
                         'groups; four numbers per job and two per read, please')
    distances = np.empty(n_jobs, dtype=np.float64)
    positions = np.empty(2 * n_jobs, dtype=np.int32)
    slopes = np.empty(n_jobs, dtype=np.float64)
    hits = np.empty(n_groups, dtype=np.int32)
    status = lib.dtw_locate_batch(samples, region_offsets, mean_std, n_reads, queries,
                                  query_offsets, n_queries, jobs, n_jobs, group_offsets, n_groups,
                                  float(threshold), distances, positions, slopes, hits)
    if status != 0:
        _failed(lib, 'dtw_locate_batch', status)
    return distances, positions.reshape(-1, 2), slopes, hits


def semi_global_dtw_with_rescaling_batch(refs, queries, resident=False):
    """``semi_global_dtw_with_rescaling`` for many pairs: each of the two passes is one launch.
    Returns a list of ``(distance, ref_start, ref_end, [(ref value, query value), ...])``.
    ``resident=True``: both passes and the fit stay on the device (``rescaled_batch``); the fit is
    then the header's normal equations, not ``lstsq``, and a constant query gives inf."""
    if resident:
        refs = [np.ascontiguousarray(r, dtype=np.float64) for r in refs]
        return [(distance, start, end, list(zip(refs[k][pairs[:, 0]], rescaled[pairs[:, 1]])))
                for k, (distance, start, end, _, pairs, rescaled)
                in enumerate(rescaled_batch(refs, queries))]
    refs = [np.ascontiguousarray(r, dtype=np.float64) for r in refs]
    queries = [np.array(q, dtype=np.float64) for q in queries]
    slopes = [1.0] * len(refs)
    results = []
    for iteration in range(ITERATIONS):
        results = semi_global_dtw_batch(refs, queries)
        if iteration == ITERATIONS - 1:
            break
        for k, (_, _, _, pairs) in enumerate(results):
            queries[k], slope = _refit(refs[k], queries[k], pairs)
            slopes[k] *= slope
    out = []
    for k, (distance, start, end, pairs) in enumerate(results):
        if slopes[k] < SLOPE_RANGE[0] or slopes[k] > SLOPE_RANGE[1]:
            distance = float('inf')
        values = list(zip(refs[k][pairs[:, 0]], queries[k][pairs[:, 1]]))
        out.append((distance, start, end, values))
    return out


def semi_global_dtw_with_rescaling(ref, query, resident=False):
    """Reference :62-95 (after https://arxiv.org/abs/1705.01620): align, fit the query to the
    reference over the aligned pairs, align again; a total slope outside 0.75 .. 1.333 means the
    fit went wrong and the distance becomes inf."""
    return semi_global_dtw_with_rescaling_batch([ref], [query], resident=resident)[0]
