"""``locate``: where in the signal a barcode call comes from (include/deepbinner_hip.h, "locate").
The evidence of a window - the post-ReLU ``conv1d_20`` output per cell of 128 samples, whose mean is
the logit - the rule that turns a read's evidence and call into a location, on the device and on the
host, and the whole route.  ``HipModel.evidence`` / ``locate_signals`` / ``locate_packed`` are these
functions with the model in front.  ``--occlude`` ("occlude" in the same header): the plan that
turns a location into three sets of blanked samples, the blanked windows, and the route that calls
every read again under each."""

import ctypes

import numpy as np

from ._abi import KIND_GENERAL, HipBackendError, _packed, _side, check, load_library
from ._device import device_arrays, synchronize

# dbh_location (include/deepbinner_hip.h, "locate"): samples are [first_sample, end_sample)
LOCATION = np.dtype([('cls', np.int32), ('window', np.int32), ('peak_cell', np.int32),
                     ('first_cell', np.int32), ('last_cell', np.int32), ('peak', np.float32),
                     ('share', np.float32), ('reserved', np.int32), ('first_sample', np.int64),
                     ('end_sample', np.int64)])
assert LOCATION.itemsize == 48
CELL_SAMPLES = 128
# dbh_occlude_plan and dbh_occlusion (include/deepbinner_hip.h, "occlude"); the variants in the
# order OUT, ONLY, CTRL
VARIANTS = ('out', 'only', 'ctrl')
OCCLUDE_PLAN = np.dtype([('first', np.int64, 3), ('end', np.int64, 3), ('invert', np.int32),
                         ('valid', np.int32), ('reserved', np.int64)])
OCCLUSION = np.dtype([('cls', np.int32), ('p', np.float32)] +
                     [(v + field, kind) for v in VARIANTS
                      for field, kind in (('_call', np.int32), ('_p', np.float32))] +
                     [('ctrl_first', np.int64), ('ctrl_end', np.int64), ('reserved', np.int64, 2)])
assert OCCLUDE_PLAN.itemsize == 64 and OCCLUSION.itemsize == 64


def _general(model, what):
    if model.kind != KIND_GENERAL:
        raise HipBackendError('{} needs a general-kind model: HipModel(weights, general=True)'
                              .format(what))


def evidence_floats(model):
    """cells * classes: the evidence floats of one window (``dbh_evidence_floats``)."""
    per = ctypes.c_int64(0)
    check(load_library().dbh_evidence_floats(model.handle, ctypes.byref(per)), 'dbh_evidence_floats')
    return per.value


def evidence(model, windows):
    """windows [N, L] (or [N, L, 1]) float -> (probs float32 [N, C] - the bits of ``model.predict``
    - , evidence float32 [N, cells, C]) (``dbh_evidence_dev``)."""
    _general(model, 'evidence')
    x = np.asarray(windows)
    if x.ndim == 3 and x.shape[2] == 1:
        x = x[:, :, 0]
    if x.ndim != 2 or x.shape[1] != model.input_size:
        raise ValueError('expected input of shape (N, {}, 1)'.format(model.input_size))
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, per = x.shape[0], evidence_floats(model)
    cells = per // model.n_classes
    if n == 0:
        return (np.empty((0, model.n_classes), np.float32),
                np.empty((0, cells, model.n_classes), np.float32))
    with device_arrays(x, n * model.n_classes * 4, n * per * 4) as (d_x, d_probs, d_evidence):
        check(load_library().dbh_evidence_dev(model.handle, d_x.ptr, n, d_probs.ptr, d_evidence.ptr,
                                              None), 'dbh_evidence_dev')
        synchronize()
        return (d_probs.download((n, model.n_classes), np.float32),
                d_evidence.download((n, cells, model.n_classes), np.float32))


def _rule_arguments(evidence, calls, lengths):
    evidence = np.ascontiguousarray(evidence, dtype=np.float32)
    calls = np.ascontiguousarray(calls, dtype=np.int32)
    lengths = np.asarray(lengths, dtype=np.int64)
    if evidence.ndim != 4 or calls.shape != evidence.shape[:1] or lengths.shape != calls.shape:
        raise ValueError('evidence must be [reads, steps, cells, classes], with one call and one '
                         'length per read')
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return evidence, calls, offsets


def locate_rule(evidence, calls, lengths, input_size, side):
    """The rule on the host (``dbh_locate_host``, the CPU model of the kernel): evidence float32
    [N, steps, cells, C], the side's calls int32 [N] and the reads' lengths [N] -> LOCATION [N]."""
    evidence, calls, offsets = _rule_arguments(evidence, calls, lengths)
    n, steps, cells, n_classes = evidence.shape
    out = np.zeros(n, dtype=LOCATION)
    check(load_library().dbh_locate_host(evidence.ctypes.data, calls.ctypes.data, offsets.ctypes.data,
                                         n, steps, cells, n_classes, int(input_size), _side(side),
                                         out.ctypes.data), 'dbh_locate_host')
    return out


def locate_rule_dev(evidence, calls, lengths, input_size, side):
    """The same arrays through the kernel (``dbh_locate_dev``; parity tests)."""
    evidence, calls, offsets = _rule_arguments(evidence, calls, lengths)
    n, steps, cells, n_classes = evidence.shape
    if n == 0:
        return np.zeros(0, dtype=LOCATION)
    with device_arrays(evidence, calls, offsets, n * LOCATION.itemsize) as \
            (d_evidence, d_calls, d_offsets, d_out):
        check(load_library().dbh_locate_dev(d_evidence.ptr, d_calls.ptr, d_offsets.ptr, n, steps,
                                            cells, n_classes, int(input_size), _side(side),
                                            d_out.ptr, None), 'dbh_locate_dev')
        synchronize()
        return d_out.download((n,), LOCATION)


def locate_workspace_bytes(model, n_reads, scan_size):
    n = ctypes.c_size_t(0)
    check(load_library().dbh_locate_workspace_bytes(model.handle, int(n_reads), int(scan_size),
                                                    ctypes.byref(n)), 'dbh_locate_workspace_bytes')
    return n.value


def locate_packed(model, samples, offsets, side, scan_size, score_diff):
    """Packed WHOLE reads (read i is ``samples[offsets[i]:offsets[i+1]]``: end-side positions need
    the true length) through the whole route (``dbh_locate_i16``) -> (probs float32 [N, C], calls
    int32 [N] - what ``classify_packed`` gives on this model - , locations LOCATION [N])."""
    _general(model, 'locate')
    samples, offsets, n = _packed(samples, offsets)
    probs = np.zeros((max(n, 0), model.n_classes), dtype=np.float32)
    calls = np.zeros(max(n, 0), dtype=np.int32)
    locations = np.zeros(max(n, 0), dtype=LOCATION)
    if n > 0:
        check(load_library().dbh_locate_i16(
            model.handle, samples.ctypes.data if samples.size else None, offsets.ctypes.data, n,
            _side(side), int(scan_size), float(score_diff), probs.ctypes.data, calls.ctypes.data,
            locations.ctypes.data), 'dbh_locate_i16')
    return probs, calls, locations


def locate_signals(model, signals, side, scan_size, score_diff):
    """``locate_packed`` for a list of 1-D int16 signals, kept whole."""
    parts = [np.asarray(s, dtype=np.int16) for s in signals]
    if any(p.ndim != 1 for p in parts):
        raise ValueError('signals must be one-dimensional')
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    samples = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)
    return locate_packed(model, samples, offsets, side, scan_size, score_diff)


def _offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def occlude_plan(locations, lengths, steps, input_size, side, device=False):
    """LOCATION [N] and the reads' lengths [N] -> (OCCLUDE_PLAN [N], OCCLUSION [N] with cls, the
    control samples and the "no result" fields) on the host (``dbh_occlude_plan_host``, the CPU
    model) or, ``device=True``, through the kernel (``dbh_occlude_plan_dev``)."""
    locations = np.ascontiguousarray(locations, dtype=LOCATION)
    offsets = _offsets_of(lengths)
    n = len(locations)
    if locations.ndim != 1 or len(offsets) != n + 1:
        raise ValueError('one location and one length per read')
    plans, occlusions = np.zeros(n, dtype=OCCLUDE_PLAN), np.zeros(n, dtype=OCCLUSION)
    lib = load_library()
    if not device:
        check(lib.dbh_occlude_plan_host(locations.ctypes.data, offsets.ctypes.data, n, int(steps),
                                        int(input_size), _side(side), plans.ctypes.data,
                                        occlusions.ctypes.data), 'dbh_occlude_plan_host')
        return plans, occlusions
    if n == 0:
        return plans, occlusions
    with device_arrays(locations, offsets, n * 64, n * 64) as (d_loc, d_offsets, d_plans, d_occ):
        check(lib.dbh_occlude_plan_dev(d_loc.ptr, d_offsets.ptr, n, int(steps), int(input_size),
                                       _side(side), d_plans.ptr, d_occ.ptr, None),
              'dbh_occlude_plan_dev')
        synchronize()
        return d_plans.download((n,), OCCLUDE_PLAN), d_occ.download((n,), OCCLUSION)


def occlude_windows(x, lengths, plans, side, device=False):
    """x float32 [N, steps, L] normalised windows, the reads' lengths [N] and OCCLUDE_PLAN [N] ->
    float32 [3, N, steps, L], the windows of OUT, ONLY and CTRL (``dbh_occlude_windows_host``, or
    ``dbh_occlude_windows_dev`` with ``device=True``)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    plans = np.ascontiguousarray(plans, dtype=OCCLUDE_PLAN)
    offsets = _offsets_of(lengths)
    if x.ndim != 3 or plans.shape != x.shape[:1] or len(offsets) != len(plans) + 1:
        raise ValueError('x must be [reads, steps, L], with one plan and one length per read')
    n, steps, input_size = x.shape
    out = np.zeros((3,) + x.shape, dtype=np.float32)
    lib = load_library()
    if not device:
        check(lib.dbh_occlude_windows_host(x.ctypes.data, offsets.ctypes.data, plans.ctypes.data, n,
                                           steps, input_size, _side(side), out.ctypes.data),
              'dbh_occlude_windows_host')
        return out
    if out.size == 0:
        return out
    with device_arrays(x, offsets, plans, out.nbytes) as (d_x, d_offsets, d_plans, d_out):
        check(lib.dbh_occlude_windows_dev(d_x.ptr, d_offsets.ptr, d_plans.ptr, n, steps, input_size,
                                          _side(side), d_out.ptr, None), 'dbh_occlude_windows_dev')
        synchronize()
        return d_out.download(out.shape, np.float32)


def locate_occluded_workspace_bytes(model, n_reads, scan_size):
    n = ctypes.c_size_t(0)
    check(load_library().dbh_locate_occluded_workspace_bytes(
        model.handle, int(n_reads), int(scan_size), ctypes.byref(n)),
        'dbh_locate_occluded_workspace_bytes')
    return n.value


def locate_occluded_packed(model, samples, offsets, side, scan_size, score_diff):
    """``locate_packed`` with every read called again under the three variants
    (``dbh_locate_occluded_i16``) -> (probs, calls, locations - the bits of ``locate_packed`` - ,
    occlusions OCCLUSION [N])."""
    _general(model, 'locate')
    samples, offsets, n = _packed(samples, offsets)
    probs = np.zeros((max(n, 0), model.n_classes), dtype=np.float32)
    calls = np.zeros(max(n, 0), dtype=np.int32)
    locations = np.zeros(max(n, 0), dtype=LOCATION)
    occlusions = np.zeros(max(n, 0), dtype=OCCLUSION)
    if n > 0:
        check(load_library().dbh_locate_occluded_i16(
            model.handle, samples.ctypes.data if samples.size else None, offsets.ctypes.data, n,
            _side(side), int(scan_size), float(score_diff), probs.ctypes.data, calls.ctypes.data,
            locations.ctypes.data, occlusions.ctypes.data), 'dbh_locate_occluded_i16')
    return probs, calls, locations, occlusions


def locate_occluded_signals(model, signals, side, scan_size, score_diff):
    """``locate_occluded_packed`` for a list of 1-D int16 signals, kept whole."""
    parts = [np.asarray(s, dtype=np.int16) for s in signals]
    if any(p.ndim != 1 for p in parts):
        raise ValueError('signals must be one-dimensional')
    samples = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)
    return locate_occluded_packed(model, samples, _offsets_of([len(p) for p in parts]), side,
                                  scan_size, score_diff)
