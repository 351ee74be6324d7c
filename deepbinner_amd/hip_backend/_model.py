"""``HipModel``, the object that stands where the reference has a Keras ``Model``, the classify
entries that take both models in one call, and the GPU inflate's host entry."""

import ctypes

import numpy as np

from .._cabi import Finalised, Owner
from ..model_format import ModelWeights
from ._abi import (COMBINE_MODES, KIND_GENERAL, MODEL_AUTO, MODEL_GENERAL, HipBackendError,
                   _handle, _packed, _ptr, _side, check, load_library)
from ._device import device_count, get_device, set_device
from ._locate import (evidence, locate_occluded_packed, locate_occluded_signals, locate_packed,
                      locate_signals)
from ._scan import SCAN_EVENT, host_window_offsets
from ._sweep import sweep_pair


def combine_calls_dev(start_calls_ptr, end_calls_ptr, n_reads, mode, out_ptr, stream=None):
    """combine_calls (classify.py:298-322) over device arrays of call numbers; ``mode`` is one of
    COMBINE_MODES.  Does not block."""
    check(load_library().dbh_combine_calls_dev(start_calls_ptr, end_calls_ptr, int(n_reads),
                                               COMBINE_MODES[mode], out_ptr, stream),
          'dbh_combine_calls_dev')


def classify_pair(start_model, end_model, samples, offsets, scan_size, score_diff,
                  mode='require_either', want_sides=False, want_probs=False):
    """One batch of packed reads (``samples`` int16, ``offsets`` int64: read i is
    ``samples[offsets[i]:offsets[i+1]]``, long reads possibly cut to their scanned ends) through
    the start and the end model in ONE call of the C ABI: one upload, both models' kernels, the
    min/max merges and ``combine_calls`` on the device -> final calls int32 [N] (0 = 'none').
    Either model may be None.  ``want_sides`` / ``want_probs``: also return the per-side calls /
    probabilities: (calls, (start_calls, end_calls), (start_probs, end_probs))."""
    lib = load_library()
    models = (start_model, end_model)
    if start_model is None and end_model is None:
        raise ValueError('no model')
    samples, offsets, n = _packed(samples, offsets)
    calls = np.empty(max(n, 0), dtype=np.int32)
    n_classes = next(m.n_classes for m in models if m is not None)
    side_calls = [np.empty(n, dtype=np.int32) if (want_sides and m is not None) else None
                  for m in models]
    side_probs = [np.empty((n, n_classes), dtype=np.float32) if (want_probs and m is not None)
                  else None for m in models]
    if n > 0:
        check(lib.dbh_classify_pair_i16(
            _handle(start_model), _handle(end_model),
            samples.ctypes.data if samples.size else None, offsets.ctypes.data, n, int(scan_size),
            float(score_diff), COMBINE_MODES[mode], calls.ctypes.data, _ptr(side_calls[0]),
            _ptr(side_calls[1]), _ptr(side_probs[0]), _ptr(side_probs[1])), 'dbh_classify_pair_i16')
    if want_sides or want_probs:
        return calls, tuple(side_calls), tuple(side_probs)
    return calls


INFLATE_ZLIB, INFLATE_STORED, INFLATE_VBZ = 0, 1, 2
# HDF5's shuffle filter (int16) undone on the GPU: u32 LE N, then a zlib stream of the N shuffled
# bytes / the N shuffled bytes themselves; the status of a stream these modes refuse
INFLATE_ZLIB_SHUFFLE, INFLATE_STORED_SHUFFLE = 4, 5
INFLATE_SHUFFLE_REFUSED = 32
# a row of a POD5 signal table: u32 LE 2n, then its svb16 stream / the zstd frame of it as stored
INFLATE_SVB16, INFLATE_SVB16_ZSTD = 6, 7
# dbh_inflate_stream (include/deepbinner_hip.h)
INFLATE_STREAM = np.dtype([('comp_offset', '<i8'), ('comp_bytes', '<i8'), ('out_offset', '<i8'),
                           ('out_bytes', '<i8'), ('mode', '<i4'), ('reserved', '<i4')])


def inflate(comp, streams, out_bytes, streams_per_lane=0):
    """zlib streams inflated on the GPU (``dbh_inflate``: host buffers in and out - tests and
    tools; the classify path keeps everything on the device).  ``comp``: uint8 array holding the
    streams, ``streams``: array of INFLATE_STREAM records, ``out_bytes``: size of the output
    buffer, ``streams_per_lane``: must be >= 0 and is otherwise ignored (it belonged to a retired
    form of kernel 1) -> (output uint8 array, status int32 per stream,
    milliseconds the two kernels took)."""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    streams = np.ascontiguousarray(streams, dtype=INFLATE_STREAM)
    out = np.zeros(int(out_bytes), dtype=np.uint8)
    status = np.zeros(len(streams), dtype=np.int32)
    ms = ctypes.c_double(0)
    check(load_library().dbh_inflate(comp.ctypes.data, comp.nbytes, streams.ctypes.data,
                                     len(streams), out.ctypes.data, out.nbytes, status.ctypes.data,
                                     int(streams_per_lane), ctypes.byref(ms)), 'dbh_inflate')
    return out, status, ms.value


def classify_pair_deflated(start_model, end_model, comp, streams, offsets, scan_size, score_diff,
                           mode='require_either', want_samples=False, want_stages=False,
                           want_sides=False):
    """A raw batch of the native loader (``fast5_native.stream_raw``: the reads' Signal chunks
    as stored) -> final calls int32 [N] and the decoder's status per stream, in ONE call of the C
    ABI: upload, inflate on the GPU, both models, ``combine_calls``.  ``comp`` must include its 64
    bytes of padding (``stream_raw``'s arrays do).  ``want_samples``: also the decoded signals
    (int16, all reads back to back); ``want_stages``: milliseconds of upload / inflate / classify
    on the device; ``want_sides``: also what the verbose table prints - a dict with the sides'
    own calls (``start_calls`` / ``end_calls``, int32 [N]) and merged probabilities
    (``start_probs`` / ``end_probs``, float32 [N, classes]); None for a side without a model."""
    lib = load_library()
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    streams = np.ascontiguousarray(streams)
    if streams.dtype.itemsize != INFLATE_STREAM.itemsize:
        raise ValueError('stream records of {} bytes'.format(streams.dtype.itemsize))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    calls = np.empty(max(n, 0), dtype=np.int32)
    status = np.zeros(len(streams), dtype=np.int32)
    samples = np.empty(int(offsets[-1]) if want_samples and n > 0 else 0, dtype=np.int16)
    stages = (ctypes.c_double * 3)()
    sides = {'start_calls': None, 'end_calls': None, 'start_probs': None, 'end_probs': None}
    if want_sides:
        for side, model in (('start', start_model), ('end', end_model)):
            if model is not None:
                sides[side + '_calls'] = np.zeros(max(n, 0), dtype=np.int32)
                sides[side + '_probs'] = np.zeros((max(n, 0), model.n_classes), dtype=np.float32)

    if n > 0:
        check(lib.dbh_classify_pair_deflated_verbose(
            _handle(start_model), _handle(end_model),
            comp.ctypes.data, max(comp.nbytes - 64, 0), streams.ctypes.data, len(streams),
            offsets.ctypes.data, n, int(scan_size), float(score_diff), COMBINE_MODES[mode],
            calls.ctypes.data, status.ctypes.data, samples.ctypes.data if want_samples else None,
            stages if want_stages else None, _ptr(sides['start_calls']), _ptr(sides['end_calls']),
            _ptr(sides['start_probs']), _ptr(sides['end_probs'])), 'dbh_classify_pair_deflated_verbose')
    out = [calls, status]
    if want_samples:
        out.append(samples)
    if want_stages:
        out.append(list(stages))
    if want_sides:
        out.append(sides)
    return tuple(out)


class _TensorSpec:
    """Minimal stand-in for the Keras tensors load_trained_model looks at (classify.py:93-97)."""

    def __init__(self, shape):
        self.shape = tuple(shape)


class HipModel(Owner, Finalised):
    """A trained Deepbinner model resident on one MI355X.  Models of the shipped geometry (input
    size 1024, at most 32 classes) run on the persistent forward kernel; any other supported
    geometry - or ``general=True`` - on the general path (``kind``: KIND_PERSISTENT / KIND_GENERAL)."""

    _release = 'dbh_model_destroy'

    def __init__(self, weights, device=None, general=False):
        if not isinstance(weights, ModelWeights):
            raise TypeError('weights must be a ModelWeights')
        self._lib = load_library()
        if device_count() < 1:
            raise HipBackendError('no HIP device is visible - Deepbinner-AMD needs an MI355X '
                                  '(gfx950) GPU; there is no CPU fallback')
        if device is not None:
            set_device(device)
        self.device = get_device()
        self.weights = weights
        flat = weights.flat()
        handle = ctypes.c_void_p()
        check(self._lib.dbh_model_create_ex(flat, flat.size, weights.n_classes, weights.input_size,
                                            MODEL_GENERAL if general else MODEL_AUTO,
                                            ctypes.byref(handle)), 'dbh_model_create_ex')
        self._handle = handle
        self.general = bool(general)
        kind = ctypes.c_int(0)
        check(self._lib.dbh_model_kind(handle, ctypes.byref(kind)), 'dbh_model_kind')
        self.kind = kind.value
        self.n_classes = weights.n_classes
        self.input_size = weights.input_size
        self.inputs = [_TensorSpec((None, self.input_size, 1))]
        self.outputs = [_TensorSpec((None, self.n_classes))]

    @property
    def handle(self):
        return self._handle

    def close(self):
        # further queues on the same GPU that realtime.queue_clones made of this model go with it
        for _pair, more in self.__dict__.pop('_queue_clones', []):
            for clones in more:
                for clone in clones:
                    if clone is not None and clone is not self:
                        clone.close()
        Owner.close(self)

    # -- seam b1 ------------------------------------------------------------------------------
    def predict(self, x, batch_size=None, verbose=0):
        """x: [N, L, 1] (or [N, L]) float -> float32 [N, n_classes], a fresh writable array.
        ``batch_size`` is accepted for signature compatibility; results do not depend on it."""
        x = np.asarray(x)
        if x.ndim == 3:
            if x.shape[2] != 1:
                raise ValueError('expected input of shape (N, {}, 1)'.format(self.input_size))
            x = x[:, :, 0]
        if x.ndim != 2 or x.shape[1] != self.input_size:
            raise ValueError('expected input of shape (N, {}, 1)'.format(self.input_size))
        x = np.ascontiguousarray(x, dtype=np.float32)      # Keras casts float64 -> float32 too
        probs = np.empty((x.shape[0], self.n_classes), dtype=np.float32)
        if x.shape[0]:
            check(self._lib.dbh_predict(self._handle, x, x.shape[0], probs), 'dbh_predict')
        return probs

    # -- seam b2 ------------------------------------------------------------------------------
    def classify_signals(self, signals, side, scan_size, score_diff):
        """signals: list of 1-D integer arrays -> (probs float32 [N, C], calls int32 [N])."""
        n = len(signals)
        keep = int(scan_size) + self.input_size // 2      # samples any window can touch
        parts = []
        offsets = np.zeros(n + 1, dtype=np.int64)
        for i, s in enumerate(signals):
            s = np.asarray(s)
            if s.ndim != 1:
                raise ValueError('signals must be one-dimensional')
            if s.dtype != np.int16 and len(s) and (s.min() < -32768 or s.max() > 32767):
                raise ValueError('signal values do not fit int16')
            # only the scanned end of the read is shipped to the GPU; window contents and
            # positions are unchanged by dropping samples no window reaches
            part = s[:keep] if side == 'start' else s[max(len(s) - keep, 0):]
            parts.append(np.asarray(part, dtype=np.int16))
            offsets[i + 1] = offsets[i] + len(part)
        samples = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)
        return self.classify_packed(samples, offsets, side, scan_size, score_diff)

    def classify_packed(self, samples, offsets, side, scan_size, score_diff):
        """``classify_signals`` for reads that are already packed the way the C ABI takes them:
        read i is ``samples[offsets[i]:offsets[i+1]]`` (int16, int64).  A long read may have had
        its middle dropped as long as the first and the last ``scan_size + input_size // 2``
        samples are there (what the loaders keep): no window reaches further."""
        samples, offsets, n = _packed(samples, offsets)
        if samples.size == 0:
            samples = np.zeros(1, dtype=np.int16)
        probs = np.empty((max(n, 0), self.n_classes), dtype=np.float32)
        calls = np.empty(max(n, 0), dtype=np.int32)
        if n > 0:
            check(self._lib.dbh_classify_i16(self._handle, samples, offsets, n, _side(side),
                                             int(scan_size), float(score_diff), probs, calls),
                  'dbh_classify_i16')
        return probs, calls

    def sweep_packed(self, samples, offsets, side, max_scan_size):
        """``classify_packed``'s reads through the window pass at ``max_scan_size`` and the fold
        over scan sizes -> (best int32 [N, K], margin float64 [N, K]): see ``sweep_pair``."""
        pair = sweep_pair(self if side == 'start' else None, None if side == 'start' else self,
                          samples, offsets, max_scan_size)
        return pair[0] if side == 'start' else pair[1]

    def scan_packed(self, samples, offsets, side, threshold, min_windows=1, skip_windows=0,
                    track=False):
        """EVERY window of the packed reads through the network (``dbh_scan_i16``) -> the events
        of the track as a SCAN_EVENT array ordered by (read, first): runs of at least
        ``min_windows`` consecutive windows of one read whose best class is one barcode leading
        by ``threshold``; an event is interior when ``first >= skip_windows``.  ``track=True``:
        (events, best int32, margin float64, window_offsets int64 [N + 1]) - the whole ragged
        track in global window order."""
        samples, offsets, n = _packed(samples, offsets)
        window_offsets = host_window_offsets(self.input_size, offsets)
        total = int(window_offsets[-1])
        events = np.zeros(total, dtype=SCAN_EVENT)          # (no more events than windows)
        best = np.zeros(total, dtype=np.int32) if track else None
        margin = np.zeros(total, dtype=np.float64) if track else None
        found, interior = ctypes.c_int64(0), ctypes.c_int64(0)
        if n > 0:
            check(self._lib.dbh_scan_i16(
                self._handle, samples.ctypes.data if samples.size else None, offsets.ctypes.data,
                n, _side(side), float(threshold), int(min_windows), int(skip_windows),
                _ptr(best), _ptr(margin), events.ctypes.data, total,
                ctypes.byref(found), ctypes.byref(interior)), 'dbh_scan_i16')
        events = events[:found.value]
        assert int((events['first'] >= skip_windows).sum()) == interior.value
        return (events, best, margin, window_offsets) if track else events

    # -- locate (general-kind models: _locate.py) ------------------------------------------------
    def evidence(self, windows):
        """windows [N, L] -> (probs [N, C], the bits of ``predict``; evidence [N, cells, C])."""
        return evidence(self, windows)

    def locate_signals(self, signals, side, scan_size, score_diff):
        """Whole reads -> (probs [N, C], calls [N], locations LOCATION [N])."""
        return locate_signals(self, signals, side, scan_size, score_diff)

    def locate_packed(self, samples, offsets, side, scan_size, score_diff):
        """``locate_signals`` for whole reads already packed."""
        return locate_packed(self, samples, offsets, side, scan_size, score_diff)

    def locate_occluded_signals(self, signals, side, scan_size, score_diff):
        """Whole reads -> (probs, calls, locations as ``locate_signals``, occlusions OCCLUSION [N])."""
        return locate_occluded_signals(self, signals, side, scan_size, score_diff)

    def locate_occluded_packed(self, samples, offsets, side, scan_size, score_diff):
        """``locate_occluded_signals`` for whole reads already packed."""
        return locate_occluded_packed(self, samples, offsets, side, scan_size, score_diff)

    # -- device-resident entry points (inputs/outputs are raw device pointers) -----------------
    def workspace_bytes(self, n_reads, scan_size):
        n = ctypes.c_size_t(0)
        check(self._lib.dbh_classify_workspace_bytes(self._handle, n_reads, int(scan_size),
                                                     ctypes.byref(n)),
              'dbh_classify_workspace_bytes')
        return n.value

    def classify_dev(self, samples_ptr, offsets_ptr, n_reads, side, scan_size, score_diff,
                     probs_ptr, calls_ptr, workspace_ptr, stream=None):
        check(self._lib.dbh_classify_i16_dev(self._handle, samples_ptr, offsets_ptr, n_reads,
                                             _side(side), int(scan_size), float(score_diff),
                                             probs_ptr, calls_ptr, workspace_ptr, stream),
              'dbh_classify_i16_dev')

    def classify_batched_dev(self, samples_ptr, offsets_ptr, n_reads, batch_size, side, scan_size,
                             score_diff, probs_ptr, calls_ptr, stream=None):
        check(self._lib.dbh_classify_i16_batched_dev(
            self._handle, samples_ptr, offsets_ptr, n_reads, int(batch_size), _side(side),
            int(scan_size), float(score_diff), probs_ptr, calls_ptr, stream),
            'dbh_classify_i16_batched_dev')

    def predict_dev(self, x_ptr, n_windows, probs_ptr, stream=None):
        check(self._lib.dbh_predict_dev(self._handle, x_ptr, n_windows, probs_ptr, stream),
              'dbh_predict_dev')

    def forward_truncated_dev(self, x_ptr, n_windows, last_stage, stream=None):
        check(self._lib.dbh_forward_truncated_dev(self._handle, x_ptr, n_windows, last_stage,
                                                  stream), 'dbh_forward_truncated_dev')

    def timeline(self, x):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, self.input_size))
        out = np.zeros((x.shape[0], 8, 64), dtype=np.int64)
        check(self._lib.dbh_forward_timeline(self._handle, x, x.shape[0], out),
              'dbh_forward_timeline')
        return out

    def set_host_group(self, windows_per_group=0):
        """Windows per model and group of the host-buffer pipeline (0 = the default 32,768)."""
        check(self._lib.dbh_model_set_host_group(self._handle, int(windows_per_group)),
              'dbh_model_set_host_group')

    def reserve_cus(self, n_cus=0):
        """Leave ``n_cus`` CUs out of this model's forward launches (0 = take all again): room
        for the inflate kernels of the containers that follow on other queues."""
        check(self._lib.dbh_model_reserve_cus(self._handle, int(n_cus)), 'dbh_model_reserve_cus')

    def clone(self):
        """The same weights as another model on the same GPU: its own streams and buffers - one
        more queue."""
        return HipModel(self.weights, device=self.device, general=self.general)

    def set_read_length_hint(self, read_length, capacity_samples=0):
        """Tell the ``*_dev`` entry points that every read is ``read_length`` samples long (0
        clears it); the hint is checked on the device, a wrong one only costs time."""
        check(self._lib.dbh_model_set_read_length_hint(self._handle, int(read_length),
                                                       int(capacity_samples)),
              'dbh_model_set_read_length_hint')

    def timeline_i16(self, reads):
        reads = np.ascontiguousarray(np.asarray(reads, dtype=np.int16).reshape(-1, self.input_size))
        out = np.zeros((reads.shape[0], 8, 64), dtype=np.int64)
        check(self._lib.dbh_forward_timeline_i16(self._handle, reads, reads.shape[0], out),
              'dbh_forward_timeline_i16')
        return out

    def timing_enable(self, every_nth=1, span=1):
        """Bracket a run of ``span`` consecutive forward launches with one HIP event pair at
        every n-th launch (0/False = off, True = every launch on its own)."""
        check(self._lib.dbh_forward_timing_enable_span(self._handle, int(every_nth), int(span)),
              'dbh_forward_timing_enable_span')

    def clock_enable(self, on=True):
        """Have production launches of the forward kernel note the shader clock against the wall
        clock (see dbh_forward_clock_enable)."""
        check(self._lib.dbh_forward_clock_enable(self._handle, 1 if on else 0),
              'dbh_forward_clock_enable')

    def phases_enable(self, on=True):
        """Have production launches keep the phase stamps as well (on top of clock_enable): about 1 % of
        the kernel's time, so not for timed runs."""
        check(self._lib.dbh_forward_phases_enable(self._handle, 1 if on else 0), 'dbh_forward_phases_enable')

    def phases_read(self):
        """Mean shader cycles of the five phases of a group of windows in this model's latest forward
        launch (see dbh_forward_phases_read): stages A-C, the stage D-E chain, stage F, the batched
        tail, what lies between two groups; and the number of groups averaged."""
        count = ctypes.c_int(0)
        check(self._lib.dbh_forward_phases_count(ctypes.byref(count)), 'dbh_forward_phases_count')
        out = (ctypes.c_double * count.value)()
        n = ctypes.c_int64(0)
        check(self._lib.dbh_forward_phases_read(self._handle, out, ctypes.byref(n)), 'dbh_forward_phases_read')
        return [float(v) for v in out], int(n.value)

    def clock_read(self):
        """Shader clock (GHz) during this model's latest forward launch."""
        ghz = ctypes.c_double(0)
        check(self._lib.dbh_forward_clock_read(self._handle, ctypes.byref(ghz)),
              'dbh_forward_clock_read')
        return ghz.value

    def timing_read(self):
        ms, launches, windows = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._lib.dbh_forward_timing_read(self._handle, ctypes.byref(ms),
                                                ctypes.byref(launches), ctypes.byref(windows)),
              'dbh_forward_timing_read')
        return ms.value, launches.value, windows.value

    # -- introspection ------------------------------------------------------------------------
    def debug_stage(self, x, stage):
        """Activations after stage 'A'..'G' (or 'logits') for windows x [N, 1024]."""
        idx = {'A': 0, 'B': 1, 'C': 2, 'D': 3, 'E': 4, 'F': 5, 'G': 6, 'logits': 7}[stage]
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, self.input_size))
        per = ctypes.c_int64(0)
        check(self._lib.dbh_stage_floats(idx, ctypes.byref(per)), 'dbh_stage_floats')
        out = np.empty((x.shape[0], per.value), dtype=np.float32)
        check(self._lib.dbh_debug_forward(self._handle, x, x.shape[0], idx, out),
              'dbh_debug_forward')
        shapes = {0: (512, 48), 1: (256, 48), 2: (128, 48), 3: (64, 48), 4: (32, 192),
                  5: (16, 48), 6: (8, 48), 7: (32,)}
        return out.reshape((x.shape[0],) + shapes[idx])


def general_model(model):
    """The model ``locate`` needs from the one ``classify.build_model`` made: general-kind, whatever
    the geometry.  A persistent-kind model is closed and its weights loaded again on the general
    path; a general-kind one comes back as it is."""
    if model is None or model.kind == KIND_GENERAL:
        return model
    general = HipModel(model.weights, device=model.device, general=True)
    model.close()
    return general


def forward_executed_mfmas(n_classes):
    """(MFMA instructions, FLOP) the forward kernel issues per window."""
    n, f = ctypes.c_int64(0), ctypes.c_int64(0)
    check(load_library().dbh_forward_executed_mfmas(int(n_classes), ctypes.byref(n),
                                                    ctypes.byref(f)), 'dbh_forward_executed_mfmas')
    return n.value, f.value


def forward_kernel_info():
    t, l, v = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(load_library().dbh_forward_kernel_info(ctypes.byref(t), ctypes.byref(l),
                                                 ctypes.byref(v)), 'dbh_forward_kernel_info')
    return {'threads_per_block': t.value, 'lds_bytes': l.value, 'vgprs': v.value}
