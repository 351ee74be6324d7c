"""Training-data text on the device: the parser of blocks of lines (include/deepbinner_hip.h,
"training-data text"), and random signals and the formatter that writes
such text.  Reading a whole file is ``_training_file``'s."""

import ctypes

import numpy as np

from .._cabi import Owner, Scoped
from ._abi import _seed64, check, load_library
from ._device import DeviceBuffer, Event, Stream

TEXT_OK, TEXT_FORM, TEXT_COUNT, TEXT_RANGE = 0, 1, 2, 3


def _parse_text_block(entry, data, input_size, max_lines):
    lib = load_library()
    text, input_size = np.frombuffer(data, dtype=np.uint8), int(input_size)    # no copy
    own_bound = max_lines is None
    if own_bound:
        # 2 * input_size + 2 bytes: the shortest line that can be TEXT_OK
        max_lines = text.size // (2 * max(input_size, 1) + 2) + 1
    n_lines, first_bad = ctypes.c_int64(0), ctypes.c_int64(-1)
    for attempt in range(2):
        samples = np.empty((max_lines, max(input_size, 0)), dtype=np.int16)
        labels = np.empty(max_lines, dtype=np.int32)
        kinds = np.empty(max_lines, dtype=np.uint8)
        status = getattr(lib, entry)(text.ctypes.data if text.size else None, text.size, input_size,
                                     max_lines, samples.ctypes.data,
                                     labels.ctypes.data, kinds.ctypes.data, ctypes.byref(n_lines),
                                     ctypes.byref(first_bad))
        if not (own_bound and status == 1 and attempt == 0 and n_lines.value > max_lines):
            break
        max_lines = int(n_lines.value)      # lines shorter than a strict one: the block's own count
    check(status, entry)
    n = int(n_lines.value)
    return samples[:n], labels[:n], kinds[:n], int(first_bad.value)


def parse_training_text(data, input_size, max_lines=None):
    """dbh_text_parse: a block of whole lines (bytes, or any buffer, ending in a LF) parsed on the GPU ->
    (int16 samples [n_lines, input_size], int32 labels, uint8 kinds, first line whose kind is not
    TEXT_OK or -1).  Rows and labels of lines that are not TEXT_OK are unspecified.  ``max_lines``
    None: as many as strict lines would fit, and the block's own count where that is too few."""
    return _parse_text_block('dbh_text_parse', data, input_size, max_lines)


def parse_training_text_host(data, input_size, max_lines=None):
    """dbh_text_parse_host: the same parser as parse_training_text, run on the CPU; no device."""
    return _parse_text_block('dbh_text_parse_host', data, input_size, max_lines)


def text_stage_ms():
    """(upload, kernels, download) in ms of this thread's last parse_training_text"""
    ms = [ctypes.c_double(0) for _ in range(3)]
    check(load_library().dbh_text_stage_ms(*[ctypes.byref(m) for m in ms]), 'dbh_text_stage_ms')
    return tuple(m.value for m in ms)


# ---- random signals and training-data text written (include/deepbinner_hip.h, "random signals" and
# "training-data text, written") -------------------------------------------
class DeviceSignals:
    """int16 signals [n, input_size] in a ResidentText's device buffer, queued on its stream: what
    ResidentText.random_signals returns and ResidentText.format_training_text takes."""

    def __init__(self, owner, n):
        self.owner, self.n, self.input_size = owner, int(n), owner.input_size

    def download(self):
        return self.owner.samples.download((self.n, self.input_size), np.int16, self.owner.stream.ptr)


class ResidentText(Owner, Scoped):
    """Generator and formatter on the device for chunks of up to ``max_signals`` signals of
    ``input_size`` values: one stream, the device buffers and one pinned host buffer, all sized here
    and kept from chunk to chunk.  A chunk is random_signals() then format_training_text(): two
    entries queued on the stream, the text's length and the text brought down by one copy into
    the pinned buffer, ONE synchronisation; the int16 values never visit the host.
    ``last_ms``: (generator, formatter) of the last chunk in ms, by device events."""

    _held, _release = '_host', 'dbh_free_host'      # the pinned buffer; close() sees to the rest

    def __init__(self, max_signals, input_size):
        lib = self._lib = load_library()
        self.max_signals, self.input_size = int(max_signals), int(input_size)
        self.bound = text_format_bound(self.max_signals, self.input_size)
        work = ctypes.c_size_t(0)
        check(lib.dbh_text_format_workspace_bytes(self.max_signals, ctypes.byref(work)),
              'dbh_text_format_workspace_bytes')
        self.stream = Stream()
        self.samples = DeviceBuffer(self.max_signals * self.input_size * 2)
        self.labels = DeviceBuffer(self.max_signals * 4)
        self.text = DeviceBuffer(8 + self.bound)             # the length, then the text behind it
        self.work = DeviceBuffer(work.value)
        self.events = [Event() for _ in range(3)]
        host = ctypes.c_void_p()
        check(lib.dbh_malloc_host(ctypes.byref(host), 8 + self.bound), 'dbh_malloc_host')
        self._host = host.value
        self._view = memoryview((ctypes.c_ubyte * (8 + self.bound)).from_address(self._host)).cast('B')
        self.last_ms = (0.0, 0.0)

    def random_signals(self, seed, first_signal, n_signals, input_size=None):
        """dbh_random_signals_dev into the resident buffer: queued, not synchronised"""
        n = int(n_signals)
        if not 1 <= n <= self.max_signals or input_size not in (None, self.input_size):
            raise ValueError('expected 1 to {} signals of {} values'.format(self.max_signals,
                                                                            self.input_size))
        self.events[0].record(self.stream.ptr)
        check(self._lib.dbh_random_signals_dev(_seed64(seed), int(first_signal), n,
                                               self.input_size, self.samples.ptr, self.stream.ptr),
              'dbh_random_signals_dev')
        self.events[1].record(self.stream.ptr)
        return DeviceSignals(self, n)

    def format_training_text(self, labels, signals):
        """dbh_text_format_dev behind the generator -> the text, as a view of the pinned buffer
        that is good until the next call."""
        lib, stream = self._lib, self.stream.ptr
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if not isinstance(signals, DeviceSignals) or signals.owner is not self or \
                labels.shape != (signals.n,):
            raise ValueError('expected the signals random_signals() returned, and a label for each')
        n, bound = signals.n, text_format_bound(signals.n, self.input_size)
        check(lib.dbh_memcpy_h2d(self.labels.ptr, labels.ctypes.data, labels.nbytes, stream),
              'dbh_memcpy_h2d')
        check(lib.dbh_text_format_dev(self.labels.ptr, self.samples.ptr, n, self.input_size,
                                      self.text.ptr + 8, bound, self.text.ptr, self.work.ptr, stream),
              'dbh_text_format_dev')
        self.events[2].record(stream)
        check(lib.dbh_memcpy_d2h(self._host, self.text.ptr, 8 + bound, stream), 'dbh_memcpy_d2h')
        self.stream.synchronize()                        # the one synchronisation
        total = int.from_bytes(self._view[:8], 'little', signed=True)
        if total < 0:
            check(1, 'dbh_text_format_dev')              # a label outside +-(10^9 - 1)
        self.last_ms = (self.events[0].elapsed_ms(self.events[1]),
                        self.events[1].elapsed_ms(self.events[2]))
        return self._view[8:8 + total]

    def close(self):
        if self._host:
            self._view.release()                         # (raises while a text it handed out is held)
            Owner.close(self)
            for buffer in (self.samples, self.labels, self.text, self.work):
                buffer.free()
            self.stream.close()


def random_signals(seed, first_signal, n_signals, input_size, host=False):
    """dbh_random_signals: signals ``first_signal .. first_signal + n_signals`` of ``seed`` as int16
    [n_signals, input_size].  ``host``: dbh_random_signals_host, the CPU model, no device."""
    seed, first, n, size = _seed64(seed), int(first_signal), int(n_signals), int(input_size)
    out = np.empty((max(n, 0), max(size, 0)), dtype=np.int16)
    entry = 'dbh_random_signals_host' if host else 'dbh_random_signals'
    check(getattr(load_library(), entry)(seed, first, n, size, out.ctypes.data), entry)
    return out


def text_format_bound(n_lines, input_size):
    """dbh_text_format_bound: the bytes that the text of ``n_lines`` lines never exceeds"""
    bound = ctypes.c_int64(0)
    check(load_library().dbh_text_format_bound(int(n_lines), int(input_size), ctypes.byref(bound)),
          'dbh_text_format_bound')
    return bound.value


def format_training_text(labels, samples, host=False):
    """dbh_text_format: the training-data text of int32 ``labels`` [n] and int16 ``samples`` [n, L]
    as bytes - what parse_training_text reads back.  ``host``: dbh_text_format_host, the CPU model,
    no device."""
    lib = load_library()
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    given = np.asarray(samples)
    samples = np.ascontiguousarray(given, dtype=np.int16)
    if samples.ndim != 2 or labels.shape != (samples.shape[0],) or not np.array_equal(samples, given):
        raise ValueError('expected int16 samples of shape (n, input_size) and n labels')
    n, size = samples.shape
    entry = 'dbh_text_format_host' if host else 'dbh_text_format'
    bound = text_format_bound(n, size)
    out, n_bytes = np.empty(bound, dtype=np.uint8), ctypes.c_int64(0)
    check(getattr(lib, entry)(labels.ctypes.data, samples.ctypes.data, n, size, out.ctypes.data, bound,
                              ctypes.byref(n_bytes)), entry)
    return out[:n_bytes.value].tobytes()


def write_training_data(path, labels, samples, host=False):
    """The counterpart of read_training_data: ``labels`` and ``samples`` as a training-data text
    file at ``path``, formatted by format_training_text."""
    with open(path, 'wb') as out:
        out.write(format_training_text(labels, samples, host=host))
