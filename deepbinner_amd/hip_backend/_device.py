"""Devices, and what a process owns on one through the C ABI: streams, events, raw buffers, and
the pinned host memory the native fast5 loader can be told to use."""

import contextlib
import ctypes

import numpy as np

from .._cabi import Finalised, Owner
from ._abi import check, load_library


def device_count():
    n = ctypes.c_int(0)
    return n.value if load_library().dbh_device_count(ctypes.byref(n)) == 0 else 0


def device_name(ordinal=0):
    lib = load_library()
    buf = ctypes.create_string_buffer(256)
    check(lib.dbh_device_name(ordinal, buf, 256), 'dbh_device_name')
    return buf.value.decode()


def set_device(ordinal):
    check(load_library().dbh_set_device(int(ordinal)), 'dbh_set_device')


def get_device():
    ordinal = ctypes.c_int(0)
    check(load_library().dbh_get_device(ctypes.byref(ordinal)), 'dbh_get_device')
    return ordinal.value


def synchronize():
    check(load_library().dbh_device_synchronize(), 'dbh_device_synchronize')


LDS_CU_SLOTS = 1024                 # DBH_LDS_CU_SLOTS
LDS_ARENA_WORDS = 160 * 1024 // 4


def fill_lds(pattern, device=0, grid_multiple=0, hold_us=-1):
    """Store the 32-bit ``pattern`` in every word of every CU's LDS (test support: what a kernel
    launched next finds in the words it has not written yet).  Null stream, synchronised.  Returns
    (distinct CUs a workgroup ran on, CUs of the device): the fill counts when the two are equal."""
    seen, total = ctypes.c_int(0), ctypes.c_int(0)
    check(load_library().dbh_lds_fill(device, pattern & 0xFFFFFFFF, grid_multiple, hold_us,
                                      ctypes.byref(seen), ctypes.byref(total)), 'dbh_lds_fill')
    return seen.value, total.value


def survey_lds(pattern, device=0, grid_multiple=0, hold_us=-1):
    """Count, storing nothing to LDS, the words of every CU's LDS that equal ``pattern``.  Returns
    (matching, looked_at, CUs of the device): int64 arrays with one row per CU a workgroup ran on."""
    matching, looked_at = (np.zeros(LDS_CU_SLOTS, np.int64) for _ in range(2))
    seen, total = ctypes.c_int(0), ctypes.c_int(0)
    check(load_library().dbh_lds_survey(device, pattern & 0xFFFFFFFF, grid_multiple, hold_us,
                                        matching, looked_at, ctypes.byref(seen),
                                        ctypes.byref(total)), 'dbh_lds_survey')
    ran = looked_at > 0
    assert int(ran.sum()) == seen.value
    return matching[ran], looked_at[ran], total.value


_PINNED_LOADER = False


def use_pinned_loader_buffers(on=True):
    """Have the native fast5 loader keep its packed batches in pinned host memory (this library's
    ``dbh_host_alloc`` / ``dbh_host_release`` handed to ``f5_set_sample_allocator`` as plain C
    function pointers: the two libraries do not link each other), so that ``classify_packed`` /
    ``classify_pair`` upload them without a staging copy.  Needs a GPU; idempotent."""
    global _PINNED_LOADER
    from .. import fast5_native
    if on == _PINNED_LOADER:
        return
    if on:
        lib = load_library()
        fast5_native.set_sample_allocator(ctypes.cast(lib.dbh_host_alloc, ctypes.c_void_p).value,
                                          ctypes.cast(lib.dbh_host_release, ctypes.c_void_p).value)
    else:
        fast5_native.set_sample_allocator(None, None)
    _PINNED_LOADER = bool(on)


def is_pinned(array):
    """Does this numpy array lie in pinned host memory?"""
    flag = ctypes.c_int(0)
    check(load_library().dbh_host_is_pinned(array.ctypes.data, array.nbytes, ctypes.byref(flag)),
          'dbh_host_is_pinned')
    return bool(flag.value)


class Stream(Owner):
    """A non-blocking HIP stream owned through the C ABI; ``ptr`` is the raw hipStream_t (what the
    ``*_dev`` entry points take, and what ``torch.cuda.ExternalStream`` wraps).

    It has ``close()`` and, on purpose, no finaliser: callers (the benchmark, the sharded path,
    tests) keep the raw ``ptr`` and let the Stream object go while work is still queued on it."""

    _held, _release = 'ptr', 'dbh_stream_destroy'

    def __init__(self):
        self._lib = load_library()
        s = ctypes.c_void_p()
        check(self._lib.dbh_stream_create(ctypes.byref(s)), 'dbh_stream_create')
        self.ptr = s.value

    def synchronize(self):
        check(self._lib.dbh_stream_synchronize(self.ptr), 'dbh_stream_synchronize')

    def wait_event(self, event):
        """Work queued from now on waits for ``event`` (an ``Event`` recorded on another stream)."""
        check(self._lib.dbh_stream_wait_event(self.ptr, event.handle), 'dbh_stream_wait_event')


class DeviceBuffer(Owner, Finalised):
    """A raw HBM allocation owned through the C ABI (no torch / no other GPU library)."""

    _held, _release = 'ptr', 'dbh_free'

    def __init__(self, nbytes):
        self._lib = load_library()
        self.nbytes = int(nbytes)
        ptr = ctypes.c_void_p()
        check(self._lib.dbh_malloc(ctypes.byref(ptr), self.nbytes), 'dbh_malloc')
        self.ptr = ptr.value

    @classmethod
    def from_array(cls, array, stream=None):
        array = np.ascontiguousarray(array)
        buf = cls(max(array.nbytes, 1))
        buf.upload(array, stream)
        return buf

    def upload(self, array, stream=None):
        array = np.ascontiguousarray(array)
        assert array.nbytes <= self.nbytes
        check(self._lib.dbh_memcpy_h2d(self.ptr, array.ctypes.data, array.nbytes, stream),
              'dbh_memcpy_h2d')
        check(self._lib.dbh_stream_synchronize(stream), 'dbh_stream_synchronize')

    def download(self, shape, dtype, stream=None):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(self._lib.dbh_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, stream),
              'dbh_memcpy_d2h')
        check(self._lib.dbh_stream_synchronize(stream), 'dbh_stream_synchronize')
        return out

    free = Owner.close


class Event(Owner, Finalised):
    _held, _release = 'handle', 'dbh_event_destroy'

    def __init__(self):
        self._lib = load_library()
        e = ctypes.c_void_p()
        check(self._lib.dbh_event_create(ctypes.byref(e)), 'dbh_event_create')
        self.handle = e.value

    def record(self, stream=None):
        check(self._lib.dbh_event_record(self.handle, stream), 'dbh_event_record')

    def synchronize(self):
        check(self._lib.dbh_event_synchronize(self.handle), 'dbh_event_synchronize')

    def elapsed_ms(self, later):
        ms = ctypes.c_float(0)
        check(self._lib.dbh_event_elapsed_ms(self.handle, later.handle, ctypes.byref(ms)),
              'dbh_event_elapsed_ms')
        return ms.value


@contextlib.contextmanager
def device_arrays(*items):
    """DeviceBuffers for the length of a ``with``, one per item, in order: an array is uploaded,
    an integer is a buffer of that many bytes left as it comes.  All are freed on the way out."""
    held = []
    try:
        for item in items:
            held.append(DeviceBuffer(item) if isinstance(item, (int, np.integer))
                        else DeviceBuffer.from_array(item))
        yield held
    finally:
        for buf in held:
            buf.free()
