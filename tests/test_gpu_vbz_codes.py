"""The streamvbyte decoder on the GPU (deepbinner_amd/csrc/dbh_vbz.hip) held to tests/
vbz_reference.py, bit for bit: every code at every place of a lane, the seams of its lanes, steps
and store paths, damaged streams (refused exactly where the host's decoder refuses, zeros there,
the reference's samples where it accepts), a launch long enough for the kernel's stream loop to
come round, and the memory beside every stream's output.  The conditions that keep these inputs
from being hollow are asserted in tests/test_vbz_reference.py, on the reference alone.

Everything goes through dbh_inflate_dev on device buffers the test fills itself: the output with
a sentinel byte, the statuses with a value no kernel writes.

Every record's comp_offset / comp_bytes and out_offset / out_bytes lie inside their buffers
(``Batch.records`` asserts it): these tests check decisions about a stream's CONTENT.  Records
that point outside a buffer are left out on purpose - a wrong bounds check there would touch
memory outside an allocation, on a machine others may share, and dbh_inflate and the loader
validate records on the host."""

import ctypes
import time

import numpy as np
import pytest

import vbz_reference as ref
from test_inflate import kernel1, valid_cases          # noqa: F401 - kernel1 is a fixture

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
UNWRITTEN = 0x5A5A5A5A        # (the kernels' statuses are small: 0, 1, the inflate error numbers)
ZLIB, STORED, VBZ = 0, 1, 2


class Batch:
    """Streams in record order, their outputs laid out in another order with gaps between them."""

    def __init__(self):
        self.names, self.payloads, self.out_bytes, self.modes, self.aligns = [], [], [], [], []
        self.ok, self.want = [], []

    def add(self, name, payload, out_bytes, mode, ok, want, align=None):
        want = np.frombuffer(bytes(want), dtype=np.uint8)
        assert len(want) == out_bytes
        self.names.append(name)
        self.payloads.append(bytes(payload))
        self.out_bytes.append(int(out_bytes))
        self.modes.append(mode)
        self.aligns.append(align)
        self.ok.append(bool(ok))
        self.want.append(want)

    def add_case(self, c):
        ok, want = ref.expected(c.payload, c.out_bytes)
        self.add('%s/%s' % (c.family, c.name), c.payload, c.out_bytes, VBZ, ok, want.tobytes(), c.align)

    def __len__(self):
        return len(self.names)

    def records(self, hip, rng=None):
        """(comp with its 64 bytes of padding, records, size of the output buffer); ``rng``: the
        outputs in shuffled order (None: in record order), gaps of 2..30 bytes either way"""
        n = len(self)
        gaps = np.random.default_rng(30)
        order = np.arange(n) if rng is None else rng.permutation(n)
        out_offset = np.zeros(n, dtype=np.int64)
        at = 16 + 2 * int(gaps.integers(1, 16))
        for k in order:
            at += at & 1
            if self.aligns[k] is not None:
                at += (self.aligns[k] - at) % 16
            out_offset[k] = at
            at += self.out_bytes[k] + 2 * int(gaps.integers(1, 16))
        out_total = at + 64
        comp_bytes = np.array([len(p) for p in self.payloads], dtype=np.int64)
        comp_offset = np.cumsum(comp_bytes) - comp_bytes
        comp = np.frombuffer(b''.join(self.payloads) + bytes(64), dtype=np.uint8)
        records = np.zeros(n, dtype=hip.INFLATE_STREAM)
        records['comp_offset'], records['comp_bytes'] = comp_offset, comp_bytes
        records['out_offset'], records['out_bytes'] = out_offset, self.out_bytes
        records['mode'] = self.modes
        assert (records['comp_offset'] >= 0).all() and (records['comp_bytes'] >= 0).all()
        assert (records['comp_offset'] + records['comp_bytes'] <= len(comp) - 64).all()
        assert (records['out_offset'] >= 0).all() and (records['out_offset'] % 2 == 0).all()
        assert (records['out_offset'] + records['out_bytes'] <= out_total).all()
        return comp, records, out_total


def inflate_dev(hip, comp, records, out_total):
    """dbh_inflate_dev over device buffers -> (the whole output buffer, statuses, seconds)"""
    lib = hip.load_library()
    work = ctypes.c_size_t(0)
    hip.check(lib.dbh_inflate_workspace_bytes(out_total, len(records), ctypes.byref(work)))
    d_comp = hip.DeviceBuffer.from_array(comp)
    d_records = hip.DeviceBuffer.from_array(records)
    d_out = hip.DeviceBuffer.from_array(np.full(out_total, SENTINEL, dtype=np.uint8))
    d_status = hip.DeviceBuffer.from_array(np.full(len(records), UNWRITTEN, dtype=np.int32))
    d_work = hip.DeviceBuffer(max(work.value, 1))
    try:
        t0 = time.perf_counter()
        hip.check(lib.dbh_inflate_dev(d_comp.ptr, len(comp) - 64, d_records.ptr, len(records),
                                      out_total, d_out.ptr, d_work.ptr, d_status.ptr, 0, None),
                  'dbh_inflate_dev')
        hip.synchronize()
        seconds = time.perf_counter() - t0
        return (d_out.download((out_total,), np.uint8), d_status.download((len(records),), np.int32),
                seconds)
    finally:
        for buf in (d_comp, d_records, d_out, d_status, d_work):
            buf.free()


def check(batch, records, out, status):
    """every region as expected, every status zero exactly where the stream is accepted, every
    byte outside the regions still the sentinel"""
    wrong = []
    outside = np.ones(len(out), dtype=bool)
    for k, rec in enumerate(records):
        a, b = int(rec['out_offset']), int(rec['out_offset'] + rec['out_bytes'])
        outside[a:b] = False
        if status[k] == UNWRITTEN:
            wrong.append((k, batch.names[k], 'status not written'))
        elif (status[k] == 0) != batch.ok[k]:
            wrong.append((k, batch.names[k], 'status %d' % status[k]))
        elif not np.array_equal(out[a:b], batch.want[k]):
            first = int(np.nonzero(out[a:b] != batch.want[k])[0][0])
            wrong.append((k, batch.names[k], 'byte %d of %d differs' % (first, b - a)))
    assert not wrong, (len(wrong), wrong[:12])
    dirty = np.nonzero(outside & (out != SENTINEL))[0]
    if len(dirty):
        by_offset = np.argsort(records['out_offset'], kind='stable')
        ends = (records['out_offset'] + records['out_bytes'])[by_offset]
        found = []
        for at in dirty[:12]:
            j = int(np.searchsorted(records['out_offset'][by_offset], at, side='right')) - 1
            k = int(by_offset[j]) if j >= 0 else -1
            found.append((int(at), 'behind ' + batch.names[k] if k >= 0 else 'start',
                          int(at - ends[j]) if j >= 0 else int(at)))
        assert False, ('%d bytes written outside every region' % len(dirty), found)


def interleaved(vbz_cases):
    """the VBZ cases with zlib and stored streams of test_inflate.valid_cases() between them"""
    others = []
    for k, (stream, cap, want) in enumerate(valid_cases()):
        others.append(('zlib/%d' % k, stream, cap, ZLIB, want + bytes(cap - len(want))))
        if k % 4 == 0 and len(want) <= 100000:
            extend = 77 if k % 8 == 0 else 0
            others.append(('stored/%d' % k, want, len(want) + extend, STORED, want + bytes(extend)))
    batch = Batch()
    every = max(1, len(vbz_cases) // (len(others) + 1))
    for k, c in enumerate(vbz_cases):
        batch.add_case(c)
        if k % every == every - 1 and others:
            name, payload, out_bytes, mode, want = others.pop()
            batch.add(name, payload, out_bytes, mode, True, want)
    for name, payload, out_bytes, mode, want in others:
        batch.add(name, payload, out_bytes, mode, True, want)
    return batch


@pytest.fixture(scope='module')
def families():
    cases = ref.all_cases()
    print(ref.census_text(ref.census(cases)))
    batch = interleaved(cases)
    assert sum(m == VBZ for m in batch.modes) == len(cases)       # no case is left out
    assert batch.modes.count(ZLIB) > 100 and batch.modes.count(STORED) > 10
    return batch


def test_every_family_beside_zlib_and_stored_streams(hip, kernel1, families):
    """codes, unwrapped deltas, padding bits, output shapes and mutants in ONE launch between zlib
    and stored streams, behind each form of the inflate kernels"""
    comp, records, out_total = families.records(hip, np.random.default_rng(5))
    out, status, seconds = inflate_dev(hip, comp, records, out_total)
    print('%s: %d streams (%d VBZ), %.1f MB in, %.1f MB out, %.3f s' % (
        kernel1, len(records), families.modes.count(VBZ), len(comp) / 1e6, out_total / 1e6, seconds))
    check(families, records, out, status)


def test_a_batch_twice_and_in_reversed_record_order(hip, families):
    comp, records, out_total = families.records(hip, np.random.default_rng(6))
    first = inflate_dev(hip, comp, records, out_total)
    check(families, records, first[0], first[1])
    again = inflate_dev(hip, comp, records, out_total)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    back = inflate_dev(hip, comp, records[::-1].copy(), out_total)
    assert np.array_equal(first[0], back[0]) and np.array_equal(first[1], back[1][::-1])


def test_a_launch_that_loops(hip):
    """40,000 streams: more than the 8,192 workgroups of four waves one trip of the kernel's loop
    over the streams takes; then VBZ streams in the second trip only, behind 33,000 stored ones"""
    cases = ref.loop_cases()
    batch = Batch()
    for c in cases:
        batch.add_case(c)
    assert len(batch) == 40000 and batch.ok.count(False) == 400
    comp, records, out_total = batch.records(hip, np.random.default_rng(7))
    out, status, seconds = inflate_dev(hip, comp, records, out_total)
    print('%d streams, %.1f MB in, %.3f s' % (len(records), len(comp) / 1e6, seconds))
    check(batch, records, out, status)
    rng = np.random.default_rng(8)
    upper = Batch()
    for k in range(33000):
        data = rng.integers(0, 256, 2 * int(rng.integers(0, 9)), dtype=np.uint8).tobytes()
        upper.add('stored/%d' % k, data, len(data) + 2, STORED, True, data + bytes(2))
    for c in cases[33000:]:
        upper.add_case(c)
    assert len(upper) == 40000 and upper.modes[32999] == STORED and upper.modes[33000] == VBZ
    comp, records, out_total = upper.records(hip, np.random.default_rng(9))
    out, status, _ = inflate_dev(hip, comp, records, out_total)
    check(upper, records, out, status)


def test_the_long_read(hip):
    """1,500,000 values (1,465 steps: the carry and the data offset over a long read), whole, cut
    to 12,288 bytes, and zero-extended; at an output offset the packed stores take and one they
    do not"""
    payload = ref.long_read_stream()
    batch = Batch()
    for out_bytes in (2 * ref.LONG_READ, 12288, 2 * ref.LONG_READ + 4096):
        for align in (0, 6):
            ok, want = ref.expected(payload, out_bytes)
            assert ok
            batch.add('long_read/out%d_at%d' % (out_bytes, align), payload, out_bytes, VBZ, ok,
                      want.tobytes(), align)
    comp, records, out_total = batch.records(hip)
    out, status, seconds = inflate_dev(hip, comp, records, out_total)
    print('%d streams of %d values, %.3f s' % (len(records), ref.LONG_READ, seconds))
    check(batch, records, out, status)


def test_mutants_between_intact_neighbours(hip):
    """one launch: a valid stream, a mutant of it, a valid stream, ... in the order of the records
    and of the outputs - refused exactly where the reference refuses and zeros there, the
    reference's samples where it accepts, and every neighbour intact"""
    mutants = ref.mutant_cases()
    batch = Batch()
    for c in mutants:
        batch.add_case(ref.case('origin', c.name, c.origin, c.out_bytes))
        batch.add_case(c)
    batch.add_case(ref.case('origin', 'last', mutants[-1].origin, mutants[-1].out_bytes))
    assert batch.ok[::2] == [True] * (len(mutants) + 1)
    refused = batch.ok[1::2].count(False)
    assert refused >= 300 and len(mutants) - refused >= 300
    comp, records, out_total = batch.records(hip)
    out, status, seconds = inflate_dev(hip, comp, records, out_total)
    print('%d mutants: %d refused, %d accepted; %.3f s' % (len(mutants), refused,
                                                           len(mutants) - refused, seconds))
    check(batch, records, out, status)
