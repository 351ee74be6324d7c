"""What the GPU tests of the zstd stage share (tests/test_gpu_zstd.py, tests/test_gpu_zstd_written.py):
one dbh_inflate_dev call over a list of streams, with sentinels around everything it may write."""

import ctypes
import struct

import numpy as np

VBZ_ZSTD = 3
SENTINEL = 0xA5


def run(hip, items):
    """items: [(bytes, out_bytes, mode)] as one dbh_inflate_dev call -> (per stream output bytes,
    status, per stream workspace slots).  The outputs lie at even offsets of every residue modulo
    16 with gaps between them; the output buffer is filled with a sentinel first and every byte
    outside the streams' regions must still hold it.

    So is the workspace's token region (4 bytes per byte of output).  In a call that holds streams
    of mode 3 only, every byte of it outside the streams' own slots - [4 * out_offset, 4 *
    (out_offset + out_bytes)) - must still hold the sentinel: the inflate kernels pass such streams
    by, the zstd kernel writes a frame's content and its parked literals into the stream's slots
    alone, and the streamvbyte kernel behind it only reads them (dbh_inflate.hip, dbh_vbz.hip).
    With other modes in the call the token region is the inflate kernels' to write and is not
    looked at.  The per-stream records behind the token region are uploaded as zeros."""
    lib = hip.load_library()
    streams, comp_at, out_at = [], 0, 0
    for k, (data, out_bytes, mode) in enumerate(items):
        out_at += 2 * (k % 8) + 2
        streams.append((comp_at, len(data), out_at, out_bytes, mode, 0))
        comp_at += len(data)
        out_at += out_bytes
    total_out = out_at + 64
    comp = np.zeros(comp_at + 64, dtype=np.uint8)
    comp[:comp_at] = np.frombuffer(b''.join(d for d, _, _ in items), dtype=np.uint8)
    records = np.array(streams, dtype=hip.INFLATE_STREAM)
    work_bytes = ctypes.c_size_t(0)
    hip.check(lib.dbh_inflate_workspace_bytes(total_out, len(records), ctypes.byref(work_bytes)))
    work0 = np.zeros(work_bytes.value, dtype=np.uint8)
    work0[:4 * total_out] = SENTINEL
    d_comp = hip.DeviceBuffer.from_array(comp)
    d_rec = hip.DeviceBuffer.from_array(records)
    d_out = hip.DeviceBuffer.from_array(np.full(total_out, SENTINEL, dtype=np.uint8))
    d_work = hip.DeviceBuffer.from_array(work0)
    d_status = hip.DeviceBuffer.from_array(np.full(len(records), -7, dtype=np.int32))
    try:
        hip.check(lib.dbh_inflate_dev(d_comp.ptr, comp_at, d_rec.ptr, len(records), total_out, d_out.ptr,
                                      d_work.ptr, d_status.ptr, 0, None), 'dbh_inflate_dev')
        hip.synchronize()
        raw = d_out.download(total_out, np.uint8)
        status = d_status.download(len(records), np.int32)
        work = d_work.download(4 * total_out, np.uint8)
    finally:
        for b in (d_comp, d_rec, d_out, d_work, d_status):
            b.free()
    outside = np.ones(total_out, dtype=bool)
    for r in records:
        outside[r['out_offset']:r['out_offset'] + r['out_bytes']] = False
    assert (raw[outside] == SENTINEL).all(), 'a byte outside the streams\' regions was changed'
    if all(mode == VBZ_ZSTD for _, _, mode in items):
        touched = np.flatnonzero(work[np.repeat(outside, 4)] != SENTINEL)
        assert touched.size == 0, 'a workspace byte outside the streams\' slots was changed: %d of them, the ' \
            'first at %d' % (touched.size, np.flatnonzero(np.repeat(outside, 4))[touched[0]])
    outs = [raw[r['out_offset']:r['out_offset'] + r['out_bytes']] for r in records]
    slots = [work[4 * r['out_offset']:4 * (r['out_offset'] + r['out_bytes'])] for r in records]
    return outs, status, slots


def samples_of(content, n):
    from deepbinner_amd import fast5_native
    return fast5_native.vbz_decode(struct.pack('<I', 2 * n) + content, (0, 2, 1, 0), n)
