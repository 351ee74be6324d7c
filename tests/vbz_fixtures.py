"""
VBZ fixtures for the tests: an encoder of ONT's VBZ filter (HDF5 filter 32020, version 0) as
DESIGN.md's section "VBZ" pins it - NumPy streamvbyte, zstd through the system's libzstd - and
VBZ copies of fast5 files, written through deepbinner_amd/hdf5_write.py's ``signal_filter``.
Nothing here is committed as a file: the copies are built in a test's temporary directory from
the golden fast5 files.
"""

import ctypes
import os
import struct

import numpy as np

VBZ = 32020


def zstd_lib():
    try:
        lib = ctypes.CDLL('libzstd.so.1')
    except OSError:
        return None
    lib.ZSTD_compressBound.restype = ctypes.c_size_t
    lib.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    lib.ZSTD_compress.restype = ctypes.c_size_t
    lib.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                  ctypes.c_size_t, ctypes.c_int]
    lib.ZSTD_isError.restype = ctypes.c_uint
    lib.ZSTD_isError.argtypes = [ctypes.c_size_t]
    return lib


def zstd_compress(data, level=1):
    lib = zstd_lib()
    data = bytes(data)
    out = ctypes.create_string_buffer(lib.ZSTD_compressBound(len(data)))
    k = lib.ZSTD_compress(out, len(out), data, len(data), int(level))
    assert not lib.ZSTD_isError(k)
    return out.raw[:k]


def streamvbyte(samples, wrap=True):
    """int16 samples -> streamvbyte bytes of their zigzagged deltas (delta from 0).  ``wrap``: the
    delta of two samples wrapped to int16 (codes of 1 and 2 bytes only); False: taken in 32 bits
    as it is, so that a jump beyond +-32,767 takes a 3-byte code.  Both decode to the same samples
    (the decoder sums modulo 2^32 and truncates)."""
    x = np.asarray(samples, dtype=np.int16).astype(np.int64)
    delta = np.diff(np.concatenate([[0], x]))
    if wrap:
        delta = ((delta + 32768) % 65536) - 32768         # the int16 delta, wrapped
    u = (((delta << 1) ^ (delta >> 63)) & 0xFFFFFFFF).astype(np.uint32)
    return pack_values(u)


def pack_values(u, lengths=None):
    """uint32 values -> control bytes + data bytes; ``lengths`` (1..4 each) may force longer codes
    than the values need."""
    u = np.asarray(u, dtype=np.uint32)
    n = len(u)
    need = np.where(u < 1 << 8, 1, np.where(u < 1 << 16, 2, np.where(u < 1 << 24, 3, 4)))
    lengths = need if lengths is None else np.maximum(need, np.asarray(lengths))
    codes = np.zeros(((n + 3) // 4) * 4, dtype=np.uint8)
    codes[:n] = lengths - 1
    ctrl = (codes.reshape(-1, 4).astype(np.uint32) << np.array([0, 2, 4, 6], dtype=np.uint32)).sum(1)
    data = u.astype('<u4').view(np.uint8).reshape(-1, 4)[np.arange(4)[None, :] < lengths[:, None]]
    return ctrl.astype(np.uint8).tobytes() + data.tobytes()


def vbz_chunk(samples, level=1, original_size=None, wrap=True):
    """One chunk as the VBZ filter stores it: u32 original_size, then the zstd frame of the
    streamvbyte bytes (level 0: the streamvbyte bytes themselves)."""
    samples = np.asarray(samples, dtype=np.int16)
    packed = streamvbyte(samples, wrap)
    size = len(samples) * 2 if original_size is None else original_size
    return struct.pack('<I', size) + (zstd_compress(packed, level) if level else packed)


def pipeline_message(cd=(0, 2, 1, 1), version=1, name=b'vbz'):
    """The body of a filter pipeline message holding the one VBZ entry."""
    cd = [int(v) for v in cd]
    if version == 1:
        name_field = (name + b'\0' + b'\0' * (-(len(name) + 1) % 8)) if name else b''
        body = struct.pack('<BB6x', 1, 1)
        body += struct.pack('<HHHH', VBZ, len(name_field), 1, len(cd)) + name_field
        body += struct.pack('<%dI' % len(cd), *cd)
        if len(cd) % 2:
            body += b'\0' * 4
        return body
    name_field = name + b'\0' if name else b''
    body = struct.pack('<BB', 2, 1) + struct.pack('<HHHH', VBZ, len(name_field), 1, len(cd))
    return body + name_field + struct.pack('<%dI' % len(cd), *cd)


def signal_filter(samples, cd=(0, 2, 1, 1), version=1, name=b'vbz', chunk=None, raw_chunks=(),
                  encode=None):
    """hdf5_write's ``signal_filter`` for ``samples`` as VBZ: chunks of ``chunk`` samples (None:
    one chunk of exactly the read), the last one padded to the chunk size as libhdf5 does; chunks
    whose index is in ``raw_chunks`` stored unfiltered (filter mask bit 0 set).  ``encode``: a
    chunk's samples -> its bytes as stored (default: vbz_chunk at cd[3]'s level)."""
    samples = np.asarray(samples, dtype=np.int16)
    n = len(samples)
    chunk = n if chunk is None else int(chunk)
    level = cd[3] if len(cd) > 3 else 0
    encode = encode or (lambda s: vbz_chunk(s, level))
    chunks = []
    for k in range(-(-n // chunk)):
        part = np.zeros(chunk, dtype=np.int16)
        piece = samples[k * chunk:(k + 1) * chunk]
        part[:len(piece)] = piece
        if k in raw_chunks:
            chunks.append((part.tobytes(), 1))
        else:
            chunks.append((encode(part), 0))
    return {'pipeline': pipeline_message(cd, version, name), 'chunk': chunk, 'chunks': chunks}


# the shapes a copy may take, dealt over the files in turn
VARIANTS = [
    dict(version=1, name=b'vbz', chunk=None),
    dict(version=2, name=b'vbz', chunk=None),
    dict(version=2, name=None, chunk=None),
    dict(version=1, name=None, chunk=4000),
    dict(version=1, name=b'vbz', chunk=3000, raw_chunks=(1,)),
    dict(version=2, name=b'vbz', chunk=None, cd=(0, 2, 1, 0)),
]


def read_all(path):
    """[(read_id, signal)] of a fast5 file, through the pure-Python reader."""
    from deepbinner_amd import hdf5_lite
    out = []
    with hdf5_lite.File(path, 'r') as f:
        keys = list(f.keys())
        if 'Raw' in keys:
            for group in f['Raw/Reads'].values():
                out.append((_text(group.attrs['read_id']), np.asarray(group['Signal'][:], np.int16)))
        else:
            for key in sorted(k for k in keys if k.startswith('read_')):
                raw = f[key + '/Raw']
                out.append((_text(raw.attrs['read_id']), np.asarray(raw['Signal'][:], np.int16)))
    return out


def _text(v):
    return v.decode() if isinstance(v, bytes) else str(v)


def write_vbz_copy(reads, path, variant, multi=None):
    """The reads (read_id, signal) as a VBZ fast5 at ``path``: one read -> the single-read (new)
    layout, several (or multi=True) -> a multi-read container."""
    from deepbinner_amd import hdf5_write
    v = dict(variant)
    cd = v.pop('cd', (0, 2, 1, 1))
    if multi is None:
        multi = len(reads) != 1
    items = []
    for rid, signal in reads:
        sf = signal_filter(signal, cd=cd, **v) if len(signal) else None
        items.append((rid, signal, sf))
    if multi:
        image = hdf5_write.multi_read_fast5_bytes([(rid, s, None, None, sf) for rid, s, sf in items])
    else:
        rid, s, sf = items[0]
        image = hdf5_write.single_read_fast5_bytes(rid, s, signal_filter=sf)
    with open(path, 'wb') as f:
        f.write(image)
    return path


def golden_fast5():
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.join(here, 'golden', 'fast5')
    out = []
    for sub in ('single', 'multi', 'h5py_variants'):
        d = os.path.join(root, sub)
        out += sorted(os.path.join(d, n) for n in os.listdir(d) if n.endswith('.fast5'))
    return out
