"""
HDF5's shuffle filter for tests: the filter in NumPy, ``signal_filter`` builders for
deepbinner_amd/hdf5_write.py and shuffled copies of fast5 files.  Nothing here is committed as a
file: the copies are built in a test's temporary directory.

Shuffle of N bytes of int16 puts byte j of element i at j * (N/2) + i: the low bytes of all
samples, then their high bytes.
"""

import os
import struct
import zlib

import numpy as np

SHUFFLE, DEFLATE, FLETCHER32 = 2, 1, 3


def shuffle(samples):
    """int16 samples -> their bytes as the shuffle filter leaves them."""
    b = np.ascontiguousarray(samples, dtype='<i2').view(np.uint8).reshape(-1, 2)
    return np.concatenate([b[:, 0], b[:, 1]]).tobytes()


def unshuffle(data):
    """Shuffled bytes (an even number) -> the int16 samples."""
    b = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(b) // 2
    return np.stack([b[:n], b[n:2 * n]], axis=1).reshape(-1).view('<i2').copy()


def fletcher32(data):
    """HDF5's Fletcher32 of ``data`` (H5_checksum_fletcher32: big-endian 16-bit words, sums folded
    every 360 words), as the 4 bytes the filter appends."""
    b = bytes(data)
    words = np.frombuffer(b[:len(b) & ~1], dtype='>u2').astype(np.uint64)
    s1 = s2 = 0
    for k in range(0, len(words), 360):
        run = s1 + np.cumsum(words[k:k + 360])
        s2 += int(run.sum())
        s1 = int(run[-1])
        s1 = (s1 & 0xFFFF) + (s1 >> 16)
        s2 = (s2 & 0xFFFF) + (s2 >> 16)
    if len(b) & 1:
        s1 += b[-1] << 8
        s2 += s1
        s1 = (s1 & 0xFFFF) + (s1 >> 16)
        s2 = (s2 & 0xFFFF) + (s2 >> 16)
    s1 = (s1 & 0xFFFF) + (s1 >> 16)
    s2 = (s2 & 0xFFFF) + (s2 >> 16)
    return struct.pack('<I', (s2 << 16) | s1)


def pipeline_message(filters):
    """The body of a version-1 filter pipeline message: ``filters`` = [(id, [client values])]."""
    body = struct.pack('<BB6x', 1, len(filters))
    for fid, cd in filters:
        cd = [int(v) for v in cd]
        body += struct.pack('<HHHH', fid, 0, 1, len(cd)) + struct.pack('<%dI' % len(cd), *cd)
        if len(cd) % 2:
            body += b'\0' * 4
    return body


# the pipelines of the raw route's table: applied filters -> the pipeline message's entries
PIPELINES = {
    'shuffle_deflate': [(SHUFFLE, [2]), (DEFLATE, [1])],
    'shuffle_deflate_fletcher': [(SHUFFLE, [2]), (DEFLATE, [1]), (FLETCHER32, [])],
    'shuffle': [(SHUFFLE, [2])],
    'shuffle_fletcher': [(SHUFFLE, [2]), (FLETCHER32, [])],
    'deflate': [(DEFLATE, [1])],
}


def damage_deflate(stream):
    """A zlib stream with one byte of its deflate data changed so that a CODE breaks: zlib meets an
    invalid code, distance or block before it has produced as many bytes as the stream held (not
    merely other literals, which only the checksum at the end would tell)."""
    n = len(zlib.decompress(stream))
    mid = len(stream) // 2                     # (from the middle on, then backwards from there)
    for at in list(range(mid, len(stream) - 4)) + list(range(mid - 1, 1, -1)):
        bad = stream[:at] + bytes([stream[at] ^ 0x5A]) + stream[at + 1:]
        try:
            zlib.decompressobj().decompress(bad, max(n, 1))
        except zlib.error as e:
            if 'invalid' in str(e):
                return bad
    raise AssertionError('no byte whose change breaks a code')


def encode_chunk(part, kind, level=1, damage=False):
    """One chunk's samples -> its bytes as the pipeline ``kind`` stores them.  ``damage``: one byte
    inside the deflate data is changed (damage_deflate; a checksum behind it is that of the
    damaged bytes: what is wrong is the deflate data alone)."""
    data = shuffle(part) if kind.startswith('shuffle') else np.asarray(part, '<i2').tobytes()
    if 'deflate' in kind:
        data = zlib.compress(data, level)
        if damage:
            data = damage_deflate(data)
    if kind.endswith('fletcher'):
        data += fletcher32(data)
    return data


def signal_filter(samples, kind='shuffle_deflate', chunk=None, level=1, damage_chunks=()):
    """hdf5_write's ``signal_filter`` for ``samples`` through the pipeline ``kind`` (a key of
    PIPELINES): chunks of ``chunk`` samples (None: one chunk of exactly the read), the last one
    padded to the chunk size as libhdf5 does."""
    samples = np.asarray(samples, dtype=np.int16)
    n = len(samples)
    chunk = n if chunk is None else int(chunk)
    chunks = []
    for k in range(-(-n // chunk)):
        part = np.zeros(chunk, dtype=np.int16)
        piece = samples[k * chunk:(k + 1) * chunk]
        part[:len(piece)] = piece
        chunks.append((encode_chunk(part, kind, level, damage=k in damage_chunks), 0))
    return {'pipeline': pipeline_message(PIPELINES[kind]), 'chunk': chunk, 'chunks': chunks}


def write_copy(reads, path, kind='shuffle_deflate', chunk=None, level=1, multi=None, damage=None):
    """The reads (read_id, signal) as a fast5 at ``path`` whose Signals went through the pipeline
    ``kind``: one read -> the single-read layout, several (or multi=True) -> a multi-read
    container.  ``chunk``: samples per chunk, or a function of the read's index and length.
    ``damage``: {read index: chunks whose deflate data are damaged}."""
    from deepbinner_amd import hdf5_write
    if multi is None:
        multi = len(reads) != 1
    items = []
    for i, (rid, signal) in enumerate(reads):
        c = chunk(i, len(signal)) if callable(chunk) else chunk
        sf = None
        if len(signal):
            sf = signal_filter(signal, kind, c, level, damage_chunks=(damage or {}).get(i, ()))
        items.append((rid, signal, sf))
    if multi:
        image = hdf5_write.multi_read_fast5_bytes([(rid, s, None, None, sf) for rid, s, sf in items])
    else:
        rid, s, sf = items[0]
        image = hdf5_write.single_read_fast5_bytes(rid, s, signal_filter=sf)
    with open(path, 'wb') as f:
        f.write(image)
    return path


def squiggle(rng, n):
    """Something like a nanopore signal: levels of a few samples each, noise on top."""
    levels = rng.integers(350, 650, size=n // 6 + 2)
    base = np.repeat(levels, rng.integers(3, 12, size=len(levels)))[:n]
    if len(base) < n:
        base = np.concatenate([base, np.full(n - len(base), 500)])
    return (base + rng.integers(-12, 13, size=n)).astype(np.int16)


def small_container(path, n_reads=200, kind='shuffle_deflate', seed=5, damage=None, chunk='mixed'):
    """A multi-read container of ``n_reads`` squiggle-like reads of 1,500 - 9,000 samples; with
    chunk='mixed' every third read is one chunk, the others in chunks of 1,000 or 3,125 samples
    (their last chunk partial).  -> (path, [(read_id, signal)])."""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n_reads):
        n = int(rng.integers(1500, 9000))
        rid = '%08x-5bf1-4c6e-9d6e-%012x' % (seed * 1000 + i, i)
        reads.append((rid, squiggle(rng, n)))

    def mixed(i, n):
        return (None, 1000, 3125)[i % 3]
    write_copy(reads, path, kind, mixed if chunk == 'mixed' else chunk, multi=True, damage=damage)
    return path, reads


H5PY_SHUFFLED = ('many_chunks_shuffle_fletcher_old.fast5', 'many_chunks_shuffle_fletcher_new.fast5')


def golden(name):
    here = os.path.dirname(os.path.abspath(__file__))
    return os.path.join(here, 'golden', 'fast5', 'h5py_variants', name)
