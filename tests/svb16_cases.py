"""The case families the svb16 decoders (POD5's 16-bit streamvbyte code) are
held to: the NumPy restatement (``pod5_lite.decode_svb16``), the host entry of the GPU's core
(``dbh_svb16_decode_host``) and the GPU itself (tests/test_gpu_svb16.py).  The reference of all
three is ``plain_decode`` below: one value at a time in plain Python.  No GPU, no ctypes.
"""
import struct

import numpy as np

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025, 2049)
LONG = 102400
STEP, PER_LANE = 1024, 16               # the wave's step: 64 lanes x 16 values


def plain_encode(samples):
    """int16 samples -> svb16 stream, one value at a time"""
    keys = bytearray((len(samples) + 7) // 8)
    data = bytearray()
    before = 0
    for i, s in enumerate(int(x) & 0xFFFF for x in samples):
        delta = (s - before) & 0xFFFF
        before = s
        v = ((delta << 1) ^ (0xFFFF if delta & 0x8000 else 0)) & 0xFFFF
        data.append(v & 0xFF)
        if v > 0xFF:
            keys[i >> 3] |= 1 << (i & 7)
            data.append(v >> 8)
    return bytes(keys) + bytes(data)


def plain_decode(stream, n):
    """svb16 stream of n values -> int16 array, one value at a time; None where the key bytes do
    not fit or the data do not end exactly where the stream does"""
    stream = bytes(stream)
    n_keys = (n + 7) // 8
    if n_keys > len(stream):
        return None
    at, total, out = n_keys, 0, []
    for i in range(n):
        two = (stream[i >> 3] >> (i & 7)) & 1
        if at + 1 + two > len(stream):
            return None
        v = stream[at] | (stream[at + 1] << 8 if two else 0)
        at += 1 + two
        total = (total + ((v >> 1) ^ (0xFFFF if v & 1 else 0))) & 0xFFFF
        out.append(total)
    if at != len(stream):
        return None
    return np.array(out, dtype=np.uint16).view(np.int16)


def from_deltas(deltas):
    return np.cumsum(np.asarray(deltas, dtype=np.int64)).astype(np.uint16).view(np.int16)


def key_patterns(n, rng):
    """{name: samples} of n values: every value one byte, every value two, alternating, random, a
    two-byte value at both sides of every lane boundary and of every step boundary, and deltas that
    wrap (-32,768, 32,767 and back)"""
    small = rng.integers(-128, 128, n)
    large = np.where(rng.integers(0, 2, n) == 1, rng.integers(128, 32768, n),
                     -rng.integers(129, 32769, n))
    index = np.arange(n)
    lane_edge = np.isin(index % PER_LANE, (0, PER_LANE - 1))
    wrap = np.resize(np.array([-32768, 32767, 32767, -32768, 1, -1, -32768, -32768]), n)
    return {
        'all0': from_deltas(small),
        'all1': from_deltas(large),
        'alternating': from_deltas(np.where(index % 2 == 0, small, large)),
        'random': from_deltas(np.where(rng.integers(0, 2, n) == 1, small, large)),
        'lane_edges': from_deltas(np.where(lane_edge, large, small)),
        'wrapping': from_deltas(wrap),
    }


def families(long=True):
    """[(name, samples)] over LENGTHS (and LONG) x key_patterns"""
    rng = np.random.default_rng(16)
    out = []
    for n in LENGTHS + ((LONG,) if long else ()):
        for name, samples in key_patterns(n, rng).items():
            out.append(('n%d_%s' % (n, name), samples))
    return out


def prefixed(stream, n):
    return struct.pack('<I', 2 * n) + bytes(stream)


def mutants(stream, n):
    """[(name, record bytes)] - prefix and payload - each of which must be refused: the stream cut
    by a byte, extended by a byte, an odd prefix, a prefix that claims more keys than there are
    bytes, and a record of three bytes"""
    stream = bytes(stream)
    out = [('added', prefixed(stream + b'\x00', n)),
           ('odd_prefix', struct.pack('<I', 2 * n + 1) + stream),
           ('too_many_keys', struct.pack('<I', 2 * (8 * len(stream) + 8)) + stream),
           ('three_bytes', prefixed(stream, n)[:3])]
    if stream:
        out.append(('cut', prefixed(stream[:-1], n)))
    return out
