"""POD5's 16-bit streamvbyte code on the GPU (`-m gpu`): the stream modes DBH_INFLATE_SVB16 and
DBH_INFLATE_SVB16_ZSTD through ``hip_backend.inflate`` (deepbinner_amd/csrc/dbh_vbz.hip:
svb16_stream; the rules: dbh_svb16_core.h) on the case families of tests/svb16_cases.py.  Expected
values come from the NumPy reference (``pod5_lite.decode_svb16``) alone; everything is compared to
the bit.  Every call's output regions tile its buffer, with stored canary streams between the
streams under test, so that a byte written outside a stream's region shows in a neighbour.
"""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import svb16_cases as sc
from conftest import REPO
from deepbinner_amd import pod5_lite

pytestmark = pytest.mark.gpu

ZLIB, STORED, VBZ, VBZ_ZSTD, ZLIB_SHUFFLE, STORED_SHUFFLE, SVB16, SVB16_ZSTD = range(8)


class Call:
    """The records of one ``inflate`` call and what it must give."""

    def __init__(self):
        self.comp, self.records, self.want, self.status, self.names = bytearray(), [], bytearray(), [], []

    def add(self, name, mode, record, expected, status=0, out_bytes=None):
        """``expected``: the bytes of the stream's output region (its length is out_bytes)"""
        expected = bytes(expected)
        self.records.append((len(self.comp), len(record), len(self.want),
                             len(expected) if out_bytes is None else out_bytes, mode, 0))
        self.comp += record
        self.want += expected
        self.status.append(status)
        self.names.append(name)

    def canary(self, size):
        fill = bytes((0xC0 + k) & 0xFF for k in range(size))
        self.add('canary', STORED, fill, fill)

    def to_residue(self, residue):
        """canary bytes up to the next output offset that is ``residue`` modulo 16"""
        self.canary(16 + (residue - len(self.want)) % 16)

    def run(self, hip):
        streams = np.array(self.records, dtype=hip.INFLATE_STREAM)
        out, status, _ = hip.inflate(np.frombuffer(bytes(self.comp), np.uint8), streams, len(self.want))
        return out, status

    def check(self, hip, result=None):
        out, status = result if result is not None else self.run(hip)
        wrong = [(name, got, want) for name, got, want in zip(self.names, status.tolist(), self.status)
                 if got != want]
        assert not wrong, wrong[:5]
        if out.tobytes() != bytes(self.want):
            want = np.frombuffer(bytes(self.want), np.uint8)
            first = int(np.flatnonzero(out != want)[0])
            inside = [name for name, r in zip(self.names, self.records) if r[2] <= first < r[2] + r[3]]
            raise AssertionError('output differs first at byte %d, in %s' % (first, inside))
        return out, status


def valid(samples):
    """-> (record: prefix + stream, expected bytes by the NumPy reference)"""
    stream = pod5_lite.encode_svb16(samples)
    decoded = pod5_lite.decode_svb16(stream, len(samples))
    assert np.array_equal(decoded, samples)
    return sc.prefixed(stream, len(samples)), decoded.tobytes()


@pytest.fixture(scope='module')
def families():
    """[(name, samples, record, expected bytes)] of every length and key pattern, once"""
    return [(name, samples) + valid(samples) for name, samples in sc.families()]


def test_every_length_and_key_pattern(hip, families):
    """n = 0 .. 2,049 around every lane and step boundary, and 102,400; keys all 0, all 1,
    alternating, random, two-byte values on every lane and step boundary, wrapping deltas"""
    call = Call()
    assert {len(s) for _, s, _, _ in families} == set(sc.LENGTHS) | {sc.LONG}
    for name, samples, record, expected in families:
        call.to_residue(0)
        call.add(name, SVB16, record, expected)
    call.canary(32)
    call.check(hip)


def test_every_offset_residue_and_out_bytes(hip, families):
    """out_offset at every even residue modulo 16 (the 16-byte stores and the single ones), with
    out_bytes below, at and above 2 n: cut, exact, zero-extended"""
    chosen = [f for f in families if f[0] in ('n17_random', 'n1025_alternating', 'n2049_lane_edges',
                                              'n1024_all1', 'n0_all0')]
    assert len(chosen) == 5
    call = Call()
    for name, samples, record, expected in chosen:
        for residue in range(0, 16, 2):
            for delta in (-34, -2, 0, 6, 70):
                size = max(0, len(expected) + delta)
                call.to_residue(residue)
                call.add('%s_r%d_%+d' % (name, residue, delta), SVB16, record,
                         (expected + bytes(70))[:size])
    call.canary(32)
    call.check(hip)


def test_mutants_are_refused_and_their_neighbours_intact(hip, families):
    """one byte cut, one byte added, an odd prefix, a prefix claiming more keys than there are,
    comp_bytes 3: status 1 and zeros, between valid streams that come out to the bit"""
    call, refused = Call(), 0
    for name, samples, record, expected in families:
        if len(samples) > 2049 or name.split('_', 1)[1] not in ('random', 'all1', 'lane_edges'):
            continue
        call.to_residue(0)
        call.add(name, SVB16, record, expected)
        for what, mutant in sc.mutants(record[4:], len(samples)):
            call.add(name + '_' + what, SVB16, mutant, bytes(len(expected)), status=1)
            call.add(name + '_again', SVB16, record, expected)
            refused += 1
    call.canary(32)
    assert refused >= 150
    call.check(hip)


def test_an_odd_out_offset_is_not_written_at_all(hip, families):
    """(a region outside the buffer is refused by the same test in the kernel; ``dbh_inflate``'s own
    argument check keeps such a record from reaching it through this entry)"""
    _, samples, record, expected = next(f for f in families if f[0] == 'n1025_random')
    call = Call()
    call.add('before', SVB16, record, expected)
    call.canary(32)
    streams = np.array(call.records + [(0, len(record), 1, 64, SVB16, 0)], dtype=hip.INFLATE_STREAM)
    out, status, _ = hip.inflate(np.frombuffer(bytes(call.comp), np.uint8), streams, len(call.want))
    assert status.tolist() == [0, 0, 1]
    assert out.tobytes() == bytes(call.want)


@pytest.mark.parametrize('delta', [-3, -1, 1, 5])
def test_an_odd_out_bytes_is_filled_to_the_byte(delta, hip, families):
    """out_bytes odd: whole samples up to it, and the half sample behind them zero - cut, extended,
    and all zeros for a refused stream.  (The region is the buffer's last: the canaries and the
    streams in front of it keep their even offsets.)"""
    _, samples, record, expected = next(f for f in families if f[0] == 'n1025_random')
    size = len(expected) + delta
    want = (expected + bytes(8))[:size - 1] + b'\x00'
    for mutant, status in ((record, 0), (record[:-1], 1)):
        call = Call()
        call.canary(32)
        call.add('even', SVB16, record, expected)
        call.to_residue(2)
        call.add('odd%+d' % delta, SVB16, mutant, want if status == 0 else bytes(size), status=status)
        call.check(hip)


def old_mode_streams(rng):
    """[(name, mode, record, expected)]: one stream of every mode the decoder had"""
    import vbz_fixtures as vf
    out = []
    for mode, name in ((ZLIB, 'zlib'), (STORED, 'stored'), (VBZ, 'vbz'), (VBZ_ZSTD, 'vbz_zstd'),
                       (ZLIB_SHUFFLE, 'zlib_shuffle'), (STORED_SHUFFLE, 'stored_shuffle')):
        s = np.clip(np.rint(np.repeat(rng.normal(450, 80, 400), 8) + rng.normal(0, 8, 3200)), 0, 2047)
        s = s.astype(np.int16)[:int(rng.integers(2500, 3200))]
        raw = s.tobytes()
        shuffled = np.frombuffer(raw, np.uint8).reshape(-1, 2).T.tobytes()
        prefix = struct.pack('<I', len(raw))
        record = {ZLIB: lambda: zlib.compress(raw, 1), STORED: lambda: raw,
                  VBZ: lambda: prefix + vf.streamvbyte(s),
                  VBZ_ZSTD: lambda: prefix + vf.zstd_compress(vf.streamvbyte(s)),
                  ZLIB_SHUFFLE: lambda: prefix + zlib.compress(shuffled, 1),
                  STORED_SHUFFLE: lambda: prefix + shuffled}[mode]()
        out.append((name, mode, record, raw))
    return out


def test_one_call_with_every_mode(hip, families):
    """every existing mode beside the new two: the old modes' outputs and verdicts are those of a
    call without the new streams"""
    import vbz_fixtures as vf
    assert vf.zstd_lib() is not None, 'libzstd.so.1, which the product needs for POD5, is not on this host'
    old = old_mode_streams(np.random.default_rng(7))
    new = [f for f in families if f[0] in ('n2049_random', 'n1025_all1')]
    alone, mixed = Call(), Call()
    for name, mode, record, expected in old:
        alone.to_residue(0)
        alone.add(name, mode, record, expected)
    for k, (name, mode, record, expected) in enumerate(old):
        mixed.to_residue(0)
        mixed.add(name, mode, record, expected)
        fname, samples, frecord, fexpected = new[k % 2]
        mixed.add(fname, SVB16, frecord, fexpected)
        frame = frecord[:4] + vf.zstd_compress(frecord[4:], 1 + 18 * (k % 2))
        mixed.add(fname + '_zstd', SVB16_ZSTD, frame, fexpected)
    alone.canary(32)
    mixed.canary(32)
    out_alone, status_alone = alone.check(hip)
    out_mixed, status_mixed = mixed.check(hip)
    for name, _, _, expected in old:
        a, m = alone.records[alone.names.index(name)], mixed.records[mixed.names.index(name)]
        assert out_alone[a[2]:a[2] + a[3]].tobytes() == out_mixed[m[2]:m[2] + m[3]].tobytes() == expected
        assert status_alone[alone.names.index(name)] == status_mixed[mixed.names.index(name)] == 0


def launch_trip():
    """streams one trip of the kernel's stream loop covers: waves per workgroup x the grid's cap"""
    source = open(os.path.join(REPO, 'deepbinner_amd', 'csrc', 'dbh_vbz.hip')).read()
    waves = int(re.search(r'constexpr int kWaves = (\d+);', source).group(1))
    cap = int(re.search(r'blocks < (\d+) \? blocks : \1', source).group(1))
    return waves * cap


def test_more_streams_than_one_trip_of_the_launch(hip):
    """40,000 streams of 1..64 values, every hundredth one a cut mutant: more than the 32,768 one
    trip of the kernel's loop over the streams takes"""
    n_streams = 40000
    assert launch_trip() == 32768 < n_streams
    rng = np.random.default_rng(8192)
    lengths = rng.integers(1, 65, n_streams)
    ends = np.cumsum(lengths)
    starts = ends - lengths
    total = int(ends[-1])
    deltas = np.where(rng.integers(0, 2, total) == 1, rng.integers(-128, 128, total),
                      rng.integers(-32768, 32768, total))
    sums = np.cumsum(deltas)
    before = np.repeat(np.where(starts > 0, sums[starts - 1], 0), lengths)
    sample_bytes = (sums - before).astype(np.uint16).tobytes()
    d16 = deltas.astype(np.uint16)
    v = ((d16 << np.uint16(1)) ^ (np.uint16(0) - (d16 >> np.uint16(15)))).astype(np.uint16)
    two = v > 0xFF
    take = np.ones((total, 2), dtype=bool)
    take[:, 1] = two
    data = v.astype('<u2').view(np.uint8).reshape(-1, 2)[take].tobytes()
    data_at = np.concatenate([[0], np.cumsum(1 + two.astype(np.int64))]).tolist()
    call = Call()
    for k, (a, b) in enumerate(zip(starts.tolist(), ends.tolist())):
        record = (struct.pack('<I', 2 * (b - a)) + np.packbits(two[a:b], bitorder='little').tobytes() +
                  data[data_at[a]:data_at[b]])
        expected = sample_bytes[2 * a:2 * b]
        if k % 997 == 0:                    # (the streams built here are what the reference reads)
            assert pod5_lite.decode_svb16(record[4:], b - a).tobytes() == expected
        if k % 100 == 99:
            call.add('k%d_cut' % k, SVB16, record[:-1], bytes(len(expected)), status=1)
        else:
            call.add('k%d' % k, SVB16, record, expected)
    call.check(hip)


def test_zstd_frames_of_the_same_streams(hip, families):
    """mode SVB16_ZSTD: every family's stream as a level-1 and as a level-19 frame of libzstd; a
    frame whose svb16 content is a refused mutant has status 1, a damaged frame the zstd stage's
    own status (16 .. 28) - zeros both, neighbours to the bit"""
    import vbz_fixtures as vf
    assert vf.zstd_lib() is not None, 'libzstd.so.1, which the product needs for POD5, is not on this host'
    call = Call()
    damaged = []
    for name, samples, record, expected in families:
        for level in (1, 19):
            if len(samples) > 2049 and level == 19 and not name.endswith('random'):
                continue
            call.to_residue(2 * (len(call.records) % 8))
            frame = vf.zstd_compress(record[4:], level)
            call.add('%s_l%d' % (name, level), SVB16_ZSTD, record[:4] + frame, expected)
        if name.endswith('_random') and 0 < len(samples) <= 2049:
            cut = vf.zstd_compress(record[4:-1], 1)
            call.add(name + '_cut_inside', SVB16_ZSTD, record[:4] + cut, bytes(len(expected)), status=1)
            broken = bytearray(frame)
            broken[0] ^= 0xFF                                   # no zstd magic
            damaged.append(len(call.records))
            call.add(name + '_no_magic', SVB16_ZSTD, record[:4] + bytes(broken), bytes(len(expected)),
                     status=-1)
            call.add(name + '_behind', SVB16_ZSTD, record[:4] + frame, expected)
    call.canary(32)
    assert len(damaged) >= 8
    out, status = call.run(hip)
    for k in damaged:
        assert 16 <= status[k] <= 28, (call.names[k], status[k])
        call.status[k] = int(status[k])
    call.check(hip, (out, status))
