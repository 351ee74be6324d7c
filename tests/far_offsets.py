"""Layouts that put reads and DTW path words beyond 2^31 elements / 2^32 bytes of a buffer that is
really allocated from byte 0 (a plain module, not a conftest: tests import it).

A layout is a sparse description of a huge sample buffer: the ``offsets`` of its reads and the few
``pieces`` (position, int16 samples) that a correct kernel reads - the scanned end of every read.
Besides them only ``decoys`` are uploaded: other samples in the places a wrong address would hit.
The same pieces packed back to back are the ``compact`` form: the same windows at small offsets,
whose results the far results must equal bit for bit.  ``stream_plan`` does the same for the
compressed and the output buffer of dbh_inflate_dev, ``dtw_far_plan`` for the DTW's path words.

An address whose upper half is dropped (or that is computed modulo 2^31 / 2^32) lands on an
*alias* of the right place, inside the allocation.  ``alias_report`` says what the layout puts at
every alias of every checked piece; tests/test_far_offsets.py asserts that it differs.
"""
import os

import numpy as np

from conftest import GOLD

B31 = 1 << 31
B32 = 1 << 32
BOUNDARIES = (B31, B32)
ALIAS_SHIFTS = (B31, B32, B31 + B32)

WINDOW = 1024
SCAN = 6144
KEEP = SCAN + WINDOW // 2          # samples any window of a scan of 6,144 can touch
TOTAL_SAMPLES = B32 + (1 << 22)    # int16 samples in the far buffer: 8 GiB + 8 MiB
MAX_PEAK_BYTES = 26 << 30
MAX_READ = 1 << 26
NEAR = 2 * SCAN                    # "near a boundary": compared with the fp64 oracle too


# ---- content --------------------------------------------------------------------------------
_pool = None


def signal_pool():
    """[n, KEEP] int16: the head and the tail of every golden signal that is long enough, and
    seeded squiggles."""
    global _pool
    if _pool is None:
        reads = np.load(os.path.join(GOLD, 'reads.npz'))
        rows = []
        for samples, offsets in ((reads['samples'], reads['offsets']),
                                 (reads['multi_samples'], reads['multi_offsets'])):
            for i in range(len(offsets) - 1):
                s = samples[offsets[i]:offsets[i + 1]]
                if len(s) >= KEEP:
                    rows.append(s[:KEEP])
                    rows.append(s[len(s) - KEEP:])
        rng = np.random.default_rng(2031)
        for _ in range(16):
            levels = rng.normal(500.0, 90.0, size=KEEP // 5 + 1)
            sq = np.repeat(levels, rng.integers(5, 12, size=len(levels)))[:KEEP]
            rows.append(np.clip(sq + rng.normal(0.0, 8.0, KEEP), 0, 2047))
        _pool = np.stack([np.asarray(r, dtype=np.int16) for r in rows])
    return _pool


def read_content(seed, r, n):
    """The ``n`` scanned samples of read ``r``: a pool signal, perturbed so that no two reads of a
    layout share a window."""
    pool = signal_pool()
    rng = np.random.default_rng([seed, r])
    base = np.resize(pool[(r * 7 + seed) % len(pool)], n).astype(np.int32)
    return (base + rng.integers(-6, 7, size=n)).astype(np.int16)


# ---- layouts --------------------------------------------------------------------------------
class Layout:
    """offsets [n + 1] int64 into a buffer of TOTAL_SAMPLES; ``pieces[r]`` = (position, samples)
    of the part of read r that side ``side`` scans (the whole read if it is short)."""

    def __init__(self, name, side, lengths, seed, flat=()):
        self.name, self.side = name, side
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
        np.cumsum(self.lengths, out=self.offsets[1:])
        assert self.offsets[-1] <= TOTAL_SAMPLES
        self.pieces = []
        for r, n in enumerate(self.lengths):
            n = int(n)
            k = min(n, KEEP)
            data = np.full(k, 480, np.int16) if r in flat else read_content(seed, r, k)
            at = int(self.offsets[r]) if side == 'start' else int(self.offsets[r + 1]) - k
            self.pieces.append((at, data))
        self._plan_decoys(seed + 500)

    @property
    def n_reads(self):
        return len(self.lengths)

    def compact(self):
        """(samples, offsets): the pieces back to back - the same windows at small offsets."""
        offsets = np.zeros(self.n_reads + 1, dtype=np.int64)
        np.cumsum([len(d) for _, d in self.pieces], out=offsets[1:])
        samples = np.concatenate([d for _, d in self.pieces] + [np.zeros(1, np.int16)])
        return samples, offsets

    def signals(self, reads):
        return [self.pieces[r][1] for r in reads]

    def window_slice(self, r, step, input_size=WINDOW):
        """[a, b) in the far buffer of scan step ``step`` of read r."""
        half = input_size // 2
        base, n = int(self.offsets[r]), int(self.lengths[r])
        if self.side == 'start':
            return base + min(step * half, n), base + min(step * half + input_size, n)
        return base + max(n - step * half - input_size, 0), base + max(n - step * half, 0)

    def reads_beyond(self, boundary):
        """Reads whose scanned piece has samples at or beyond ``boundary``."""
        return [r for r, (at, d) in enumerate(self.pieces) if len(d) and at + len(d) > boundary]

    def windows_beyond(self, boundary, scan=SCAN, input_size=WINDOW):
        n = 0
        for r in range(self.n_reads):
            for s in range(scan // (input_size // 2)):
                a, b = self.window_slice(r, s, input_size)
                n += b > a and b > boundary
        return n

    def reads_near(self, boundary, reach=NEAR):
        """Reads whose scanned piece lies within ``reach`` samples of ``boundary`` (empty reads by
        their offset)."""
        return [r for r, (at, d) in enumerate(self.pieces)
                if at - reach <= boundary <= at + len(d) + reach]

    def straddling_windows(self, boundary, scan=SCAN):
        """(read, step) whose slice holds samples on both sides of ``boundary``."""
        out = []
        for r in self.reads_near(boundary, KEEP):
            for s in range(scan // (WINDOW // 2)):
                a, b = self.window_slice(r, s)
                if a < boundary < b:
                    out.append((r, s))
        return out

    def uploads(self):
        """Everything that is written to the far buffer: the pieces, then the decoys."""
        return [p for p in self.pieces if len(p[1])] + self.decoys

    def written_extents(self):
        return sorted((at, at + len(d)) for at, d in self.uploads())

    def content_at(self, a, b):
        """(values int32 [b - a], written bool [b - a]) of what the layout uploads in [a, b)."""
        values = np.zeros(b - a, dtype=np.int32)
        written = np.zeros(b - a, dtype=bool)
        i = max(int(np.searchsorted(self._start_list, a, side='right')) - 1, 0)
        while i < len(self._order) and self._order[i][0] < b:
            at, d = self._order[i]
            lo, hi = max(at, a), min(at + len(d), b)
            if lo < hi:
                values[lo - a:hi - a] = d[lo - at:hi - at]
                written[lo - a:hi - a] = True
            i += 1
        return values, written

    def _index(self):
        self._order = sorted(self.uploads(), key=lambda p: p[0])
        self._start_list = np.array([p[0] for p in self._order], dtype=np.int64)

    def aliases(self):
        """(read, shift, [a, b)) of every alias inside the buffer of every piece that has samples
        at or beyond 2^31; b - a is the piece's length unless the alias begins below sample 0."""
        for r, (at, d) in enumerate(self.pieces):
            if len(d) and at + len(d) > B31:
                for shift in ALIAS_SHIFTS:
                    if at + len(d) - shift > 0:
                        yield r, shift, max(at - shift, 0), at + len(d) - shift

    def _plan_decoys(self, seed):
        """Other samples wherever an alias of a far piece would otherwise stay unwritten (the
        middle of a long read, which no window reaches)."""
        self.decoys = []
        self._index()
        for pass_shift in ALIAS_SHIFTS:
            fresh = []
            for r, shift, a, b in self.aliases():
                if shift != pass_shift:
                    continue
                _, written = self.content_at(a, b)
                edges = np.flatnonzero(np.diff(np.concatenate([[True], written, [True]])))
                for lo, hi in zip(edges[::2], edges[1::2]):
                    fresh.append((a + int(lo), read_content(seed + shift % 1000 + 1, r,
                                                            int(hi - lo))))
            self.decoys += fresh
            self._index()

    def alias_report(self):
        """(read, shift, samples of the alias, how many of them the layout writes, how many of
        those differ from the piece's sample in the same place, whether the alias holds more than
        one level) for every alias."""
        out = []
        for r, shift, a, b in self.aliases():
            at, d = self.pieces[r]
            values, written = self.content_at(a, b)
            mine = d[a + shift - at:b + shift - at].astype(np.int32)
            out.append((r, shift, b - a, int(written.sum()),
                        int((written & (values != mine)).sum()),
                        bool(len(values) > 1 and values.min() != values.max())))
        return out


def _equal_length(side):
    """The largest L < 2^20, no power of two, with a read whose first ('start') or last ('end')
    window holds sample 2^31 strictly inside it, and another such read for 2^32."""
    for length in range((1 << 20) - 1, (1 << 20) - 20000, -1):
        ok = True
        for boundary in BOUNDARIES:
            r = boundary % length
            # start: read k = boundary // L begins r samples below the boundary;
            # end: read k - 1 ends L - r samples above it
            inside = (0 < r < WINDOW) if side == 'start' else (0 < length - r < WINDOW)
            ok = ok and inside
        if ok:
            return length
    raise AssertionError('no read length puts a window across both boundaries')


EQUAL_LENGTH = {'start': _equal_length('start'), 'end': _equal_length('end')}


def equal_layout(side):
    length = EQUAL_LENGTH[side]
    n = TOTAL_SAMPLES // length
    return Layout('equal', side, [length] * n, seed=11 if side == 'start' else 12)


SMALL = (0, 1, 300, 511, 1024, 1025, 6144)
LONG = (MAX_READ, 40000, MAX_READ - 7, (1 << 25) + 3, (1 << 25) - 11, (1 << 26) - (1 << 20) - 1,
        (1 << 24) + 5)
# read lengths around a boundary B, from B + CLUSTER_START['edge']: a zero-length and a one-sample
# read just below, exactly at and just above B, short reads on either side
# (the flat read stands elsewhere at 2^32 than at 2^31, or it would be its own alias: a flat window
# normalises to zeros whatever its level)
EDGE_CLUSTER = {B31: (6144, 1025, 511, 0, 1, 0, 1, 0, 1, 300, 1024, 511, 6144),
                B32: (6144, 1025, 511, 0, 1, 0, 1, 0, 1, 511, 300, 1024, 6144)}
EDGE_START = -(6144 + 1025 + 511 + 1)
# ... and with one read of 6,144 samples lying across B instead
STRADDLE_CLUSTER = {B31: (1025, 300, 6144, 511, 1, 0, 1024),
                    B32: (300, 1025, 6144, 511, 1, 0, 1024)}
STRADDLE_START = -(1025 + 300 + 3000)


def ragged_layout(side, variant):
    """About 200 reads of lengths 0 .. 2^26 from sample 0 to beyond 2^32.  ``variant`` 'edge':
    read boundaries at B - 1, B and B + 1 for B = 2^31 and 2^32, with a zero-length, a one-sample
    and a short read in each place; 'straddle': a read of 6,144 samples across each B (no layout
    can have both: a read that starts at B ends every read below it)."""
    cluster, start = (EDGE_CLUSTER, EDGE_START) if variant == 'edge' else \
        (STRADDLE_CLUSTER, STRADDLE_START)
    lengths, flat, pos, i = [], set(), 0, 0

    def add(n):
        nonlocal pos
        if n == 300:
            flat.add(len(lengths))
        lengths.append(n)
        pos += n

    for boundary in BOUNDARIES:
        target = boundary + start
        while target - pos > MAX_READ + 7000:
            add(SMALL[i % len(SMALL)])
            add(LONG[i % len(LONG)])
            i += 1
        if target - pos > MAX_READ:
            add(7000)
        add(target - pos)
        for n in cluster[boundary]:
            add(n)
    add(SMALL[3])
    add(min(TOTAL_SAMPLES - pos, 2 * KEEP + 17))
    seed = {'edge': 21, 'straddle': 23}[variant] + (side == 'end')
    return Layout('ragged-' + variant, side, lengths, seed, flat)


LAYOUTS = [('equal', None), ('ragged', 'edge'), ('ragged', 'straddle')]


def make_layout(kind, variant, side):
    return equal_layout(side) if kind == 'equal' else ragged_layout(side, variant)


def first_read_beyond(layout, boundary=B31):
    """The first read that starts at or beyond ``boundary``: where an advanced offsets pointer
    begins."""
    return int(np.searchsorted(layout.offsets[:-1], boundary, side='left'))


def part_a_peak_bytes(n_reads):
    """Device bytes of Part A at its peak: the far samples, the compact samples, offsets, the
    normalised windows of both forms, results and workspace."""
    steps = SCAN // (WINDOW // 2)
    windows = 2 * n_reads * steps * WINDOW * 4
    return (TOTAL_SAMPLES * 2 + (n_reads * KEEP + 1) * 2 + 2 * (n_reads + 1) * 8 + windows
            + 4 * n_reads * 13 * 4 + 4 * n_reads * 4 + 2 * (n_reads * steps * 13 * 4 + 256))


# ---- DTW ------------------------------------------------------------------------------------
DTW_LANES = 64
DTW_PANEL = 1024                   # query columns per panel


def dtw_path_bytes(ref_len, query_len):
    """Direction words of one pair: panels x (R + 63) steps x 64 lanes x 4 bytes
    (include/deepbinner_dtw.h)."""
    panels = -(-query_len // DTW_PANEL)
    return panels * (ref_len + DTW_LANES - 1) * DTW_LANES * 4


def dtw_far_plan(seed=31, n_small=40, n_far=100, ref_len=40000):
    """(ref lengths, query lengths, where each far query is cut): 40 small pairs of all three
    lane widths, then 100 pairs of five panels each."""
    rng = np.random.default_rng(seed)
    small_q = [1, 3, 64, 200, 256, 257, 400, 512, 513, 700, 1000, 1024, 1025, 1500]
    refs, queries, cut = [], [], []
    for k in range(n_small):
        queries.append(small_q[k % len(small_q)])
        refs.append(int(rng.integers(1, 600)))
        cut.append(None)
    for k in range(n_far):
        q = (4097, 5000)[k] if k < 2 else int(rng.integers(4097, 5001))
        queries.append(q)
        refs.append(ref_len)
        cut.append(int(rng.integers(1, ref_len - q)))
    return refs, queries, cut


# ---- streams of dbh_inflate_dev ---------------------------------------------------------------
ZLIB, STORED, VBZ, VBZ_ZSTD, ZLIB_SHUFFLE, STORED_SHUFFLE = 0, 1, 2, 3, 4, 5
TOTAL_OUT = B32 + (1 << 21)        # bytes of the output buffer; the workspace is 4 x as much
TOTAL_COMP = B32 + (1 << 21)
SENTINEL = 0xA5
PLACE_BYTES = 1 << 22              # what is uploaded and read back around 0, 2^31 and 2^32
# [begin, end) of the three places of either buffer: everything a stream reads or writes, and
# every alias of it, lies inside them (a place minus 2^31 or 2^32 is inside another place)
PLACES = ((0, PLACE_BYTES), (B31 - PLACE_BYTES // 2, B31 + PLACE_BYTES // 2),
          (B32 - PLACE_BYTES // 2, B32 + PLACE_BYTES // 2))
# (samples, mode) of the valid streams of each place: 2 bytes .. 400,000 bytes of output
STREAM_KINDS = ((1, ZLIB), (1000, ZLIB), (200000, ZLIB), (3, STORED), (50000, STORED),
                (5, VBZ), (27000, VBZ), (200, VBZ_ZSTD), (4000, VBZ_ZSTD), (100000, VBZ_ZSTD),
                (2, ZLIB_SHUFFLE), (60000, ZLIB_SHUFFLE), (7, STORED_SHUFFLE),
                (30000, STORED_SHUFFLE))
REFUSED_KINDS = ('damaged_deflate', 'zstd_literals_header', 'streamvbyte_data_short',
                 'odd_shuffle_size')


class Stream:
    def __init__(self, name, data, mode, out_bytes, want, content=None):
        self.name, self.data, self.mode, self.out_bytes = name, bytes(data), mode, out_bytes
        self.want = want               # the bytes of its output region; None: refused, zeros
        self.content = content         # mode 3: what the zstd stage leaves in the workspace
        self.comp_offset = self.out_offset = None
        self.out_place = self.comp_place = None


def _encode(samples, mode, level):
    import struct
    import zlib
    import shuffle_fixtures as sf
    import vbz_fixtures as vf
    raw = samples.astype('<i2').tobytes()
    prefix = struct.pack('<I', len(raw))
    if mode == ZLIB:
        return zlib.compress(raw, level), None
    if mode == STORED:
        return raw, None
    packed = vf.streamvbyte(samples)
    if mode == VBZ:
        return prefix + packed, None
    if mode == VBZ_ZSTD:
        return prefix + vf.zstd_compress(packed, level), packed
    if mode == ZLIB_SHUFFLE:
        return prefix + zlib.compress(sf.shuffle(samples), level), None
    return prefix + sf.shuffle(samples), None


def _refused(kind, seed):
    """(bytes, mode, out_bytes) of a stream that its decoder must refuse, from the generators of
    the decoders' own tests."""
    import struct
    import zlib
    import shuffle_fixtures as sf
    import zstd_cases as zc
    samples = zc.random_walk(3000, seed)
    if kind == 'damaged_deflate':
        return sf.damage_deflate(zlib.compress(samples.tobytes(), 1)), ZLIB, 6000
    if kind == 'zstd_literals_header':
        frames = [f for f in zc.valid_frames(sizes=(4000,), levels=(1,)) if f[0] == 'walk_4000_l1']
        lib = zc.lib()
        for label, frame in zc.mutants(frames, seed=seed, random_per_frame=0):
            if ':literals_header@' in label and zc.zstd_decompress(frame, 1 << 16)[0] is None:
                return struct.pack('<I', 8000) + frame, VBZ_ZSTD, 8000
        raise AssertionError('no literals header whose damage libzstd refuses ({})'.format(lib))
    if kind == 'streamvbyte_data_short':
        return dict(zc.damaged_vbz_chunks(seed))['data_short'], VBZ_ZSTD, 6000
    assert kind == 'odd_shuffle_size'
    return struct.pack('<I', 5999) + sf.shuffle(samples)[:5999], STORED_SHUFFLE, 6000


def stream_plan(have_zstd=True):
    """About 60 streams of every mode, valid and refused, in three groups: their outputs around
    byte 0, around and across byte 2^31 and around and across byte 2^32 of the output buffer; their
    compressed bytes dealt over the same three places of the compressed buffer, independently."""
    import zstd_cases as zc
    streams = []
    for place in range(3):
        valid, refused = [], []
        for k, (n, mode) in enumerate(STREAM_KINDS):
            if mode == VBZ_ZSTD and not have_zstd:
                continue
            samples = zc.random_walk(n, seed=1000 * place + k + 1)
            data, content = _encode(samples, mode, (1, 6, 9)[k % 3])
            valid.append(Stream('{}:{}x{}'.format(place, mode, n), data, mode, 2 * n,
                                samples.astype('<i2').tobytes(), content))
        for k, kind in enumerate(REFUSED_KINDS):
            if 'zstd' in kind or 'streamvbyte' in kind:
                if not have_zstd:
                    continue
            data, mode, out_bytes = _refused(kind, seed=50 + 10 * place + k)
            refused.append(Stream('{}:{}'.format(place, kind), data, mode, out_bytes, None))
        # the refused streams stand elsewhere in every group: behind the valid ones, in front of
        # them, among them - the zeros of one are never at an alias of another's
        group = (valid + refused, refused + valid, valid[:7] + refused + valid[7:])[place]
        for s in group:
            s.out_place = place
        streams += group
    # a stream's compressed bytes stand in another place than its output, in another order
    for i, s in enumerate(streams):
        s.comp_place = (s.out_place + 1 + i % 2) % 3
    _lay_out(streams, 'out_place', 'out_offset', lambda s: s.out_bytes, align=2, gap=130)
    _lay_out(streams[::-1], 'comp_place', 'comp_offset', lambda s: len(s.data), align=1, gap=7)
    return streams


def _lay_out(streams, place_of, offset_of, size_of, align, gap):
    """Regions one after the other with gaps; the group of place 1 (2) is moved so that the middle
    of its largest region is byte 2^31 (2^32)."""
    for place in range(3):
        group = [s for s in streams if getattr(s, place_of) == place]
        at, rel = 192, []
        for s in group:
            at = -(-at // align) * align
            rel.append(at)
            at += size_of(s) + gap
        shift = 0
        if place:
            big = max(range(len(group)), key=lambda i: size_of(group[i]))
            shift = (B31, B32)[place - 1] - rel[big] - (size_of(group[big]) // 2 // align) * align
        for s, r in zip(group, rel):
            setattr(s, offset_of, r + shift)
        lo, hi = PLACES[place]
        assert lo <= rel[0] + shift - 64 and at + shift + 64 <= hi, (place, rel[0] + shift, at)


def compact_stream_layout(streams):
    """[(comp_offset, out_offset)] of the same streams in a small launch, and its sizes."""
    comp_at, out_at, where = 0, 64, []
    for k, s in enumerate(streams):
        out_at += 2 * (k % 8) + 64
        where.append((comp_at, out_at))
        comp_at += len(s.data)
        out_at += s.out_bytes
    return where, comp_at, out_at + 64


def place_of(offset):
    for k, (lo, hi) in enumerate(PLACES):
        if lo <= offset < hi:
            return k
    raise AssertionError(offset)


def comp_places(streams, seed=77):
    """The three places of the compressed buffer as they are uploaded: other bytes everywhere, the
    streams in them."""
    rng = np.random.default_rng(seed)
    places = [rng.integers(0, 256, size=hi - lo, dtype=np.uint8) for lo, hi in PLACES]
    for s in streams:
        lo = PLACES[s.comp_place][0]
        places[s.comp_place][s.comp_offset - lo:s.comp_offset - lo + len(s.data)] = \
            np.frombuffer(s.data, dtype=np.uint8)
    return places


def inflate_peak_bytes(workspace_bytes):
    return TOTAL_OUT + TOTAL_COMP + workspace_bytes
