"""The layouts of tests/far_offsets.py do what tests/test_gpu_far_offsets.py relies on: reads and
windows at and across sample 2^31 and 2^32, nothing written twice, something else at every alias of
a checked piece, and a bounded allocation."""
import numpy as np
import pytest

import far_offsets as fo
from far_offsets import B31, B32, BOUNDARIES, KEEP, WINDOW

CASES = [(kind, variant, side) for kind, variant in fo.LAYOUTS for side in ('start', 'end')]


@pytest.fixture(scope='module')
def layouts():
    return {case: fo.make_layout(*case) for case in CASES}


def test_equal_read_lengths():
    for side, length in fo.EQUAL_LENGTH.items():
        assert abs(length - (1 << 20)) < 2048 and length & (length - 1)
        assert fo.TOTAL_SAMPLES // length > 4 * 256 * 4      # every workgroup: more than one group
    assert fo.EQUAL_LENGTH == {'start': 1047042, 'end': 1047553}


@pytest.mark.parametrize('side', ['start', 'end'])
def test_equal_layout_has_a_window_across_each_boundary(layouts, side):
    lay = layouts[('equal', None, side)]
    length = fo.EQUAL_LENGTH[side]
    assert np.array_equal(lay.offsets, np.arange(lay.n_reads + 1, dtype=np.int64) * length)
    assert lay.offsets[0] == 0 and lay.offsets[-1] > B32 and 4096 < lay.n_reads < 4200
    for boundary in BOUNDARIES:
        # the read's first (start) or last (end) window: scan step 0
        hits = [(r, s) for r, s in lay.straddling_windows(boundary) if s == 0]
        assert len(hits) == 1
        a, b = lay.window_slice(hits[0][0], 0)
        assert b - a == WINDOW and a < boundary < b
    assert len(lay.reads_beyond(B31)) > 2000 and len(lay.reads_beyond(B32)) >= 4


@pytest.mark.parametrize('side', ['start', 'end'])
def test_ragged_edge_layout_puts_tiny_reads_on_each_boundary(layouts, side):
    lay = layouts[('ragged', 'edge', side)]
    off, lens = lay.offsets, lay.lengths
    assert off[0] == 0 and off[-1] > B32 and 180 <= lay.n_reads <= 260
    assert set(fo.SMALL) <= set(lens.tolist()) and lens.max() == fo.MAX_READ
    for boundary in BOUNDARIES:
        for at in (boundary - 1, boundary, boundary + 1):
            here = [r for r in range(lay.n_reads) if off[r] == at]
            assert sorted(lens[here].tolist())[:2] == [0, 1], (boundary, at)   # empty, one sample
        below = [r for r in range(lay.n_reads) if 1 < lens[r] < WINDOW and off[r + 1] == boundary - 1]
        above = [r for r in range(lay.n_reads) if 1 < lens[r] < WINDOW and off[r] == boundary + 2]
        assert below and above
        assert not lay.straddling_windows(boundary)      # (a read begins at the boundary)


@pytest.mark.parametrize('side', ['start', 'end'])
def test_ragged_straddle_layout_has_windows_across_each_boundary(layouts, side):
    lay = layouts[('ragged', 'straddle', side)]
    assert lay.offsets[0] == 0 and lay.offsets[-1] > B32 and 180 <= lay.n_reads <= 260
    for boundary in BOUNDARIES:
        hits = lay.straddling_windows(boundary)
        assert len(hits) >= 2 and len({r for r, _ in hits}) == 1
        r = hits[0][0]
        assert lay.lengths[r] == 6144 and lay.offsets[r] < boundary < lay.offsets[r + 1]
        for r, s in hits:
            a, b = lay.window_slice(r, s)
            assert b - a == WINDOW and a < boundary < b


@pytest.mark.parametrize('case', CASES, ids=str)
def test_nothing_is_written_twice_and_every_alias_differs(layouts, case):
    lay = layouts[case]
    extents = lay.written_extents()
    assert extents[0][0] >= 0 and extents[-1][1] <= fo.TOTAL_SAMPLES
    assert all(a[1] <= b[0] for a, b in zip(extents, extents[1:]))
    # what is written is small: pieces of at most KEEP samples, and as much again in decoys
    assert sum(b - a for a, b in extents) <= 2 * lay.n_reads * KEEP
    for at, data in lay.pieces:
        assert len(data) <= KEEP
    report = lay.alias_report()
    far = [r for r in lay.reads_beyond(B31)]
    assert {r for r, *_ in report} == set(far)
    for r, shift, n, written, differ, varied in report:
        assert written == n, (r, shift)                   # the alias is planned, not left to chance
        if len(lay.pieces[r][1]) > 1:
            # (a one-sample window and a flat one normalise to zeros: what tells their alias apart
            # is that it is neither)
            assert differ >= 0.9 * n and (varied or n == 1), (r, shift, n, differ)
    shifts = {shift for _, shift, *_ in report}
    assert shifts == {B31, B32}                           # 2^31 + 2^32 lies below every piece
    # all reads of a layout differ in their scanned windows
    rows = {d.tobytes() for _, d in lay.pieces if len(d) > 1 and d.min() != d.max()}
    assert len(rows) == sum(1 for _, d in lay.pieces if len(d) > 1 and d.min() != d.max())


def test_compact_form_holds_the_same_pieces(layouts):
    lay = layouts[('ragged', 'edge', 'end')]
    samples, offsets = lay.compact()
    assert offsets[-1] + 1 == len(samples) < 2 ** 21
    for r, (at, data) in enumerate(lay.pieces):
        assert np.array_equal(samples[offsets[r]:offsets[r + 1]], data)
        assert len(data) == min(lay.lengths[r], KEEP)
        assert at == (lay.offsets[r + 1] - len(data))


def test_advanced_offsets_begin_beyond_the_boundary(layouts):
    for case, lay in layouts.items():
        k = fo.first_read_beyond(lay)
        assert 0 < k < lay.n_reads - 3 and lay.offsets[k] >= B31 > lay.offsets[k - 1]


def test_planned_peak_allocation():
    assert fo.part_a_peak_bytes(4200) <= fo.MAX_PEAK_BYTES
    assert fo.TOTAL_SAMPLES * 2 == (8 << 30) + (8 << 20)
    refs, queries, _ = fo.dtw_far_plan()
    words = sum(fo.dtw_path_bytes(r, q) for r, q in zip(refs, queries))
    assert 2 ** 32 < words < 8 << 30                      # one launch of the default budget


def test_dtw_plan():
    refs, queries, cut = fo.dtw_far_plan()
    assert len(refs) == 140 and all(c is None for c in cut[:40])
    widths = {(q + 63) // 64 for q in queries[:40] if q <= 1024}
    assert min(widths) <= 4 and any(4 < w <= 8 for w in widths) and max(widths) > 8
    far = queries[40:]
    assert min(far) == 4097 and max(far) == 5000
    assert all(fo.dtw_path_bytes(40000, q) == 5 * (40000 + 63) * 64 * 4 for q in far)
    before = np.cumsum([0] + [fo.dtw_path_bytes(r, q) for r, q in zip(refs, queries)])
    assert before[-1] > B32 and before[-1] // 4 > 1 << 30
    assert sum(1 for b in before[:-1] if b >= B32) >= 10  # pairs that begin beyond 4 GiB


# ---- the streams of dbh_inflate_dev -------------------------------------------------------------
@pytest.fixture(scope='module')
def streams():
    import vbz_fixtures as vf
    return fo.stream_plan(have_zstd=vf.zstd_lib() is not None)


def test_stream_plan_modes_sizes_and_boundaries(streams):
    import vbz_fixtures as vf
    have_zstd = vf.zstd_lib() is not None
    assert len(streams) == (54 if have_zstd else 39)
    for place in range(3):
        group = [s for s in streams if s.out_place == place]
        modes = {s.mode for s in group if s.want is not None}
        assert modes == ({0, 1, 2, 3, 4, 5} if have_zstd else {0, 1, 2, 4, 5})
        assert len([s for s in group if s.want is None]) == (4 if have_zstd else 2)
        assert min(s.out_bytes for s in group) == 2 and max(s.out_bytes for s in group) == 400000
        assert {s.comp_place for s in group} == {0, 1, 2} - {place}
    for boundary, place in ((B31, 1), (B32, 2)):
        across = [s for s in streams if s.out_offset < boundary < s.out_offset + s.out_bytes]
        assert len(across) == 1 and across[0].want is not None and across[0].out_place == place
        # its token slots (4 bytes of workspace per byte of output) cross 2^33 / 2^34
        assert 4 * across[0].out_offset < 4 * boundary < 4 * (across[0].out_offset + 400000)
        group = [s for s in streams if s.out_place == place]
        assert any(s.out_offset + s.out_bytes <= boundary for s in group)
        assert any(s.out_offset >= boundary for s in group)
        comp = [s for s in streams if s.comp_offset < boundary < s.comp_offset + len(s.data)]
        assert len(comp) == 1 and comp[0].comp_place == place
    assert all(s.out_offset % 2 == 0 for s in streams)


def test_stream_regions_keep_apart_and_stay_in_their_places(streams):
    out = sorted((s.out_offset, s.out_offset + s.out_bytes) for s in streams)
    assert all(a[1] + 128 <= b[0] for a, b in zip(out, out[1:]))     # 64 sentinels on either side
    comp = sorted((s.comp_offset, s.comp_offset + len(s.data)) for s in streams)
    assert all(a[1] <= b[0] for a, b in zip(comp, comp[1:]))
    assert out[-1][1] + 64 <= fo.TOTAL_OUT and comp[-1][1] + 64 <= fo.TOTAL_COMP
    for s in streams:
        lo, hi = fo.PLACES[s.out_place]
        assert lo + 64 <= s.out_offset and s.out_offset + s.out_bytes + 64 <= hi
        lo, hi = fo.PLACES[s.comp_place]
        assert lo <= s.comp_offset and s.comp_offset + len(s.data) + 64 <= hi
    # a place less 2^31 or 2^32 lies inside another place: every alias is uploaded and read back
    for lo, hi in fo.PLACES[1:]:
        for shift in (B31, B32):
            if hi - shift > 0:
                a, b = max(lo - shift, 0), hi - shift
                assert fo.place_of(a) == fo.place_of(b - 1)


def test_every_alias_of_a_far_stream_differs(streams):
    places = fo.comp_places(streams)

    def comp_at(a, b):
        k = fo.place_of(a)
        return places[k][a - fo.PLACES[k][0]:b - fo.PLACES[k][0]]

    want_out = {s.out_offset: s for s in streams}
    checked = 0
    for s in streams:
        for shift in (B31, B32):
            a, b = s.comp_offset - shift, s.comp_offset - shift + len(s.data)
            if a >= 0:
                other = comp_at(a, b)
                assert len(other) == len(s.data)
                differ = (other != np.frombuffer(s.data, dtype=np.uint8)).mean()
                assert differ > 0.5 or (len(s.data) < 64 and differ > 0), (s.name, shift)
                checked += 1
            # the alias of the output region: sentinels, or another stream's other bytes
            a, b = s.out_offset - shift, s.out_offset - shift + s.out_bytes
            if a >= 0:
                for o in streams:
                    lo, hi = max(a, o.out_offset), min(b, o.out_offset + o.out_bytes)
                    if lo < hi:
                        # (a refused stream leaves zeros: its alias may only meet a valid one)
                        assert s.want is not None or o.want is not None, (s.name, o.name)
                        theirs = (o.want or bytes(o.out_bytes))[lo - o.out_offset:hi - o.out_offset]
                        mine = (s.want or bytes(s.out_bytes))[lo - a:hi - a]
                        assert theirs != mine, (s.name, o.name)
    assert checked >= len(streams) // 3


def test_valid_streams_decode_on_the_host(streams):
    import struct
    import zlib
    import shuffle_fixtures as sf
    from deepbinner_amd import fast5_native
    for s in streams:
        if s.want is None:
            continue
        n = s.out_bytes // 2
        if s.mode == fo.ZLIB:
            got = zlib.decompress(s.data)
        elif s.mode == fo.STORED:
            got = s.data
        elif s.mode in (fo.VBZ, fo.VBZ_ZSTD):
            got = fast5_native.vbz_decode(s.data, (0, 2, 1, 1 if s.mode == fo.VBZ_ZSTD else 0),
                                          n).tobytes()
        else:
            assert struct.unpack('<I', s.data[:4])[0] == s.out_bytes
            body = s.data[4:] if s.mode == fo.STORED_SHUFFLE else zlib.decompress(s.data[4:])
            got = sf.unshuffle(body).tobytes()
        assert got == s.want, s.name


def test_planned_peak_of_the_stream_launch():
    # the workspace: four bytes per byte of output and a record per stream
    assert fo.inflate_peak_bytes(4 * fo.TOTAL_OUT + (64 << 20)) <= fo.MAX_PEAK_BYTES
    where, comp_bytes, out_bytes = fo.compact_stream_layout(fo.stream_plan(have_zstd=False))
    assert comp_bytes < 1 << 22 and out_bytes < 1 << 22
