"""64-bit addressing on the device: reads, and DTW path words, that lie beyond 2^31 elements and
2^32 bytes of their buffers (layouts: tests/far_offsets.py, checked by tests/test_far_offsets.py).

Every far buffer is really allocated from byte 0, so a truncated address lands inside it, on an
alias that holds other data: a wrong address fails a comparison, it does not fault.  Only the
samples a correct kernel reads (and the decoys at their aliases) are uploaded.  What a far result
must equal, bit for bit, is the result of the same content at small offsets through the same entry
point ("a window's result does not depend on the chunk, the batch or the stream it travels in");
the reads next to a boundary are held to the fp64 oracle as well."""
import ctypes
import time

import numpy as np
import pytest

import far_offsets as fo
from far_offsets import B31, B32, BOUNDARIES, SCAN, TOTAL_SAMPLES, WINDOW
from general_fixtures import ENDS, STARTS, geometry
from oracle_compare import assert_log_close, oracle_call_batch
from test_gpu_general_models import compare_calls

pytestmark = pytest.mark.gpu

CASES = [(kind, variant, side) for kind, variant in fo.LAYOUTS for side in ('start', 'end')]
MODEL = {'start': STARTS, 'end': ENDS}
_layouts = {}
_peak = {'now': 0, 'peak': 0}


def layout_of(case):
    if case not in _layouts:
        _layouts[case] = fo.make_layout(*case)
    return _layouts[case]


def allocate(hip, nbytes):
    """hip.DeviceBuffer, counted; out of memory is the one reason to skip."""
    try:
        buf = hip.DeviceBuffer(nbytes)
    except hip.HipBackendError as e:
        if 'out of device memory' in str(e):
            pytest.skip('dbh_malloc: out of device memory for {} bytes'.format(nbytes))
        raise
    _peak['now'] += nbytes
    _peak['peak'] = max(_peak['peak'], _peak['now'])
    return buf


def allocate_all(hip, *sizes):
    """Several buffers; if one cannot be had, those before it are given back before the skip."""
    got = []
    try:
        for nbytes in sizes:
            got.append(allocate(hip, nbytes))
    except BaseException:
        release(*got)
        raise
    return got


def release(*buffers):
    for buf in buffers:
        if buf.ptr:
            _peak['now'] -= buf.nbytes
        buf.free()


def upload_at(hip, buf, byte_offset, array):
    array = np.ascontiguousarray(array)
    assert 0 <= byte_offset and byte_offset + array.nbytes <= buf.nbytes
    hip.check(hip.load_library().dbh_memcpy_h2d(buf.ptr + byte_offset, array.ctypes.data,
                                                array.nbytes, None), 'dbh_memcpy_h2d')


def uploaded(hip, array):
    buf = allocate(hip, max(np.ascontiguousarray(array).nbytes, 1))
    buf.upload(array)
    return buf


class Staged:
    """One layout in the far buffer, and its compact form beside it."""

    def __init__(self, hip, far, case):
        self.case, self.layout, self.far = case, layout_of(case), far
        lay = self.layout
        for at, data in lay.uploads():
            upload_at(hip, far, 2 * at, data)
        hip.synchronize()
        self.far_offsets = uploaded(hip, lay.offsets)
        samples, offsets = lay.compact()
        self.compact_samples = uploaded(hip, samples)
        self.compact_offsets = uploaded(hip, offsets)
        self.n = lay.n_reads
        self.side = lay.side

    def free(self):
        release(self.far_offsets, self.compact_samples, self.compact_offsets)


_holder = {'buf': None, 'staged': None}


def drop_far_samples():
    """Free the sample buffer and what is staged beside it (the stream tests need the memory);
    ``stage`` allocates it again if a sample test runs afterwards."""
    if _holder['staged'] is not None:
        _holder['staged'].free()
        _holder['staged'] = None
    if _holder['buf'] is not None:
        release(_holder['buf'])
        _holder['buf'] = None


@pytest.fixture(scope='module')
def far_samples(hip):
    """2^32 + 2^22 int16 samples from byte 0, allocated by the first ``stage``."""
    yield _holder
    drop_far_samples()
    assert _peak['now'] == 0 and _peak['peak'] <= fo.MAX_PEAK_BYTES
    print('peak device bytes of the module\'s own buffers: {}'.format(_peak['peak']))


def stage(hip, holder, case):
    if holder['buf'] is None:
        holder['buf'] = allocate(hip, 2 * TOTAL_SAMPLES)
    if holder['staged'] is None or holder['staged'].case != case:
        if holder['staged'] is not None:
            holder['staged'].free()
            holder['staged'] = None
        holder['staged'] = Staged(hip, holder['buf'], case)
    return holder['staged']


@pytest.fixture(scope='module', params=CASES, ids=lambda c: '-'.join(str(x) for x in c if x))
def staged(request, hip, far_samples):
    """(a callable: the layout is staged when the test runs, whatever ran in between)"""
    return lambda: stage(hip, far_samples, request.param)


@pytest.fixture(scope='module', params=[c for c in CASES if c[0] == 'equal'],
                ids=lambda c: c[2])
def staged_equal(request, hip, far_samples):
    """(a callable: the layout is staged when the test runs, whatever ran in between)"""
    return lambda: stage(hip, far_samples, request.param)


@pytest.fixture(scope='module', params=[c for c in CASES if c[0] == 'ragged'],
                ids=lambda c: '-'.join(c[1:]))
def staged_ragged(request, hip, far_samples):
    """(a callable: the layout is staged when the test runs, whatever ran in between)"""
    return lambda: stage(hip, far_samples, request.param)


class Runner:
    """classify_dev / classify_batched_dev of one model into fresh result buffers."""

    def __init__(self, hip, model, n, scan, side):
        self.hip, self.model, self.n, self.scan, self.side = hip, model, n, scan, side
        self.classes = model.n_classes
        self.probs, self.calls, self.work = allocate_all(
            hip, n * self.classes * 4, n * 4, max(model.workspace_bytes(n, scan), 1))

    def _results(self, n, run):
        self.probs.upload(np.full((n, self.classes), -1.0, np.float32))
        self.calls.upload(np.full(n, -7, np.int32))
        run()
        self.hip.synchronize()
        return (self.probs.download((n, self.classes), np.float32),
                self.calls.download((n,), np.int32))

    def whole(self, samples, offsets, first=0):
        n = self.n - first
        return self._results(n, lambda: self.model.classify_dev(
            samples.ptr, offsets.ptr + 8 * first, n, self.side, self.scan, 0.5, self.probs.ptr,
            self.calls.ptr, self.work.ptr))

    def batched(self, samples, offsets, batch):
        return self._results(self.n, lambda: self.model.classify_batched_dev(
            samples.ptr, offsets.ptr, self.n, batch, self.side, self.scan, 0.5, self.probs.ptr,
            self.calls.ptr))

    def free(self):
        release(self.probs, self.calls, self.work)


def assert_same_bits(got, want, layout, what, first=0):
    """Probabilities and calls of the far reads == those of the same reads at small offsets."""
    (probs, calls), (w_probs, w_calls) = got, want
    assert probs.shape == w_probs.shape and calls.shape == w_calls.shape
    bad = np.flatnonzero((probs.view(np.uint32) != w_probs.view(np.uint32)).any(axis=1)
                         | (calls != w_calls))
    if len(bad):
        r = int(bad[0]) + first
        raise AssertionError(
            '{}: {} of {} reads differ from the same reads at small offsets; the first is read {} '
            'at sample offset {} (2^31 {:+d}, 2^32 {:+d}), length {}: far {} call {}, compact {} '
            'call {}'.format(what, len(bad), len(calls), r, int(layout.offsets[r]),
                             int(layout.offsets[r]) - B31, int(layout.offsets[r]) - B32,
                             int(layout.lengths[r]), probs[bad[0]][:4], calls[bad[0]],
                             w_probs[bad[0]][:4], w_calls[bad[0]]))


def sweep(hip, model, st, scan, what):
    """classify_dev from read 0 and from a read beyond 2^31, classify_batched_dev in batches of 1,
    7 and 256: all equal to the compact run.  -> the far (probs, calls)."""
    lay = st.layout
    run = Runner(hip, model, st.n, scan, st.side)
    try:
        want = run.whole(st.compact_samples, st.compact_offsets)
        assert (want[1] >= 0).all() and np.isfinite(want[0]).all() and (want[0] >= 0).all()
        got = run.whole(st.far, st.far_offsets)
        assert_same_bits(got, want, lay, what + ' classify_dev')
        first = fo.first_read_beyond(lay)
        assert lay.offsets[first] >= B31
        tail = run.whole(st.far, st.far_offsets, first)
        assert_same_bits(tail, (want[0][first:], want[1][first:]), lay,
                         what + ' classify_dev from read {}'.format(first), first)
        for batch in (1, 7, 256):
            assert_same_bits(run.batched(st.far, st.far_offsets, batch), want, lay,
                             what + ' classify_batched_dev batch {}'.format(batch))
        return got
    finally:
        run.free()


def boundary_reads(lay):
    return sorted({r for b in BOUNDARIES for r in lay.reads_near(b)})


def against_the_oracle(weights, lay, got, scan, what):
    """The reads next to a boundary against the fp64 oracle, as tests/test_gpu_log_space.py
    compares a whole batch."""
    reads = boundary_reads(lay)
    assert reads and all(any(r in lay.reads_near(b) for r in reads) for b in BOUNDARIES)
    probs, calls = got[0][reads], got[1][reads]
    o_calls, o_probs, scale = oracle_call_batch(weights, lay.signals(reads), scan, 0.5, lay.side)
    compare_calls(calls, probs, o_calls, o_probs)
    assert_log_close(probs, probs=o_probs, scale=scale, what=what)


# ---- Part A: sample offsets -------------------------------------------------------------------
@pytest.mark.parametrize('scan', [512, SCAN])
def test_persistent_classify_beyond_4g_samples(hip, hip_models, weights, staged, scan):
    """scan 512: the fused finish, one launch; 6144: the merge kernel.  With > 4 x 256 x 4 reads
    every workgroup takes several groups, so the cold fetch, the steady-state prefetch and the
    staging fetch all meet offsets beyond 2^31 and 2^32."""
    t0 = time.time()
    staged = staged()
    lay = staged.layout
    model = hip_models[MODEL[staged.side]]
    assert model.kind == 0
    if lay.name == 'equal':
        assert staged.n > 4 * 256 * 4
    what = '{} {} scan {}'.format(lay.name, lay.side, scan)
    got = sweep(hip, model, staged, scan, what)
    against_the_oracle(weights[MODEL[staged.side]], lay, got, scan, what)
    print('{}: {} reads, {} beyond 2^31, {} beyond 2^32; windows beyond: {}, {}; {:.2f} s'.format(
        what, staged.n, len(lay.reads_beyond(B31)), len(lay.reads_beyond(B32)),
        lay.windows_beyond(B31, scan), lay.windows_beyond(B32, scan), time.time() - t0))


@pytest.mark.parametrize('scan', [512, SCAN])
def test_read_length_hint_beyond_4g_samples(hip, hip_models, staged_equal, scan):
    """The speculative fetch from (read0 + read) x hint: a right hint whose guess itself passes
    2^32, a wrong one, and a capacity that ends between the boundaries all give the unhinted bits."""
    st = staged_equal()
    lay = st.layout
    model = hip_models[MODEL[st.side]]
    length = int(lay.lengths[0])
    run = Runner(hip, model, st.n, scan, st.side)
    try:
        model.set_read_length_hint(0)
        plain = run.whole(st.far, st.far_offsets)
        assert_same_bits(plain, run.whole(st.compact_samples, st.compact_offsets), lay,
                         'equal {} scan {} without a hint'.format(st.side, scan))
        between = B31 + (B32 - B31) // 2 + 12345
        assert (st.n - 1) * length > B32 and B31 < between < B32
        for hint, capacity in ((length, TOTAL_SAMPLES), (length - 2, TOTAL_SAMPLES),
                               (length, between)):
            model.set_read_length_hint(hint, capacity)
            what = 'equal {} scan {} hint {} capacity {}'.format(st.side, scan, hint, capacity)
            assert_same_bits(run.whole(st.far, st.far_offsets), plain, lay, what)
            for batch in (1, 7, 256):
                assert_same_bits(run.batched(st.far, st.far_offsets, batch), plain, lay,
                                 what + ' batch {}'.format(batch))
    finally:
        model.set_read_length_hint(0)
        run.free()


def test_normalise_windows_beyond_4g_samples(hip, staged):
    st = staged()
    lay = st.layout
    steps = SCAN // (WINDOW // 2)
    lib = hip.load_library()
    side = 0 if st.side == 'start' else 1
    out = allocate(hip, st.n * steps * WINDOW * 4)
    try:
        windows = []
        for samples, offsets in ((st.compact_samples, st.compact_offsets),
                                 (st.far, st.far_offsets)):
            hip.check(lib.dbh_normalise_windows_dev(samples.ptr, offsets.ptr, st.n, side, SCAN,
                                                    out.ptr, None), 'dbh_normalise_windows_dev')
            hip.synchronize()
            windows.append(out.download((st.n, steps, WINDOW), np.uint32))
        bad = np.argwhere((windows[0] != windows[1]).any(axis=2))
        assert not len(bad), '{} {}: {} windows differ, the first is step {} of read {} at {}' \
            .format(lay.name, lay.side, len(bad), bad[0][1], bad[0][0],
                    int(lay.offsets[bad[0][0]]))
        assert np.isfinite(windows[1].view(np.float32)).all()
        assert windows[1].any(axis=2).sum() > st.n          # (not all empty)
    finally:
        release(out)


@pytest.fixture(scope='module')
def general_2048(hip):
    models = {side: hip.HipModel(geometry(2048, 13, name=MODEL[side]), device=0, general=True)
              for side in ('start', 'end')}
    yield models
    for m in models.values():
        m.close()


def test_general_classify_beyond_4g_samples(hip, general_2048, staged_ragged):
    st = staged_ragged()
    lay = st.layout
    model = general_2048[st.side]
    assert model.kind == 1
    scan = 3 * 1024
    what = 'general L=2048 {} {}'.format(lay.name, lay.side)
    got = sweep(hip, model, st, scan, what)
    against_the_oracle(model.weights, lay, got, scan, what)


# ---- Part B: stream offsets of dbh_inflate_dev ------------------------------------------------
@pytest.fixture(scope='module')
def stream_plan():
    import vbz_fixtures as vf
    return fo.stream_plan(have_zstd=vf.zstd_lib() is not None)


def launch_streams(hip, records, d_comp, comp_bytes, total_out, d_out, d_work):
    lib = hip.load_library()
    d_rec, d_status = allocate_all(hip, records.nbytes, 4 * len(records))
    try:
        d_rec.upload(records)
        d_status.upload(np.full(len(records), -7, dtype=np.int32))
        hip.check(lib.dbh_inflate_dev(d_comp.ptr, comp_bytes, d_rec.ptr, len(records), total_out,
                                      d_out.ptr, d_work.ptr, d_status.ptr, 0, None),
                  'dbh_inflate_dev')
        hip.synchronize()
        return d_status.download(len(records), np.int32)
    finally:
        release(d_rec, d_status)


def download_at(hip, buf, byte_offset, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    assert 0 <= byte_offset and byte_offset + nbytes <= buf.nbytes
    hip.check(hip.load_library().dbh_memcpy_d2h(out.ctypes.data, buf.ptr + byte_offset, nbytes,
                                                None), 'dbh_memcpy_d2h')
    hip.synchronize()
    return out


def workspace_bytes(hip, total_out, n):
    size = ctypes.c_size_t(0)
    hip.check(hip.load_library().dbh_inflate_workspace_bytes(total_out, n, ctypes.byref(size)))
    return size.value


def compact_streams(hip, streams):
    """The same streams back to back in a small launch -> (outputs, status, zstd slots)."""
    where, comp_bytes, total_out = fo.compact_stream_layout(streams)
    comp = np.zeros(comp_bytes + 64, dtype=np.uint8)
    comp[:comp_bytes] = np.frombuffer(b''.join(s.data for s in streams), dtype=np.uint8)
    records = np.array([(c, len(s.data), o, s.out_bytes, s.mode, 0)
                        for s, (c, o) in zip(streams, where)], dtype=hip.INFLATE_STREAM)
    d_comp, d_out, d_work = allocate_all(hip, comp.nbytes, total_out,
                                         workspace_bytes(hip, total_out, len(streams)))
    try:
        d_comp.upload(comp)
        d_out.upload(np.full(total_out, fo.SENTINEL, dtype=np.uint8))
        status = launch_streams(hip, records, d_comp, comp_bytes, total_out, d_out, d_work)
        raw = d_out.download(total_out, np.uint8)
        slots = [download_at(hip, d_work, 4 * o, len(s.content)) if s.content else None
                 for s, (c, o) in zip(streams, where)]
    finally:
        release(d_comp, d_out, d_work)
    outside = np.ones(total_out, dtype=bool)
    for s, (c, o) in zip(streams, where):
        outside[o:o + s.out_bytes] = False
    assert (raw[outside] == fo.SENTINEL).all()
    return [raw[o:o + s.out_bytes] for s, (c, o) in zip(streams, where)], status, slots


@pytest.mark.parametrize('form', ['pair', 'two_launches'])
def test_streams_beyond_4g_bytes(hip, stream_plan, monkeypatch, form):
    """One launch whose streams read and write around byte 0, across byte 2^31 and across byte 2^32
    of the compressed and of the output buffer (token slots: across 2^33 and 2^34 of the
    workspace), against the same streams in a small launch and against the host's decoders."""
    t0 = time.time()
    if form == 'two_launches':
        monkeypatch.setenv('DEEPBINNER_INFLATE_PAIR', '0')
    else:
        monkeypatch.delenv('DEEPBINNER_INFLATE_PAIR', raising=False)
    streams = stream_plan
    # every mode, the zstd stage and its refusals included
    assert len(streams) == 54 and {s.mode for s in streams} == {0, 1, 2, 3, 4, 5}
    c_out, c_status, c_slots = compact_streams(hip, streams)
    for s, out, status, slot in zip(streams, c_out, c_status, c_slots):
        if s.want is None:
            assert status != 0 and not out.any(), s.name
        else:
            assert status == 0 and out.tobytes() == s.want, (s.name, status)
            if s.content:
                assert slot.tobytes() == s.content, s.name

    work_bytes = workspace_bytes(hip, fo.TOTAL_OUT, len(streams))
    assert 4 * fo.TOTAL_OUT <= work_bytes
    assert fo.inflate_peak_bytes(work_bytes) <= fo.MAX_PEAK_BYTES
    drop_far_samples()                       # Part A's 8 GiB, if its tests ran before
    assert _peak['now'] == 0
    d_comp, d_out, d_work = allocate_all(hip, fo.TOTAL_COMP, fo.TOTAL_OUT, work_bytes)
    try:
        sentinels = np.full(fo.PLACE_BYTES, fo.SENTINEL, dtype=np.uint8)
        comp = fo.comp_places(streams)
        for (lo, hi), data in zip(fo.PLACES, comp):
            upload_at(hip, d_comp, lo, data)
            upload_at(hip, d_out, lo, sentinels[:hi - lo])
        hip.synchronize()
        records = np.array([(s.comp_offset, len(s.data), s.out_offset, s.out_bytes, s.mode, 0)
                            for s in streams], dtype=hip.INFLATE_STREAM)
        status = launch_streams(hip, records, d_comp, fo.TOTAL_COMP - 64, fo.TOTAL_OUT, d_out,
                                d_work)
        places = [download_at(hip, d_out, lo, hi - lo) for lo, hi in fo.PLACES]
        slots = [download_at(hip, d_work, 4 * s.out_offset, len(s.content)) if s.content else None
                 for s in streams]
    finally:
        release(d_comp, d_out, d_work)
    untouched = [np.ones(hi - lo, dtype=bool) for lo, hi in fo.PLACES]
    for k, s in enumerate(streams):
        lo = fo.PLACES[s.out_place][0]
        got = places[s.out_place][s.out_offset - lo:s.out_offset - lo + s.out_bytes]
        untouched[s.out_place][s.out_offset - lo:s.out_offset - lo + s.out_bytes] = False
        where = '{} (out {} comp {})'.format(s.name, s.out_offset, s.comp_offset)
        assert status[k] == c_status[k], (where, status[k], c_status[k])
        assert np.array_equal(got, c_out[k]), where
        if s.content:
            assert slots[k].tobytes() == s.content, where
    # 64 bytes on either side of every region, and every alias of a far region that lies between
    # regions (a place less 2^31 or 2^32 is inside another place): all still sentinels.  An alias
    # that lies on another stream's region holds other bytes - for a refused stream's zeros always
    # a valid stream's output (tests/test_far_offsets.py) - and shows in that stream's comparison.
    for place, keep in zip(places, untouched):
        assert (place[keep] == fo.SENTINEL).all(), 'a byte outside the regions was written'
    beyond = [sum(1 for s in streams if s.out_offset + s.out_bytes > b) for b in BOUNDARIES]
    comp_beyond = [sum(1 for s in streams if s.comp_offset + len(s.data) > b) for b in BOUNDARIES]
    print('{}: {} streams; output beyond 2^31: {}, beyond 2^32: {}; compressed bytes beyond 2^31: '
          '{}, beyond 2^32: {}; peak device bytes {}; {:.2f} s'.format(
              form, len(streams), beyond[0], beyond[1], comp_beyond[0], comp_beyond[1],
              _peak['peak'], time.time() - t0))


# ---- Part C: DTW direction words beyond 4 GiB -------------------------------------------------
def test_dtw_path_words_beyond_4g(monkeypatch):
    """One call of the default path budget whose launch of five-panel pairs holds more than 2^32
    bytes (2^30 words) of directions; 40 small pairs in front make the alignment offsets uneven,
    and those of the widest lanes stand behind the long pairs in the same launch."""
    from deepbinner_amd import dtw_semi_global as dtw
    from oracle import dtw_ref
    t0 = time.time()
    drop_far_samples()
    monkeypatch.delenv('DEEPBINNER_DTW_PATH_BYTES', raising=False)     # the default: 8 GiB
    ref_lens, query_lens, cut = fo.dtw_far_plan()
    rng = np.random.default_rng(32)
    refs, queries = [], []
    for r, q, at in zip(ref_lens, query_lens, cut):
        refs.append(rng.normal(size=r))
        queries.append(rng.normal(size=q) if at is None else refs[-1][at:at + q].copy())
    wide = [k for k, q in enumerate(query_lens) if q > 512]            # one launch: 16 per lane
    far = [k for k in wide if cut[k] is not None]
    assert len(far) == 100
    for k in far:
        assert fo.dtw_path_bytes(ref_lens[k], query_lens[k]) == 5 * (40000 + 63) * 64 * 4
    launch_bytes = sum(fo.dtw_path_bytes(ref_lens[k], query_lens[k]) for k in wide)
    assert B32 < launch_bytes < 8 << 30 and launch_bytes // 4 > 1 << 30
    # the launch takes its pairs longest first: these begin beyond byte 2^32 of the words
    order = sorted(wide, key=lambda k: -ref_lens[k] * query_lens[k])
    begin = np.cumsum([0] + [fo.dtw_path_bytes(ref_lens[k], query_lens[k]) for k in order])[:-1]
    beyond = [k for k, b in zip(order, begin) if b >= B32]
    across = [k for k, b in zip(order, begin)
              if b < B32 < b + fo.dtw_path_bytes(ref_lens[k], query_lens[k])]
    assert len([k for k in beyond if cut[k] is not None]) >= 10 and len(across) == 1
    assert len([k for k in beyond if cut[k] is None]) >= 5

    got = dtw.semi_global_dtw_batch(refs, queries)
    # every cell of the call was computed (under the default budget, in force here, the wide
    # pairs' words fit one launch: asserted above)
    assert dtw.last_kernel_time()[1] == sum(r * q for r, q in zip(ref_lens, query_lens))
    for k in range(len(refs)):
        distance, start, end, pairs = got[k]
        if cut[k] is None:
            want = dtw_ref.semi_global_dtw(refs[k], queries[k], 'restatement')
            assert (distance, start, end) == want[:3], (k, ref_lens[k], query_lens[k])
            assert np.array_equal(pairs, np.array(want[3], dtype=np.int32).reshape(-1, 2)), k
        else:
            at, n = cut[k], query_lens[k]
            assert distance == 0.0 and end == at + n - 1, (k, distance, end, at, n)
            assert pairs[-1][1] == n - 1 and pairs[0][1] == 0 and len(pairs) >= n
            # column 0 is free; from column 1 on the path is the diagonal
            assert np.array_equal(pairs[1:, 0] - pairs[1:, 1], np.full(len(pairs) - 1, at)), k
    without = dtw.semi_global_dtw_batch(refs, queries, alignments=False)
    assert [w[:3] for w in without] == [g[:3] for g in got]
    assert all(w[3] is None for w in without)
    print('dtw: {} pairs, {} bytes of direction words (the library\'s own allocation) in one '
          'launch; pairs that begin beyond '
          '2^32 bytes: {} ({} long), one across it; {:.2f} s'.format(
              len(refs), launch_bytes, len(beyond),
              len([k for k in beyond if cut[k] is not None]), time.time() - t0))


def test_dtw_ties_at_the_widest_lanes_and_across_panel_seams():
    """Integer-valued signals tie all the time; queries of 1,025 .. 2,100 samples run 16 columns
    per lane in two or three panels.  Held to the restatement like the narrow queries of
    test_gpu_ties_give_the_same_distance_and_a_valid_path."""
    from deepbinner_amd import dtw_semi_global as dtw
    from oracle import dtw_ref
    from test_dtw import check_path, path_cost
    rng = np.random.default_rng(33)
    lengths = [1025, 1026, 2047, 2048, 2049, 2050, 2100, 1500] + \
        [int(v) for v in rng.integers(1025, 2101, size=16)]
    refs = [rng.integers(0, 4, size=int(rng.integers(2, 601))).astype(np.float64) for _ in lengths]
    refs[0], refs[3] = refs[0][:2], np.resize(refs[3], 600)
    queries = [rng.integers(0, 4, size=n).astype(np.float64) for n in lengths]
    assert all(n > 1024 for n in lengths) and {-(-n // 1024) for n in lengths} == {2, 3}
    for ref, query, (distance, start, end, pairs) in zip(refs, queries,
                                                        dtw.semi_global_dtw_batch(refs, queries)):
        want = dtw_ref.semi_global_dtw(ref, query, 'restatement')
        assert (distance, start, end) == want[:3]
        assert np.array_equal(pairs, np.array(want[3], dtype=np.int32).reshape(-1, 2))
        check_path(ref, query, start, end, pairs)
        assert path_cost(ref, query, pairs) == distance
