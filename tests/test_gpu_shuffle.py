"""HDF5's shuffle filter undone on the GPU: streams of mode DBH_INFLATE_ZLIB_SHUFFLE (u32 LE N, a
zlib stream of the N shuffled bytes) and DBH_INFLATE_STORED_SHUFFLE (u32 LE N, the N shuffled
bytes) beside zlib, stored and VBZ streams in one launch, under both forms of the inflate kernels,
held against NumPy bit for bit.  Through dbh_inflate_dev the output buffer is filled with a
sentinel first: every byte outside the streams' regions must still hold it."""

import contextlib
import ctypes
import io
import os
import shutil
import struct
import zlib

import numpy as np
import pytest

import shuffle_fixtures as sf
import vbz_fixtures as vf
from conftest import MODEL_DIR

pytestmark = pytest.mark.gpu

ZLIB, STORED, VBZ, ZLIB_SHUFFLE, STORED_SHUFFLE = 0, 1, 2, 4, 5
REFUSED = 32
SENTINEL = 0xA5
START, END = 'EXP-NBD103_read_starts', 'EXP-NBD103_read_ends'
FILTER_WARNING = 'Warning: skipping reads whose signal is compressed with a filter'
# both forms of the inflate kernels: one launch of a pair of waves per stream / two launches.
# 'lane_rounds' exports the two retired switches (it once selected the older kernels they named):
# nothing reads them any more, so it must be the pair, with the same bytes and statuses
FORMS = {'pair': {},
         'two_launches': {'DEEPBINNER_INFLATE_PAIR': '0'},
         'lane_rounds': {'DEEPBINNER_INFLATE_KERNEL': 'lane', 'DEEPBINNER_INFLATE_RESOLVE': 'rounds'}}
SIZES = (2, 4, 6, 30, 32, 34, 1022, 1024, 1026, 2046, 2048, 2050, 6250, 65538, 400000)


def set_form(monkeypatch, form):
    monkeypatch.delenv('DEEPBINNER_INFLATE_PAIR', raising=False)
    for name, value in FORMS[form].items():
        monkeypatch.setenv(name, value)


class Item:
    """One stream of a launch: its bytes, mode, out_bytes, the residue of its out_offset modulo 16,
    and what its output region must hold / what its status must be (a set of values)."""

    def __init__(self, data, mode, out_bytes, want, residue=0, status=(0,), label=''):
        self.data, self.mode, self.out_bytes, self.residue = bytes(data), mode, int(out_bytes), residue
        self.want = np.frombuffer(bytes(want), dtype=np.uint8)
        assert len(self.want) == self.out_bytes
        self.status, self.label = tuple(status), label


def layout(items, seed=1):
    """-> (comp, records in a shuffled order, the place of every item's record, total_out)"""
    rows, comp_at, out_at = [], 0, 0
    for it in items:
        out_at = (out_at + 15) // 16 * 16 + 16 + it.residue
        rows.append((comp_at, len(it.data), out_at, it.out_bytes, it.mode, 0))
        comp_at += len(it.data)
        out_at += it.out_bytes
    total_out = out_at + 64
    comp = np.zeros(comp_at + 64, dtype=np.uint8)
    comp[:comp_at] = np.frombuffer(b''.join(it.data for it in items), dtype=np.uint8)
    order = np.random.default_rng(seed).permutation(len(items))
    return comp, rows, order, total_out, comp_at


def run_dev(hip, items, seed=1):
    """The items as one dbh_inflate_dev call -> (per item output bytes, per item status)"""
    lib = hip.load_library()
    comp, rows, order, total_out, comp_at = layout(items, seed)
    records = np.array([rows[i] for i in order], dtype=hip.INFLATE_STREAM)
    work_bytes = ctypes.c_size_t(0)
    hip.check(lib.dbh_inflate_workspace_bytes(total_out, len(records), ctypes.byref(work_bytes)))
    d_comp = hip.DeviceBuffer.from_array(comp)
    d_rec = hip.DeviceBuffer.from_array(records)
    d_out = hip.DeviceBuffer.from_array(np.full(total_out, SENTINEL, dtype=np.uint8))
    d_work = hip.DeviceBuffer(work_bytes.value)
    d_status = hip.DeviceBuffer.from_array(np.full(len(records), -7, dtype=np.int32))
    try:
        hip.check(lib.dbh_inflate_dev(d_comp.ptr, comp_at, d_rec.ptr, len(records), total_out, d_out.ptr,
                                      d_work.ptr, d_status.ptr, 0, None), 'dbh_inflate_dev')
        hip.synchronize()
        raw = d_out.download(total_out, np.uint8)
        status_in_order = d_status.download(len(records), np.int32)
    finally:
        for b in (d_comp, d_rec, d_out, d_work, d_status):
            b.free()
    outside = np.ones(total_out, dtype=bool)
    for row in rows:
        outside[row[2]:row[2] + row[3]] = False
    assert (raw[outside] == SENTINEL).all(), 'a byte outside the streams\' regions was changed'
    status = np.zeros(len(items), dtype=np.int32)
    status[order] = status_in_order
    return [raw[row[2]:row[2] + row[3]] for row in rows], status


def run_inflate(hip, items, seed=2):
    """The same through hip_backend.inflate (dbh_inflate: host buffers in and out)"""
    comp, rows, order, total_out, comp_at = layout(items, seed)
    records = np.array([rows[i] for i in order], dtype=hip.INFLATE_STREAM)
    raw, status_in_order, _ = hip.inflate(comp[:comp_at], records, total_out)
    status = np.zeros(len(items), dtype=np.int32)
    status[order] = status_in_order
    return [raw[row[2]:row[2] + row[3]] for row in rows], status


def check(items, outs, status):
    for k, (it, got, st) in enumerate(zip(items, outs, status)):
        assert st in it.status, (k, it.label, int(st), it.status)
        if not np.array_equal(got, it.want):
            at = int(np.nonzero(got != it.want)[0][0])
            raise AssertionError('item %d (%s): first wrong byte at %d of %d' % (k, it.label, at, it.out_bytes))


# ---- contents -----------------------------------------------------------------------------------
def content(kind, n_samples, seed):
    rng = np.random.default_rng(seed)
    if kind == 'squiggle':
        return sf.squiggle(rng, n_samples)
    if kind == 'constant':                 # its planes are maximal matches at distance 1
        return np.full(n_samples, 0x01F3, dtype=np.int16)
    return rng.integers(-32768, 32768, size=n_samples).astype(np.int16)


CONTENTS = ('squiggle', 'constant', 'noise')
VARIANTS = ('level1', 'level9', 'stored_blocks', 'mode5')


def shuffled_item(n_bytes, kind, variant, extra, residue):
    """A valid stream of N = n_bytes: out_bytes = N + extra (extra < 0: mode 5 only)"""
    samples = content(kind, n_bytes // 2, seed=n_bytes + 7 * residue)
    planes = sf.shuffle(samples)
    out_bytes = n_bytes + extra
    want = samples.tobytes()[:out_bytes & ~1].ljust(out_bytes, b'\0')
    label = '%d %s %s %+d @%d' % (n_bytes, kind, variant, extra, residue)
    prefix = struct.pack('<I', n_bytes)
    if variant == 'mode5':
        return Item(prefix + planes, STORED_SHUFFLE, out_bytes, want, residue, label=label)
    level = {'level1': 1, 'level9': 9, 'stored_blocks': 0}[variant]
    return Item(prefix + zlib.compress(planes, level), ZLIB_SHUFFLE, out_bytes, want, residue, label=label)


def other_modes(seed):
    """zlib, stored and VBZ streams to stand between the shuffled ones"""
    rng = np.random.default_rng(seed)
    s = sf.squiggle(rng, int(rng.integers(200, 3000)))
    raw = s.tobytes()
    return [Item(zlib.compress(raw, 1), ZLIB, len(raw) + 10, raw + b'\0' * 10, 2 * (seed % 8), label='zlib'),
            Item(raw, STORED, len(raw), raw, 2 * ((seed + 3) % 8), label='stored'),
            Item(vf.vbz_chunk(s, 0), VBZ, len(raw), raw, 2 * ((seed + 5) % 8), label='vbz'),
            Item(zlib.compress(raw, 6)[:-9], ZLIB, len(raw) - 64, raw[:-64], 2 * ((seed + 1) % 8),
                 label='zlib, cut')]


_MATRIX = []


def matrix():
    """Every N at every even residue of out_offset modulo 16, the contents, compressions and output
    sizes dealt over them; three sizes with everything crossed; modes 0, 1 and 2 in between."""
    if _MATRIX:
        return _MATRIX
    items = []
    for n in SIZES:
        for j in range(8):
            items.append(shuffled_item(n, CONTENTS[j % 3], VARIANTS[j % 4], (0, 2, 1000)[(j + j // 3) % 3], 2 * j))
        items += other_modes(n)
    for n in (34, 2050, 6250):
        k = 0
        for kind in CONTENTS:
            for variant in VARIANTS:
                for extra in (0, 2, 1000):
                    items.append(shuffled_item(n, kind, variant, extra, 2 * (k % 8)))
                    k += 1
    # mode 5 is random access: any out_bytes
    for n in (6, 34, 1026, 6250, 65538):
        for k, out_bytes in enumerate((0, 2, n // 2 // 2 * 2, n - 2)):
            items.append(shuffled_item(n, CONTENTS[k % 3], 'mode5', out_bytes - n, 2 * ((k + n) % 8)))
    # N = 0: nothing but zeros
    items.append(Item(struct.pack('<I', 0) + zlib.compress(b'', 1), ZLIB_SHUFFLE, 40, b'\0' * 40, 6, label='empty'))
    items.append(Item(struct.pack('<I', 0), STORED_SHUFFLE, 40, b'\0' * 40, 10, label='empty 5'))
    _MATRIX.extend(items)
    return _MATRIX


@pytest.mark.parametrize('form', list(FORMS))
def test_every_size_offset_content_and_compression(hip, monkeypatch, form):
    set_form(monkeypatch, form)
    items = matrix()
    assert {it.mode for it in items} == {ZLIB, STORED, VBZ, ZLIB_SHUFFLE, STORED_SHUFFLE}
    outs, status = run_dev(hip, items)
    check(items, outs, status)


def test_through_hip_backend_inflate(hip, monkeypatch):
    set_form(monkeypatch, 'pair')
    items = matrix()
    outs, status = run_inflate(hip, items)
    check(items, outs, status)


def refusals():
    rng = np.random.default_rng(12)
    good = sf.squiggle(rng, 1500)

    def neighbour(k):
        return shuffled_item(3000, 'squiggle', VARIANTS[k % 4], 2, 2 * (k % 8))

    def z(n_bytes, level=1):                   # a zlib stream holding n_bytes shuffled bytes
        return zlib.compress(sf.shuffle(content('squiggle', n_bytes // 2, 5))[:n_bytes], level)

    p = struct.pack
    planes = sf.shuffle(good)
    zeros = lambda n: b'\0' * n
    odd = zlib.compress(planes + b'\x07', 1)
    damaged = sf.damage_deflate(z(3000))
    bad_block = bytearray(z(3000))
    bad_block[2] = 0x07                        # BFINAL = 1, BTYPE = 3: no code at all
    cases = [
        Item(p('<I', 3001) + odd, ZLIB_SHUFFLE, 3002, zeros(3002), 2, (REFUSED,), 'N odd'),
        Item(p('<I', 3001) + planes + b'\x07', STORED_SHUFFLE, 3002, zeros(3002), 4, (REFUSED,), 'N odd, mode 5'),
        Item(p('<I', 3000) + z(3000), ZLIB_SHUFFLE, 2998, zeros(2998), 6, (REFUSED,), 'N > out_bytes'),
        Item(p('<I', 3000) + z(3002), ZLIB_SHUFFLE, 3000, zeros(3000), 8, (REFUSED,), 'stream holds N + 2'),
        Item(p('<I', 3000) + z(3002), ZLIB_SHUFFLE, 3400, zeros(3400), 8, (REFUSED,), 'stream holds N + 2, room'),
        Item(p('<I', 3000) + z(2998), ZLIB_SHUFFLE, 3000, zeros(3000), 10, (REFUSED,), 'stream holds N - 2'),
        Item(p('<I', 3000) + z(2998, 0), ZLIB_SHUFFLE, 3200, zeros(3200), 10, (REFUSED,), 'stored blocks hold N - 2'),
        Item(p('<I', 3000) + planes + b'\0\0', STORED_SHUFFLE, 3000, zeros(3000), 12, (REFUSED,), 'comp_bytes > 4 + N'),
        Item(p('<I', 3000) + planes[:-2], STORED_SHUFFLE, 3000, zeros(3000), 14, (REFUSED,), 'comp_bytes < 4 + N'),
        Item(b'\x10\x00', ZLIB_SHUFFLE, 100, zeros(100), 0, (REFUSED,), 'no room for the prefix'),
        Item(b'\x10\x00\x00', STORED_SHUFFLE, 100, zeros(100), 2, (REFUSED,), 'no room for the prefix, mode 5'),
        Item(p('<I', 3000) + bytes(damaged), ZLIB_SHUFFLE, 3000, zeros(3000), 4, tuple(range(1, 11)),
             'a damaged code'),
        Item(p('<I', 3000) + bytes(bad_block), ZLIB_SHUFFLE, 3100, zeros(3100), 6, (2,), 'block type 3'),
        Item(p('<I', 3000) + z(3000)[:-700], ZLIB_SHUFFLE, 3000, zeros(3000), 8, tuple(range(1, 11)), 'truncated'),
    ]
    # the damaged stream's twin as a plain zlib stream: the same verdict
    twin = Item(bytes(damaged), ZLIB, 3000, zeros(3000), 4, tuple(range(1, 11)), 'the damaged code as mode 0')
    items = []
    for k, case in enumerate(cases):
        items += [neighbour(2 * k), case, neighbour(2 * k + 1)]
    return items + [twin], 3 * 11 + 1, len(items)


@pytest.mark.parametrize('form', list(FORMS))
def test_refused_streams_are_zeros_with_their_neighbours_intact(hip, monkeypatch, form):
    """Each refusal with zeros out, and the new status - or the zlib stage's own where it failed"""
    set_form(monkeypatch, form)
    items, damaged_at, twin_at = refusals()
    assert items[damaged_at].label == 'a damaged code'
    with pytest.raises(zlib.error):
        zlib.decompress(items[twin_at].data)
    outs, status = run_dev(hip, items)
    check(items, outs, status)
    assert status[damaged_at] == status[twin_at] != REFUSED
    assert sum(1 for it, st in zip(items, status) if st == 0) == 2 * (len(items) - 1) // 3


# ---- end to end ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def models(hip):
    from deepbinner_amd.model_format import ModelWeights
    start = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, START + '.dbw'))[0])
    end = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, END + '.dbw'))[0])
    yield start, end
    start.close()
    end.close()


def through_the_raw_route(hip, models, path, route, **kw):
    from deepbinner_amd import fast5_native
    (index, ids, offsets, status, comp, records), = list(
        fast5_native.stream_raw([path], threads=2, shuffle=route, **kw))
    calls, stream_status, samples = hip.classify_pair_deflated(models[0], models[1], comp, records, offsets,
                                                               6144, 0.5, want_samples=True)
    return ids, offsets, status, records, calls, stream_status, samples


def test_a_shuffled_container_on_both_routes_and_packed(hip, models, tmp_path):
    """~200 reads, two thirds of them in chunks with a partial last one; one stream damaged inside
    its deflate data: the device refuses it (the host, asked again, refuses the read), the host
    route's loader marks the read."""
    from deepbinner_amd import fast5_native
    victim = 57                                   # (57 % 3 == 0: one chunk of exactly the read)
    path, reads = sf.small_container(str(tmp_path / 'c.fast5'), n_reads=200, damage={victim: (0,)})
    want_ids, want_samples, want_offsets, want_status = fast5_native.load_reads(path, threads=2)
    assert want_status[victim] != 0 and int(np.count_nonzero(want_status)) == 1
    packed_calls = hip.classify_pair(models[0], models[1], want_samples, want_offsets, 6144, 0.5)
    got = {r: through_the_raw_route(hip, models, path, r) for r in ('host', 'gpu')}
    ids, offsets, status, records, calls, stream_status, samples = got['gpu']
    modes = records['mode']
    assert (modes == ZLIB_SHUFFLE).sum() > 400 and (modes == STORED).sum() > 100      # (partial chunks)
    bad = np.nonzero(stream_status)[0]
    assert len(bad) == 1 and records['read'][bad[0]] == victim and 1 <= stream_status[bad[0]] <= 10
    assert not status.any() and np.array_equal(offsets, want_offsets)
    h_ids, h_offsets, h_status, h_records, h_calls, h_stream_status, h_samples = got['host']
    assert (h_records['mode'] == STORED).all() and not h_stream_status.any()
    assert np.array_equal(h_status, want_status) and h_ids == want_ids
    lo, hi = want_offsets[victim], want_offsets[victim + 1]
    assert not samples[lo:hi].any()                # (refused: zeros)
    for s in (samples, h_samples):
        assert np.array_equal(s[:lo], want_samples[:lo]) and np.array_equal(s[hi:], want_samples[hi:])
    keep = np.arange(len(reads)) != victim
    assert np.array_equal(calls[keep], h_calls[keep]) and np.array_equal(calls[keep], packed_calls[keep])
    assert np.array_equal(np.concatenate([s for i, (_, s) in enumerate(reads) if i != victim]),
                          np.concatenate([samples[:lo], samples[hi:]]))


@pytest.mark.parametrize('name', sf.H5PY_SHUFFLED)
def test_libhdf5_s_own_shuffled_files(hip, models, name):
    from deepbinner_amd import fast5_native
    path = sf.golden(name)
    want = fast5_native.load_reads(path)
    got = {r: through_the_raw_route(hip, models, path, r) for r in ('host', 'gpu')}
    assert (got['gpu'][3]['mode'] == ZLIB_SHUFFLE).sum() == 25
    for r in ('host', 'gpu'):
        ids, offsets, status, records, calls, stream_status, samples = got[r]
        assert ids == want[0] and not stream_status.any() and not status.any()
        assert np.array_equal(samples, want[1])
        assert np.array_equal(calls, hip.classify_pair(models[0], models[1], want[1], want[2], 6144, 0.5))


def test_classify_and_realtime_on_either_route(hip, tmp_path, monkeypatch, capsys):
    """`classify --multi_read` prints the default run's table byte for byte with
    DEEPBINNER_SHUFFLE=gpu, `realtime` files byte-identical one-read files into the same bins.  The
    read with damage inside its deflate data has no row on either route - and no warning: to the
    host's loader a corrupt deflate stream is a damaged file, as it is in an unshuffled container
    (the filter warning is for filters this build cannot decode)."""
    from deepbinner_amd import classify, deepbinner as cli
    import deepbinner_amd.realtime as realtime
    in_dir = tmp_path / 'in'
    in_dir.mkdir()
    victim = 9
    path, reads = sf.small_container(str(in_dir / 'c.fast5'), n_reads=60, damage={victim: (0,)})
    for name in ('DEEPBINNER_HOST_INFLATE_SHARE', 'DEEPBINNER_FAST5_READER', 'DEEPBINNER_VBZ_ZSTD',
                 'DEEPBINNER_DEVICE_ORDINALS', 'DEEPBINNER_REALTIME_TABLE_ONLY'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('DEEPBINNER_GPU_INFLATE', '1')
    monkeypatch.setattr(realtime, 'POLL_SECONDS', 0)
    monkeypatch.setattr(shutil, 'which', lambda tool: None)
    models = ['-s', os.path.join(MODEL_DIR, START + '.dbw'), '-e', os.path.join(MODEL_DIR, END + '.dbw')]

    def route(name):
        if name == 'gpu':
            monkeypatch.setenv('DEEPBINNER_SHUFFLE', 'gpu')
        else:
            monkeypatch.delenv('DEEPBINNER_SHUFFLE', raising=False)
        monkeypatch.setattr(classify, '_FILTER_WARNING_GIVEN', False)

    tables, bins = {}, {}
    for name in ('host', 'gpu'):
        route(name)
        capsys.readouterr()
        cli.main(['classify', '--verbose', '--multi_read', str(in_dir)] + models)
        done = capsys.readouterr()
        tables[name] = (done.out, done.err.count('Warning'))
        assert FILTER_WARNING not in done.err and 'Warning' not in done.err, (name, done.err)
        rows = done.out.splitlines()[1:]
        assert len(rows) == 59 and reads[victim][0] not in [r.split('\t')[0] for r in rows]
        out_dir = tmp_path / ('out_' + name)
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            cli.main(['realtime', '--in_dir', str(in_dir), '--out_dir', str(out_dir), '--stop'] + models)
        capsys.readouterr()
        assert 'Warning' not in err.getvalue(), (name, err.getvalue())
        files = {}
        for top, _, names in os.walk(str(out_dir)):
            for n in names:
                with open(os.path.join(top, n), 'rb') as f:
                    files[os.path.relpath(os.path.join(top, n), str(out_dir))] = f.read()
        bins[name] = files
        assert sum(1 for n in files if n.endswith('.fast5')) == 59
    assert tables['gpu'] == tables['host']
    assert sorted(bins['gpu']) == sorted(bins['host'])
    for n in bins['host']:
        if n.endswith('.fast5'):
            assert bins['gpu'][n] == bins['host'][n], n
        else:                                      # the table: the same rows
            assert sorted(bins['gpu'][n].splitlines()) == sorted(bins['host'][n].splitlines()), n
