"""HDF5's shuffle filter on the raw route, host side: with ``shuffle='gpu'`` the loader hands whole
chunks of shuffle (+ deflate) (+ fletcher32) to the GPU as stored, behind a 4-byte size
(RAW_ZLIB_SHUFFLE, RAW_STORED_SHUFFLE); without it every record is what it was.  The records are
undone here in NumPy (zlib + unshuffle) and held against the packed loader's samples."""

import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

import shuffle_fixtures as sf
import vbz_fixtures as vf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..')


def fn():
    from deepbinner_amd import fast5_native
    return fast5_native


def undo(comp, records, n_samples):
    """What a decoder makes of raw records: every stream decoded, cut or zero-extended to its
    out_bytes, at its out_offset -> int16 samples."""
    out = np.zeros(2 * n_samples, dtype=np.uint8)
    comp = np.asarray(comp, dtype=np.uint8)
    for r in records:
        data = comp[r['comp_offset']:r['comp_offset'] + r['comp_bytes']].tobytes()
        mode = int(r['mode'])
        if mode == fn().RAW_ZLIB:
            d = zlib.decompressobj()
            got = d.decompress(data)
            assert d.eof and d.unused_data == b''
        elif mode == fn().RAW_STORED:
            got = data
        elif mode == fn().RAW_ZLIB_SHUFFLE:
            size, = struct.unpack('<I', data[:4])
            d = zlib.decompressobj()
            shuffled = d.decompress(data[4:])
            assert d.eof and d.unused_data == b''          # (the stream alone: no checksum behind it)
            assert size == len(shuffled) == r['out_bytes']
            got = sf.unshuffle(shuffled).tobytes()
        elif mode == fn().RAW_STORED_SHUFFLE:
            size, = struct.unpack('<I', data[:4])
            assert size == len(data) - 4 == r['out_bytes']
            got = sf.unshuffle(data[4:]).tobytes()
        else:
            raise AssertionError('mode %d' % mode)
        got = np.frombuffer(got[:r['out_bytes']], dtype=np.uint8)
        out[r['out_offset']:r['out_offset'] + len(got)] = got
    return out.view('<i2')


def raw_of(path, api, **kw):
    """(ids, offsets, status, comp, records) of one file through ``load_batch_raw`` / ``stream_raw``"""
    if api == 'batch':
        return fn().load_batch_raw([path], 2, **kw)
    (index, ids, offsets, status, comp, records), = list(fn().stream_raw([path], threads=2, **kw))
    assert ids is not None, path
    return ids, offsets, status, comp, records


def in_read_order(records):
    return np.sort(records, order=['read', 'out_offset'])


@pytest.mark.parametrize('api', ['batch', 'stream'])
@pytest.mark.parametrize('name', sf.H5PY_SHUFFLED)
def test_libhdf5_s_shuffle_deflate_fletcher32_chunks_go_out_as_stored(name, api):
    """[(2,[2]), (1,[9]), (3,[])] as h5py wrote it, 25,001 samples in chunks of 1,000: 25 whole chunks
    are mode 4 - the prefix, then the stored bytes less the fletcher32 word, which follows the
    stream in the file; the 26th, 1 of 1,000 samples, is the host's."""
    path = sf.golden(name)
    ids, offsets, status, comp, records = raw_of(path, api, shuffle='gpu')
    assert list(status) == [0] and len(records) == 26
    want = fn().load_reads(path)[1]
    assert len(want) == 25001
    with open(path, 'rb') as f:
        image = f.read()
    rec = in_read_order(records)
    for k, r in enumerate(rec[:25]):
        assert r['mode'] == fn().RAW_ZLIB_SHUFFLE
        assert (r['out_offset'], r['out_bytes']) == (2000 * k, 2000)
        data = comp[r['comp_offset']:r['comp_offset'] + r['comp_bytes']].tobytes()
        assert data[:4] == struct.pack('<I', 2000)
        at = image.find(data[4:])
        assert at > 0 and image[at + len(data) - 4:at + len(data)] == sf.fletcher32(data[4:])
    last = rec[25]
    assert (last['mode'], last['out_offset'], last['out_bytes'], last['comp_bytes']) == \
        (fn().RAW_STORED, 50000, 2, 2)
    assert np.array_equal(undo(comp, records, 25001), want)
    # the records go out longest deflate stream first, the shuffled ones as the streams they are
    sizes = [int(r['comp_bytes']) for r in records if r['mode'] == fn().RAW_ZLIB_SHUFFLE]
    assert sizes == sorted(sizes, reverse=True) and records[-1]['mode'] == fn().RAW_STORED


def copies(tmp_path, chunk=1000, n=4300):
    rng = np.random.default_rng(3)
    signal = sf.squiggle(rng, n)
    out = {}
    for kind in sf.PIPELINES:
        out[kind] = sf.write_copy([('read-' + kind, signal)], str(tmp_path / (kind + '.fast5')), kind, chunk)
    return signal, out


@pytest.mark.parametrize('api', ['batch', 'stream'])
def test_modes_by_the_filters_applied(tmp_path, api):
    signal, paths = copies(tmp_path)
    want_mode = {'shuffle_deflate': fn().RAW_ZLIB_SHUFFLE, 'shuffle_deflate_fletcher': fn().RAW_ZLIB_SHUFFLE,
                 'shuffle': fn().RAW_STORED_SHUFFLE, 'shuffle_fletcher': fn().RAW_STORED_SHUFFLE,
                 'deflate': fn().RAW_ZLIB}
    for kind, path in paths.items():
        assert np.array_equal(fn().load_reads(path)[1], signal), kind
        ids, offsets, status, comp, records = raw_of(path, api, shuffle='gpu')
        assert list(status) == [0], kind
        rec = in_read_order(records)
        assert [int(m) for m in rec['mode'][:4]] == [want_mode[kind]] * 4, kind
        # 300 of the last chunk's 1,000 samples are wanted: a shuffled one is the host's
        assert rec['mode'][4] == (fn().RAW_ZLIB if kind == 'deflate' else fn().RAW_STORED), kind
        assert rec['out_bytes'][4] == 600
        for r in rec[:4]:
            stored = len(sf.encode_chunk(signal[r['out_offset'] // 2:][:1000], kind))
            less = 4 if kind.endswith('fletcher') else 0
            more = 0 if kind == 'deflate' else 4
            assert r['comp_bytes'] == stored - less + more, kind
        assert np.array_equal(undo(comp, records, len(signal)), signal), kind


@pytest.mark.parametrize('api', ['batch', 'stream'])
def test_without_the_keyword_nothing_changes(tmp_path, api):
    """Default, shuffle='host' and the calls without flags give the same records and bytes: every
    shuffled chunk decoded by the host (RAW_STORED, its samples).  And shuffle='gpu' changes
    nothing for a file without the shuffle filter."""
    signal, paths = copies(tmp_path)
    files = [paths[k] for k in sorted(paths)] + [sf.golden(n) for n in sf.H5PY_SHUFFLED]
    for path in files:
        a = raw_of(path, api)
        b = raw_of(path, api, shuffle='host')
        assert a[0] == b[0] and a[4].tobytes() == b[4].tobytes() and bytes(a[3]) == bytes(b[3]), path
        shuffled = 'deflate.fast5' != os.path.basename(path)
        if shuffled:
            assert (a[4]['mode'] == fn().RAW_STORED).all() and (a[4]['comp_bytes'] == a[4]['out_bytes']).all()
            n = int(a[1][-1])
            assert np.array_equal(np.asarray(a[3][:2 * n]).view('<i2'), fn().load_reads(path)[1])
        else:
            c = raw_of(path, api, shuffle='gpu')
            assert a[4].tobytes() == c[4].tobytes() and bytes(a[3]) == bytes(c[3])
    # the entry points without flags
    lib = fn().load_library()
    handle = ctypes.c_void_p()
    arr = (ctypes.c_char_p * 1)(os.fsencode(files[0]))
    assert lib.f5_load_batch_raw(arr, 1, 1, 0, ctypes.byref(handle)) == 0
    n = lib.f5_batch_n_streams(handle)
    got = ctypes.string_at(lib.f5_batch_streams(handle), n * fn().RAW_STREAM.itemsize)
    lib.f5_batch_free(handle)
    assert got == raw_of(files[0], 'batch')[4].tobytes()
    handle = ctypes.c_void_p()
    assert lib.f5_load_batch_raw_ex(arr, 1, 1, 0, 4, ctypes.byref(handle)) != 0       # (an unknown flag)


def test_every_golden_file_undone_in_numpy_is_the_loader_s_samples(tmp_path):
    """shuffle='gpu' over every committed fast5 file and the shuffled copies: the records, undone
    in NumPy, are f5_load_reads' samples."""
    _, paths = copies(tmp_path, chunk=None)
    container, reads = sf.small_container(str(tmp_path / 'c.fast5'), n_reads=40)
    files = vf.golden_fast5() + sorted(paths.values()) + [container]
    seen = set()
    for index, ids, offsets, status, comp, records in fn().stream_raw(files, threads=2, shuffle='gpu'):
        path = files[index]
        try:
            want = fn().load_reads(path, threads=2)
        except OSError:
            assert ids is None, path
            continue
        assert ids == want[0] and np.array_equal(offsets, want[2]) and np.array_equal(status, want[3]), path
        if ((records['mode'] == fn().RAW_VBZ) | (records['mode'] == fn().RAW_VBZ_ZSTD)).any():
            continue
        assert np.array_equal(undo(comp, records, int(offsets[-1])), want[1]), path
        seen |= set(int(m) for m in records['mode'])
    assert seen == {0, 1, 4, 5}
    assert np.array_equal(np.concatenate([s for _, s in reads]), fn().load_reads(container)[1])


def test_long_streams_and_the_host_s_share_take_shuffled_deflate_as_deflate(tmp_path):
    """zlib_above (host_inflate_above > 0) and the host's share (-p) move mode-4 pieces to the host
    exactly as they move plain deflate pieces of the same sizes."""
    rng = np.random.default_rng(8)
    reads = [('r%02d' % i, sf.squiggle(rng, 1000 * (i + 2))) for i in range(12)]
    twin = sf.write_copy(reads, str(tmp_path / 'deflate.fast5'), 'deflate', None, multi=True)
    shuf = sf.write_copy(reads, str(tmp_path / 'shuffle.fast5'), 'shuffle_deflate', None, multi=True)
    want = np.concatenate([s for _, s in reads])
    for above in (0, 9000, 1, -30, -100):
        _, offsets, status, comp, rec = raw_of(shuf, 'stream', shuffle='gpu', host_inflate_above=above)
        assert not np.asarray(status).any()
        assert np.array_equal(undo(comp, rec, len(want)), want), above
        rec = in_read_order(rec)
        sizes = np.array([len(zlib.compress(sf.shuffle(s), 1)) for _, s in reads])
        on_gpu = rec['mode'] == fn().RAW_ZLIB_SHUFFLE
        assert ((rec['mode'] == fn().RAW_STORED) == ~on_gpu).all()
        if above > 0:
            assert (on_gpu == (sizes <= above)).all(), above
        elif above == 0:
            assert on_gpu.all()
        elif above == -100:
            assert not on_gpu.any()
        else:
            # the longest streams holding 30 % of the bytes: as the rule reads for the deflate twin
            _, _, _, _, rec_twin = raw_of(twin, 'stream', host_inflate_above=above)
            order = np.argsort(-sizes, kind='stable')
            taken, host = 0, set()
            for i in order:
                if taken * 100 >= sizes.sum() * 30:
                    break
                taken += sizes[i]
                host.add(int(i))
            assert set(np.nonzero(~on_gpu)[0].tolist()) == host and 0 < len(host) < 12
            assert int((in_read_order(rec_twin)['mode'] == fn().RAW_STORED).sum()) > 0
    # one-read files: the batch loader's share, the staged stream inflated and unshuffled
    singles = [sf.write_copy([r], str(tmp_path / (r[0] + '.fast5')), 'shuffle_deflate', None) for r in reads]
    for above in (-30, -100, 9000):
        _, offsets, status, comp, rec = fn().load_batch_raw(singles, 2, above, shuffle='gpu')
        assert not np.asarray(status).any()
        assert np.array_equal(undo(comp, rec, len(want)), want), above
        stored = int((rec['mode'] == fn().RAW_STORED).sum())
        assert stored == 12 if above == -100 else 0 < stored < 12


def test_numpy_s_unshuffle_is_hdf5_s():
    """byte j of element i at j * (N/2) + i"""
    s = np.array([0x0102, 0x0304, -2], dtype=np.int16)
    assert sf.shuffle(s) == bytes([0x02, 0x04, 0xFE, 0x01, 0x03, 0xFF])
    assert np.array_equal(sf.unshuffle(sf.shuffle(s)), s)


def test_a_bad_keyword_is_refused():
    with pytest.raises(ValueError):
        fn().load_batch_raw([], shuffle='device')
    with pytest.raises(ValueError):
        next(fn().stream_raw([], shuffle=True))
    with pytest.raises(ValueError):
        fn()._raw_flags('host', 'GPU')


def test_shuffle_route_reads_the_environment(monkeypatch):
    monkeypatch.delenv('DEEPBINNER_SHUFFLE', raising=False)
    assert fn().shuffle_route() == 'host'
    monkeypatch.setenv('DEEPBINNER_SHUFFLE', 'gpu')
    assert fn().shuffle_route() == 'gpu'
    monkeypatch.setenv('DEEPBINNER_SHUFFLE', 'both')
    with pytest.raises(ValueError):
        fn().shuffle_route()


def defines(header):
    with open(os.path.join(ROOT, 'include', header)) as f:
        return {m.group(1): int(m.group(2).rstrip('u'), 0)
                for m in re.finditer(r'^#define\s+(\w+)\s+(\d+u?)\s*$', f.read(), re.M)}


def test_the_headers_constants_are_python_s():
    from deepbinner_amd import hip_backend
    f5, dbh = defines('deepbinner_fast5.h'), defines('deepbinner_hip.h')
    assert (f5['F5_RAW_ZLIB_SHUFFLE'], f5['F5_RAW_STORED_SHUFFLE'], f5['F5_RAW_FLAG_SHUFFLE_GPU']) == \
        (fn().RAW_ZLIB_SHUFFLE, fn().RAW_STORED_SHUFFLE, fn().RAW_FLAG_SHUFFLE_GPU) == (4, 5, 2)
    assert (dbh['DBH_INFLATE_ZLIB_SHUFFLE'], dbh['DBH_INFLATE_STORED_SHUFFLE']) == \
        (hip_backend.INFLATE_ZLIB_SHUFFLE, hip_backend.INFLATE_STORED_SHUFFLE) == (4, 5)
    assert dbh['DBH_INFLATE_SHUFFLE_REFUSED'] == hip_backend.INFLATE_SHUFFLE_REFUSED
    # outside the statuses in use: zlib's 1-10, VBZ's 1, zstd's 16-28
    assert hip_backend.INFLATE_SHUFFLE_REFUSED > 28
    # the loader's modes are the decoder's
    for name in ('ZLIB', 'STORED', 'VBZ', 'VBZ_ZSTD', 'ZLIB_SHUFFLE', 'STORED_SHUFFLE'):
        assert f5['F5_RAW_' + name] == dbh['DBH_INFLATE_' + name]
