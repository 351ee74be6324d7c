"""VBZ-compressed fast5 (ONT's HDF5 filter 32020, version 0): both readers' decoders, both readers
over VBZ copies of the golden fast5 files, every API of the native loader, the refusals and the
self-checks ("VBZ").  Host only."""

import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import vbz_fixtures as vf
import vbz_reference
from deepbinner_amd import fast5_native, hdf5_lite, load_fast5s

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CD = (0, 2, 1, 1)

pytestmark = pytest.mark.skipif(vf.zstd_lib() is None, reason='no libzstd.so.1 on this host')


def both_decoders(chunk, cd, max_samples):
    native = fast5_native.vbz_decode(chunk, cd, max_samples)
    try:
        python = np.frombuffer(hdf5_lite.vbz_decode(chunk, cd, 2 * max_samples), dtype=np.int16)
    except hdf5_lite.Hdf5FormatError:
        python = None
    return native, python


UNWRAPPED = ('codes',)


def codec_cases():
    rng = np.random.default_rng(32020)
    cases = {'n%d' % n: rng.integers(-32768, 32768, n).astype(np.int16)
             for n in (0, 1, 3, 4, 5, 4 * 37 + 1, 4 * 37 + 2, 4 * 37 + 3)}
    cases['jumps'] = np.array([-32768, 32767] * 50 + [0, -32768, 32767, -1], dtype=np.int16)
    squiggle = np.cumsum(rng.integers(-40, 41, 10 ** 6)) + 500
    cases['n1e6'] = squiggle.astype(np.int16)
    # deltas that need 1, 2 and 3 bytes, in every position of a control byte (five deltas that
    # sum to zero, over and over; encoded with the deltas taken in 32 bits: UNWRAPPED below)
    cases['codes'] = (np.cumsum(np.array([1, 200, -300, 40000, -39901] * 64)) - 20000).astype(np.int16)
    return cases


@pytest.mark.parametrize('name', sorted(codec_cases()))
@pytest.mark.parametrize('level', [1, 0])
def test_codec_round_trip_through_both_decoders(name, level):
    samples = codec_cases()[name]
    chunk = vf.vbz_chunk(samples, level, wrap=name not in UNWRAPPED)
    if name == 'codes':
        lengths = vbz_reference.code_lengths(struct.pack('<I', 2 * len(samples)) +
                                             vf.streamvbyte(samples, wrap=False))
        assert {(int(n), k % 4) for k, n in enumerate(lengths)} >= {
            (n, at) for n in (1, 2, 3) for at in range(4)}
    native, python = both_decoders(chunk, CD[:3] + (level,), len(samples))
    assert native is not None and python is not None
    assert np.array_equal(native, samples) and np.array_equal(python, samples)


def test_every_two_bit_code_decodes():
    """values forced onto 1-, 2-, 3- and 4-byte codes (a writer may choose a longer code than the
    value needs) decode the same"""
    rng = np.random.default_rng(4)
    u = rng.integers(0, 200, 4096).astype(np.uint32)
    lengths = np.tile(np.arange(1, 5), 1024)
    packed = vf.pack_values(u, lengths)
    assert set(np.frombuffer(packed[:1024], np.uint8).tolist()) == {0b11100100}
    want = np.cumsum(((u >> 1) ^ (0 - (u & 1))).astype(np.uint32), dtype=np.uint32).astype(np.uint16).view(np.int16)
    chunk = struct.pack('<I', 2 * len(u)) + vf.zstd_compress(packed)
    native, python = both_decoders(chunk, CD, len(u))
    assert np.array_equal(native, want) and np.array_equal(python, want)


@pytest.fixture(scope='module')
def copies(tmp_path_factory):
    """(original reads, VBZ copy) of each of the 42 golden fast5 files"""
    d = tmp_path_factory.mktemp('vbz')
    out = []
    for k, path in enumerate(vf.golden_fast5()):
        reads = vf.read_all(path)
        copy = vf.write_vbz_copy(reads, str(d / ('%02d_%s' % (k, os.path.basename(path)))),
                                 vf.VARIANTS[k % len(vf.VARIANTS)])
        out.append((path, reads, copy))
    return out


def test_the_copies_are_vbz_and_cover_every_shape(copies):
    assert len(copies) == 42
    for _, reads, copy in copies:
        data = open(copy, 'rb').read()
        assert any(len(s) for _, s in reads) == (struct.pack('<H', vf.VBZ) in data)


def test_both_readers_return_the_original_samples(copies):
    for _, reads, copy in copies:
        got = vf.read_all(copy)
        assert [r for r, _ in got] == [r for r, _ in reads]
        assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(got, reads))
        ids, samples, offsets, status = fast5_native.load_reads(copy)
        assert list(status) == [0] * len(reads)
        assert list(ids) == [r for r, _ in reads]
        for i, (_, s) in enumerate(reads):
            assert np.array_equal(samples[offsets[i]:offsets[i + 1]], s)
        if len(reads) == 1 and 'multi' not in os.path.basename(copy):
            rid, signal = fast5_native.get_read_id_and_signal(copy)
            assert rid == reads[0][0] and np.array_equal(signal, reads[0][1])
            rid, signal = load_fast5s._python_get_read_id_and_signal(copy)
            assert rid == reads[0][0] and np.array_equal(signal, reads[0][1])


def decode_raw(comp, records, offsets):
    """a raw batch decoded on the host: what the GPU decoders are to produce"""
    out = np.zeros(int(offsets[-1]), dtype=np.int16)
    for rec in records:
        a, b = int(rec['comp_offset']), int(rec['comp_offset'] + rec['comp_bytes'])
        o, n = int(rec['out_offset']) // 2, int(rec['out_bytes']) // 2
        if rec['mode'] == fast5_native.RAW_VBZ:
            got = fast5_native.vbz_decode(comp[a:b], (0, 2, 1, 0), 1 << 24)
            assert got is not None
        elif rec['mode'] == fast5_native.RAW_ZLIB:
            import zlib
            got = np.frombuffer(zlib.decompress(bytes(comp[a:b])), dtype=np.int16)
        else:
            got = np.frombuffer(bytes(comp[a:b]), dtype=np.int16)
        got = got[:n]
        out[o:o + len(got)] = got
    return out


def test_every_native_api_agrees(copies):
    singles = [c for _, r, c in copies if len(r) == 1 and len(r[0][1]) and 'multi' not in c]
    want = [vf.read_all(c)[0] for c in singles]
    ids, samples, offsets, status = fast5_native.load_batch(singles, None, 4)
    assert list(status) == [0] * len(singles)
    for i, (rid, s) in enumerate(want):
        assert ids[i] == rid and np.array_equal(samples[offsets[i]:offsets[i + 1]], s)
    # a kept end: first and last 500 samples
    ids, samples, offsets, status = fast5_native.load_batch(singles, 500, 4)
    for i, (_, s) in enumerate(want):
        keep = s if len(s) <= 1000 else np.concatenate([s[:500], s[-500:]])
        assert np.array_equal(samples[offsets[i]:offsets[i + 1]], keep)
    # raw, one-read files: the VBZ chunks handed over with their zstd stage undone
    ids, offsets, status, comp, records = fast5_native.load_batch_raw(singles, 4)
    assert list(status) == [0] * len(singles)
    assert (records['mode'] == fast5_native.RAW_VBZ).sum() >= len(singles) // 2
    decoded = decode_raw(comp, records, offsets)
    for i, (_, s) in enumerate(want):
        assert np.array_equal(decoded[offsets[i]:offsets[i + 1]], s)
    # containers: the sample stream and the raw stream
    multis = [(r, c) for _, r, c in copies if len(r) > 1]
    paths = [c for _, c in multis]
    for index, ids, samples, offsets, status in fast5_native.stream_reads(paths, threads=4):
        reads = multis[index][0]
        assert list(ids) == [r for r, _ in reads]
        for i, (_, s) in enumerate(reads):
            assert np.array_equal(samples[offsets[i]:offsets[i + 1]], s)
    seen = 0
    for item in fast5_native.stream_raw(paths, threads=4):
        index, ids, offsets, status, comp, records = item
        reads = multis[index][0]
        assert list(status) == [0] * len(reads)
        assert (records['mode'] == fast5_native.RAW_VBZ).any()
        decoded = decode_raw(comp, records, offsets)
        for i, (_, s) in enumerate(reads):
            assert np.array_equal(decoded[offsets[i]:offsets[i + 1]], s)
        seen += 1
    assert seen == len(paths)


def refused_file(tmp_path, name, cd=CD, encode=None, samples=None):
    if samples is None:
        samples = (np.cumsum(np.random.default_rng(1).integers(-30, 31, 5000)) + 400).astype(np.int16)
    path = str(tmp_path / (name + '.fast5'))
    sf = vf.signal_filter(samples, cd=cd, encode=encode)
    with open(path, 'wb') as f:
        from deepbinner_amd import hdf5_write
        f.write(hdf5_write.single_read_fast5_bytes('read-' + name, samples, signal_filter=sf))
    return path


def refusal_cases():
    return {
        'version_1': dict(cd=(1, 2, 1, 1)),
        'int32': dict(cd=(0, 4, 1, 1)),
        'no_delta': dict(cd=(0, 2, 0, 1)),
        'two_values': dict(cd=(0, 2)),
        'odd_size': dict(encode=lambda s: vf.vbz_chunk(s, 1, original_size=2 * len(s) - 1)),
        'too_large': dict(encode=lambda s: vf.vbz_chunk(s, 1, original_size=2 * len(s) + 2)),
        'truncated_zstd': dict(encode=lambda s: vf.vbz_chunk(s, 1)[:-3]),
        'payload_short': dict(cd=(0, 2, 1, 0), encode=lambda s: vf.vbz_chunk(s, 0)[:-1]),
        'payload_long': dict(cd=(0, 2, 1, 0), encode=lambda s: vf.vbz_chunk(s, 0) + b'\0'),
        'zstd_payload_long': dict(encode=lambda s: struct.pack('<I', 2 * len(s)) +
                                  vf.zstd_compress(vf.streamvbyte(s) + b'\0')),
    }


def assert_refused(path):
    assert fast5_native.get_read_id_and_signal(path) == (None, None)
    assert load_fast5s._python_get_read_id_and_signal(path) == (None, None)
    assert list(fast5_native.load_batch([path], 0, 1)[3]) == [fast5_native.F5_ERR_FILTER]
    assert list(fast5_native.load_reads(path)[3]) == [fast5_native.F5_ERR_FILTER]
    # the raw route checks sizes and zstd on the host; what only the streamvbyte stage can tell
    # is the GPU decoder's to refuse (then the host decodes the read itself, and refuses it)
    ids, offsets, status, comp, records = fast5_native.load_batch_raw([path], 1)
    if list(status) != [fast5_native.F5_ERR_FILTER]:
        assert list(status) == [0] and list(records['mode']) == [fast5_native.RAW_VBZ]
        rec = records[0]
        payload = comp[rec['comp_offset']:rec['comp_offset'] + rec['comp_bytes']]
        assert fast5_native.vbz_decode(payload, (0, 2, 1, 0), 1 << 20) is None


@pytest.mark.parametrize('name', sorted(refusal_cases()))
def test_refusals_are_filter_errors_in_both_readers(tmp_path, name):
    assert_refused(refused_file(tmp_path, name, **refusal_cases()[name]))


def test_a_missing_libzstd_refuses_vbz(tmp_path):
    path = refused_file(tmp_path, 'fine')
    assert fast5_native.get_read_id_and_signal(path)[0] == 'read-fine'
    code = ('import sys; sys.path.insert(0, {!r}); sys.path.insert(0, {!r}); import test_vbz; '
            'test_vbz.assert_refused({!r}); print("refused")').format(
                REPO, os.path.join(REPO, 'tests'), path)
    env = dict(os.environ, DEEPBINNER_ZSTD_LIB='/nonexistent/libzstd.so.1')
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True,
                         cwd=REPO, timeout=300)
    assert out.returncode == 0 and 'refused' in out.stdout, out.stderr


def test_byte_mutations_never_crash(copies, tmp_path):
    """several hundred damaged copies: a status in range for every read, samples only as the
    originals or not at all"""
    rng = np.random.default_rng(7)
    sources = [c for _, r, c in copies if len(r) == 1 and len(r[0][1])][:12]
    for k in range(360):
        data = bytearray(open(sources[k % len(sources)], 'rb').read())
        for _ in range(1 + k % 3):
            data[int(rng.integers(0, len(data)))] ^= int(rng.integers(1, 256))
        path = str(tmp_path / ('m%d.fast5' % k))
        with open(path, 'wb') as f:
            f.write(bytes(data))
        status = fast5_native.load_batch([path], 0, 1)[3]
        assert 0 <= int(status[0]) <= fast5_native.F5_ERR_EXISTS
        try:
            for st in fast5_native.load_reads(path)[3]:
                assert 0 <= int(st) <= fast5_native.F5_ERR_EXISTS
        except fast5_native.Fast5NativeError:          # (the file as a whole refused)
            pass
        raw_status = fast5_native.load_batch_raw([path], 1)[2]
        assert 0 <= int(raw_status[0]) <= fast5_native.F5_ERR_EXISTS
        try:
            load_fast5s._python_get_read_id_and_signal(path)
        except SystemExit:                 # (a mutation that makes it look like a container)
            pass
        os.unlink(path)


def test_classify_prints_the_table_of_the_originals(copies, tmp_path, oracle_backend, capsys,
                                                    monkeypatch):
    from deepbinner_amd import deepbinner as cli
    singles = [(p, c) for p, r, c in copies if '/single/' in p]
    orig, vbz = tmp_path / 'orig', tmp_path / 'vbz'
    orig.mkdir()
    vbz.mkdir()
    for p, c in singles:
        os.symlink(p, str(orig / os.path.basename(p)))
        os.symlink(c, str(vbz / os.path.basename(p)))
    model = os.path.join(REPO, 'deepbinner_amd', 'models', 'EXP-NBD103_read_starts.dbw')
    tables = []
    for d in (orig, vbz):
        monkeypatch.setattr(sys, 'argv', ['deepbinner', 'classify', '--start_model', model, str(d)])
        cli.main()
        tables.append(capsys.readouterr().out)
    assert tables[0] == tables[1] and tables[0].count('\n') == len(singles) + 1


def test_binning_a_vbz_container_writes_plain_deflate_files(copies, tmp_path):
    """realtime's writer: a VBZ read comes out as a one-read file with one deflated chunk, the
    original samples in it, readable without any VBZ decoder"""
    path, reads, copy = next(c for c in copies if len(c[1]) > 1)
    outs = [str(tmp_path / ('%d.fast5' % i)) for i in range(len(reads))]
    status, _ = fast5_native.write_single_reads(copy, list(range(len(reads))), outs, 2)
    assert list(status) == [0] * len(reads)
    for out, (rid, signal) in zip(outs, sorted(reads)):
        with hdf5_lite.File(out, 'r') as f:
            assert [fid for fid, _ in f['read_%s/Raw/Signal' % rid]._filters()] == [1]
        got = load_fast5s._python_get_read_id_and_signal(out)
        assert got[0] == rid and np.array_equal(got[1], signal)
