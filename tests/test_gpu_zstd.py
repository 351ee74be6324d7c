"""The zstd stage of VBZ on the GPU: streams of mode DBH_INFLATE_VBZ_ZSTD through dbh_inflate_dev
beside zlib, stored and mode-2 streams.  The output buffer is filled with a sentinel before the
call and the workspace is read back behind it, so that every stream's zstd content - what the
device-only copies, fills and matches of dbh_zstd.hip produced - is held byte for byte against the
decoder's CPU model (which tests/test_zstd_model.py holds against libzstd), and every byte outside
the streams' regions is seen to be untouched."""

import contextlib
import io
import os
import struct
import uuid
import zlib

import numpy as np
import pytest

import vbz_fixtures as vf
import zstd_cases as zc
from conftest import MODEL_DIR
from zstd_gpu import VBZ_ZSTD, run, samples_of

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(vf.zstd_lib() is None, reason='no libzstd.so.1 on this host')]

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, '..', 'deepbinner_amd', 'libdeepbinner_hip.so')


def signal_frames():
    """[(name, frame, content, samples)]: frames whose content is the streamvbyte bytes of a signal -
    the random walks at every level, the constant and the square wave (RLE blocks, long matches
    that overlap their own output), and the same contents as windowed and flushed frames (several
    blocks, treeless literals, repeat tables)."""
    out = []
    for n in zc.SIGNAL_SIZES:
        s = zc.random_walk(n, seed=n)
        packed = vf.streamvbyte(s)
        for level in zc.LEVELS:
            out.append(('walk_%d_l%d' % (n, level), vf.zstd_compress(packed, level), packed, s))
    shaped = [('constant', np.full(60000, 431, dtype=np.int16)),
              ('square', np.tile(np.r_[np.full(50, 400), np.full(50, 620)], 900).astype(np.int16)),
              ('steps', np.repeat(zc.random_walk(700, 5), 97).astype(np.int16)),
              ('walk', zc.random_walk(40000, 11))]
    for name, s in shaped:
        packed = vf.streamvbyte(s)
        for level in (1, 19):
            out.append(('%s_l%d' % (name, level), vf.zstd_compress(packed, level), packed, s))
        out.append((name + '_windowed', zc.with_content_size(
            zc.zstd_compress_adv(packed, [(zc.C_LEVEL, 3), (zc.C_WINDOWLOG, 10)]), len(packed)), packed, s))
        out.append((name + '_flushed', zc.with_content_size(
            zc.zstd_compress_adv(packed, [(zc.C_LEVEL, 3)], range(1200, len(packed), 1200)), len(packed)),
            packed, s))
    return out


def test_signal_frames_beside_zlib_stored_and_vbz_streams(hip):
    items, want, contents = [], [], []
    for k, (name, frame, content, s) in enumerate(signal_frames()):
        n = len(s)
        items.append((struct.pack('<I', 2 * n) + frame, 2 * n, VBZ_ZSTD))
        want.append(s)
        contents.append(content)
        other = [(zlib.compress(s.tobytes(), 1), 0), (s.tobytes(), 1),
                 (struct.pack('<I', 2 * n) + content, 2)][k % 3 if n <= 120000 else 2]
        items.append((other[0], 2 * n, other[1]))
        want.append(s)
        contents.append(None)
    got, status, slots = run(hip, items)
    for i, (g, w) in enumerate(zip(got, want)):
        assert status[i] == 0, (i, items[i][1:], status[i])
        if contents[i] is not None:
            assert bytes(slots[i][:len(contents[i])]) == contents[i], i
        assert np.array_equal(g.view(np.int16), w), (i, items[i][1:])


def test_every_valid_frame_of_the_model_test(hip):
    """All the frames of tests/test_zstd_model.py - every block and literals type, both tree
    descriptions, every sequence mode, the repeat offset - as mode-3 streams: the zstd content in
    the workspace is the frame's content; the streamvbyte stage behind it says what the host's says
    of those bytes (most are not streamvbyte bytes of that many samples: refused with its status 1,
    never with a status of the zstd stage)."""
    frames = zc.valid_frames()
    info = {'blocks': set(), 'literals': set(), 'modes': set(), 'tree': set()}
    items = []
    for name, frame, content in frames:
        w = zc.walk(frame)
        for key in info:
            info[key] |= w[key]
        n = max(len(content), 1)
        items.append((struct.pack('<I', 2 * n) + frame, 2 * n, VBZ_ZSTD))
    assert info['blocks'] == {'raw', 'rle', 'compressed'}
    assert info['literals'] == {'raw', 'rle', 'huffman', 'treeless'} and info['tree'] == {'direct', 'fse'}
    assert len(info['modes']) == 12
    got, status, slots = run(hip, items)
    for i, (name, frame, content) in enumerate(frames):
        assert status[i] in (0, 1), (name, status[i])
        assert bytes(slots[i][:len(content)]) == content, name
        host = samples_of(content, items[i][1] // 2)
        if host is None:
            assert status[i] == 1 and not got[i].any(), name
        else:
            assert status[i] == 0 and np.array_equal(got[i].view(np.int16), host), name


def test_outputs_cut_short_and_zero_extended(hip):
    items, want = [], []
    for n in (5, 200, 4000, 27000, 100000):
        s = zc.random_walk(n, seed=n)
        content = len(vf.streamvbyte(s))
        for level in (1, 19):
            chunk = vf.vbz_chunk(s, level)
            for out_bytes in sorted({max(0, 2 * n - 10), 2 * n + 12, 2 * (n * 3 // 4), 2 * n + 4000}):
                if 4 * out_bytes < content:        # (cut below the workspace rule: may be refused)
                    continue
                items.append((chunk, out_bytes, VBZ_ZSTD))
                expect = np.zeros(out_bytes // 2, dtype=np.int16)
                m = min(n, out_bytes // 2)
                expect[:m] = s[:m]
                want.append(expect)
    got, status, _ = run(hip, items)
    assert not status.any()
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.view(np.int16), w), (i, items[i][1])


def test_a_stream_cut_below_the_workspace_rule_is_refused_for_space(hip):
    s = zc.random_walk(4000, 1)
    got, status, _ = run(hip, [(vf.vbz_chunk(s, 1), 400, VBZ_ZSTD), (vf.vbz_chunk(s, 1), 8000, VBZ_ZSTD)])
    assert status[0] == 27 and not got[0].any()
    assert status[1] == 0 and np.array_equal(got[1].view(np.int16), s)


def test_wide_codes_fit_the_workspace(hip):
    """Deltas that take 3- and 4-byte codes: 4.25 bytes per sample at the most, and the stream's
    own slots hold them when out_bytes covers the original size."""
    r = np.random.RandomState(3)
    samples = r.randint(-32768, 32768, size=20000).astype(np.int16)
    values = r.randint(0, 1 << 32, size=3000, dtype=np.uint64).astype(np.uint32)
    packed = vf.pack_values(values, lengths=np.full(3000, 4))
    chunk = struct.pack('<I', 6000) + vf.zstd_compress(packed, 3)
    got, status, slots = run(hip, [(vf.vbz_chunk(samples, 1, wrap=False), 40000, VBZ_ZSTD),
                                   (chunk, 6000, VBZ_ZSTD)])
    assert list(status) == [0, 0]
    assert np.array_equal(got[0].view(np.int16), samples)
    assert bytes(slots[1][:len(packed)]) == packed
    assert np.array_equal(got[1].view(np.int16), samples_of(packed, 3000))


def test_forty_thousand_streams_in_one_call(hip):
    r = np.random.RandomState(5)
    items, want = [], []
    chunks = [(s, vf.vbz_chunk(s, 1)) for s in (zc.random_walk(int(n), seed=int(n)) for n in r.randint(1, 900, size=50))]
    for k in range(40000):
        s, c = chunks[k % len(chunks)]
        items.append((c, 2 * len(s), VBZ_ZSTD))
        want.append(s)
    got, status, _ = run(hip, items)
    assert not status.any()
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.int16), w)


def test_mutants_as_the_cpu_model(hip):
    """Every mutant of the model's test, and mutants of signal frames sent with their right
    original_size: where the model refuses, the device's status is the model's and the output
    zeros (also where blocks in front of the damage had been stored); where it accepts, the zstd
    content in the workspace is the model's bytes and the streamvbyte stage behind it gives what
    the host's gives for those bytes."""
    model = zc.model_lib(LIB)
    parents = zc.mutant_parents(zc.valid_frames(sizes=(0, 5, 200, 4000, 27000), levels=(1, 3, 19)))
    cases = [(label, m, max(1, len(next(c for n, _, c in parents if n == label.split(':')[0]))))
             for label, m in zc.mutants(parents)]
    signal = [(name, frame, content) for name, frame, content, s in signal_frames()
              if name in ('walk_4000_l1', 'walk_4000_l19', 'square_l19', 'steps_flushed', 'walk_flushed',
                          'constant_windowed')]
    sizes = {name: len(s) for name, _, _, s in signal_frames()}
    cases += [(label, m, sizes[label.split(':')[0]]) for label, m in zc.mutants(signal, seed=77)]
    assert len(cases) >= 1000
    items, verdicts = [], []
    for label, m, n in cases:
        items.append((struct.pack('<I', 2 * n) + m, 2 * n, VBZ_ZSTD))
        verdicts.append(zc.model_decode(model, m, 8 * n))
    got, status, slots = run(hip, items)
    decoded = 0
    for i, (label, m, n) in enumerate(cases):
        st, content = verdicts[i]
        if st != 0:
            assert status[i] == st, (label, status[i], st)
            assert not got[i].any(), label
            continue
        assert status[i] in (0, 1), (label, status[i])
        assert bytes(slots[i][:len(content)]) == content, label
        host = samples_of(content, n)
        if host is None:
            assert status[i] == 1 and not got[i].any(), label
        else:
            decoded += 1
            assert status[i] == 0 and np.array_equal(got[i].view(np.int16), host), label
    assert decoded >= 50                   # (accepted mutants that decode all the way to samples)


def test_damaged_streamvbyte_bytes_inside_intact_frames(hip):
    items = [(chunk, 6000, VBZ_ZSTD) for _, chunk in zc.damaged_vbz_chunks()]
    good = zc.random_walk(3000, 99)
    items.insert(3, (vf.vbz_chunk(good, 1), 6000, VBZ_ZSTD))
    got, status, _ = run(hip, items)
    for i, (g, st) in enumerate(zip(got, status)):
        if i == 3:
            assert st == 0 and np.array_equal(g.view(np.int16), good)
        else:
            assert st == 1 and not g.any(), i


# ---- end to end ---------------------------------------------------------------------------------
def vbz_singles(tmp_path):
    paths = []
    for k, path in enumerate(p for p in vf.golden_fast5() if '/single/' in p):
        paths.append(vf.write_vbz_copy(vf.read_all(path), str(tmp_path / os.path.basename(path)),
                                       vf.VARIANTS[k % len(vf.VARIANTS)]))
    return paths


def test_classify_pair_deflated_on_mode_3_records_is_mode_2(hip, tmp_path):
    from deepbinner_amd import fast5_native
    from deepbinner_amd.model_format import ModelWeights
    start = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'))[0])
    end = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw'))[0])
    paths = vbz_singles(tmp_path)
    results = {}
    for route in ('host', 'gpu'):
        ids, offsets, status, comp, records = fast5_native.load_batch_raw(paths, 4, vbz_zstd=route)
        assert list(status) == [0] * len(paths)
        assert (records['mode'] == (3 if route == 'gpu' else 2)).any()
        if route == 'host':
            assert not (records['mode'] == 3).any()
        calls, stream_status, samples = hip.classify_pair_deflated(start, end, comp, records, offsets,
                                                                   6144, 0.5, want_samples=True)
        assert not stream_status.any(), route
        results[route] = (list(ids), calls, samples)
    assert results['gpu'][0] == results['host'][0]
    assert np.array_equal(results['gpu'][1], results['host'][1])
    assert np.array_equal(results['gpu'][2], results['host'][2])
    start.close()
    end.close()


FILTER_WARNING = 'Warning: skipping reads whose signal is compressed with a filter'


def test_classify_and_realtime_with_the_gpu_route_print_the_host_route_s_tables(hip, tmp_path, monkeypatch,
                                                                               capsys):
    """`classify --native` over one-read VBZ files and `realtime` over a VBZ container with
    DEEPBINNER_VBZ_ZSTD=gpu and without it: the same tables; the read with damage inside its zstd
    frame is skipped with the filter warning on both routes."""
    from deepbinner_amd import classify, deepbinner as cli, hdf5_write
    from test_gpu_streaming import run_realtime
    rng = np.random.default_rng(41)

    def damaged(s):
        chunk = bytearray(vf.vbz_chunk(s, 1))
        for at in range(12, 20):                       # inside the frame: the literals section's head
            chunk[at] ^= 0xFF
        return bytes(chunk)

    reads = []
    for k in range(8):
        n = int(rng.integers(3000, 9000))
        levels = np.repeat(rng.normal(450, 80, n // 8 + 1), 8)[:n]
        s = np.clip(np.rint(levels + rng.normal(0, 8, n)), 0, 2047).astype(np.int16)
        reads.append((str(uuid.UUID(bytes=rng.bytes(16), version=4)), s, damaged if k == 3 else None))
    bad = reads[3][0]
    assert zc.zstd_decompress(damaged(reads[3][1])[4:], 1 << 20)[0] is None     # (libzstd refuses it)
    single, multi = tmp_path / 'single', tmp_path / 'multi'
    single.mkdir()
    multi.mkdir()
    filters = [vf.signal_filter(s, encode=e) for _, s, e in reads]
    (multi / 'reads.fast5').write_bytes(hdf5_write.multi_read_fast5_bytes(
        [(rid, s, None, None, sf) for (rid, s, _), sf in zip(reads, filters)]))
    for (rid, s, _), sf in zip(reads, filters):
        (single / (rid + '.fast5')).write_bytes(hdf5_write.single_read_fast5_bytes(rid, s, signal_filter=sf))
    monkeypatch.setenv('DEEPBINNER_RAW_CLASSIFY_MIN_FILES', '1')
    monkeypatch.setenv('DEEPBINNER_GPU_INFLATE', '1')
    monkeypatch.delenv('DEEPBINNER_HOST_INFLATE_SHARE', raising=False)

    def route(name):
        if name == 'gpu':
            monkeypatch.setenv('DEEPBINNER_VBZ_ZSTD', 'gpu')
        else:
            monkeypatch.delenv('DEEPBINNER_VBZ_ZSTD', raising=False)
        monkeypatch.setattr(classify, '_FILTER_WARNING_GIVEN', False)

    tables = {}
    for name in ('host', 'gpu'):
        route(name)
        capsys.readouterr()
        cli.main(['classify', '--native', str(single)])
        done = capsys.readouterr()
        rows = done.out.splitlines()
        tables[name] = (rows[0], sorted(r.split('\t') for r in rows[1:]))
        assert done.err.count(FILTER_WARNING) == 1, (name, done.err)
        assert bad not in [r[0] for r in tables[name][1]] and len(tables[name][1]) == 7
    assert tables['gpu'] == tables['host']
    streamed = {}
    for name in ('host', 'gpu'):
        route(name)
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            table, _ = run_realtime(str(multi), str(tmp_path / ('out_' + name)), 1, monkeypatch, capsys)
        streamed[name] = sorted(r[:2] for r in table)
        assert err.getvalue().count(FILTER_WARNING) == 1, (name, err.getvalue())
        assert len(streamed[name]) == 7
    assert streamed['gpu'] == streamed['host']
