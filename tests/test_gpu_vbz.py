"""VBZ on the GPU: streams of mode DBH_INFLATE_VBZ through dbh_inflate beside zlib and stored
streams, and VBZ raw batches through dbh_classify_pair_deflated(_verbose) and the raw stream of
a 4,000-read container ("VBZ"); and, end to end, reads whose damage or unusual encoding
sits inside an intact zstd frame, with the GPU decoding and with the host decoding.  The decoder
itself against its reference: tests/test_gpu_vbz_codes.py."""

import os
import struct
import uuid
import zlib

import numpy as np
import pytest

import vbz_fixtures as vf
from conftest import MODEL_DIR

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(vf.zstd_lib() is None, reason='no libzstd.so.1 on this host')]


def payload(samples, original_size=None):
    """what the loader hands the GPU for a VBZ chunk: u32 original_size + streamvbyte bytes"""
    size = 2 * len(samples) if original_size is None else original_size
    return struct.pack('<I', size) + vf.streamvbyte(samples)


def test_vbz_streams_beside_zlib_and_stored_streams(hip):
    from deepbinner_amd import fast5_native
    rng = np.random.default_rng(2020)
    kinds, pieces, streams, want = [], [], [], []
    comp_at = out_at = 0
    for k in range(3000):
        n = int(rng.choice([0, 1, 3, 4, 5, 63, 1023, 1024, 1025, 4099, 27000, 120000]) if k % 7 == 0
                else rng.integers(1, 40000))
        step = int(rng.choice([3, 40, 700, 70000]))
        samples = np.cumsum(rng.integers(-step, step + 1, n)).astype(np.int16)
        mode = [2, 2, 2, 0, 1][k % 5]
        out_bytes = 2 * n
        if mode == 2:
            data = payload(samples)
            if k % 11 == 0 and n > 8:            # a partial last chunk: less wanted than held
                out_bytes = 2 * (n - 5)
            if k % 13 == 0:                       # a short chunk: zero-extended
                out_bytes = 2 * n + 10
        elif mode == 0:
            data = zlib.compress(samples.tobytes(), 1)
        else:
            data = samples.tobytes()
        expect = np.zeros(out_bytes // 2, dtype=np.int16)
        m = min(n, out_bytes // 2)
        expect[:m] = samples[:m]
        if mode == 2:
            host = fast5_native.vbz_decode(data, (0, 2, 1, 0), n)
            assert np.array_equal(host, samples)
        out_at += (rng.integers(0, 8) * 2)         # odd alignments of the output
        streams.append((comp_at, len(data), out_at, out_bytes, mode, 0))
        pieces.append(data)
        want.append(expect)
        kinds.append(mode)
        comp_at += len(data)
        out_at += out_bytes
    # malformed VBZ streams: one byte short, one long, an odd size, control bytes beyond the stream
    bad = []
    good = np.arange(5000, dtype=np.int16)
    for data in (payload(good)[:-1], payload(good) + b'\x00', payload(good, 2 * 5000 - 1),
                 struct.pack('<I', 400000) + b'\x01' * 10):
        streams.append((comp_at, len(data), out_at, 10000, 2, 0))
        pieces.append(data)
        bad.append(len(streams) - 1)
        want.append(np.zeros(5000, dtype=np.int16))
        comp_at += len(data)
        out_at += 10000
    comp = np.frombuffer(b''.join(pieces), dtype=np.uint8)
    records = np.array(streams, dtype=hip.INFLATE_STREAM)
    out_total = out_at + 64
    out, status, ms = hip.inflate(comp, records, out_total)
    raw = np.asarray(out, dtype=np.uint8)
    for i, rec in enumerate(records):
        got = raw[rec['out_offset']:rec['out_offset'] + rec['out_bytes']].view(np.int16)
        if i in bad:
            assert status[i] != 0 and not got.any(), i
        else:
            assert status[i] == 0, (i, kinds[i] if i < len(kinds) else None)
            assert np.array_equal(got, want[i]), (i, kinds[i])
    print('%d streams (%d VBZ) in %.2f ms' % (len(records), kinds.count(2), ms))


def vbz_singles(tmp_path):
    paths = []
    for k, path in enumerate(p for p in vf.golden_fast5() if '/single/' in p):
        reads = vf.read_all(path)
        paths.append(vf.write_vbz_copy(reads, str(tmp_path / os.path.basename(path)),
                                       vf.VARIANTS[k % len(vf.VARIANTS)]))
    return paths


@pytest.mark.parametrize('verbose', [False, True])
def test_classify_pair_deflated_over_vbz_is_classify_pair_i16(hip, tmp_path, verbose):
    from deepbinner_amd import fast5_native
    from deepbinner_amd.model_format import ModelWeights
    start = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'))[0])
    end = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw'))[0])
    paths = vbz_singles(tmp_path)
    ids, offsets, status, comp, records = fast5_native.load_batch_raw(paths, 4)
    assert list(status) == [0] * len(paths) and (records['mode'] == 2).any()
    _, samples, s_offsets, s_status = fast5_native.load_batch(paths, None, 4)
    assert np.array_equal(offsets, s_offsets)
    for s_model, e_model in ((start, None), (None, end), (start, end)):
        got = hip.classify_pair_deflated(s_model, e_model, comp, records, offsets, 6144, 0.5,
                                         want_sides=verbose, want_samples=not verbose)
        want = hip.classify_pair(s_model, e_model, samples, offsets, 6144, 0.5,
                                     want_sides=verbose, want_probs=verbose)
        assert not got[1].any()
        if verbose:
            assert np.array_equal(got[0], want[0])
            sides = got[2]
            for j, side in enumerate(('start', 'end')):
                if sides[side + '_calls'] is not None:
                    assert np.array_equal(sides[side + '_calls'], want[1][j])
                    assert np.array_equal(sides[side + '_probs'], want[2][j])
        else:
            assert np.array_equal(got[0], want)
            assert np.array_equal(got[2], samples)
    start.close()
    end.close()


def test_a_vbz_container_streams_to_the_calls_of_its_deflate_twin(hip, tmp_path):
    from deepbinner_amd import fast5_native, hdf5_write
    from deepbinner_amd.model_format import ModelWeights
    rng = np.random.default_rng(32020)
    reads = []
    for k in range(4000):
        n = int(rng.integers(2000, 9000))
        levels = np.repeat(rng.normal(450, 80, n // 8 + 1), 8)[:n]
        signal = np.clip(np.rint(levels + rng.normal(0, 8, n)), 0, 2047).astype(np.int16)
        reads.append((str(uuid.UUID(bytes=rng.bytes(16), version=4)), signal))
    twin = str(tmp_path / 'deflate.fast5')
    with open(twin, 'wb') as f:
        f.write(hdf5_write.multi_read_fast5_bytes(reads))
    vbz = vf.write_vbz_copy(reads, str(tmp_path / 'vbz.fast5'), vf.VARIANTS[0], multi=True)
    start = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'))[0])
    end = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw'))[0])
    calls = []
    for path in (twin, vbz):
        for index, ids, offsets, status, comp, records in fast5_native.stream_raw([path], threads=8):
            assert list(status) == [0] * 4000
            assert (records['mode'] == (2 if path == vbz else 0)).all()
            got, stream_status, samples = hip.classify_pair_deflated(
                start, end, comp, records, offsets, 6144, 0.5, want_samples=True)
            assert not stream_status.any()
            by_id = dict(reads)
            assert all(np.array_equal(samples[offsets[i]:offsets[i + 1]], by_id[ids[i]])
                       for i in range(0, 4000, 97))
            calls.append(got)
    assert np.array_equal(calls[0], calls[1])
    start.close()
    end.close()


# ---- end to end: damage and unusual encodings INSIDE an intact zstd frame -----------------------
def unusual_reads():
    """[(read id, signal, encode or None)]: ordinary VBZ reads and, between them, 'damaged' (its
    streamvbyte bytes a refused mutant of unchanged length - one control code changed - compressed
    again, so that the zstd frame is intact and of a plausible size: only the streamvbyte
    self-check can tell), 'forced' (every value on a 3- or 4-byte code) and 'unwrapped' (a
    full-range signal, its deltas taken in 32 bits) -> (reads, {kind: read id})"""
    import vbz_reference as ref
    rng = np.random.default_rng(13)

    def squiggle(n):
        levels = np.repeat(rng.normal(450, 80, n // 8 + 1), 8)[:n]
        return np.clip(np.rint(levels + rng.normal(0, 8, n)), 0, 2047).astype(np.int16)

    def damaged(s):
        good = struct.pack('<I', 2 * len(s)) + vf.streamvbyte(s)
        mutant = bytearray(good)
        i = len(s) // 3
        ref.set_code(mutant, i, int(ref.code_lengths(good)[i]) % 4)      # (one byte longer, or 4 -> 1)
        assert len(mutant) == len(good) and ref.decode(good) is not None
        assert ref.decode(bytes(mutant)) is None
        return bytes(mutant[:4]) + vf.zstd_compress(bytes(mutant[4:]))

    def forced(s):
        d = np.diff(np.concatenate([[0], s.astype(np.int64)]))
        u = ((d << 1) ^ (d >> 63)).astype(np.uint32)
        payload = struct.pack('<I', 2 * len(s)) + vf.pack_values(u, rng.integers(3, 5, len(s)))
        assert set(ref.code_lengths(payload).tolist()) == {3, 4}
        assert np.array_equal(ref.decode(payload), s)
        return payload[:4] + vf.zstd_compress(payload[4:])

    def unwrapped(s):
        chunk = vf.vbz_chunk(s, 1, wrap=False)
        assert (ref.code_lengths(struct.pack('<I', 2 * len(s)) + vf.streamvbyte(s, wrap=False)) == 3).any()
        return chunk

    kinds = [None, None, damaged, None, forced, None, unwrapped, None]
    reads, special = [], {}
    for encode in kinds:
        n = int(rng.integers(3000, 9000))
        signal = rng.integers(-32768, 32768, n).astype(np.int16) if encode is unwrapped else squiggle(n)
        rid = str(uuid.UUID(bytes=rng.bytes(16), version=4))
        reads.append((rid, signal, encode))
        if encode is not None:
            special[encode.__name__] = rid
    return reads, special


def write_unusual(tmp_path, reads):
    """the reads as a VBZ container, as a directory of one-read VBZ files, and the deflate twins
    of both -> {'multi': dir, 'multi_twin': dir, 'single': dir, 'single_twin': dir}"""
    from deepbinner_amd import hdf5_write
    dirs = {}
    for name in ('multi', 'multi_twin', 'single', 'single_twin'):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
    filters = [vf.signal_filter(s, encode=encode) for _, s, encode in reads]
    (dirs['multi'] / 'reads.fast5').write_bytes(hdf5_write.multi_read_fast5_bytes(
        [(rid, s, None, None, sf) for (rid, s, _), sf in zip(reads, filters)]))
    (dirs['multi_twin'] / 'reads.fast5').write_bytes(hdf5_write.multi_read_fast5_bytes(
        [(rid, s) for rid, s, _ in reads]))
    for (rid, s, _), sf in zip(reads, filters):
        (dirs['single'] / (rid + '.fast5')).write_bytes(
            hdf5_write.single_read_fast5_bytes(rid, s, signal_filter=sf))
        (dirs['single_twin'] / (rid + '.fast5')).write_bytes(hdf5_write.single_read_fast5_bytes(rid, s))
    return {k: str(v) for k, v in dirs.items()}


FILTER_WARNING = 'Warning: skipping reads whose signal is compressed with a filter'


def test_damage_inside_an_intact_zstd_frame_end_to_end(hip, tmp_path, monkeypatch, capsys):
    """`classify --native` over one-read files and `realtime` over a container, with the GPU
    decoding the streams and with the host decoding them: the same table; the damaged read skipped
    with the filter warning either way; the reads with forced long codes and with unwrapped deltas
    called as their deflate twins are."""
    import contextlib
    import io
    from deepbinner_amd import classify, deepbinner as cli
    from test_gpu_streaming import run_realtime
    reads, special = unusual_reads()
    assert set(special) == {'damaged', 'forced', 'unwrapped'}
    dirs = write_unusual(tmp_path, reads)
    monkeypatch.setenv('DEEPBINNER_RAW_CLASSIFY_MIN_FILES', '1')
    monkeypatch.delenv('DEEPBINNER_HOST_INFLATE_SHARE', raising=False)

    def classify_table(directory, gpu_inflate):
        monkeypatch.setenv('DEEPBINNER_GPU_INFLATE', gpu_inflate)
        monkeypatch.setattr(classify, '_FILTER_WARNING_GIVEN', False)
        capsys.readouterr()
        cli.main(['classify', '--native', directory])
        done = capsys.readouterr()
        rows = done.out.splitlines()
        return rows[0], sorted(r.split('\t') for r in rows[1:]), done.err

    def realtime_table(directory, out, gpu_inflate):
        monkeypatch.setenv('DEEPBINNER_GPU_INFLATE', gpu_inflate)
        monkeypatch.setattr(classify, '_FILTER_WARNING_GIVEN', False)
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            table, _ = run_realtime(directory, str(tmp_path / out), 1, monkeypatch, capsys)
        return sorted(r[:2] for r in table), err.getvalue()

    kept = sorted(rid for rid, _, _ in reads if rid != special['damaged'])
    header, want, err = classify_table(dirs['single_twin'], '0')
    assert [r[0] for r in want] == sorted(rid for rid, _, _ in reads) and FILTER_WARNING not in err
    want = [r for r in want if r[0] != special['damaged']]
    for flag in ('1', '0'):
        got_header, got, err = classify_table(dirs['single'], flag)
        assert got_header == header and [r[0] for r in got] == kept, flag
        assert got == want, flag
        assert err.count(FILTER_WARNING) == 1, (flag, err)
    twin, err = realtime_table(dirs['multi_twin'], 'out_twin', '1')
    assert FILTER_WARNING not in err and len(twin) == len(reads)
    assert [r for r in twin if r[0] != special['damaged']] == want
    for flag in ('1', '0'):
        got, err = realtime_table(dirs['multi'], 'out_' + flag, flag)
        assert got == want, flag
        assert err.count(FILTER_WARNING) == 1, (flag, err)


def test_unusual_vbz_batches_through_classify_pair_deflated(hip, tmp_path):
    """the raw batches of the same files and container: the original samples for the reads with
    forced long codes and with unwrapped deltas, a non-zero stream status for the damaged read
    alone, and the calls the host-decoded samples give"""
    from deepbinner_amd import fast5_native
    from deepbinner_amd.model_format import ModelWeights
    reads, special = unusual_reads()
    dirs = write_unusual(tmp_path, reads)
    by_id = {rid: s for rid, s, _ in reads}
    start = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'))[0])
    end = hip.HipModel(ModelWeights.load(os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw'))[0])
    paths = sorted(os.path.join(dirs['single'], n) for n in os.listdir(dirs['single']))
    batches = [fast5_native.load_batch_raw(paths, 4)]
    batches += [b[1:] for b in fast5_native.stream_raw([os.path.join(dirs['multi'], 'reads.fast5')],
                                                       threads=2)]
    assert len(batches) == 2
    for ids, offsets, status, comp, records in batches:
        assert list(status) == [0] * len(reads) and (records['mode'] == 2).all()
        calls, stream_status, samples = hip.classify_pair_deflated(
            start, end, comp, records, offsets, 6144, 0.5, want_samples=True)
        refused = {ids[int(r)] for r in records['read'][stream_status != 0]}
        assert refused == {special['damaged']}
        clean = np.zeros(len(samples), dtype=np.int16)
        for i, rid in enumerate(ids):
            got = samples[offsets[i]:offsets[i + 1]]
            if rid == special['damaged']:
                assert not got.any()
            else:
                assert np.array_equal(got, by_id[rid]), rid
                clean[offsets[i]:offsets[i + 1]] = by_id[rid]
        assert np.array_equal(calls, hip.classify_pair(start, end, clean, offsets, 6144, 0.5))
    start.close()
    end.close()
