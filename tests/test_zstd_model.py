"""
The GPU's zstd decoder run on the host (dbh_zstd_decode_host: deepbinner_amd/csrc/dbh_zstd_core.h,
the kernel's own code with loops standing in for the lanes, the speculative literal rounds
included) held against the system's libzstd: every valid frame decoded, none refused, every byte
equal; wherever the model accepts a damaged frame libzstd accepts it too and the bytes are equal.

DEEPBINNER_ZSTD_MODEL_LIB names another build of the entry point (csrc/Makefile, zstd_asan: the
same source under AddressSanitizer + UBSan).
"""

import os

import pytest

import vbz_fixtures
import zstd_cases as zc

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.environ.get('DEEPBINNER_ZSTD_MODEL_LIB') or os.path.join(HERE, '..', 'deepbinner_amd',
                                                                   'libdeepbinner_hip.so')

pytestmark = pytest.mark.skipif(vbz_fixtures.zstd_lib() is None, reason='no libzstd.so.1 on this machine')


@pytest.fixture(scope='module')
def model():
    return zc.model_lib(LIB)


@pytest.fixture(scope='module')
def frames():
    return zc.valid_frames()


def test_valid_frames_decode_as_libzstd_does(model, frames):
    wrong = []
    for name, frame, content in frames:
        ref, _ = zc.zstd_decompress(frame, len(content))
        assert ref == content, name                 # (libzstd itself accepts every one of them)
        status, got = zc.model_decode(model, frame, len(content))
        if status != 0 or got != content:
            wrong.append((name, status, len(got), len(content)))
    assert not wrong, wrong


def test_valid_frames_with_room_to_spare(model, frames):
    """The literals are parked at the end of the region: its size must not matter."""
    for name, frame, content in frames[::5]:
        status, got = zc.model_decode(model, frame, len(content) + 12345)
        assert (status, got) == (0, content), name


def test_the_frames_hold_every_part_of_the_format(frames):
    seen = {'blocks': set(), 'literals': set(), 'streams': set(), 'modes': set(), 'tree': set()}
    several = False
    for _, frame, _ in frames:
        info = zc.walk(frame)
        for k in seen:
            seen[k] |= info[k]
        several = several or info['n_blocks'] > 1
    assert seen['blocks'] == {'raw', 'rle', 'compressed'}
    assert seen['literals'] == {'raw', 'rle', 'huffman', 'treeless'}
    assert seen['streams'] == {1, 4}
    assert seen['tree'] == {'direct', 'fse'}
    assert seen['modes'] == {(t, m) for t in ('ll', 'of', 'ml')
                             for m in ('predefined', 'rle', 'compressed', 'repeat')}
    assert several
    assert any(zc.walk(f)['repeat_offset'] for _, f, _ in frames)
    assert any(not zc.walk(f)['single'] for _, f, _ in frames)


def test_damaged_frames_never_accepted_where_libzstd_refuses(model, frames):
    parents = zc.mutant_parents(frames)
    assert len(parents) >= 12
    mutants = zc.mutants(parents)
    assert len(mutants) >= 1000
    stricter, accepted = [], 0
    for label, m in mutants:
        capacity = len(next(c for n, _, c in parents if n == label.split(':')[0])) + 300
        status, got = zc.model_decode(model, m, capacity)
        ref, _ = zc.zstd_decompress(m, capacity)
        if status == 0:
            accepted += 1
            assert ref is not None, 'the model accepts what libzstd refuses: ' + label
            assert got == ref, 'the model differs from libzstd: ' + label
        elif ref is not None:
            stricter.append((label, status))
    print('%d mutants: %d accepted by both, %d refused by the model alone (%.1f %%)'
          % (len(mutants), accepted, len(stricter), 100.0 * len(stricter) / len(mutants)))
    for label, status in stricter:
        print('  model alone refuses', label, status)
    # what the model alone refuses is by design (dbh_zstd_core.h): bytes or frames behind the
    # frame, the checksum flag, reserved bits, a bitstream read beyond its first bit
    assert len(stricter) <= len(mutants) // 10


# ---- the loader: VBZ chunks handed on with their zstd stage (F5_RAW_FLAG_VBZ_ZSTD_GPU) ----------
def vbz_copies(tmp_path):
    """VBZ copies of the golden fast5 files, every variant of vbz_fixtures in turn -> [(path,
    reads, variant)]"""
    out = []
    for k, path in enumerate(vbz_fixtures.golden_fast5()):
        reads = vbz_fixtures.read_all(path)
        variant = vbz_fixtures.VARIANTS[k % len(vbz_fixtures.VARIANTS)]
        copy = vbz_fixtures.write_vbz_copy(reads, str(tmp_path / ('%02d_' % k + os.path.basename(path))), variant)
        out.append((copy, reads, variant))
    return out


def decode_records(comp, records, offsets, n_reads):
    """the reads of a raw batch, every mode-3 record through libzstd + fast5_native.vbz_decode,
    mode-2 records through vbz_decode alone, stored ones as they are"""
    import numpy as np
    from deepbinner_amd import fast5_native
    samples = np.zeros(int(offsets[-1]), dtype=np.int16)
    for r in records:
        data = bytes(comp[r['comp_offset']:r['comp_offset'] + r['comp_bytes']])
        n = int(r['out_bytes']) // 2
        if r['mode'] == fast5_native.RAW_VBZ_ZSTD:
            content, _ = zc.zstd_decompress(data[4:], 1 << 22)      # (a last chunk holds more than is wanted)
            assert content is not None
            got = fast5_native.vbz_decode(data[:4] + content, (0, 2, 1, 0), 1 << 24)
        elif r['mode'] == fast5_native.RAW_VBZ:
            got = fast5_native.vbz_decode(data, (0, 2, 1, 0), 1 << 24)
        else:
            assert r['mode'] == fast5_native.RAW_STORED
            got = np.frombuffer(data, dtype=np.int16)
        assert got is not None
        at = r['out_offset'] // 2
        m = min(n, len(got))
        samples[at:at + m] = got[:m]
    return samples


def test_loader_hands_vbz_chunks_on_as_stored_under_the_flag(tmp_path):
    import numpy as np
    from deepbinner_amd import fast5_native
    copies = vbz_copies(tmp_path)
    singles = [(p, reads, v) for p, reads, v in copies if len(reads) == 1]
    paths = [p for p, _, _ in singles]
    ids, offsets, status, comp, records = fast5_native.load_batch_raw(paths, 2, vbz_zstd='gpu')
    assert list(status) == [0] * len(paths)
    samples = decode_records(comp, records, offsets, len(paths))
    for i, (_, reads, variant) in enumerate(singles):
        assert ids[i] == reads[0][0]
        assert np.array_equal(samples[offsets[i]:offsets[i + 1]], reads[0][1])
        modes = set(records['mode'][records['read'] == i].tolist())
        if variant.get('cd', (0, 2, 1, 1))[3] == 0:
            assert modes <= {fast5_native.RAW_VBZ}                 # no zstd stage: mode 2 under the flag
        elif len(reads[0][1]):
            assert fast5_native.RAW_VBZ_ZSTD in modes and fast5_native.RAW_VBZ not in modes
            if variant.get('raw_chunks') and len(reads[0][1]) > variant['chunk']:
                assert fast5_native.RAW_STORED in modes            # a chunk with a filter mask stays
    assert (records['mode'] == fast5_native.RAW_VBZ_ZSTD).any() and (records['mode'] == fast5_native.RAW_VBZ).any()
    # containers, streamed
    multis = [(p, reads) for p, reads, v in copies if len(reads) > 1 and v.get('cd', (0, 2, 1, 1))[3]]
    assert multis
    seen = 0
    for index, m_ids, m_offsets, m_status, m_comp, m_records in fast5_native.stream_raw(
            [p for p, _ in multis], threads=2, vbz_zstd='gpu'):
        reads = multis[index][1]
        assert list(m_status) == [0] * len(reads)
        assert (m_records['mode'] == fast5_native.RAW_VBZ_ZSTD).any()
        assert not (m_records['mode'] == fast5_native.RAW_VBZ).any()
        got = decode_records(m_comp, m_records, m_offsets, len(reads))
        by_id = dict(reads)
        for i, rid in enumerate(m_ids):
            assert np.array_equal(got[m_offsets[i]:m_offsets[i + 1]], by_id[rid])
        seen += 1
    assert seen == len(multis)


def test_loader_without_the_flag_is_the_old_entry_point_byte_for_byte(tmp_path):
    import ctypes
    import numpy as np
    from deepbinner_amd import fast5_native
    copies = vbz_copies(tmp_path)
    paths = [p for p, reads, _ in copies if len(reads) == 1]
    new = fast5_native.load_batch_raw(paths, 2)                     # (flags 0 through the _ex call)
    lib = fast5_native.load_library()
    c_paths = (ctypes.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    handle = ctypes.c_void_p()
    assert lib.f5_load_batch_raw(c_paths, len(paths), 2, 0, ctypes.byref(handle)) == 0
    old = fast5_native._unpack_raw_batch(lib, handle)
    assert list(new[0]) == list(old[0])
    for a, b in zip(new[1:], old[1:]):
        assert np.array_equal(a, b)
    assert not (new[4]['mode'] == fast5_native.RAW_VBZ_ZSTD).any() and (new[4]['mode'] == fast5_native.RAW_VBZ).any()
    with pytest.raises(ValueError):
        fast5_native.load_batch_raw(paths, 2, vbz_zstd='both')


def test_the_route_switch_reads_the_environment(monkeypatch):
    from deepbinner_amd import fast5_native
    monkeypatch.delenv('DEEPBINNER_VBZ_ZSTD', raising=False)
    assert fast5_native.vbz_zstd_route() == 'host'
    monkeypatch.setenv('DEEPBINNER_VBZ_ZSTD', 'gpu')
    assert fast5_native.vbz_zstd_route() == 'gpu'
    monkeypatch.setenv('DEEPBINNER_VBZ_ZSTD', 'host')
    assert fast5_native.vbz_zstd_route() == 'host'
    monkeypatch.setenv('DEEPBINNER_VBZ_ZSTD', 'sometimes')
    with pytest.raises(ValueError):
        fast5_native.vbz_zstd_route()
