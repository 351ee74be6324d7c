"""
The GPU's zstd decoder run on the host (dbh_zstd_decode_host, deepbinner_amd/csrc/dbh_zstd_core.h)
on the frames of tests/zstd_written.py - written bit by bit, what libzstd's encoder never writes -
with the system's libzstd as the judge: every valid frame decodes there to the replay's bytes, the
model gives the same bytes at every capacity from the content's size upwards, and every refused
frame is refused with the status its case names, by libzstd as well except for the frames named in
MODEL_ALONE.

DEEPBINNER_ZSTD_MODEL_LIB names another build of the entry point, as in tests/test_zstd_model.py.
"""

import ctypes
import os
import re

import pytest

import vbz_fixtures
import zstd_cases as zc
import zstd_written as zw

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.environ.get('DEEPBINNER_ZSTD_MODEL_LIB') or os.path.join(HERE, '..', 'deepbinner_amd',
                                                                   'libdeepbinner_hip.so')
CORE = os.path.join(HERE, '..', 'deepbinner_amd', 'csrc', 'dbh_zstd_core.h')

pytestmark = pytest.mark.skipif(vbz_fixtures.zstd_lib() is None, reason='no libzstd.so.1 on this machine')

# The frames the model refuses and libzstd takes, by name, each with the words of dbh_zstd_core.h's
# header that make it so by design.  The test below holds this dict to what is observed: a frame
# more or a frame fewer fails it.
MODEL_ALONE = {
    'a_checksum': 'the checksum flag',
    'a_dictionary_id_1_zero': 'a dictionary id field, also one that holds 0',
    'a_dictionary_id_2_zero': 'a dictionary id field, also one that holds 0',
    'a_dictionary_id_4_zero': 'a dictionary id field, also one that holds 0',
    'a_no_content_size': 'no content size',
    'a_skippable_in_front': 'a skippable frame in front of the frame',
    'a_second_frame_behind': 'a second frame behind it',
    'c_depth_12': 'codes longer than 11 bits (libzstd takes 12: the one place this decoder is narrower by design)',
    'd_reserved_mode_bits': "reserved bits set in the sequences' modes byte",
    'd_offset_beyond_window': 'an offset beyond the window but inside the output',
    'd_bits_left_over': 'sequence bits left over behind the last sequence',
    'd_byte_left_over': 'sequence bits left over behind the last sequence',
    'd_one_bit_short': "a last sequence whose fields reach beyond the stream's first bit",
}


@pytest.fixture(scope='module')
def model():
    return zc.model_lib(LIB)


@pytest.fixture(scope='module')
def cases():
    return zw.all_cases()


def valid(cases):
    return [c for c in cases if c[2] is not None]


def refused(cases):
    return [c for c in cases if c[2] is None]


def test_the_families_are_there(cases):
    fams = zw.families()
    assert set(fams) == {'A', 'B', 'C', 'D', 'R'}
    assert len(fams['R']) == 300 and all(c[2] is not None and len(c[2]) <= 65536 for c in fams['R'])
    assert len(valid(cases)) >= 500 and len(refused(cases)) >= 45
    assert all(c[3] is not None and c[0] in zw.ROOM for c in refused(cases))
    assert set(zw.VERSION_DEPENDENT) <= {c[0] for c in cases}


def test_libzstd_decodes_every_valid_frame_to_the_replay_s_bytes(cases):
    wrong = []
    for name, frame, content, _ in valid(cases):
        if name in zw.VERSION_DEPENDENT:
            continue
        ref, code = zc.zstd_decompress(frame, len(content))
        if ref != content:
            wrong.append((name, code, None if ref is None else len(ref), len(content)))
    assert not wrong, wrong


def test_the_model_gives_the_same_bytes_at_every_capacity(model, cases):
    wrong = []
    for name, frame, content, _ in valid(cases):
        n = len(content)
        for capacity in [n + k for k in range(8)] + [n + 12345]:
            status, got = zc.model_decode(model, frame, capacity)
            if status != 0 or got != content:
                wrong.append((name, capacity - n, status, len(got), n))
    assert not wrong, wrong[:20]


def test_the_model_needs_the_content_s_size_and_no_more(model, cases):
    for name, frame, content, _ in valid(cases)[::7]:
        if content:
            assert zc.model_decode(model, frame, len(content) - 1) == (zw.NO_SPACE, b''), name


def test_refused_frames_have_their_status_and_libzstd_refuses_them_too(model, cases):
    wrong, alone = [], set()
    for name, frame, _, want in refused(cases):
        status, got = zc.model_decode(model, frame, zw.ROOM[name])
        if status != want or got:
            wrong.append((name, status, want))
        if name in zw.VERSION_DEPENDENT:
            continue
        ref, _ = zc.zstd_decompress(frame, zw.ROOM[name])
        if ref is not None:
            alone.add(name)
    assert not wrong, wrong
    assert alone == set(MODEL_ALONE), (sorted(alone - set(MODEL_ALONE)), sorted(set(MODEL_ALONE) - alone))
    # the words quoted for each stand in the core's header
    with open(CORE) as f:
        header = f.read().split('#pragma once')[0]
    header = re.sub(r'\s+', ' ', header.replace('//', ' '))
    for name, words in MODEL_ALONE.items():
        assert words in header, (name, words)


def test_what_differs_between_libzstd_versions_is_judged_one_way(model, cases):
    """A compressed block of 2 bytes, a repeat offset of rep[0] - 1 = 0 and 4 streams of fewer than
    6 literals are taken by some versions of libzstd and refused by others: where the model accepts,
    libzstd must accept and the bytes must be equal."""
    z = zc.lib()
    z.ZSTD_versionString.restype = ctypes.c_char_p
    print('libzstd', z.ZSTD_versionString().decode())
    by_name = {c[0]: c for c in cases}
    for name in zw.VERSION_DEPENDENT:
        _, frame, content, want = by_name[name]
        room = len(content) if content is not None else zw.ROOM[name]
        status, got = zc.model_decode(model, frame, room)
        ref, _ = zc.zstd_decompress(frame, room)
        print('  %-28s model %2d, libzstd %s' % (name, status, 'refuses' if ref is None else 'accepts'))
        assert status == (0 if content is not None else want), name
        if status == 0:
            assert ref is not None, 'the model accepts what libzstd refuses: ' + name
            assert got == ref == content, name


def test_the_families_hold_what_they_are_written_for(cases):
    info = {}
    for name, frame, content, _ in valid(cases):
        zw.walk(frame, info)
    assert info['fcs'] == {1, 2, 4, 8} and info['windowed'] == {False, True}
    assert info['blocks'] == {'raw', 'rle', 'compressed'}
    # every size format of every literals type
    assert info['literals'] == {(t, sf) for t in ('raw', 'rle', 'huffman', 'treeless') for sf in range(4)}
    # every form of the count, at its edges
    assert {(1, 1), (2, 1), (2, 5), (1, 127), (2, 127), (2, 128), (2, 0x7EFF), (3, 0x7F00), (3, 0x7F07)} <= info['counts']
    # accuracy 5 and the largest of every table, and every combination of modes
    assert {('ll', 5), ('ll', 9), ('of', 5), ('of', 8), ('ml', 5), ('ml', 9)} <= info['accuracy']
    assert info['modes'] == {(a, b, c) for a in range(4) for b in range(4) for c in range(4)}
    # trees: both descriptions, depth 11, 1 to 128 direct weights; single streams ending at every bit
    assert info['trees'] == {'direct', 'fse'}
    assert 11 in info['depths'] and max(info['depths']) == 11
    assert {1, 2, 3, 127, 128} <= info['given']
    assert info['markers'] == set(range(8))
    assert {(1, 1), (1, 1023)} <= info['streams']
    assert {(4, n) for n in (3, 4, 6, 7, 8, 9, 64, 65)} <= info['streams']
    # the random frames alone reach every mode, every literals type and both stream counts
    info = {}
    for name, frame, content, _ in zw.families()['R']:
        zw.walk(frame, info)
    assert {t for t, _ in info['literals']} == {'raw', 'rle', 'huffman', 'treeless'}
    assert {m for combo in info['modes'] for m in combo} == {0, 1, 2, 3}
    assert {s for s, _ in info['streams']} == {1, 4} and info['trees'] == {'direct', 'fse'}


def test_the_dump_for_the_sanitizer_check(tmp_path, cases):
    path = str(tmp_path / 'frames.bin')
    zw.dump(path)
    with open(path, 'rb') as f:
        data = f.read()
    at = records = 0
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], 'little')
        at += 8 + n
        records += 1
    assert at == len(data) and records == 2 * len(valid(cases)) + len(refused(cases))
