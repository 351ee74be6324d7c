"""The frames of tests/zstd_written.py - written bit by bit, what libzstd's encoder never writes -
through the zstd stage on the GPU, as mode-3 streams of dbh_inflate_dev.  What is expected comes
from no decoder: the bytes are the writer's replay, the statuses of refused frames are the cases'
own (the CPU model agrees with both: tests/test_zstd_written.py, where libzstd is the judge).

Every valid frame goes twice: once with out_bytes = 2 * ceil(content / 8), a region at most 7 bytes
larger than the content and exactly its size for the exact-fit frames, whose parked Huffman literals
lie where the output lands (WaveExec::copy with its destination a few bytes below its source); and
once with room to spare.  The output buffer and the workspace are filled with a sentinel first, and
every byte outside the streams' own regions and slots must still hold it (zstd_gpu.run: in a call
of mode-3 streams alone no stage writes the workspace outside a stream's slots, so all of it
outside them is checked, not only the gaps)."""

import os
import struct

import numpy as np
import pytest

import zstd_cases as zc
import zstd_written as zw
from zstd_gpu import VBZ_ZSTD, run, samples_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, '..', 'deepbinner_amd', 'libdeepbinner_hip.so')


def tight(content):
    return 2 * ((len(content) + 7) // 8)


@pytest.fixture(scope='module')
def sent(hip):
    """Two calls: every valid frame in its tight region; every valid frame with room to spare and
    every refused frame.  -> {(name, 'tight' | 'roomy' | 'refused'): (out_bytes, output, status, slots)}"""
    valid = [c for c in zw.all_cases() if c[2] is not None]
    refused = [c for c in zw.all_cases() if c[2] is None]
    calls = [[(name, 'tight', frame, tight(content)) for name, frame, content, _ in valid],
             [(name, 'roomy', frame, tight(content) + 2 * (17 + 101 * (k % 7)))
              for k, (name, frame, content, _) in enumerate(valid)] +
             [(name, 'refused', frame, 2 * ((zw.ROOM[name] + 7) // 8)) for name, frame, _, _ in refused]]
    got = {}
    for call in calls:
        outs, status, slots = run(hip, [(struct.pack('<I', out_bytes) + frame, out_bytes, VBZ_ZSTD)
                                        for _, _, frame, out_bytes in call])
        for i, (name, kind, _, out_bytes) in enumerate(call):
            got[name, kind] = (out_bytes, outs[i], int(status[i]), slots[i])
    return got


def test_exact_fit_frames_are_among_them():
    fit = [c for c in zw.all_cases() if c[0].startswith('d_fit_')]
    assert len(fit) >= 7
    for name, frame, content, _ in fit:
        info = zw.walk(frame)
        assert 4 * tight(content) == len(content) and len(content) % 8 == 0, name
        assert any(t == 'huffman' for t, _ in info['literals']), name
        assert info['counts'], name


@pytest.mark.parametrize('kind', ['tight', 'roomy'])
def test_every_valid_frame_gives_the_replay_s_bytes(sent, kind):
    wrong = []
    for name, frame, content, _ in zw.all_cases():
        if content is None:
            continue
        out_bytes, out, status, slots = sent[name, kind]
        if status not in (0, 1):
            wrong.append((name, 'status', status))
        elif bytes(slots[:len(content)]) != content:
            got = np.frombuffer(bytes(slots[:len(content)]), dtype=np.uint8)
            first = int(np.flatnonzero(got != np.frombuffer(content, dtype=np.uint8))[0])
            wrong.append((name, 'bytes', first, len(content)))
    assert not wrong, wrong[:20]


@pytest.mark.parametrize('kind', ['tight', 'roomy'])
def test_the_streamvbyte_stage_behind_it_says_what_the_host_s_says(sent, kind):
    """Nearly no content here is the streamvbyte bytes of that many samples: refused with that
    stage's status 1 and zeros, never with a status of the zstd stage."""
    for name, frame, content, _ in zw.all_cases():
        if content is None:
            continue
        out_bytes, out, status, slots = sent[name, kind]
        host = samples_of(content, out_bytes // 2)
        if host is None:
            assert status == 1 and not out.any(), (name, status)
        else:
            assert status == 0, (name, status)
            want = np.zeros(out_bytes // 2, dtype=np.int16)
            want[:len(host)] = host
            assert np.array_equal(out.view(np.int16), want), name


def test_refused_frames_have_the_status_of_their_case_and_zeros(sent):
    model = zc.model_lib(LIB)
    wrong = []
    for name, frame, content, want in zw.all_cases():
        if content is not None:
            continue
        out_bytes, out, status, slots = sent[name, 'refused']
        assert zc.model_decode(model, frame, 4 * out_bytes)[0] == want, name
        if status != want or out.any():
            wrong.append((name, status, want, bool(out.any())))
    assert not wrong, wrong
