"""POD5's 16-bit streamvbyte code on the host: ``pod5_lite.decode_svb16`` /
``encode_svb16`` (NumPy) and ``dbh_svb16_decode_host`` (the GPU's core with loops for lanes) against
a one-value-at-a-time decoder in plain Python (tests/svb16_cases.py), on the case families the GPU
test uses, with every stream's refused mutants.  No GPU.
"""
import ctypes
import os

import numpy as np
import pytest

import svb16_cases as sc
from conftest import REPO
from deepbinner_amd import hip_backend, pod5_lite

CSRC = os.path.join(REPO, 'deepbinner_amd', 'csrc')


def host_decode(stream, n):
    """dbh_svb16_decode_host -> (status, samples)"""
    lib = hip_backend.load_library()
    raw = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    out = np.full(n, 0x5A5A, dtype=np.int16)
    status = ctypes.c_int32(-1)
    assert lib.dbh_svb16_decode_host(raw.ctypes.data if len(raw) else None, len(raw), n,
                                     out.ctypes.data if n else None, ctypes.byref(status)) == 0
    return status.value, out


@pytest.fixture(scope='module')
def cases():
    """[(name, samples, stream, plain decode)]: the reference once, for every test here"""
    out = []
    for name, samples in sc.families():
        stream = sc.plain_encode(samples)
        out.append((name, samples, stream, sc.plain_decode(stream, len(samples))))
    return out


def test_the_plain_decoder_gives_the_samples_back(cases):
    assert len(cases) == 13 * 6
    for name, samples, stream, plain in cases:
        assert plain is not None and np.array_equal(plain, samples), name
    # the key bits are what the family says: one byte each, two bytes each
    by_name = {name: stream for name, _, stream, _ in cases}
    assert len(by_name['n1024_all0']) == 128 + 1024 and len(by_name['n1024_all1']) == 128 + 2048
    assert by_name['n16_lane_edges'][:2] == bytes([0x01, 0x80])


def test_numpy_encoder_and_decoder(cases):
    for name, samples, stream, plain in cases:
        assert pod5_lite.encode_svb16(samples) == stream, name
        got = pod5_lite.decode_svb16(stream, len(samples))
        assert got is not None and got.dtype == np.int16 and np.array_equal(got, plain), name


def test_host_entry_of_the_gpu_core(cases):
    for name, samples, stream, plain in cases:
        status, got = host_decode(stream, len(samples))
        assert status == 0 and np.array_equal(got, plain), name


def test_mutants_are_refused_by_all_three(cases):
    refused = 0
    for name, samples, stream, _ in cases:
        n = len(samples)
        if n > 2049:
            continue
        for payload in ([stream[:-1]] if stream else []) + [stream + b'\x00', stream + b'\xff']:
            assert sc.plain_decode(payload, n) is None, name
            assert pod5_lite.decode_svb16(payload, n) is None, name
            status, got = host_decode(payload, n)
            assert status == 1 and not got.any(), name
            refused += 1
    assert refused > 200


def test_unused_bits_of_the_last_key_byte_are_not_looked_at():
    samples = np.array([1, -300, 7], dtype=np.int16)
    stream = bytearray(sc.plain_encode(samples))
    stream[0] |= 0xF8
    assert np.array_equal(sc.plain_decode(stream, 3), samples)
    assert np.array_equal(pod5_lite.decode_svb16(bytes(stream), 3), samples)
    status, got = host_decode(stream, 3)
    assert status == 0 and np.array_equal(got, samples)


def test_host_entry_refuses_bad_arguments():
    lib = hip_backend.load_library()
    status = ctypes.c_int32(0)
    out = np.zeros(4, dtype=np.int16)
    raw = np.zeros(8, dtype=np.uint8)
    assert lib.dbh_svb16_decode_host(raw.ctypes.data, 8, -1, out.ctypes.data, ctypes.byref(status)) == 1
    assert lib.dbh_svb16_decode_host(None, 8, 4, out.ctypes.data, ctypes.byref(status)) == 1
    assert lib.dbh_svb16_decode_host(raw.ctypes.data, 8, 4, None, ctypes.byref(status)) == 1
    assert lib.dbh_svb16_decode_host(raw.ctypes.data, 8, 4, out.ctypes.data, None) == 1


def test_the_modes_and_the_workspace_of_the_old_ones():
    """the two modes take the next free numbers; the workspace is what it was: four bytes per byte
    of output, 512, and a record of 24 bytes per stream"""
    assert (hip_backend.INFLATE_SVB16, hip_backend.INFLATE_SVB16_ZSTD) == (6, 7)
    assert (pod5_lite.RAW_SVB16, pod5_lite.RAW_SVB16_ZSTD, pod5_lite.RAW_STORED) == (6, 7, 1)
    header = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    assert '#define DBH_INFLATE_SVB16 6' in header and '#define DBH_INFLATE_SVB16_ZSTD 7' in header
    lib = hip_backend.load_library()
    size = ctypes.c_size_t(0)
    for total, n in ((0, 0), (1000, 3), (1 << 20, 4000)):
        assert lib.dbh_inflate_workspace_bytes(total, n, ctypes.byref(size)) == 0
        assert size.value == 4 * total + 512 + 24 * n
    from deepbinner_amd import realtime
    for modes in ([0, 0, 4], [2, 3], [1, 5]):
        sizes = [70000] * len(modes)
        assert realtime.inflate_cus_for(sizes + [10, 10], modes + [6, 7]) == \
            realtime.inflate_cus_for(sizes, modes)


def test_the_model_check_program_is_there():
    text = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'svb16_asan:' in text and 'svb16_model_check.cpp' in text
    assert '-fsanitize=address,undefined' in text[text.index('svb16_asan:'):]
    source = open(os.path.join(CSRC, 'svb16_model_check.cpp')).read()
    assert 'int main()' in source and 'dbh_svb16_core.h' in source
    kernels = open(os.path.join(CSRC, 'dbh_vbz.hip')).read()
    assert 'dbh_svb16_core.h' in kernels and 'svb16_stream' in kernels
    for rule in ('lane_span', 'lane_keys', 'group_start', 'lane_decode', 'shape', 'prefix_ok'):
        assert 'sv::' + rule in kernels, rule
