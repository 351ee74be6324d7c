"""The reference the GPU streamvbyte decoder is tested against (tests/vbz_reference.py) held to both
host decoders on every case of every family, and the conditions on those cases that keep the GPU
tests (tests/test_gpu_vbz_codes.py) from being hollow.  Host only."""

import struct

import numpy as np
import pytest

import vbz_reference as ref
from deepbinner_amd import hdf5_lite

CD = (0, 2, 1, 0)             # streamvbyte bytes as they are behind the size: no zstd stage


@pytest.fixture(scope='module')
def cases():
    return ref.all_cases()


@pytest.fixture(scope='module')
def counted(cases):
    c = ref.census(cases)
    print(ref.census_text(c))
    return c


def room(payload):
    """max_samples for a host decoder: above it the host's chunk-size rule (original_size <= the
    chunk's bytes) refuses a stream, a rule the device does not have - it is handed out_bytes, not
    a chunk size.  Every case is decoded with room for its own original_size, so none falls under
    that rule and all of them are compared."""
    size = struct.unpack_from('<I', payload)[0] if len(payload) >= 4 else 0
    return max(16, (size + 1) // 2)


def test_the_vectorised_reference_is_the_plain_one(cases):
    for c in cases:
        fast, plain = ref.decode(c.payload), ref.decode_plain(c.payload)
        assert (fast is None) == (plain is None), c.name
        assert fast is None or np.array_equal(fast, plain), c.name


def test_the_reference_is_the_python_decoder(cases):
    for c in cases:
        want = ref.decode(c.payload)
        assert struct.unpack_from('<I', c.payload + b'\0\0\0\0')[0] <= 2 * room(c.payload)
        try:
            got = np.frombuffer(hdf5_lite.vbz_decode(c.payload, CD, 2 * room(c.payload)), np.int16)
        except hdf5_lite.Hdf5FormatError:
            got = None
        assert (got is None) == (want is None), c.name
        assert want is None or np.array_equal(got, want), c.name
        if want is not None:
            n = len(want)
            assert np.array_equal(hdf5_lite.vbz_unpack(c.payload[4:], n), want), c.name


def test_the_reference_is_the_native_decoder(cases):
    from deepbinner_amd import fast5_native
    try:
        fast5_native.load_library()
    except (OSError, fast5_native.Fast5NativeError) as e:
        pytest.skip('native loader not built: %s' % e)
    for c in cases:
        want = ref.decode(c.payload)
        got = fast5_native.vbz_decode(c.payload, CD, room(c.payload))
        assert (got is None) == (want is None), c.name
        assert want is None or np.array_equal(got, want), c.name


def test_expected_cuts_extends_and_zeroes():
    good = ref.stream_of(np.array([2, 4, 1, 600, 70000, 1 << 31], dtype=np.uint32))
    samples = ref.decode(good)
    assert samples.tolist() == [1, 3, 2, 302, -30234, -30234]
    for out_bytes, want in ((0, []), (2, [1]), (12, samples.tolist()), (16, samples.tolist() + [0, 0])):
        ok, got = ref.expected(good, out_bytes)
        assert ok and got.dtype == np.int16 and got.tolist() == want
    for bad in (good[:-1], good + b'\0', struct.pack('<I', 11) + good[4:], good[:3], b''):
        ok, got = ref.expected(bad, 12)
        assert not ok and got.tolist() == [0] * 6


def test_both_encodings_of_a_signal_decode_to_it(cases):
    seen = 0
    for c in cases:
        if c.family == 'unwrapped':
            assert np.array_equal(ref.decode(c.payload), c.samples), c.name
            assert np.array_equal(ref.decode(c.twin), c.samples), c.name
            if c.unwrapped and len(c.samples) > 100:
                assert c.payload != c.twin and (ref.code_lengths(c.payload) == 3).any()
                assert ref.code_lengths(c.twin).max() == 2
            seen += 1
    assert seen >= 10


def test_padding_bits_change_nothing(cases):
    seen = 0
    for c in cases:
        if c.family == 'padding':
            assert c.payload != c.twin and len(c.payload) == len(c.twin)
            assert np.array_equal(ref.decode(c.payload), ref.decode(c.twin)), c.name
            seen += 1
    assert seen >= 900


def test_every_code_in_every_place(counted):
    every = {(code, position) for code in (1, 2, 3, 4) for position in range(16)}
    assert counted.full_lane == every
    # a partial lane holds at most 15 values: its positions are 0..14
    assert counted.partial_lane == {(c, p) for c, p in every if p < 15}
    # the 4-byte load behind a stream's last value is what reads up to 3 bytes beyond the stream
    assert counted.last_code == {1, 2, 3, 4}


def test_the_widest_lanes_and_steps_and_a_wrapping_sum(counted):
    assert counted.lane_bytes[64] >= 1 and counted.lane_bytes[16] >= 1
    assert counted.max_step_bytes == 4096
    assert counted.wrapping_streams >= 1 and counted.bit31 >= 1000


def test_long_codes_in_numbers(counted):
    assert counted.codes[2] >= 1000 and counted.codes[3] >= 1000
    assert counted.unwrapped_three_byte >= 100


def test_the_mutants_are_of_every_kind(cases, counted):
    assert counted.mutants_refused >= 300
    assert counted.mutants_accepted_other_samples >= 100
    assert counted.refused_behind_whole_steps >= 20
    mutants = [c for c in cases if c.family == 'mutants']
    assert len(mutants) >= 1000 and all(ref.decode(c.origin) is not None for c in mutants)
    assert counted.mutants_refused + counted.mutants_accepted == len(mutants)
    kinds = {c.name.split('_')[2].rstrip('0123456789+-') for c in mutants}
    assert kinds == {'cut', 'long', 'size', 'code', 'codes', 'bit'}
    # two codes changed so that the byte count holds: never refused, always other samples
    for c in mutants:
        if c.name.split('_')[2].startswith('codes'):
            assert len(c.payload) == len(c.origin)
            assert int(ref.code_lengths(c.payload).sum()) == int(ref.code_lengths(c.origin).sum())
            assert ref.decode(c.payload) is not None, c.name


def test_the_families_hold_what_the_gpu_tests_lay_out(cases):
    by = {}
    for c in cases:
        by.setdefault(c.family, []).append(c)
    assert set(by) == {'codes', 'unwrapped', 'padding', 'shapes', 'mutants'}
    counts = {len(ref.decode(c.payload)) for c in by['codes']}
    assert counts >= set(ref.CODE_COUNTS) | {ref.LONG_READ}
    shapes = by['shapes']
    assert {c.align for c in shapes} == set(range(0, 16, 2))
    for n in ref.SHAPE_COUNTS:
        assert n >= 3 * ref.STEP
        wanted = {c.out_bytes for c in shapes if ref.header(c.payload)[0] == n}
        assert wanted >= {0, 2, 30, 32, 34, 2 * n, 2 * n + 2, 2 * n + 4096, 2 * (n - 3)}
        assert wanted >= {2 * (k * ref.STEP + d) for k in (1, 2) for d in (-1, 0, 1)}
    # nothing is left out of a GPU launch: a case is a stream, an out_bytes and nothing else
    assert all(c.out_bytes % 2 == 0 and c.out_bytes >= 0 for c in cases)


def test_the_looping_launch_is_long_enough():
    cases = ref.loop_cases()
    assert len(cases) == 40000 > 8192 * 4
    refused = [k for k, c in enumerate(cases) if ref.decode(c.payload) is None]
    assert refused == list(range(99, 40000, 100))
    assert max(ref.header(c.payload)[0] for c in cases) == 64
    assert sum(len(c.payload) for c in cases) < 8 << 20
