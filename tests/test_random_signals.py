"""The random-signal generator's CPU model (dbh_random_signals_host, csrc/dbh_random_core.h; DESIGN.md
section 23) against the NumPy restatement of its contract (tests/random_signal_reference.py), its
law, and the argument errors of the three entries - none of which needs a device."""
import numpy as np
import pytest

import random_signal_reference as rr
from deepbinner_amd import hip_backend

# (seed, first signal, signals, signal size)
CASES = [(3, 0, 64, 1024), (1, 0, 64, 96), (5, 2 ** 32 - 64, 64, 102), (7, 0, 12, 16384), (2, 0, 1, 1)]


@pytest.mark.parametrize('seed,first,n,size', CASES)
def test_host_model_equals_the_restatement(seed, first, n, size):
    want, kinds, nearest = rr.signals(seed, first, n, size)
    # log and cos of two libraries may differ in their last place; that can move a truncated value
    # only where the value before truncation lies on an integer, and these cases stay clear of it
    assert nearest > rr.GUARD
    if n >= 12:
        assert set(kinds.tolist()) == {rr.FLAT, rr.GAUSSIAN, rr.MULTI_GAUSSIAN, rr.PERLIN}
    got = hip_backend.random_signals(seed, first, n, size, host=True)
    assert got.dtype == np.int16 and got.shape == (n, size)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('size', rr.LONG_SIZES)
def test_host_model_equals_the_restatement_past_one_chunk_of_segments(size):
    """8 signals of more than 256 * 500 values: the kernel draws a multi_gaussian's segments 256 at
    a time, and the device is held to this model at these sizes (tests/test_gpu_random_signals.py)"""
    seed = 3 + size
    want, kinds, nearest = rr.long_case(size)
    assert nearest > rr.GUARD
    assert set(kinds.tolist()) == {rr.FLAT, rr.GAUSSIAN, rr.MULTI_GAUSSIAN, rr.PERLIN}
    for s in np.flatnonzero(kinds == rr.MULTI_GAUSSIAN):
        assert rr.segments(seed, int(s), size)[2] > 256
    got = hip_backend.random_signals(seed, 0, rr.LONG_SIGNALS, size, host=True)
    assert got.dtype == np.int16 and np.array_equal(got, want)


def test_the_guard_of_many_short_signals():
    """tests/test_gpu_random_signals.py guards 65,600 signals of 102 values with this"""
    for seed, first, n, size in [(5, 0, 40, 102), (5, 2 ** 32 - 64, 64, 300), (9, 7, 30, 96), (4, 5, 50, 1)]:
        assert rr.nearest_of_many(seed, first, n, size) == rr.signals(seed, first, n, size)[2]
    seed, n, size = rr.MANY_SEED, rr.MANY_SIGNALS, rr.MANY_SIZE
    assert rr.many_case_nearest() > rr.GUARD
    # the model on both ends of the range; the device is held to the model on all of it
    for first, count in ((0, 300), (n - 64, 64)):
        want = rr.signals(seed, first, count, size)[0]
        assert np.array_equal(hip_backend.random_signals(seed, first, count, size, host=True), want)


def test_the_guard_of_many_one_value_signals():
    """tests/test_gpu_random_signals.py guards 70,000 signals of one value with this"""
    assert rr.nearest_at_size_one(4, 5, 300) == rr.signals(4, 5, 300, 1)[2]
    assert rr.nearest_at_size_one(8, 0, 70000) > rr.GUARD


def test_a_range_may_be_cut_anywhere_and_replayed():
    whole = hip_backend.random_signals(9, 100, 64, 300, host=True)
    parts = [hip_backend.random_signals(9, 100, 10, 300, host=True),
             hip_backend.random_signals(9, 110, 54, 300, host=True)]
    assert np.array_equal(whole, np.concatenate(parts))
    assert np.array_equal(whole, hip_backend.random_signals(9, 100, 64, 300, host=True))
    assert not np.array_equal(whole, hip_backend.random_signals(10, 100, 64, 300, host=True))


def test_multi_gaussian_segments_lie_end_to_end():
    seed, size = 7, 16384
    s = next(s for s in range(64) if rr.parameters(seed, s)['kind'] == rr.MULTI_GAUSSIAN)
    _, _, count = rr.segments(seed, s, size)
    assert size / 500 <= count <= size // 100 + 1 <= 164
    one = next(s for s in range(64) if rr.parameters(1, s)['kind'] == rr.MULTI_GAUSSIAN)
    assert rr.segments(1, one, 96)[2] == 1                # 96 values: one segment


def test_the_law():
    """4,096 signals of 256 values: each kind a quarter of them within 5 standard deviations, and
    a gaussian signal's sample mean and deviation within 5 standard errors of its drawn parameters
    (stdev / sqrt(L) and stdev / sqrt(2 L)), truncation toward zero included."""
    n, size, seed = 4096, 256, 11
    values = hip_backend.random_signals(seed, 0, n, size, host=True).astype(np.float64)
    parameters = [rr.parameters(seed, s) for s in range(n)]
    kinds = np.array([p['kind'] for p in parameters])
    sigma = np.sqrt(n * 0.25 * 0.75)
    for kind in range(4):
        assert abs((kinds == kind).sum() - n / 4) < 5 * sigma
    checked = 0
    for s in np.flatnonzero(kinds == rr.GAUSSIAN):
        mean, stdev = parameters[s]['mean'], parameters[s]['stdev']
        assert 300 <= mean <= 600 and 10 <= stdev <= 500
        assert abs(values[s].mean() - mean) < 5 * stdev / np.sqrt(size)
        assert abs(values[s].std() - stdev) < 5 * stdev / np.sqrt(2 * size)
        checked += 1
    assert checked > 900
    for s in np.flatnonzero(kinds == rr.FLAT):
        assert values[s].min() == values[s].max() == parameters[s]['level'] <= 1000
    for s in np.flatnonzero(kinds == rr.PERLIN):
        p = parameters[s]
        assert np.abs(values[s] - p['mean']).max() <= 2 * p['factor'] + 1    # |noise| <= 2 by construction
    assert values.min() > -32768 / 4 and values.max() < 32767 / 4


@pytest.mark.parametrize('entry', ['dbh_random_signals', 'dbh_random_signals_dev',
                                   'dbh_random_signals_host'])
def test_argument_errors_come_before_any_device_work(entry):
    lib = hip_backend.load_library()
    out = np.zeros(16, dtype=np.int16)
    tail = (None,) if entry.endswith('_dev') else ()

    def call(first, n, size, pointer=out.ctypes.data):
        return getattr(lib, entry)(0, first, n, size, pointer, *tail)

    invalid, unsupported = 1, 5
    assert call(0, 1, 16, None) == invalid
    assert call(0, 0, 16) == invalid and call(0, 1, 0) == invalid and call(-1, 1, 16) == invalid
    assert call(2 ** 32 - 1, 2, 16) == invalid and call(2 ** 32, 1, 16) == invalid
    assert call(0, 1, 2 ** 20 + 1) == unsupported
    assert call(0, 2 ** 20 + 1, 1024) == unsupported and call(0, 2 ** 30 + 1, 1) == unsupported
