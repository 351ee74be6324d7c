"""Random signals made on the GPU (dbh_random_signals, csrc/dbh_random.hip)
against the CPU model (dbh_random_signals_host), bit for bit.  The model itself is held to the
NumPy restatement without a device (tests/test_random_signals.py).  log and cos are the device's
own here, so every case first shows, on the restatement, that no value before truncation lies
within 2^-30 of an integer - the only place where a last-place difference could move a value."""
import numpy as np
import pytest

import random_signal_reference as rr

pytestmark = pytest.mark.gpu

SIZES = [96, 102, 1024, 16384]        # 96: one multi_gaussian segment; 102: two at least
FIRSTS = [0, 2 ** 32 - 64]
_guarded = {}


def guarded_model(hip, seed, first, n, size):
    """the CPU model's signals, once per case, after the guard"""
    key = (seed, first, n, size)
    if key not in _guarded:
        want, kinds, nearest = rr.signals(seed, first, n, size)
        assert nearest > rr.GUARD
        model = hip.random_signals(seed, first, n, size, host=True)
        assert np.array_equal(model, want)
        model.setflags(write=False)
        _guarded[key] = (model, kinds)
    return _guarded[key]


@pytest.mark.parametrize('first', FIRSTS)
@pytest.mark.parametrize('n', [1, 64])
@pytest.mark.parametrize('size', SIZES)
def test_device_equals_the_model(hip, size, n, first):
    seed = 3 + size
    model, kinds = guarded_model(hip, seed, first, n, size)
    if n == 64:
        assert set(kinds.tolist()) == {rr.FLAT, rr.GAUSSIAN, rr.MULTI_GAUSSIAN, rr.PERLIN}
    got = hip.random_signals(seed, first, n, size)
    assert got.dtype == np.int16 and np.array_equal(got, model)


@pytest.mark.parametrize('size', SIZES)
def test_one_signal_of_every_kind(hip, size):
    """n = 1 for each kind, so that a lone workgroup runs each path"""
    seed = 3 + size
    _, kinds = guarded_model(hip, seed, 0, 64, size)
    for kind in range(4):
        s = int(np.flatnonzero(kinds == kind)[0])
        model = guarded_model(hip, seed, 0, 64, size)[0][s:s + 1]
        assert np.array_equal(hip.random_signals(seed, s, 1, size), model)


def long_model(hip, size):
    """the CPU model's 8 signals of a long row, once per size, after the guard; with their kinds"""
    key = (3 + size, 0, rr.LONG_SIGNALS, size)
    if key not in _guarded:
        want, kinds, nearest = rr.long_case(size)
        assert nearest > rr.GUARD
        assert set(kinds.tolist()) == {rr.FLAT, rr.GAUSSIAN, rr.MULTI_GAUSSIAN, rr.PERLIN}
        for s in np.flatnonzero(kinds == rr.MULTI_GAUSSIAN):
            assert rr.segments(3 + size, int(s), size)[2] > 256      # a second chunk of segments
        model = hip.random_signals(3 + size, 0, rr.LONG_SIGNALS, size, host=True)
        assert np.array_equal(model, want)
        model.setflags(write=False)
        _guarded[key] = (model, kinds)
    return _guarded[key]


def first_difference(got, model, size):
    """where a row of the device first leaves the model: signal, value, and the chunk of 256
    segments in which a multi_gaussian value there lies at the earliest (a segment holds 500 at most)"""
    differ = np.flatnonzero(np.ravel(got) != np.ravel(model))
    if not differ.size:
        return None
    s, i = divmod(int(differ[0]), size)
    return 'signal {} value {} (chunk {} or later): {} against {}; {} values differ'.format(
        s, i, i // (256 * 500), np.ravel(got)[differ[0]], np.ravel(model)[differ[0]], differ.size)


@pytest.mark.parametrize('size', rr.LONG_SIZES)
def test_rows_past_one_chunk_of_segments(hip, size):
    """131,072 values: above 256 * 500, so every multi_gaussian signal takes a second chunk of 256
    segments - the start carried over, the tables in LDS written again, the bisection in a chunk
    that does not begin at 0; 2^20, the longest row: 14 chunks or so"""
    model, _ = long_model(hip, size)
    got = hip.random_signals(3 + size, 0, rr.LONG_SIGNALS, size)
    assert got.dtype == np.int16 and first_difference(got, model, size) is None


def test_one_long_signal_of_every_kind(hip):
    size = rr.LONG_SIZES[0]
    model, kinds = long_model(hip, size)
    for kind in range(4):
        s = int(np.flatnonzero(kinds == kind)[0])
        got = hip.random_signals(3 + size, s, 1, size)
        assert first_difference(got, model[s:s + 1], size) is None, kind


def test_a_range_may_be_cut_anywhere_and_replayed(hip):
    model, _ = guarded_model(hip, 3 + 1024, 0, 64, 1024)
    parts = [hip.random_signals(3 + 1024, 0, 10, 1024), hip.random_signals(3 + 1024, 10, 54, 1024)]
    assert np.array_equal(np.concatenate(parts), model)
    assert np.array_equal(hip.random_signals(3 + 1024, 0, 64, 1024), model)
    assert np.array_equal(hip.random_signals(3 + 1024, 0, 64, 1024), model)


def test_signals_stay_on_the_device(hip):
    model, _ = guarded_model(hip, 3 + 1024, 0, 64, 1024)
    with hip.ResidentText(64, 1024) as resident:
        assert np.array_equal(resident.random_signals(3 + 1024, 0, 64).download(), model)
        few = resident.random_signals(3 + 1024, 10, 54)          # the buffers are kept: a second chunk
        assert np.array_equal(few.download(), model[10:])
        text = resident.format_training_text(np.zeros(54, dtype=np.int32), few)
        assert bytes(text) == hip.format_training_text(np.zeros(54, dtype=np.int32), model[10:], host=True)
        del text
        with pytest.raises(ValueError):
            resident.random_signals(0, 0, 65)


def test_more_signals_than_the_grid_has_workgroups(hip):
    """70,000 signals of one value: a workgroup takes more than one signal"""
    assert rr.nearest_at_size_one(8, 0, 70000) > rr.GUARD
    model = hip.random_signals(8, 0, 70000, 1, host=True)
    assert np.array_equal(model[:300], rr.signals(8, 0, 300, 1)[0])
    assert np.array_equal(hip.random_signals(8, 0, 70000, 1), model)


def test_a_workgroups_second_signal_has_rows_of_its_own(hip):
    """65,536 + 64 signals of 102 values: the last 64 are their workgroups' second signals, of
    every kind, the multi_gaussian ones with two segments - behind a first signal of any kind"""
    seed, n, size = rr.MANY_SEED, rr.MANY_SIGNALS, rr.MANY_SIZE
    assert rr.many_case_nearest() > rr.GUARD                  # over all 6.7 million values
    model = hip.random_signals(seed, 0, n, size, host=True)
    for first, count in ((0, 300), (n - 64, 64)):
        want, kinds, _ = rr.signals(seed, first, count, size)
        assert np.array_equal(model[first:first + count], want)
        assert set(kinds.tolist()) == {rr.FLAT, rr.GAUSSIAN, rr.MULTI_GAUSSIAN, rr.PERLIN}
    got = hip.random_signals(seed, 0, n, size)
    assert first_difference(got, model, size) is None
