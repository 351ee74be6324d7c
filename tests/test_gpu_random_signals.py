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
