"""The feed's contract on the CPU (include/deepbinner_hip.h, "device-fed batches, validation";
DESIGN.md section 19): tests/feed_reference.py - which the device is held to bit for bit in
tests/test_gpu_feed.py - against the reference's own formula and law, dbh_epoch_order (host only)
against its restatement, and the new entries' argument checks, which come before any device work.
"""
import ctypes

import numpy as np
import pytest

import feed_reference as fr
from deepbinner_amd import hip_backend
from deepbinner_amd.model_format import param_count

INVALID, BAD_WEIGHTS, UNSUPPORTED = 1, 4, 5
# a key tie that straddles a rank boundary: (input size, seed, slot)
TIES = [(16384, 7, 29), (1024, 24, 36)]
# The same for the sizes at which an assembling thread holds 2, 3, 5 and 16 positions and the last
# busy thread fewer (tests/test_gpu_feed.py): for each size the first hit of a search over seeds
# 0..1999 and slots 0..63, seeds in order, every size found (seeds 24, 10, 1 and 8).
PARTIAL_SIZES = [1026, 2050, 5000, 16382]
PARTIAL_TIES = [(1026, 24, 36), (2050, 10, 14), (5000, 1, 13), (16382, 8, 29)]


# ---- normalise -----------------------------------------------------------------------------------
@pytest.mark.parametrize('length', [96, 1024, 16384])
def test_normalise_has_the_reference_formulas_fp32_bits(length):
    rng = np.random.default_rng([1, length])
    # signal-like windows: a level, a spread and an occasional outlier per window
    level = rng.integers(300, 700, size=(200, 1))
    spread = rng.integers(5, 120, size=(200, 1))
    windows = np.rint(level + spread * rng.standard_normal((200, length))).astype(np.int16)
    windows = np.concatenate([windows, fr.special_windows(length)])
    got = fr.normalise(windows)
    want = np.stack([fr.keras_side_normalise(w) for w in windows])
    assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all()
    _, std, d = fr.window_stats(windows)
    assert d[200] == 0 and std[200] == 0 and (got[200] == 0).all()          # the constant window
    if length == 16384:
        assert d[201] > 2 ** 53 and d[203] > 2 ** 53
        assert int(np.float64(d[203])) != int(d[203])                       # (double)D rounds


# ---- augment -------------------------------------------------------------------------------------
def test_half_is_pythons_round():
    assert [fr.half_of(n) for n in (96, 98, 102, 130, 1024, 16384)] == [24, 24, 26, 32, 256, 4096]
    assert [fr.half_of(n) for n in PARTIAL_SIZES] == [256, 512, 1250, 4096]


@pytest.mark.parametrize('length', [96, 98, 102, 130, 1024] + PARTIAL_SIZES)
def test_augment_doubles_half_drops_half_and_keeps_the_order(length):
    half = fr.half_of(length)
    for slot in range(4):
        sources = fr.augment_sources(11, slot, length)
        assert sources.size == length and (np.diff(sources) >= 0).all()
        times = np.bincount(sources, minlength=length)
        assert (times == 2).sum() == half and (times == 0).sum() == half
        assert (times == 1).sum() == length - 2 * half


def test_augmentation_one_is_the_identity_and_below_one_an_error():
    windows = fr.special_windows(98)
    assert fr.augment_threshold(1.0) == 0
    x, labels = fr.batch(windows, [0, 1, 2, 0], [2, 0, 1, 2], augmentation=1.0, seed=99)
    assert (x.view(np.uint32) == fr.normalise(windows[[2, 0, 1, 2]]).view(np.uint32)).all()
    assert list(labels) == [2, 0, 1, 2]
    assert fr.augment_threshold(2.0) == 2 ** 23 and fr.augment_threshold(1e9) == 2 ** 24 - 1
    for bad in (0.5, float('nan'), -1.0):
        with pytest.raises(ValueError):
            fr.augment_threshold(bad)


def test_doubling_is_uniform_over_positions():
    """4,096 windows of 96: a position is doubled with chance 24 / 96; each position's count lies
    within 5 standard deviations of the binomial expectation (a chance of 6e-7 per position)."""
    length, n = 96, 4096
    doubled = np.zeros(length)
    for slot in range(n):
        doubled += np.bincount(fr.augment_sources(3, slot, length), minlength=length) == 2
    p = fr.half_of(length) / length
    assert (np.abs(doubled - n * p) <= 5 * np.sqrt(n * p * (1 - p))).all()
    # and about 1 - 1/aug of the slots are augmented at all
    chosen = sum(fr.slot_is_augmented(3, slot, fr.augment_threshold(2.0)) for slot in range(n))
    assert abs(chosen - n / 2) <= 5 * np.sqrt(n / 4)


@pytest.mark.parametrize('length,seed,slot', TIES + PARTIAL_TIES)
def test_equal_keys_rank_by_index(length, seed, slot):
    keys = fr.keys_of(seed, slot, length)
    half = fr.half_of(length)
    ranks = fr.ranks_of(keys)
    copies = fr.copies_of(ranks, half)
    # the straddle: two positions with one key and different fates, the lower index ranked first
    order = np.argsort(ranks)
    tied = [(order[r], order[r + 1]) for r in (half - 1, 2 * half - 1)
            if keys[order[r]] == keys[order[r + 1]]]
    assert tied, 'no key tie across a rank boundary'
    for i, j in tied:
        assert i < j and copies[i] != copies[j]
    other = fr.augment_sources(seed, slot, length, ties='descending')
    assert (other != fr.augment_sources(seed, slot, length)).any()


# ---- epoch order ---------------------------------------------------------------------------------
@pytest.mark.parametrize('seed,epoch_pass,n', [(0, 0, 1), (7, 0, 1000), (7, 1, 1000),
                                               (2 ** 63 + 5, 16384 + 3, 5000), (1, 2, 70000)])
def test_epoch_order_equals_its_restatement(seed, epoch_pass, n):
    got = hip_backend.epoch_order(seed, epoch_pass, n)
    assert got.dtype == np.int64 and (got == fr.epoch_order(seed, epoch_pass, n)).all()
    assert (np.sort(got) == np.arange(n)).all()


def test_epoch_order_depends_on_pass_and_seed():
    base = hip_backend.epoch_order(7, 0, 1000)
    assert (hip_backend.epoch_order(7, 1, 1000) != base).mean() > 0.9
    assert (hip_backend.epoch_order(8, 0, 1000) != base).mean() > 0.9
    assert (hip_backend.epoch_order(7 + 2 ** 32, 0, 1000) != base).mean() > 0.9
    assert (hip_backend.epoch_order(7, 2 ** 14, 1000) == base).all()        # pass mod 2^14
    # 70,000 samples over 2^24 keys: equal keys exist, and keep their index order
    keys = fr.bits(1, fr.LAYER_ORDER, np.arange(70000), 2)
    assert np.unique(keys).size < 70000


def test_the_stream_runs_through_the_passes():
    n, batch = 10, 4
    stream = np.concatenate([fr.epoch_order(5, p, n) for p in range(3)])
    for t in range(7):
        assert (fr.stream_indices(5, n, t * batch, batch) == stream[t * batch:(t + 1) * batch]).all()
    from deepbinner_amd.fit import stream_indices
    assert (stream_indices(hip_backend.epoch_order, 5, n, 8, 12) == stream[8:20]).all()


# ---- the ABI -------------------------------------------------------------------------------------
NEW_SYMBOLS = ['dbh_epoch_order', 'dbh_dataset_create', 'dbh_dataset_destroy', 'dbh_dataset_count',
               'dbh_dataset_batch', 'dbh_dataset_batch_dev', 'dbh_evaluate', 'dbh_evaluate_dev',
               'dbh_trainer_step_dataset', 'dbh_trainer_step_dataset_dev',
               'dbh_trainer_evaluate_dataset']


def test_new_symbols_are_exported():
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in hip_backend.EXPORTED_SYMBOLS, name


def test_arguments_are_refused_before_any_device_work():
    lib = hip_backend.load_library()
    order = np.full(4, -1, dtype=np.int64)
    assert lib.dbh_epoch_order(0, 0, 0, order.ctypes.data) == INVALID
    assert lib.dbh_epoch_order(0, -1, 4, order.ctypes.data) == INVALID
    assert lib.dbh_epoch_order(0, 0, 4, None) == INVALID
    assert lib.dbh_epoch_order(0, 0, 2 ** 31 + 1, order.ctypes.data) == UNSUPPORTED
    assert (order == -1).all()

    handle = ctypes.c_void_p()
    samples = np.zeros((3, 96), dtype=np.int16)
    labels = np.array([0, 1, 2], dtype=np.int32)

    def create(n=3, size=96, classes=3, s=samples, lab=labels, out=ctypes.byref(handle)):
        return lib.dbh_dataset_create(s.ctypes.data if s is not None else None,
                                      lab.ctypes.data if lab is not None else None, n, size,
                                      classes, out)
    assert create(size=95) == UNSUPPORTED and create(size=16386) == UNSUPPORTED
    assert create(classes=1) == UNSUPPORTED and create(classes=257) == UNSUPPORTED
    assert create(n=0) == INVALID and create(s=None) == INVALID and create(lab=None) == INVALID
    assert create(out=None) == INVALID
    assert create(classes=2) == INVALID                              # a label outside [0, 2)
    assert create(lab=np.array([0, -1, 1], dtype=np.int32)) == INVALID
    assert not handle.value
    assert lib.dbh_dataset_destroy(None) == 0
    count = ctypes.c_int64(7)
    assert lib.dbh_dataset_count(None, ctypes.byref(count)) == INVALID and count.value == 7
    x = np.zeros((2, 96), dtype=np.float32)
    assert lib.dbh_dataset_batch(None, order.ctypes.data, 2, 2.0, 0, x.ctypes.data,
                                 labels.ctypes.data) == INVALID
    assert lib.dbh_dataset_batch_dev(None, None, 2, 2.0, 0, None, None, None) == INVALID

    loss, right = ctypes.c_double(7.0), ctypes.c_int64(7)
    blob = np.zeros(param_count(3), dtype=np.float32)

    def evaluate(n_floats=blob.size, classes=3, size=96, n=2, lab=labels):
        return lib.dbh_evaluate(blob.ctypes.data, n_floats, classes, size, x.ctypes.data,
                                lab.ctypes.data, n, ctypes.byref(loss), ctypes.byref(right), None)
    assert evaluate(size=97) == UNSUPPORTED and evaluate(classes=300) == UNSUPPORTED
    assert evaluate(n_floats=blob.size - 1) == BAD_WEIGHTS
    assert evaluate(n=0) == INVALID and evaluate(n=2 ** 20) == UNSUPPORTED
    assert evaluate(lab=np.array([0, 3], dtype=np.int32)) == INVALID
    assert lib.dbh_evaluate_dev(None, blob.size, 3, 96, None, None, 2, None, None, None, None,
                                None) == INVALID
    assert lib.dbh_trainer_step_dataset(None, None, order.ctypes.data, 2, 2.0, ctypes.byref(loss),
                                        ctypes.byref(right)) == INVALID
    assert lib.dbh_trainer_step_dataset_dev(None, None, None, 2, 2.0, None, None, None) == INVALID
    assert lib.dbh_trainer_evaluate_dataset(None, None, 0, 2, ctypes.byref(loss),
                                            ctypes.byref(right), None) == INVALID
    assert (loss.value, right.value) == (7.0, 7)


# ---- the evaluate cases the device is held to ------------------------------------------------------
@pytest.mark.parametrize('case', fr.EVAL_CASES, ids=str)
def test_no_evaluate_case_has_a_close_call(case):
    """n_correct is compared as a number: the fp64 reference's two largest logits are further
    apart than 1e-3 in every window, and its fp32 run makes the same calls."""
    ref = fr.eval_case(case)
    assert (ref['gap'] > fr.EVAL_GAP).all(), ref['gap']
    assert (ref['best32'] == ref['best64']).all()
    assert np.isfinite(ref['loss64']).all() and (ref['loss64'] > 0).all()
