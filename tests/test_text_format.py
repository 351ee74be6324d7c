"""The training-data text formatter's CPU model (dbh_text_format_host, csrc/dbh_format_core.h; DESIGN.md
section 23) against Python's own string formatting, back through the parser's CPU model
(dbh_text_parse_host), and the argument errors of every entry - none of which needs a device."""
import ctypes

import numpy as np
import pytest

import text_format_reference as fr
from deepbinner_amd import hip_backend


@pytest.mark.parametrize('size', fr.SIZES)
def test_host_model_writes_what_python_writes(size):
    labels, samples = fr.rows(size)
    got = hip_backend.format_training_text(labels, samples, host=True)
    assert got == fr.text(labels, samples)
    assert len(got) <= fr.bound(len(labels), size) == hip_backend.text_format_bound(len(labels), size)
    back, back_labels, kinds, first_bad = hip_backend.parse_training_text_host(got, size)
    assert first_bad == -1 and not kinds.any()
    assert np.array_equal(back, samples) and np.array_equal(back_labels, labels)


def test_the_bound_is_met_by_the_widest_line():
    labels = np.array([-999999999], dtype=np.int32)
    samples = np.full((1, 5), -32768, dtype=np.int16)
    assert len(hip_backend.format_training_text(labels, samples, host=True)) == fr.bound(1, 5) - 1


def test_many_short_lines_and_a_split():
    labels, samples = fr.many_short_lines(1100)
    whole = hip_backend.format_training_text(labels, samples, host=True)
    assert whole == fr.text(labels, samples)
    parts = [hip_backend.format_training_text(labels[a:b], samples[a:b], host=True)
             for a, b in ((0, 3), (3, 1100))]
    assert whole == b''.join(parts)


@pytest.mark.parametrize('size', fr.LONG_SIZES)
def test_host_model_writes_long_rows_as_python_does(size):
    """the device is held to this model at these sizes (tests/test_gpu_text_format.py)"""
    labels, samples, want = fr.long_rows(size)
    got = hip_backend.format_training_text(labels, samples, host=True)
    assert got == want
    assert len(got) <= fr.bound(2, size) == hip_backend.text_format_bound(2, size)
    back, back_labels, kinds, first_bad = hip_backend.parse_training_text_host(got, size)
    assert first_bad == -1 and not kinds.any()
    assert np.array_equal(back, samples) and np.array_equal(back_labels, labels)


def test_more_lines_than_the_tile_scan_has_threads_and_a_split():
    """1,100,000 lines are 1,075 tiles of 1,024: the device's scan over tiles gives a thread two"""
    labels, samples, want = fr.many_lines()
    assert (len(labels) + 1023) // 1024 == 1075 and fr.SPLIT % 1024
    whole = hip_backend.format_training_text(labels, samples, host=True)
    assert whole == want
    parts = [hip_backend.format_training_text(labels[a:b], samples[a:b], host=True)
             for a, b in ((0, fr.SPLIT), (fr.SPLIT, fr.MANY_LINES))]
    assert whole == b''.join(parts)


def test_write_training_data_is_read_back(tmp_path):
    labels, samples = fr.rows(65)
    path = tmp_path / 'written.txt'
    hip_backend.write_training_data(str(path), labels[:4], samples[:4], host=True)
    back, back_labels = hip_backend.read_training_data(str(path), parse='host')
    assert np.array_equal(back, samples[:4]) and np.array_equal(back_labels, labels[:4])
    with pytest.raises(ValueError):
        hip_backend.format_training_text(labels[:4], samples[:4].astype(np.int64) + 40000, host=True)


def raw(entry, labels, samples, n, size, out, capacity, n_bytes, workspace=True):
    lib = hip_backend.load_library()
    pointer = [None if a is None else a.ctypes.data for a in (labels, samples, out)]
    if entry == 'dbh_text_format_dev':
        # (no call here gets as far as a launch: any address stands for the workspace)
        return lib.dbh_text_format_dev(pointer[0], pointer[1], n, size, pointer[2], capacity,
                                       None if n_bytes is None else ctypes.addressof(n_bytes),
                                       labels.ctypes.data if workspace and labels is not None else None,
                                       None)
    return getattr(lib, entry)(pointer[0], pointer[1], n, size, pointer[2], capacity,
                               None if n_bytes is None else ctypes.byref(n_bytes))


def test_a_capacity_one_byte_short_writes_nothing():
    labels, samples = fr.rows(63)
    need = len(fr.text(labels, samples))
    out = np.full(need + 64, 0xa5, dtype=np.uint8)
    n_bytes = ctypes.c_int64(-7)
    assert raw('dbh_text_format_host', labels, samples, 6, 63, out, need - 1, n_bytes) == 1
    assert n_bytes.value == need and (out == 0xa5).all()
    assert raw('dbh_text_format_host', labels, samples, 6, 63, out, need, n_bytes) == 0
    assert out[:need].tobytes() == fr.text(labels, samples) and (out[need:] == 0xa5).all()


@pytest.mark.parametrize('entry', ['dbh_text_format', 'dbh_text_format_dev', 'dbh_text_format_host'])
def test_argument_errors_come_before_any_device_work(entry):
    labels, samples = fr.rows(2)
    out, n_bytes = np.zeros(256, dtype=np.uint8), ctypes.c_int64(0)
    invalid, unsupported = 1, 5
    assert raw(entry, None, samples, 6, 2, out, 256, n_bytes) == invalid
    assert raw(entry, labels, None, 6, 2, out, 256, n_bytes) == invalid
    assert raw(entry, labels, samples, 6, 2, None, 256, n_bytes) == invalid
    assert raw(entry, labels, samples, 6, 2, out, 256, None) == invalid
    assert raw(entry, labels, samples, 0, 2, out, 256, n_bytes) == invalid
    assert raw(entry, labels, samples, 6, 0, out, 256, n_bytes) == invalid
    assert raw(entry, labels, samples, 6, 2, out, -1, n_bytes) == invalid
    assert raw(entry, labels, samples, 1, 2 ** 20 + 1, out, 256, n_bytes) == unsupported
    assert raw(entry, labels, samples, 2 ** 29 + 1, 2, out, 256, n_bytes) == unsupported
    if entry == 'dbh_text_format_dev':
        assert raw(entry, labels, samples, 6, 2, out, 256, n_bytes, workspace=False) == invalid
    else:                                                 # the labels are the host's to read
        for label in (10 ** 9, -10 ** 9):
            labels[3] = label
            assert raw(entry, labels, samples, 6, 2, out, 256, n_bytes) == invalid


def test_the_bound_and_the_workspace_refuse_the_same():
    lib = hip_backend.load_library()
    bound, work = ctypes.c_int64(0), ctypes.c_size_t(0)
    assert lib.dbh_text_format_bound(3, 1024, ctypes.byref(bound)) == 0 and bound.value == 3 * 7180
    assert lib.dbh_text_format_bound(0, 1024, ctypes.byref(bound)) == 1
    assert lib.dbh_text_format_bound(3, 0, ctypes.byref(bound)) == 1
    assert lib.dbh_text_format_bound(3, 1024, None) == 1
    assert lib.dbh_text_format_bound(1, 2 ** 20 + 1, ctypes.byref(bound)) == 5
    assert lib.dbh_text_format_workspace_bytes(1100, ctypes.byref(work)) == 0
    assert work.value >= 1100 * 4 + 1101 * 8
    assert lib.dbh_text_format_workspace_bytes(0, ctypes.byref(work)) == 1
    assert lib.dbh_text_format_workspace_bytes(5, None) == 1
