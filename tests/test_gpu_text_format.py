"""Training-data text written on the GPU (dbh_text_format, csrc/dbh_format.hip)
against the CPU model (dbh_text_format_host), byte for byte.  The model itself is held to Python's
own formatting without a device (tests/test_text_format.py)."""
import ctypes

import numpy as np
import pytest

import text_format_reference as fr

pytestmark = pytest.mark.gpu


def both(hip, labels, samples):
    got = hip.format_training_text(labels, samples)
    assert got == hip.format_training_text(labels, samples, host=True)
    return got


@pytest.mark.parametrize('n', [1, 3, 6])
@pytest.mark.parametrize('size', fr.SIZES)
def test_device_equals_the_model(hip, size, n):
    labels, samples = fr.rows(size)
    first = 6 - n                                           # n = 1: the row of every width
    text = both(hip, labels[first:], samples[first:])
    assert text == fr.text(labels[first:], samples[first:])
    # and back through the device's parser
    back, back_labels, kinds, first_bad = hip.parse_training_text(text, size)
    assert first_bad == -1 and not kinds.any()
    assert np.array_equal(back, samples[first:]) and np.array_equal(back_labels, labels[first:])


def test_the_line_scan_spans_more_lines_than_it_has_threads(hip):
    labels, samples = fr.many_short_lines(1100)
    whole = both(hip, labels, samples)
    assert whole == fr.text(labels, samples)
    parts = [hip.format_training_text(labels[a:b], samples[a:b]) for a, b in ((0, 3), (3, 1100))]
    assert whole == b''.join(parts)
    assert hip.format_training_text(labels, samples) == whole


def test_more_lines_than_the_grid_has_waves(hip):
    """40,000 lines of one value: a wave takes more than one line"""
    labels, samples = fr.many_short_lines(40000)
    assert both(hip, labels, samples) == fr.text(labels, samples)


def first_difference(got, want):
    """where two texts part: the byte, and the line it lies in"""
    if got == want:
        return None
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    n = min(a.size, b.size)
    differ = np.flatnonzero(a[:n] != b[:n])
    at = int(differ[0]) if differ.size else n
    return 'lengths {} and {}, first difference at byte {} in line {}'.format(
        a.size, b.size, at, want.count(b'\n', 0, at))


@pytest.mark.parametrize('size', fr.LONG_SIZES)
def test_long_rows(hip, size):
    """a wave walks a row in steps of 64 values: 1,563 steps with a partial last one, and 16,384 -
    the prefix of the widths carried over millions of bytes"""
    labels, samples, want = fr.long_rows(size)
    model = hip.format_training_text(labels, samples, host=True)
    assert first_difference(model, want) is None
    got = hip.format_training_text(labels, samples)
    assert first_difference(got, model) is None
    back, back_labels, kinds, first_bad = hip.parse_training_text(got, size)
    assert first_bad == -1 and not kinds.any()
    assert np.array_equal(back, samples) and np.array_equal(back_labels, labels)


def test_the_tile_scan_spans_more_tiles_than_it_has_threads(hip):
    """1,100,000 lines of one value are 1,075 tiles: scan_tiles gives a thread two tiles, the last
    busy thread one, and the threads behind it none"""
    labels, samples, want = fr.many_lines()
    model = hip.format_training_text(labels, samples, host=True)
    assert first_difference(model, want) is None
    whole = hip.format_training_text(labels, samples)
    assert first_difference(whole, model) is None
    parts = [hip.format_training_text(labels[a:b], samples[a:b])
             for a, b in ((0, fr.SPLIT), (fr.SPLIT, fr.MANY_LINES))]
    assert first_difference(b''.join(parts), whole) is None


def test_a_refused_label_in_the_last_of_many_tiles(hip):
    """the device entry itself: 10^9 as a label in tile 1,074 of 1,075 - the length is -1 and the
    canary bytes, in front of the capacity and behind it, stay"""
    lib = hip.load_library()
    labels, samples, want = fr.many_lines()
    labels = labels.copy()
    bad = fr.MANY_LINES - 10
    assert bad // 1024 == (fr.MANY_LINES - 1) // 1024 == 1074
    labels[bad] = 10 ** 9
    n, canary = fr.MANY_LINES, 0xa5
    capacity = len(want) + 16                               # room for the line, were it written
    work = ctypes.c_size_t(0)
    assert lib.dbh_text_format_workspace_bytes(n, ctypes.byref(work)) == 0
    out = hip.DeviceBuffer.from_array(np.full(capacity + 256, canary, dtype=np.uint8))
    total = hip.DeviceBuffer.from_array(np.array([-7], dtype=np.int64))
    buffers = [out, total, hip.DeviceBuffer.from_array(labels), hip.DeviceBuffer.from_array(samples),
               hip.DeviceBuffer(work.value)]
    try:
        hip.check(lib.dbh_text_format_dev(buffers[2].ptr, buffers[3].ptr, n, 1, out.ptr, capacity,
                                          total.ptr, buffers[4].ptr, None), 'dbh_text_format_dev')
        assert total.download((1,), np.int64)[0] == -1
        assert (out.download((capacity + 256,), np.uint8) == canary).all()
        # the label put right: the same buffers hold the text
        labels[bad] = fr.many_lines()[0][bad]
        buffers[2].upload(labels)
        hip.check(lib.dbh_text_format_dev(buffers[2].ptr, buffers[3].ptr, n, 1, out.ptr, capacity,
                                          total.ptr, buffers[4].ptr, None), 'dbh_text_format_dev')
        assert total.download((1,), np.int64)[0] == len(want)
        got = out.download((capacity + 256,), np.uint8)
    finally:
        for b in buffers:
            b.free()
    assert first_difference(got[:len(want)].tobytes(), want) is None and (got[len(want):] == canary).all()


def test_a_refused_label_writes_nothing(hip):
    labels, samples = fr.rows(64)
    labels[4] = 10 ** 9
    with pytest.raises(hip.HipBackendError):
        hip.format_training_text(labels, samples)
    # in the second tile of the line scan, through the device entry itself
    labels, samples = fr.many_short_lines(1100)
    labels[1050] = -10 ** 9
    with hip.ResidentText(1100, 1) as resident:
        signals = resident.random_signals(0, 0, 1100)
        resident.samples.upload(samples, resident.stream.ptr)      # these rows in their place
        with pytest.raises(hip.HipBackendError):
            resident.format_training_text(labels, signals)
        labels[1050] = 7
        text = resident.format_training_text(labels, signals)
        assert bytes(text) == fr.text(labels, samples)
        del text


@pytest.mark.parametrize('short', [0, 1])
def test_capacity_exact_and_one_byte_short_on_the_device(hip, short):
    """the device entry itself, with canary bytes behind the capacity in device memory"""
    lib = hip.load_library()
    labels, samples = fr.rows(65)
    want = fr.text(labels, samples)
    need, canary = len(want), 0xa5
    capacity = need - short
    work = ctypes.c_size_t(0)
    assert lib.dbh_text_format_workspace_bytes(6, ctypes.byref(work)) == 0
    out = hip.DeviceBuffer.from_array(np.full(need + 256, canary, dtype=np.uint8))
    total = hip.DeviceBuffer.from_array(np.array([-7], dtype=np.int64))
    buffers = [out, total, hip.DeviceBuffer.from_array(labels), hip.DeviceBuffer.from_array(samples),
               hip.DeviceBuffer(work.value)]
    try:
        hip.check(lib.dbh_text_format_dev(buffers[2].ptr, buffers[3].ptr, 6, 65, out.ptr, capacity,
                                          total.ptr, buffers[4].ptr, None), 'dbh_text_format_dev')
        assert total.download((1,), np.int64)[0] == need
        got = out.download((need + 256,), np.uint8)
    finally:
        for b in buffers:
            b.free()
    if short:
        assert (got == canary).all()                        # nothing written
    else:
        assert got[:need].tobytes() == want and (got[need:] == canary).all()
    # the host entry: the need reported, the caller's bytes untouched
    host_out = np.full(need + 16, canary, dtype=np.uint8)
    n_bytes = ctypes.c_int64(0)
    status = lib.dbh_text_format(labels.ctypes.data, samples.ctypes.data, 6, 65, host_out.ctypes.data,
                                 capacity, ctypes.byref(n_bytes))
    assert n_bytes.value == need and status == (1 if short else 0)
    assert (host_out[capacity if short else need:] == canary).all()
    assert (host_out[:need] == canary).all() if short else host_out[:need].tobytes() == want
