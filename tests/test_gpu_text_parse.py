"""Training-data text parsed on the GPU (dbh_text_parse, csrc/dbh_text.hip)
against its CPU model (dbh_text_parse_host), bit for bit: kinds, line count, first refused line,
and the rows and labels of the lines that are OK.  The model itself is held to the grammar's
restatement on the same corpus without a device (tests/test_text_parse.py)."""
import random

import numpy as np
import pytest

import text_parse_reference as tr

pytestmark = pytest.mark.gpu


def both(hip, data, input_size):
    got = hip.parse_training_text(data, input_size)
    tr.same_results(got, hip.parse_training_text_host(data, input_size))
    return got


def test_one_line_of_four_values(hip):
    samples, labels, kinds, first_bad = both(hip, b'3\t1,-2,+3,0004\n', 4)
    assert samples.tolist() == [[1, -2, 3, 4]] and labels.tolist() == [3]
    assert kinds.tolist() == [tr.OK] and first_bad == -1


def test_the_whole_corpus(hip):
    seen = 0
    for name, data, input_size, _ in tr.blocks():
        both(hip, data, input_size)
        seen += 1
    assert seen > 16 * 50


def mixed_lines(rng, n, bad_at):
    lines = [tr.random_strict_line(rng, rng.choice([1, 7, 96, 96, 96, 700]), crlf=rng.random() < 0.1)
             for _ in range(n)]
    for k, bad in zip(bad_at, (b'1\t5,,6', b'x', b'1\t' + b','.join([b'40000'] * 96))):
        lines[k] = bad
    return lines


@pytest.mark.parametrize('case', ['3 lines', '300 lines', '5,000 lines', 'one long line'])
def test_block_sizes_and_replay(hip, case):
    rng = random.Random(5)
    if case == '3 lines':
        lines, input_size = [tr.random_strict_line(rng, 96) for _ in range(3)], 96
    elif case == '300 lines':
        lines, input_size = mixed_lines(rng, 300, (0, 150, 299)), 96
    elif case == '5,000 lines':
        few = [tr.random_strict_line(rng, 1024) for _ in range(50)]
        lines, input_size = [few[(7 * k) % 50] for k in range(5000)], 1024
    else:
        lines, input_size = [b'12\t' + b','.join([b'-012345'] * 16384)], 16384
    data = b''.join(line + b'\n' for line in lines)
    if case == '5,000 lines':
        # the model on the 50 distinct lines, spread out, is the model on the block
        assert len(data) > 18 << 20
        small = hip.parse_training_text_host(b''.join(line + b'\n' for line in few), input_size)
        order = [(7 * k) % 50 for k in range(5000)]
        first = hip.parse_training_text(data, input_size)
        tr.same_results(first, (small[0][order], small[1][order], small[2][order], -1))
    else:
        first = both(hip, data, input_size)
    tr.same_results(first, hip.parse_training_text(data, input_size))
    assert len(first[2]) == len(lines)
    if case == '300 lines':
        assert first[3] == 0 and first[2][150] == tr.FORM and first[2][299] == tr.RANGE
        assert (first[2] == tr.COUNT).sum() > 50 and (first[2] == tr.OK).sum() > 100
    else:
        assert first[3] == -1 and not first[2].any()


def test_an_lf_in_every_piece_of_two_tiles(hip):
    """Lines of 4 to 8 bytes, just over two tiles of 4,096 of them: every 16-byte piece holds one to
    four LFs, so every lane adds to the tile's prefix - on both sides of every row of 16 lanes and
    of every wave of a workgroup - and a line that started a byte off would parse as another."""
    values = [(-1) ** k * (k * 37 % 10 ** (1 + k % 4)) for k in range(1500)]
    data = b''.join(b'%d\t%d\n' % (k % 10, v) for k, v in enumerate(values))
    while len(data) > 8192 + 40:
        values.pop()
        data = data[:data.rindex(b'\n', 0, -1) + 1]
    assert 8192 < len(data) and max(len(line) for line in data.split(b'\n')) <= 7
    assert all(b'\n' in data[at:at + 16] for at in range(0, len(data) - 16, 16))
    samples, labels, kinds, first_bad = both(hip, data, 1)
    assert first_bad == -1 and not kinds.any()
    assert samples[:, 0].tolist() == values and labels.tolist() == [k % 10 for k in range(len(values))]


@pytest.mark.parametrize('refused', tr.MANY_VARIANTS, ids=str)
def test_more_lines_than_the_grid_has_waves(hip, refused):
    """70,000 lines of 7 values over 32,768 waves: lines 32,768.. are a wave's second, lines
    65,536.. its third.  The first refused line is the minimum over all trips: line 0 of the first,
    line 40,000 of the second where line 0 is strict, line 69,999 of the third where it alone is
    refused."""
    data = tr.many_lines(refused)
    samples, labels, kinds, first_bad = both(hip, data, tr.MANY_SIZE)
    assert len(kinds) == tr.MANY_LINES and first_bad == refused[0]
    assert np.flatnonzero(kinds).tolist() == list(refused)
    assert [int(kinds[k]) for k in refused] == [tr.REFUSED[k][0] for k in refused]


@pytest.mark.parametrize('shift', tr.LONG_SHIFTS)
@pytest.mark.parametrize('input_size', tr.LONG_SIZES)
def test_lines_past_16384_values(hip, input_size, shift):
    """lines of 100,003 and of 2^20 values, hundreds and thousands of steps each: OK, a value out
    of range three from the end, a value short.  (At shift > 0 the line in front is refused too:
    tests/test_text_parse.py, test_model_equals_the_restatement_on_long_lines.)"""
    lines, values = tr.long_lines(input_size)
    data, skipped = tr.block(lines, shift)
    samples, labels, kinds, first_bad = both(hip, data, input_size)
    assert kinds[skipped:].tolist() == [tr.OK, tr.RANGE, tr.COUNT]
    assert first_bad == (0 if skipped else 1) and np.flatnonzero(kinds[skipped:])[0] == 1
    differ = np.flatnonzero(samples[skipped] != np.array(values))
    assert differ.size == 0, 'the OK line differs from the restatement first at value {}'.format(differ[0])
    assert labels[skipped] == int(lines[0].split(b'\t')[0])


def test_more_lines_than_the_arrays_hold(hip):
    data = b'\n' * 5000 + b'1\t5\n'
    with pytest.raises(hip.HipBackendError):
        hip.parse_training_text(data, 1, max_lines=5000)
    got = both(hip, data, 1)           # the wrapper's bound is too small: it asks again
    assert len(got[2]) == 5001 and got[3] == 0 and got[2][5000] == tr.OK


def test_dataset_from_file_on_both_routes(hip, tmp_path):
    rng = random.Random(9)
    lines = [b'%d\t' % (k % 4) + tr.random_strict_line(rng, 96).split(b'\t')[1] for k in range(64)]
    path = tmp_path / 'train.txt'
    path.write_bytes(b''.join(line + b'\n' for line in lines))
    indices = np.arange(64)[::-1].copy()
    with hip.Dataset.from_file(str(path), 4, parse='host') as host, \
            hip.Dataset.from_file(str(path), 4, parse='gpu') as gpu:
        assert len(host) == len(gpu) == 64
        x_host, l_host = host.batch(indices, augmentation=1.0)
        x_gpu, l_gpu = gpu.batch(indices, augmentation=1.0)
    assert np.array_equal(x_host, x_gpu) and np.array_equal(l_host, l_gpu)
    for got in (hip.read_training_data(str(path), parse=route) for route in ('host', 'gpu')):
        assert got[0].shape == (64, 96) and got[1].tolist() == [k % 4 for k in range(64)]
