"""The host-side arithmetic of libdeepbinner_hip.so (deepbinner_amd/csrc/dbh_host_layout.h: buffer
layouts, the order inflate records travel in, the staged copy, scan steps, the offsets check and
the live chunk-flag mask; dbh_network.h: the
network table every native path reads; dbh_pack.h: both weight packers), compiled into a program of
its own (oracle/api_host_test.cpp, built by oracle/Makefile from the very headers the library
includes) and run on the build box, without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, REPO
from deepbinner_amd import model_format

HARNESS = os.path.join(REPO, 'oracle', '_build', 'api_host_test')
# dbh_inflate_stream (include/deepbinner_hip.h) and its modes
STREAM = np.dtype([('comp_offset', '<i8'), ('comp_bytes', '<i8'), ('out_offset', '<i8'),
                   ('out_bytes', '<i8'), ('mode', '<i4'), ('reserved', '<i4')])
ZLIB, STORED, VBZ, VBZ_ZSTD, ZLIB_SHUFFLE, STORED_SHUFFLE = range(6)

pytestmark = pytest.mark.skipif(not os.path.exists(HARNESS),
                                reason='oracle/_build/api_host_test not built (make -C oracle)')


def seeded_records():
    """A few hundred records of every mode; lengths from a small range, so that ties abound - among
    deflate streams of one length, and among all the streams that need no decoding."""
    rng = np.random.default_rng(20261018)
    records = np.zeros(400, dtype=STREAM)
    records['mode'] = rng.integers(0, 6, len(records))
    records['comp_bytes'] = rng.integers(0, 40, len(records))
    records['comp_offset'] = np.cumsum(records['comp_bytes']) - records['comp_bytes']
    records['out_bytes'] = 2 * rng.integers(0, 100, len(records))
    assert set(records['mode']) == set(range(6))
    return records


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('api_host') / 'records.bin')
    seeded_records().tofile(path)
    run = subprocess.run([HARNESS, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout.splitlines()


def test_layouts_and_staged_copy(lines):
    """The program's own checks: regions of both layouts tile their buffer in order, aligned as they
    are documented, for one model, two models, zero streams and one read; staged_copy over sizes
    on both sides of its thresholds copies every byte and no other."""
    checks = [line.split() for line in lines
              if not line.startswith(('model_steps', 'order', 'offsets_forwards', 'chunk_flags'))]
    assert all(c[0] == 'ok' for c in checks), [c for c in checks if c[0] != 'ok']
    assert sum(c[1:3] == ['layout', 'deflated'] for c in checks) >= 6
    assert sum(c[1:3] == ['layout', 'group'] for c in checks) == 12
    assert [int(c[2]) for c in checks if c[1] == 'staged_copy'] == [
        0, 1, (16 << 20) - 1, 16 << 20, 32 << 20, (32 << 20) + 4097]
    assert any(c[1] == 'uniform_length' for c in checks)


def test_sweep_layout_sizes_and_carves_alike(lines):
    """dbh_host::SweepOut, what a group of the sweep brings back: for the start model alone, the end
    model alone and both, at 0, 1 and 300 reads and 1 and 24 scan steps, the sizing pass (null base)
    ends at the same total as the carving pass, a present side's best and margin lie in order,
    256-aligned and without overlap, and an absent side has null pointers and takes no bytes."""
    checks = [line.split() for line in lines if line.split()[1:3] == ['layout', 'sweep']]
    assert all(c[0] == 'ok' for c in checks), [c for c in checks if c[0] != 'ok']
    assert sorted(tuple(int(x) for x in c[3:6]) for c in checks) == sorted(
        (has, n_reads, steps) for has in (1, 2, 3) for n_reads in (0, 1, 300) for steps in (1, 24))


def test_carve_sizes_and_carves_alike(lines):
    """dbh_host::Carve, which lays out every buffer of the training-data units: the sizing pass
    (null base) and the carving pass of one sequence of take() calls end at the same `used`, the
    sizing pass yields null pointers, every carved pointer is a multiple of 256 bytes from the base
    and starts where the region before it ended, and no elements take no bytes."""
    checks = {c[2]: c for c in (line.split() for line in lines) if c[1] == 'carve'}
    assert set(checks) == {'used', 'null_base', 'aligned', 'in_order', 'take_nothing'}
    assert all(c[0] == 'ok' for c in checks.values()), checks
    need, used = int(checks['used'][3]), int(checks['used'][4])
    # 7 counts x (char, int32, double), each region rounded up to 256 bytes
    assert need == used == sum((n * size + 255) // 256 * 256
                               for n in (0, 1, 63, 64, 65, 1000, 4097) for size in (1, 4, 8))
    assert any(line.split()[:2] == ['ok', 'blocks_for'] for line in lines)


def test_record_order_is_longest_deflate_stream_first(lines):
    records = seeded_records()
    got = [int(x) for x in next(line for line in lines if line.startswith('order')).split()[1:]]

    def key(i):
        deflate = records['mode'][i] in (ZLIB, ZLIB_SHUFFLE)
        return (-(int(records['comp_bytes'][i]) if deflate else -1), i)
    assert got == sorted(range(len(records)), key=key)
    # (ties there were: fewer distinct keys than records)
    assert len({key(i)[0] for i in range(len(records))}) < len(records) // 4


def test_model_steps_is_check_input_size(lines):
    """model_steps: scan_size / (input_size / 2) where classify.check_input_size accepts the pair
    and there is at least one window, 0 where it exits."""
    from deepbinner_amd import classify
    seen = set()
    for line in lines:
        if not line.startswith('model_steps'):
            continue
        _, input_size, scan_size, _, steps = line.split()
        input_size, scan_size, steps = int(input_size), int(scan_size), int(steps)
        try:
            classify.check_input_size(input_size, scan_size)
            want = scan_size // (input_size // 2)
        except SystemExit:
            want = 0
        assert steps == want, line
        seen.add((input_size, steps > 0))
    assert seen == {(size, fits) for size in (96, 1024, 2048) for fits in (True, False)}


def test_offsets_check_and_chunk_flag_mask(lines):
    """The pure checks every host route's arguments go through, line for line.  offsets_run_forwards:
    no read (the table is not looked at), one read of no samples, a backward step in the first, a
    middle and the last position, and a table that starts at 100 - which runs forwards, its total
    counted from there.  live_chunk_flags_ok: BEGIN, END, both and neither are a chunk's flags; bit 2
    alone, beside either flag, and bit 31 beside both are not."""
    assert [line for line in lines if line.startswith('offsets_forwards')] == [
        'offsets_forwards empty = ok 0',
        'offsets_forwards one_read_no_samples = ok 0',
        'offsets_forwards forwards = ok 10',
        'offsets_forwards backward_first = bad',
        'offsets_forwards backward_middle = bad',
        'offsets_forwards backward_last = bad',
        'offsets_forwards first_not_zero = ok 10',
    ]
    assert [line for line in lines if line.startswith('chunk_flags')] == [
        'chunk_flags 0 = ok',
        'chunk_flags 1 = ok',
        'chunk_flags 2 = ok',
        'chunk_flags 3 = ok',
        'chunk_flags 4 = bad',
        'chunk_flags 5 = bad',
        'chunk_flags 6 = bad',
        'chunk_flags {} = bad'.format(3 | 1 << 31),
    ]


# ---- dbh_network.h against the specification, dbh_pack.h against the parent's images ------------
SHIPPED = ['EXP-NBD103_read_ends', 'EXP-NBD103_read_starts', 'SQK-RBK004_read_starts']
RANDOM_CLASSES = [2, 13, 17, 32, 33, 256]     # weight_families.random_model(0, C)
STAGE_SIZES = [96, 98, 200, 1024, 16382, 16384]


@pytest.fixture(scope='module')
def network(tmp_path_factory):
    """The lines of ``api_host_test --network`` over the shipped models' blobs and the random
    family's, by their first word."""
    from weight_families import random_model
    tmp = tmp_path_factory.mktemp('api_host_network')
    blobs = []
    for name in SHIPPED:
        w, _ = model_format.ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models', name + '.dbw'))
        blobs.append((name, w))
    blobs += [('random-s0-C{}'.format(c), random_model(0, c)) for c in RANDOM_CLASSES]
    args = []
    for name, w in blobs:
        w.flat().tofile(str(tmp / name))
        args += [str(tmp / name), str(w.n_classes)]
    run = subprocess.run([HARNESS, '--network'] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = {}
    for line in run.stdout.splitlines():
        out.setdefault(line.split()[0], []).append(line.split()[1:])
    return out


def test_network_table_is_model_format(network):
    """The 20 rows, the seven BN channel counts and epsilon, the parameter count and the blob's
    offsets restate model_format.py."""
    rows = [[int(x) for x in r[:5]] for r in network['conv']]
    assert rows == [[i + 1, k, cin, cout or 0, stride]
                    for i, (_, k, cin, cout, stride, _) in enumerate(model_format.CONV_LAYERS)]
    assert [[int(x) for x in r] for r in network['bn']] == [
        [j + 1, c] for j, c in enumerate(model_format.BN_CHANNELS)]
    assert [float(r[0]) for r in network['bn_eps']] == [model_format.BN_EPSILON]
    assert [[int(x) for x in r] for r in network['param_count']] == [
        [c, model_format.param_count(c)] for c in (2, 13, 32, 33, 256)]
    for r, c in zip(network['blob'], (2, 256)):
        want, at = [c], 0
        for _, k, cin, cout, _, _ in model_format.conv_shapes(c):
            want += [at, at + k * cin * cout]
            at += k * cin * cout + cout
        for channels in model_format.BN_CHANNELS:
            want.append(at)
            at += 4 * channels
        assert at == model_format.param_count(c)
        assert [int(x) for x in r] == want


def test_stage_lengths_and_stage_indices_are_the_oracles(network):
    """stage_lengths(L) is the oracle's own stage shapes at the minimum, at sizes odd at the first
    and the third stage, the shipped size and the two largest; every convolution takes len[in] to
    len[out] by the padding rule of its row in model_format.py."""
    from test_log_space_compare import stage_lengths
    from train_reference import _pads
    got = {int(r[0]): [int(x) for x in r] for r in network['stage_lengths']}
    assert sorted(got) == STAGE_SIZES
    assert got[96][1:] == [48, 24, 12, 6, 3, 2, 1]
    assert got[98][1:3] == [49, 24]
    assert got[200][1:] == [100, 50, 25, 12, 6, 3, 1]
    for size in STAGE_SIZES:
        assert got[size][1:] == stage_lengths(size), size
        for r, (_, k, _, _, stride, padding) in zip(network['conv'], model_format.CONV_LAYERS):
            assert r[5] == 'in' and r[7] == 'out'
            assert _pads(got[size][int(r[6])], k, stride, padding)[0] == got[size][int(r[8])], (size, r)


def test_same_pad_left_is_the_training_references(network):
    from train_reference import _pads
    seen = set()
    for k, stride, lin, lout, _, pad in ([int(x) if x != '=' else x for x in r]
                                         for r in network['same_pad_left']):
        assert (lout, pad) == _pads(lin, k, stride, 'same')[:2], (k, stride, lin)
        seen.add((k, stride, lin))
    assert seen == {(k, stride, lin) for _, k, _, _, stride, _ in model_format.CONV_LAYERS
                    for lin in (1, 2, 3, 6, 7)}


def test_packed_images_are_the_parents_bit_for_bit(network):
    """Size and 64-bit FNV-1a digest of the persistent image (C <= 32) and of the general image of
    the three shipped models and of random_model(0, C), against tests/golden/packed_digests.txt:
    the lines the two packers printed when they had been moved out of dbh_api.hip and
    dbh_general.hip word for word, before they were rewritten onto dbh_network.h.  (The parent's
    pack_weights, cut out of its dbh_api.hip into a g++ program of its own, prints the same three
    persistent digests for the shipped models: 40e3dec5ca30d7b1, f7e5d613ff8f7391,
    cc10426847f67325 - profiles/network_table/packed_digests_parent.txt.)"""
    with open(os.path.join(GOLD, 'packed_digests.txt')) as f:
        golden = [line.split()[1:] for line in f.read().splitlines()]
    assert network['packed'] == golden
    kinds = {(r[0], r[1]) for r in golden}
    assert {('persistent', n) for n in SHIPPED} | {('general', n) for n in SHIPPED} <= kinds
    assert {('persistent', 'random-s0-C{}'.format(c)) for c in (2, 17, 32)} <= kinds
    assert {('general', 'random-s0-C{}'.format(c)) for c in (2, 13, 33, 256)} <= kinds
    assert all(r[3] == '153248' for r in golden if r[0] == 'persistent')
