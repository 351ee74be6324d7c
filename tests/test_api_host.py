"""The host-side arithmetic of libdeepbinner_hip.so's API layer (deepbinner_amd/csrc/
dbh_host_layout.h: buffer layouts, the order inflate records travel in, the staged copy, scan
steps), compiled into a program of its own (oracle/api_host_test.cpp, built by oracle/Makefile from
the very header dbh_api.hip includes) and run on the build box, without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

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
    checks = [line.split() for line in lines if not line.startswith(('model_steps', 'order'))]
    assert all(c[0] == 'ok' for c in checks), [c for c in checks if c[0] != 'ok']
    assert sum(c[1:3] == ['layout', 'deflated'] for c in checks) >= 6
    assert sum(c[1:3] == ['layout', 'group'] for c in checks) == 12
    assert [int(c[2]) for c in checks if c[1] == 'staged_copy'] == [
        0, 1, (16 << 20) - 1, 16 << 20, 32 << 20, (32 << 20) + 4097]
    assert any(c[1] == 'uniform_length' for c in checks)


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
