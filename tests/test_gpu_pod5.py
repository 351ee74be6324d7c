"""``deepbinner classify`` on POD5 files on the GPU (`-m gpu`): the committed files of
tests/golden/pod5 (written by tests/pod5_fixtures.py from the seven golden reads) print the rows
that ``classify`` prints for the golden fast5 directory - the calls of tests/golden/calls.json -
plain and ``--verbose``, with the rows' zstd frames undone on the host and on the GPU, and on the
lists route; the damaged file classifies its five intact reads and warns about the other two; the
decoded samples the device hands back are the golden signals.  No pyarrow here.
"""
import os

import numpy as np
import pytest

import pod5_fixtures as pf
from conftest import GOLD
from deepbinner_amd import pod5_lite

pytestmark = pytest.mark.gpu

POD5 = os.path.join(GOLD, 'pod5')
SINGLE = os.path.join(GOLD, 'fast5', 'single')
START, END = 'EXP-NBD103_read_starts', 'EXP-NBD103_read_ends'
ROUTE_NAMES = ('DEEPBINNER_GPU_INFLATE', 'DEEPBINNER_HOST_INFLATE_SHARE', 'DEEPBINNER_FAST5_READER',
               'DEEPBINNER_VBZ_ZSTD', 'DEEPBINNER_DEVICE_ORDINALS', 'DEEPBINNER_DEVICES')


def set_route(monkeypatch, **env):
    for name in ROUTE_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def run(argv, capsys):
    """-> (header, rows, stderr) of one `deepbinner classify ...`"""
    from deepbinner_amd import deepbinner as cli
    capsys.readouterr()
    cli.main(['classify'] + [str(a) for a in argv])
    done = capsys.readouterr()
    lines = done.out.splitlines()
    return lines[0], lines[1:], done.err


@pytest.fixture(scope='module')
def fast5_rows(hip):
    """{(), ('--verbose',)}: (header, {read id: row}) of `classify --native` on the golden fast5
    directory - once, for every test here"""
    from deepbinner_amd import deepbinner as cli
    import contextlib
    import io
    out = {}
    for flags in ((), ('--verbose',)):
        text = io.StringIO()
        with contextlib.redirect_stdout(text), contextlib.redirect_stderr(io.StringIO()):
            cli.main(['classify', '--native'] + list(flags) + [SINGLE])
        lines = text.getvalue().splitlines()
        out[flags] = (lines[0], {row.split('\t')[0]: row for row in lines[1:]})
    return out


def test_the_fast5_rows_are_the_references_calls(fast5_rows, gold):
    from oracle import classify_ref
    starts = dict(zip(gold['read_ids'], gold['calls'][START + '/start']))
    ends = dict(zip(gold['read_ids'], gold['calls'][END + '/end']))
    want = {rid: classify_ref.combine_calls(starts[rid], ends[rid], 'require_either') for rid in starts}
    got = {rid: row.split('\t')[1] for rid, row in fast5_rows[()][1].items()}
    assert got == want and len(got) == 7


@pytest.mark.parametrize('zstd', ['host', 'gpu'])
@pytest.mark.parametrize('name', ['golden7.pod5', 'golden7_uncompressed.pod5'])
def test_classify_prints_the_rows_of_the_fast5_directory(name, zstd, fast5_rows, gold, capsys,
                                                         monkeypatch):
    """the raw route: rows to the GPU as stored (SVB16_ZSTD), with the zstd stage undone on the
    host (SVB16), or plain samples (STORED); reads in the file's order; the verbose rows are the
    printed bytes of the fast5 route"""
    set_route(monkeypatch, DEEPBINNER_GPU_INFLATE='1', DEEPBINNER_VBZ_ZSTD=zstd)
    for flags in ((), ('--verbose',)):
        header, rows, err = run(['--native'] + list(flags) + [os.path.join(POD5, name)], capsys)
        want_header, want = fast5_rows[flags]
        assert header == want_header
        assert rows == [want[rid] for rid in gold['read_ids']], (name, zstd, flags)
        assert 'Classifying fast5s: 1 / 1' in err and 'Barcode     Count' in err
        assert 'Warning' not in err


@pytest.mark.parametrize('zstd, modes', [(None, {6}), ('gpu', {7})])
def test_the_default_route_is_the_gpu_on_a_host_with_cores_to_spare(zstd, modes, hip, fast5_rows, gold,
                                                                   capsys, monkeypatch):
    """no route variable set, 128 usable CPUs (where fast5 containers stay on the host's thread
    team): the rows of a POD5 file still go to the device, as modes 6 and 7"""
    from deepbinner_amd import realtime
    set_route(monkeypatch, **({'DEEPBINNER_VBZ_ZSTD': zstd} if zstd else {}))
    monkeypatch.setattr(realtime, 'usable_cpus', lambda: 128)
    assert realtime.host_inflate_share(1) == 100
    used = []
    real = hip.classify_pair_deflated

    def watched(start, end, comp, streams, *args, **kwargs):
        used.extend(np.asarray(streams)['mode'].tolist())
        return real(start, end, comp, streams, *args, **kwargs)

    monkeypatch.setattr(hip, 'classify_pair_deflated', watched)
    _, rows, _ = run(['--native', os.path.join(POD5, 'golden7.pod5')], capsys)
    assert rows == [fast5_rows[()][1][rid] for rid in gold['read_ids']]
    assert set(used) == modes and len(used) == 50


def test_the_lists_route_prints_the_same(fast5_rows, gold, capsys, monkeypatch):
    set_route(monkeypatch, DEEPBINNER_GPU_INFLATE='0')
    for flags in ((), ('--verbose',)):
        header, rows, _ = run(['--native'] + list(flags) + [os.path.join(POD5, 'golden7.pod5')], capsys)
        assert header == fast5_rows[flags][0]
        assert rows == [fast5_rows[flags][1][rid] for rid in gold['read_ids']]


@pytest.mark.parametrize('zstd', ['host', 'gpu'])
def test_the_damaged_file_classifies_five_reads_and_warns_about_two(zstd, fast5_rows, gold, capsys,
                                                                    monkeypatch):
    """read 1's middle row is a byte short behind a valid zstd frame: the device refuses the
    stream (a status, not a fault), the host's decoder refuses the read; read 4's row list points
    outside the signal table: it never reaches the device.  The run goes on and ends as usual."""
    set_route(monkeypatch, DEEPBINNER_GPU_INFLATE='1', DEEPBINNER_VBZ_ZSTD=zstd)
    skipped = [gold['read_ids'][k] for k in sorted(pf.GOLDEN_DAMAGE)]
    for flags in ((), ('--verbose',)):
        _, rows, err = run(['--native'] + list(flags) + [os.path.join(POD5, 'golden7_damaged.pod5')],
                           capsys)
        want = fast5_rows[flags][1]
        assert rows == [want[rid] for rid in gold['read_ids'] if rid not in skipped]
        assert err.count('Warning: skipping read') == 2 and all(rid in err for rid in skipped)
        assert 'Classifying fast5s: 1 / 1' in err and 'Barcode     Count' in err


@pytest.mark.parametrize('name', ['golden7.pod5', 'golden7_damaged.pod5'])
def test_several_units_dealt_over_two_replicas(name, fast5_rows, gold, capsys, monkeypatch):
    """units of one read each under --devices 2 (two replicas on the one GPU): rows in the file's
    order, and a refused stream is read again as the read of the FILE that the unit's read is"""
    set_route(monkeypatch, DEEPBINNER_GPU_INFLATE='1', DEEPBINNER_DEVICE_ORDINALS='0,0')
    monkeypatch.setattr(pod5_lite, 'READS_PER_UNIT', 1)
    skipped = [gold['read_ids'][k] for k in sorted(pf.GOLDEN_DAMAGE)] if 'damaged' in name else []
    for flags in ((), ('--verbose',)):
        _, rows, err = run(['--native', '--devices', '2'] + list(flags) + [os.path.join(POD5, name)],
                           capsys)
        want = fast5_rows[flags][1]
        assert rows == [want[rid] for rid in gold['read_ids'] if rid not in skipped]
        assert err.count('Warning: skipping read') == len(skipped)
        assert 'Classifying fast5s: 1 / 1' in err


def test_a_directory_with_both_kinds(fast5_rows, gold, tmp_path, capsys, monkeypatch):
    """a POD5 file beside one-read fast5 files: both listed, every read classified once"""
    import shutil
    set_route(monkeypatch, DEEPBINNER_GPU_INFLATE='1')
    names = sorted(os.listdir(SINGLE))[:3]
    for name in names:
        shutil.copy(os.path.join(SINGLE, name), str(tmp_path / name))
    from deepbinner_amd import load_fast5s
    have = {load_fast5s.get_read_id_and_signal(str(tmp_path / name))[0] for name in names}
    shutil.copy(os.path.join(POD5, 'golden7_uncompressed.pod5'), str(tmp_path / 'all.pod5'))
    _, rows, err = run(['--native', str(tmp_path)], capsys)
    want = fast5_rows[()][1]
    assert '3 fast5 and 1 pod5 files found' in err
    assert sorted(rows) == sorted([want[rid] for rid in have] + [want[rid] for rid in gold['read_ids']])
    assert 'Classifying fast5s: 4 / 4' in err


def test_want_samples_returns_the_golden_signals(hip, hip_models, gold):
    for zstd in ('host', 'gpu'):
        ids, offsets, comp, records = pod5_lite.raw_unit(os.path.join(POD5, 'golden7.pod5'), zstd=zstd)
        assert ids == gold['read_ids']
        assert set(records['mode'].tolist()) == {pod5_lite.RAW_SVB16 if zstd == 'host'
                                                 else pod5_lite.RAW_SVB16_ZSTD}
        calls, status, samples = hip.classify_pair_deflated(
            hip_models[START], hip_models[END], comp, records, offsets, 6144, 0.5, want_samples=True)
        assert not status.any() and len(calls) == 7
        assert np.array_equal(samples, np.concatenate(gold['signals']))
