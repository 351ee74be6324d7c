"""
``deepbinner classify --multi_read`` on the CPU: multi-read containers classified where they are,
with the model replaced by the oracle-backed double at seam b1 (conftest.oracle_backend).  The
anchor is the reference's own ``call_batch`` on the 30 reads of the golden containers
(tests/golden/calls.json); everything else is equality with what the reference's flow - unpack
into one-read files, then classify - prints.
"""
import argparse
import io
import os
import re
import shutil
import subprocess
import sys
import zlib

import pytest

from conftest import GOLD, MODEL_DIR, REPO
import deepbinner_amd.classify as classify
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import fast5_native, hdf5_write

MULTI = os.path.join(GOLD, 'fast5', 'multi')
SINGLE = os.path.join(GOLD, 'fast5', 'single')
CONTAINERS = sorted(os.path.join(MULTI, name) for name in os.listdir(MULTI))
NBD_START = os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw')
READERS = ['python', 'native']


def use_reader(monkeypatch, reader):
    if reader == 'native' and not fast5_native.available():
        pytest.skip('libdeepbinner_fast5.so is not built')
    monkeypatch.setenv('DEEPBINNER_FAST5_READER', reader)
    monkeypatch.delenv('DEEPBINNER_GPU_INFLATE', raising=False)
    monkeypatch.delenv('DEEPBINNER_HOST_INFLATE_SHARE', raising=False)


def run(argv, capsys):
    """-> (header, rows, stderr) of one `deepbinner classify ...`"""
    capsys.readouterr()
    cli.main(['classify'] + [str(a) for a in argv])
    done = capsys.readouterr()
    lines = done.out.splitlines()
    return lines[0], lines[1:], done.err


def last_progress(err):
    return re.findall(r'Classifying fast5s: (\d+) / (\d+)', err)[-1]


def golden(gold, key):
    """{read id: the reference's call} for the 30 reads of the golden containers"""
    return dict(zip(gold['multi_read_ids'], gold['calls'][key][len(gold['read_ids']):]))


def calls_of(rows):
    return {row.split('\t')[0]: row.split('\t')[1] for row in rows}


# ---- golden calls ------------------------------------------------------------------------------
@pytest.mark.parametrize('reader', READERS)
def test_rapid_table_is_the_references_calls(reader, oracle_backend, gold, capsys, monkeypatch):
    use_reader(monkeypatch, reader)
    header, rows, err = run(['--rapid', '--multi_read', MULTI], capsys)
    want = golden(gold, 'SQK-RBK004_read_starts/start')
    assert header + '\n' == gold['calls']['headers']['010']
    assert len(rows) == 30 and calls_of(rows) == want
    assert sum(call != 'none' for call in want.values()) == 6
    assert last_progress(err) == ('3', '3') and 'Barcode     Count' in err


def test_rows_follow_the_file_list_and_the_containers(oracle_backend, gold, capsys, monkeypatch):
    """containers in the order of the file list, reads in container order; the maps returned are
    the calls and the container each read came from"""
    use_reader(monkeypatch, 'python')
    order = [CONTAINERS[2], CONTAINERS[0], CONTAINERS[1]]
    models = classify.load_and_check_models(NBD_START, None, 6144, out_dest=io.StringIO())
    args = argparse.Namespace(verbose=False, batch_size=4, scan_size=6144, score_diff=0.5,
                              require_either=False, require_start=False, require_both=False,
                              multi_read=True)
    capsys.readouterr()
    calls, files = classify.classify_fast5_files(order, *models[:5], args)
    rows = capsys.readouterr().out.splitlines()[1:]
    from vbz_fixtures import read_all
    from deepbinner_amd import load_fast5s
    want_ids, want_files = [], {}
    for path in order:
        ids = [rid for rid, _ in load_fast5s._python_iter_reads(path)]
        assert sorted(ids) == sorted(rid for rid, _ in read_all(path))
        want_ids += ids
        want_files.update(dict.fromkeys(ids, path))
    assert [row.split('\t')[0] for row in rows] == want_ids
    assert calls == golden(gold, 'EXP-NBD103_read_starts/start') and files == want_files


def test_nbd103_start_model_calls_19_barcodes(oracle_backend, gold, capsys, monkeypatch):
    use_reader(monkeypatch, 'python')
    _, rows, _ = run(['-s', NBD_START, '--multi_read', MULTI], capsys)
    want = golden(gold, 'EXP-NBD103_read_starts/start')
    assert len(rows) == 30 and calls_of(rows) == want
    assert sum(call != 'none' for call in want.values()) == 19


@pytest.mark.parametrize('mode', ['require_either', 'require_start', 'require_both'])
def test_native_preset_under_each_two_model_rule(mode, oracle_backend, gold, capsys, monkeypatch):
    use_reader(monkeypatch, 'python')
    _, rows, _ = run(['--native', '--' + mode, '--multi_read', MULTI], capsys)
    rule = argparse.Namespace(require_either=False, require_start=False, require_both=False)
    setattr(rule, mode, True)
    starts = golden(gold, 'EXP-NBD103_read_starts/start')
    ends = golden(gold, 'EXP-NBD103_read_ends/end')
    want = {rid: classify.combine_calls(starts[rid], ends[rid], rule) for rid in starts}
    assert sum(call != 'none' for call in want.values()) >= 5
    assert len(rows) == 30 and calls_of(rows) == want


# ---- the reference's flow: unpack, then classify -------------------------------------------------
@pytest.fixture(scope='module')
def unpacked(tmp_path_factory):
    """the 30 reads of the golden containers as one-read files"""
    from vbz_fixtures import read_all
    directory = tmp_path_factory.mktemp('unpacked')
    for path in CONTAINERS:
        for read_id, signal in read_all(path):
            hdf5_write.write_single_read_fast5(str(directory / (read_id + '.fast5')), read_id,
                                               signal)
    assert len(os.listdir(str(directory))) == 30
    return str(directory)


@pytest.mark.parametrize('reader', READERS)
@pytest.mark.parametrize('models', [['--rapid'], ['--native']])
@pytest.mark.parametrize('verbose', [[], ['--verbose']])
def test_same_rows_as_unpacking_first(reader, models, verbose, unpacked, oracle_backend, capsys,
                                      monkeypatch):
    use_reader(monkeypatch, reader)
    want_header, want, _ = run(models + verbose + [unpacked], capsys)
    header, rows, _ = run(models + verbose + ['--multi_read', MULTI], capsys)
    assert header == want_header and len(rows) == 30
    assert sorted(rows) == sorted(want)
    if verbose:
        assert len(rows[0].split('\t')) == (2 + 13 if models == ['--rapid'] else 2 + 2 * 14)


# ---- one-read files and containers in one directory --------------------------------------------
def mixed_directory(tmp_path, containers=CONTAINERS):
    directory = tmp_path / 'mixed'
    directory.mkdir()
    for path in [os.path.join(SINGLE, name) for name in sorted(os.listdir(SINGLE))] + containers:
        os.symlink(path, str(directory / os.path.basename(path)))
    return str(directory)


def check_mixed(gold, rows, err, n_containers):
    ids = gold['read_ids'] + gold['multi_read_ids']
    want = dict(zip(ids, gold['calls']['SQK-RBK004_read_starts/start']))
    if n_containers == 1:
        from vbz_fixtures import read_all
        keep = set(gold['read_ids']) | {rid for rid, _ in read_all(CONTAINERS[0])}
        want = {rid: call for rid, call in want.items() if rid in keep}
    assert len(rows) == len(want) and calls_of(rows) == want
    assert last_progress(err) == (str(7 + n_containers),) * 2
    shown = [int(done) for done, _ in re.findall(r'Classifying fast5s: (\d+) / (\d+)', err)]
    assert shown == sorted(shown) and shown[0] == 0


@pytest.mark.parametrize('reader', READERS)
def test_one_read_files_beside_containers(reader, oracle_backend, gold, tmp_path, capsys,
                                          monkeypatch):
    """old-format one-read files, a new-format one and three containers: 37 reads, each once
    (without the flag the reference refuses such a directory one way or the other)"""
    use_reader(monkeypatch, reader)
    _, rows, err = run(['--rapid', '--multi_read', mixed_directory(tmp_path)], capsys)
    check_mixed(gold, rows, err, 3)


@pytest.mark.parametrize('reader', READERS)
@pytest.mark.parametrize('kind', ['single', 'multi'])
def test_a_container_among_one_read_files(kind, reader, oracle_backend, gold, tmp_path, capsys,
                                          monkeypatch):
    """seven one-read files and one container, by both routes the five sampled files may pick:
    'single' - the one-read batch paths, which set the container aside and classify it last -
    and 'multi' - every file as a container"""
    use_reader(monkeypatch, reader)
    monkeypatch.setattr(classify, 'determine_single_or_multi_fast5s', lambda files, **kw: kind)
    directory = mixed_directory(tmp_path, CONTAINERS[:1])
    _, rows, err = run(['--rapid', '--multi_read', '--batch_size', '3', directory], capsys)
    check_mixed(gold, rows, err, 1)
    if kind == 'single':        # the container's reads come last
        assert {row.split('\t')[0] for row in rows[:7]} == set(gold['read_ids'])


@pytest.mark.parametrize('reader', READERS)
def test_one_container_as_the_input(reader, oracle_backend, gold, capsys, monkeypatch):
    use_reader(monkeypatch, reader)
    from vbz_fixtures import read_all
    _, rows, err = run(['--rapid', '--multi_read', CONTAINERS[1]], capsys)
    want = golden(gold, 'SQK-RBK004_read_starts/start')
    ids = [rid for rid, _ in read_all(CONTAINERS[1])]
    assert len(rows) == len(ids) and calls_of(rows) == {rid: want[rid] for rid in ids}
    assert last_progress(err) == ('1', '1')


# ---- damage ------------------------------------------------------------------------------------
@pytest.mark.parametrize('reader', READERS)
def test_a_container_cut_in_half_costs_only_its_own_reads(reader, oracle_backend, gold, tmp_path,
                                                          capsys, monkeypatch):
    use_reader(monkeypatch, reader)
    from vbz_fixtures import read_all
    directory = tmp_path / 'cut'
    directory.mkdir()
    for path in CONTAINERS[:2]:
        shutil.copy(path, str(directory))
    data = open(CONTAINERS[2], 'rb').read()
    (directory / 'cut.fast5').write_bytes(data[:len(data) // 2])
    _, rows, err = run(['--rapid', '--multi_read', str(directory)], capsys)     # no exit, no raise
    want = golden(gold, 'SQK-RBK004_read_starts/start')
    good = [rid for path in CONTAINERS[:2] for rid, _ in read_all(path)]
    got = calls_of(rows)
    assert len(good) >= 18 and len(got) == len(rows)
    assert set(good) <= set(got) <= set(want)
    assert all(got[rid] == want[rid] for rid in got)
    assert last_progress(err) == ('3', '3') and 'Barcode     Count' in err


@pytest.mark.parametrize('reader', READERS)
def test_a_read_with_a_damaged_deflate_stream_is_dropped(reader, oracle_backend, gold, tmp_path,
                                                         capsys, monkeypatch):
    use_reader(monkeypatch, reader)
    from vbz_fixtures import read_all
    reads = read_all(CONTAINERS[0])
    victim = reads[len(reads) // 2][0]
    items = []
    for read_id, signal in reads:
        stream = bytearray(zlib.compress(signal.tobytes(), 1))
        if read_id == victim:
            stream[len(stream) // 2] ^= 0x5A
            with pytest.raises(zlib.error):
                zlib.decompress(bytes(stream))
        items.append((read_id, signal, None, bytes(stream)))
    path = tmp_path / 'damaged.fast5'
    path.write_bytes(hdf5_write.multi_read_fast5_bytes(items))
    _, rows, _ = run(['--rapid', '--multi_read', str(path)], capsys)
    want = golden(gold, 'SQK-RBK004_read_starts/start')
    assert calls_of(rows) == {rid: want[rid] for rid, _ in reads if rid != victim}
    assert len(rows) == len(reads) - 1


@pytest.mark.parametrize('reader', READERS)
def test_realtime_on_the_lists_route_still_ends_a_container_at_a_damaged_read(
        reader, oracle_backend, tmp_path, capsys, monkeypatch):
    """the units are shared, what `realtime` does is not changed by them: on the lists route its
    walk of a container ends at the first read it cannot read, as before `--multi_read`, while
    `classify --multi_read` goes on behind it (the test above)"""
    import deepbinner_amd.realtime as realtime
    from deepbinner_amd import load_fast5s
    use_reader(monkeypatch, reader)
    monkeypatch.setattr(realtime, 'POLL_SECONDS', 0)
    monkeypatch.setattr(shutil, 'which', lambda tool: None)
    monkeypatch.setenv('DEEPBINNER_REALTIME_TABLE_ONLY', '1')
    in_dir = tmp_path / 'in'
    in_dir.mkdir()
    order = [rid for rid, _ in load_fast5s.iter_reads(CONTAINERS[0])]
    signals = dict(load_fast5s.iter_reads(CONTAINERS[0]))
    victim = order[len(order) // 2]
    items = []
    for read_id in order:
        stream = bytearray(zlib.compress(signals[read_id].tobytes(), 1))
        if read_id == victim:
            stream[len(stream) // 2] ^= 0x5A
        items.append((read_id, signals[read_id], None, bytes(stream)))
    (in_dir / 'damaged.fast5').write_bytes(hdf5_write.multi_read_fast5_bytes(items))
    walked = [rid for rid, _ in load_fast5s.iter_reads(str(in_dir / 'damaged.fast5'))]
    assert 0 < len(walked) < len(order) - 1 and victim not in walked
    out_dir = tmp_path / 'out'
    cli.main(['realtime', '--in_dir', str(in_dir), '--out_dir', str(out_dir), '--stop', '--rapid'])
    capsys.readouterr()
    table = [line.split('\t')[0] for line in
             (out_dir / 'multi_read_classifications.tsv').read_text().splitlines()]
    assert table == walked


# ---- VBZ ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('reader', READERS)
@pytest.mark.parametrize('verbose', [[], ['--verbose']])
def test_vbz_containers_give_the_rows_of_the_deflate_originals(reader, verbose, oracle_backend,
                                                               tmp_path, capsys, monkeypatch):
    import vbz_fixtures as vf
    if vf.zstd_lib() is None:
        pytest.skip('no libzstd.so.1 on this host')
    use_reader(monkeypatch, reader)
    directory = tmp_path / 'vbz'
    directory.mkdir()
    for k, path in enumerate(CONTAINERS):
        vf.write_vbz_copy(vf.read_all(path), str(directory / os.path.basename(path)),
                          vf.VARIANTS[k % len(vf.VARIANTS)], multi=True)
        assert __import__('struct').pack('<H', vf.VBZ) in open(str(directory / os.path.basename(path)), 'rb').read()
    want_header, want, _ = run(['--native'] + verbose + ['--multi_read', MULTI], capsys)
    header, rows, err = run(['--native'] + verbose + ['--multi_read', str(directory)], capsys)
    assert header == want_header and len(rows) == 30 and sorted(rows) == sorted(want)
    assert 'Warning: skipping reads' not in err


# ---- off by default ----------------------------------------------------------------------------
def test_without_the_flag_containers_are_still_refused(oracle_backend, capsys):
    """(the one test of this file that the code before the flag passes too: it pins what stays)"""
    with pytest.raises(SystemExit) as e:
        cli.main(['classify', '--rapid', MULTI])
    assert 'requires one-read-per-file fast5s' in str(e.value)
    models = classify.load_and_check_models(NBD_START, None, 6144, out_dest=io.StringIO())
    args = argparse.Namespace(verbose=False, batch_size=128, scan_size=6144, score_diff=0.5,
                              require_either=False, require_start=False, require_both=False)
    assert not hasattr(args, 'multi_read')
    with pytest.raises(SystemExit) as e:
        classify.classify_fast5_files(CONTAINERS, *models[:5], args)
    assert 'requires one-read-per-file fast5s' in str(e.value)


def test_the_flag_belongs_to_classify_alone(capsys):
    """`classify` parses it (default off), `realtime` - which takes containers anyway - does not"""
    parser = cli.build_parser()
    assert parser.parse_args(['classify', '--rapid', 'x']).multi_read is False
    assert parser.parse_args(['classify', '--rapid', '--multi_read', 'x']).multi_read is True
    assert 'multi_read' not in vars(parser.parse_args(['realtime', '--in_dir', 'a',
                                                       '--out_dir', 'b']))
    with pytest.raises(SystemExit):
        parser.parse_args(['realtime', '--in_dir', 'a', '--out_dir', 'b', '--multi_read'])


# ---- one process per GPU, on the CPU -----------------------------------------------------------
RANK_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import deepbinner_amd.classify as classify
from deepbinner_amd import deepbinner as cli
from conftest import OracleModel
classify.build_model = lambda w: OracleModel(w)      # CPU box: oracle-backed model double
classify.set_tensorflow_threads = lambda args: None  # ... and no GPU to select
cli.main(['classify', '--native', '--verbose', '--multi_read', '--batch_size', '4',
          os.environ['CLASSIFY_TARGET']])
'''


def run_ranks(script, world, target, reader):
    import uuid
    name = 'deepbinner-test-' + uuid.uuid4().hex
    procs = []
    for rank in range(world):
        env = dict(os.environ, PYTHONPATH=REPO, OMP_NUM_THREADS='2', RANK=str(rank),
                   LOCAL_RANK=str(rank), WORLD_SIZE=str(world), DEEPBINNER_RDZV=name,
                   DEEPBINNER_RDZV_TIMEOUT='300', DEEPBINNER_COMM='host',
                   DEEPBINNER_FAST5_READER=reader, CLASSIFY_TARGET=target)
        procs.append(subprocess.Popen([sys.executable, str(script), REPO], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    return [(p.returncode, o, e) for p, (o, e) in zip(procs, outs)]


@pytest.mark.parametrize('n_containers', [3, 1])
def test_two_ranks_print_the_single_process_table(n_containers, tmp_path):
    """the file list sharded over two ranks (with one container, rank 1's shard is empty and it
    still takes part in every collective): the ranks' rows, in rank order, are the rows of one
    process, and rank 0 prints the summary of all of them"""
    reader = 'native' if fast5_native.available() else 'python'
    script = tmp_path / 'rank_worker.py'
    script.write_text(RANK_WORKER)
    target = tmp_path / 'containers'
    target.mkdir()
    for path in CONTAINERS[:n_containers]:
        os.symlink(path, str(target / os.path.basename(path)))
    (single,) = run_ranks(script, 1, str(target), reader)
    assert single[0] == 0, single[2][-3000:]
    want = single[1].splitlines()
    results = run_ranks(script, 2, str(target), reader)
    for rc, out, err in results:
        assert rc == 0, out[-2000:] + err[-3000:]
    rows = results[0][1].splitlines() + results[1][1].splitlines()
    assert rows[0] == want[0] and rows[0].startswith('read_ID\tbarcode_call\tstart_none')
    assert sorted(rows[1:]) == sorted(want[1:]) and len(rows) == len(want)
    assert len(rows) == 1 + (30 if n_containers == 3 else len(want) - 1) and len(want) > 5
    if n_containers == 1:
        assert results[1][1] == ''
    # rows come out in sorted-file order = rank order: the single-process table of a sorted list
    from deepbinner_amd import load_fast5s
    walk = fast5_native.iter_reads if reader == 'native' else load_fast5s._python_iter_reads
    by_file = []
    for path in sorted(str(target / os.path.basename(p)) for p in CONTAINERS[:n_containers]):
        by_file += [rid for rid, _ in walk(path)]       # (the reader's own order of a container)
    assert [row.split('\t')[0] for row in rows[1:]] == by_file
    err = results[0][2]
    assert 'Barcode     Count' in err and 'Barcode     Count' not in results[1][2]
    counts = re.findall(r'^\s*(\d+|none)\s+(\d+)\s*$', err.split('Barcode     Count')[1], re.M)
    assert sum(int(n) for _, n in counts) == len(rows) - 1
    assert last_progress(err) == (str(n_containers),) * 2
    assert all(int(a) <= int(b) for a, b in re.findall(r'Classifying fast5s: (\d+) / (\d+)', err))
