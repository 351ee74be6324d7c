"""
``deepbinner classify --multi_read`` on the GPU (`-m gpu`): the three routes a container can take
(raw chunks inflated on the device, the loader's packed buffers, per-batch lists) with the shipped
models and a general-path one, VBZ containers with either zstd route, the host's redo of streams
the device refuses, and two containers of 4,000 reads against the oracle's C port.  The anchor is
the reference's own calls on the 30 reads of the golden containers (tests/golden/calls.json).
"""
import os
import struct
import uuid
import zlib

import numpy as np
import pytest

from conftest import GOLD, MODEL_DIR
from deepbinner_amd import hdf5_write

pytestmark = pytest.mark.gpu

MULTI = os.path.join(GOLD, 'fast5', 'multi')
CONTAINERS = sorted(os.path.join(MULTI, name) for name in os.listdir(MULTI))
START, END, RAPID = 'EXP-NBD103_read_starts', 'EXP-NBD103_read_ends', 'SQK-RBK004_read_starts'
ROUTES = {'raw': {'DEEPBINNER_GPU_INFLATE': '1'},
          'packed': {'DEEPBINNER_GPU_INFLATE': '0'},
          'lists': {'DEEPBINNER_FAST5_READER': 'python'}}
MODELS = {'rapid': ['--rapid'],
          'nbd_starts': ['-s', os.path.join(MODEL_DIR, START + '.dbw')],
          'native': ['--native']}
FILTER_WARNING = 'Warning: skipping reads whose signal is compressed with a filter'


def set_route(monkeypatch, route, **more):
    for name in ('DEEPBINNER_GPU_INFLATE', 'DEEPBINNER_HOST_INFLATE_SHARE', 'DEEPBINNER_FAST5_READER',
                 'DEEPBINNER_VBZ_ZSTD', 'DEEPBINNER_DEVICE_ORDINALS'):
        monkeypatch.delenv(name, raising=False)
    for name, value in dict(ROUTES[route], **more).items():
        monkeypatch.setenv(name, value)


def run(argv, capsys, monkeypatch):
    """-> (header, rows, stderr) of one `deepbinner classify ...`"""
    from deepbinner_amd import classify, deepbinner as cli
    monkeypatch.setattr(classify, '_FILTER_WARNING_GIVEN', False)
    capsys.readouterr()
    cli.main(['classify'] + [str(a) for a in argv])
    done = capsys.readouterr()
    lines = done.out.splitlines()
    return lines[0], lines[1:], done.err


def golden(gold, key):
    return dict(zip(gold['multi_read_ids'], gold['calls'][key][len(gold['read_ids']):]))


def golden_final(gold, models, mode='require_either'):
    from oracle import classify_ref
    if models == 'rapid':
        return golden(gold, RAPID + '/start')
    starts = golden(gold, START + '/start')
    if models == 'nbd_starts':
        return starts
    ends = golden(gold, END + '/end')
    return {rid: classify_ref.combine_calls(starts[rid], ends[rid], mode) for rid in starts}


def calls_of(rows):
    return {row.split('\t')[0]: row.split('\t')[1] for row in rows}


def golden_reads():
    from vbz_fixtures import read_all
    return [read for path in CONTAINERS for read in read_all(path)]


@pytest.fixture(scope='module')
def unpacked(tmp_path_factory):
    """the 30 reads of the golden containers as one-read files (the reference's flow)"""
    directory = tmp_path_factory.mktemp('unpacked')
    for read_id, signal in golden_reads():
        hdf5_write.write_single_read_fast5(str(directory / (read_id + '.fast5')), read_id, signal)
    return str(directory)


# ---- routes x models ---------------------------------------------------------------------------
@pytest.mark.parametrize('models', sorted(MODELS))
def test_every_route_prints_the_references_calls(models, hip, gold, unpacked, capsys, monkeypatch):
    """raw, packed and lists: the calls of calls.json; the verbose rows the same strings on all
    three and the strings plain `classify` prints for the same reads as one-read files (the
    sample bytes are the same and a window's result does not depend on batch or stream:
    DESIGN.md section 14)."""
    want = golden_final(gold, models)
    assert sum(call != 'none' for call in want.values()) >= 5
    verbose = {}
    for route in ROUTES:
        set_route(monkeypatch, route)
        header, rows, err = run(MODELS[models] + ['--multi_read', MULTI], capsys, monkeypatch)
        assert header == 'read_ID\tbarcode_call'
        assert len(rows) == 30 and calls_of(rows) == want, route
        assert 'Classifying fast5s: 3 / 3' in err and 'Barcode     Count' in err
        v_header, verbose[route], _ = run(MODELS[models] + ['--verbose', '--multi_read', MULTI],
                                          capsys, monkeypatch)
        assert [r.split('\t')[:2] for r in verbose[route]] == [r.split('\t') for r in rows], route
    assert verbose['raw'] == verbose['packed']
    assert sorted(verbose['raw']) == sorted(verbose['lists'])
    set_route(monkeypatch, 'packed')
    one_header, one_read_files, _ = run(MODELS[models] + ['--verbose', unpacked], capsys,
                                        monkeypatch)
    assert one_header == v_header and sorted(one_read_files) == sorted(verbose['raw'])


@pytest.mark.parametrize('mode', ['require_start', 'require_both'])
def test_the_two_model_rules_on_the_raw_route(mode, hip, gold, capsys, monkeypatch):
    want = golden_final(gold, 'native', mode)
    assert sum(call != 'none' for call in want.values()) >= 5
    set_route(monkeypatch, 'raw')
    _, rows, _ = run(['--native', '--' + mode, '--multi_read', MULTI], capsys, monkeypatch)
    assert len(rows) == 30 and calls_of(rows) == want


@pytest.mark.parametrize('models', ['rapid', 'native'])
def test_raw_route_probabilities_against_the_oracle(models, hip, weights, capsys, monkeypatch):
    """the probabilities of the raw route's verbose rows within the project's 1e-4 of
    oracle.network_ref + classify_ref, after rounding to the two printed decimals"""
    from oracle import classify_ref, network_ref
    set_route(monkeypatch, 'raw')
    _, rows, _ = run(MODELS[models] + ['--verbose', '--multi_read', MULTI], capsys, monkeypatch)
    got = {row.split('\t')[0]: row.split('\t')[2:] for row in rows}
    reads = golden_reads()
    assert len(got) == len(reads) == 30
    sides = [(RAPID, 'start')] if models == 'rapid' else [(START, 'start'), (END, 'end')]
    at, worst = 0, 0.0
    for name, side in sides:
        w = weights[name]
        _, probs = classify_ref.call_batch(
            lambda x: network_ref.forward(w, np.asarray(x, dtype=np.float32), dtype=np.float64),
            [s for _, s in reads], 1024, 6144, 0.5, side)
        for (rid, _), row in zip(reads, np.asarray(probs)):
            printed = [float(v) for v in got[rid][at:at + 13]]
            worst = max(worst, float(np.abs(np.array(printed) - row).max()))
        at += 13 + (1 if len(sides) == 2 else 0)
    print('largest |printed - oracle| = %.5f' % worst)
    assert worst <= 0.01 + 1e-4


def test_two_device_queues_print_the_same_table(hip, gold, capsys, monkeypatch):
    """--devices 2 (both replicas on GPU 0): containers dealt over the devices by
    dispatch_batches, rows in the order of one device"""
    set_route(monkeypatch, 'raw')
    _, one, _ = run(['--native', '--verbose', '--multi_read', MULTI], capsys, monkeypatch)
    for route in ('raw', 'packed'):
        set_route(monkeypatch, route, DEEPBINNER_DEVICE_ORDINALS='0,0')
        _, two, _ = run(['--native', '--verbose', '--devices', '2', '--multi_read', MULTI], capsys,
                        monkeypatch)
        assert two == one, route


def test_one_read_files_beside_containers(hip, gold, tmp_path, capsys, monkeypatch):
    """the seven golden one-read files (old and new layout) and the three containers in one
    directory, by every route: 37 reads, each once, with the reference's calls"""
    single = os.path.join(GOLD, 'fast5', 'single')
    directory = tmp_path / 'mixed'
    directory.mkdir()
    for path in [os.path.join(single, name) for name in os.listdir(single)] + CONTAINERS:
        os.symlink(path, str(directory / os.path.basename(path)))
    want = dict(zip(gold['read_ids'] + gold['multi_read_ids'], gold['calls'][START + '/start']))
    for route in ROUTES:
        set_route(monkeypatch, route)
        _, rows, err = run(MODELS['nbd_starts'] + ['--multi_read', str(directory)], capsys,
                           monkeypatch)
        assert len(rows) == 37 and calls_of(rows) == want, route
        assert 'Classifying fast5s: 10 / 10' in err


# ---- a general-path model ----------------------------------------------------------------------
def test_a_2048_sample_model_through_every_route(hip, tmp_path, capsys, monkeypatch):
    """a model the persistent kernel does not take (L = 2048: the general forward path): the
    calls of the oracle-backed run of the same command"""
    from conftest import OracleModel
    from deepbinner_amd import classify
    from general_fixtures import ENDS, STARTS, geometry, save
    start = save(geometry(2048, 13, name=STARTS), tmp_path / 's.dbw')
    end = save(geometry(2048, 13, name=ENDS), tmp_path / 'e.dbw')
    argv = ['-s', start, '-e', end, '--multi_read', MULTI]
    with monkeypatch.context() as mp:
        mp.setattr(classify, 'build_model', lambda w: OracleModel(w, dtype=np.float64))
        set_route(mp, 'lists')
        _, oracle_rows, _ = run(argv, capsys, mp)
    want = calls_of(oracle_rows)
    assert len(want) == 30 and sum(call != 'none' for call in want.values()) >= 5
    for route in ROUTES:
        set_route(monkeypatch, route)
        _, rows, _ = run(argv, capsys, monkeypatch)
        assert len(rows) == 30 and calls_of(rows) == want, route


# ---- VBZ ---------------------------------------------------------------------------------------
def test_vbz_containers_with_either_zstd_route(hip, tmp_path, capsys, monkeypatch):
    import vbz_fixtures as vf
    if vf.zstd_lib() is None:
        pytest.skip('no libzstd.so.1 on this host')
    directory = tmp_path / 'vbz'
    directory.mkdir()
    for k, path in enumerate(CONTAINERS):
        copy = str(directory / os.path.basename(path))
        vf.write_vbz_copy(vf.read_all(path), copy, vf.VARIANTS[k % len(vf.VARIANTS)], multi=True)
        assert struct.pack('<H', vf.VBZ) in open(copy, 'rb').read()
    set_route(monkeypatch, 'raw')
    _, want, _ = run(['--native', '--verbose', '--multi_read', MULTI], capsys, monkeypatch)
    assert len(want) == 30
    for zstd in ('host', 'gpu'):
        set_route(monkeypatch, 'raw', DEEPBINNER_VBZ_ZSTD=zstd)
        _, rows, err = run(['--native', '--verbose', '--multi_read', str(directory)], capsys,
                           monkeypatch)
        assert rows == want, zstd
        assert FILTER_WARNING not in err


# ---- the host's redo ---------------------------------------------------------------------------
def squiggle(rng, n):
    levels = np.repeat(rng.normal(450, 80, n // 8 + 1), 8)[:n]
    return np.clip(np.rint(levels + rng.normal(0, 8, n)), 0, 2047).astype(np.int16)


def test_a_stream_the_device_and_the_host_refuse(hip, gold, tmp_path, capsys, monkeypatch):
    """a container with one deflate stream whose first block header names the reserved block
    type 3 (tests/test_inflate.py, damaged_cases): the device decoder refuses it (a status, not a
    fault), zlib on the host refuses it too - that read has no row, its neighbours have the rows
    of the intact container, on the raw and on the packed route.  (Not a byte flipped among the
    literals: the device decodes the samples it was asked for and checks the Adler-32 only of a
    stream it saw the end of, so such a read gets a row on the raw route: DESIGN.md section
    15.)"""
    reads = golden_reads()[:12]
    victim = reads[5][0]
    items = []
    for read_id, signal in reads:
        stream = bytearray(zlib.compress(signal.tobytes(), 1))
        if read_id == victim:
            stream[2] = 0x07                        # BFINAL = 1, BTYPE = 3
            with pytest.raises(zlib.error):
                zlib.decompress(bytes(stream))
        items.append((read_id, signal, None, bytes(stream)))
    intact, damaged = tmp_path / 'intact.fast5', tmp_path / 'damaged.fast5'
    intact.write_bytes(hdf5_write.multi_read_fast5_bytes([(rid, s) for rid, s in reads]))
    damaged.write_bytes(hdf5_write.multi_read_fast5_bytes(items))
    want = golden_final(gold, 'native')
    for verbose in ([], ['--verbose']):
        set_route(monkeypatch, 'raw')
        _, whole, _ = run(['--native'] + verbose + ['--multi_read', intact], capsys, monkeypatch)
        assert len(whole) == 12 and calls_of(whole) == {rid: want[rid] for rid, _ in reads}
        for route in ('raw', 'packed'):
            set_route(monkeypatch, route)
            _, rows, _ = run(['--native'] + verbose + ['--multi_read', damaged], capsys,
                             monkeypatch)
            assert rows == [row for row in whole if row.split('\t')[0] != victim], route


def test_a_vbz_stream_only_the_self_checks_refuse(hip, tmp_path, capsys, monkeypatch):
    """a VBZ read whose streamvbyte bytes are a refused mutant inside an intact zstd frame: the
    device refuses the stream (a status, not a fault), the host's decoder refuses the read - no
    row, the filter warning once - and its neighbours have the rows of their deflate twins"""
    import vbz_fixtures as vf
    import vbz_reference as ref
    if vf.zstd_lib() is None:
        pytest.skip('no libzstd.so.1 on this host')
    rng = np.random.default_rng(13)

    def damaged(s):
        good = struct.pack('<I', 2 * len(s)) + vf.streamvbyte(s)
        mutant = bytearray(good)
        i = len(s) // 3
        ref.set_code(mutant, i, int(ref.code_lengths(good)[i]) % 4)
        assert len(mutant) == len(good) and ref.decode(bytes(mutant)) is None
        return bytes(mutant[:4]) + vf.zstd_compress(bytes(mutant[4:]))

    reads = [(str(uuid.UUID(bytes=rng.bytes(16), version=4)), squiggle(rng, int(rng.integers(3000, 9000))))
             for _ in range(8)]
    victim = reads[2][0]
    filters = [vf.signal_filter(s, encode=damaged if rid == victim else None) for rid, s in reads]
    vbz, twin = tmp_path / 'vbz.fast5', tmp_path / 'twin.fast5'
    vbz.write_bytes(hdf5_write.multi_read_fast5_bytes(
        [(rid, s, None, None, sf) for (rid, s), sf in zip(reads, filters)]))
    twin.write_bytes(hdf5_write.multi_read_fast5_bytes(reads))
    set_route(monkeypatch, 'raw')
    _, want, err = run(['--native', '--verbose', '--multi_read', twin], capsys, monkeypatch)
    assert len(want) == 8 and FILTER_WARNING not in err
    want = [row for row in want if row.split('\t')[0] != victim]
    for route, zstd in (('raw', 'host'), ('raw', 'gpu'), ('packed', 'host')):
        set_route(monkeypatch, route, DEEPBINNER_VBZ_ZSTD=zstd)
        _, rows, err = run(['--native', '--verbose', '--multi_read', vbz], capsys, monkeypatch)
        assert rows == want, (route, zstd)
        assert err.count(FILTER_WARNING) == 1, (route, zstd, err)


# ---- scale -------------------------------------------------------------------------------------
READS_PER_CONTAINER = 4000


def build_containers(directory, gold, n_containers):
    """containers of 4,000 synthetic reads (2,000 distinct seeded squiggles of 2,000-9,000
    samples, deflated once each, under fresh read ids) with the 30 golden reads dealt over them
    -> (paths, [(read id, signal)] in table order)"""
    from concurrent.futures import ThreadPoolExecutor
    rng = np.random.default_rng(20261017)
    pool = [squiggle(rng, int(rng.integers(2000, 9000))) for _ in range(2000)]
    with ThreadPoolExecutor(16) as workers:
        deflated = list(workers.map(lambda s: zlib.compress(s.tobytes(), 1), pool))
    fixture = list(zip(gold['multi_read_ids'], gold['multi_signals']))
    jobs, every_read = [], []
    for c in range(n_containers):
        reads = []
        for _ in range(READS_PER_CONTAINER):
            j = int(rng.integers(0, len(pool)))
            reads.append((str(uuid.UUID(bytes=rng.bytes(16), version=4)), pool[j], None,
                          deflated[j]))
        reads += fixture[c::n_containers]
        every_read += [(r[0], r[1]) for r in reads]
        jobs.append((os.path.join(directory, 'scale_%02d.fast5' % c), reads))

    def write(job):
        with open(job[0], 'wb') as f:
            f.write(hdf5_write.multi_read_fast5_bytes(job[1]))

    with ThreadPoolExecutor(4) as workers:
        list(workers.map(write, jobs))
    return [job[0] for job in jobs], every_read


def test_two_containers_of_4000_reads_against_the_oracle(hip, gold, weights, tmp_path, capsys,
                                                         monkeypatch):
    """`classify --native --multi_read` on the raw route over 8,030 reads: every read tabulated
    once, the golden reads with their golden calls, and every call what the oracle's C port
    (oracle.dbref) and the reference's combine_calls make of the same signals - no read left out"""
    from oracle import classify_ref, dbref
    paths, reads = build_containers(str(tmp_path), gold, 2)
    ids = [rid for rid, _ in reads]
    assert len(ids) == len(set(ids)) == 2 * READS_PER_CONTAINER + 30
    set_route(monkeypatch, 'raw')
    _, rows, err = run(['--native', '--multi_read', str(tmp_path)], capsys, monkeypatch)
    got = calls_of(rows)
    assert len(rows) == len(ids) and sorted(got) == sorted(ids)
    assert 'Classifying fast5s: 2 / 2' in err
    want = golden_final(gold, 'native')
    assert all(got[rid] == want[rid] for rid in gold['multi_read_ids'])
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for _, s in reads])
    samples = np.concatenate([s for _, s in reads]).astype(np.int16)
    side_calls = {}
    for side, name in (('start', START), ('end', END)):
        side_calls[side] = dbref.CModel(weights[name]).classify(samples, offsets, side, 6144, 0.5)[1]
    as_name = lambda c: 'none' if c == 0 else str(int(c))                # noqa: E731
    differ = [rid for rid, a, b in zip(ids, side_calls['start'], side_calls['end'])
              if got[rid] != classify_ref.combine_calls(as_name(a), as_name(b), 'require_either')]
    print('%d reads, %d called, %d differ from the oracle' % (
        len(ids), sum(call != 'none' for call in got.values()), len(differ)))
    assert not differ, '%d of %d rows differ from the oracle' % (len(differ), len(ids))
