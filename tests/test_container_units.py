"""
The container units of deepbinner_amd/containers.py on the CPU, on all three routes: the device
is replaced by a stand-in with the device library's Python surface - models with ``handle``,
``classify_packed``, ``clone`` and ``reserve_cus`` backed by the oracle's C port (oracle.dbref),
and ``hip_backend.classify_pair`` / ``classify_pair_deflated`` emulated with zlib on the host - so
that the route choice, the inflate queues, the row formatting of the raw route and the host's
redo of a refused stream run without a GPU, for ``classify --multi_read`` and for ``realtime``.
(What the device computes is the business of tests/test_gpu_classify_multi_read.py.)
"""
import os
import shutil
import zlib

import numpy as np
import pytest

from conftest import GOLD, MODEL_DIR
import deepbinner_amd.classify as classify
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import fast5_native, hdf5_write, hip_backend

MULTI = os.path.join(GOLD, 'fast5', 'multi')
CONTAINERS = sorted(os.path.join(MULTI, name) for name in os.listdir(MULTI))
START, END = 'EXP-NBD103_read_starts', 'EXP-NBD103_read_ends'

pytestmark = pytest.mark.skipif(not fast5_native.available(),
                                reason='libdeepbinner_fast5.so is not built')


class StandInModel:
    """The Python surface of hip_backend.HipModel the classify path uses, on the oracle's C port"""
    device = 0
    clones = []             # every model a clone() made (the raw route's extra queues)

    def __init__(self, weights):
        from oracle import dbref
        self.weights = weights
        self.oracle = dbref.CModel(weights)
        self.n_classes, self.input_size = weights.n_classes, weights.input_size
        self.inputs = [hip_backend._TensorSpec((None, weights.input_size, 1))]
        self.outputs = [hip_backend._TensorSpec((None, weights.n_classes))]
        self.handle = object()
        self.reserved = []

    def classify_packed(self, samples, offsets, side, scan_size, score_diff):
        if len(offsets) < 2:
            return np.zeros((0, self.n_classes), np.float32), np.zeros(0, np.int32)
        return self.oracle.classify(samples, offsets, side, int(scan_size), score_diff)

    def classify_signals(self, signals, side, scan_size, score_diff):
        offsets = np.zeros(len(signals) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(s) for s in signals])
        samples = (np.concatenate(signals) if offsets[-1] else np.zeros(0)).astype(np.int16)
        return self.classify_packed(samples, offsets, side, scan_size, score_diff)

    def predict(self, x, batch_size=None):
        return self.oracle.predict(x)

    def clone(self):
        twin = StandInModel(self.weights)
        self.clones.append(twin)
        return twin

    def reserve_cus(self, n_cus=0):
        self.reserved.append(n_cus)

    def close(self):
        self.handle = None


def pair(start, end, samples, offsets, scan_size, score_diff, mode):
    rule = {'require_either': dict(require_either=True, require_start=False, require_both=False),
            'require_start': dict(require_either=False, require_start=True, require_both=False),
            'require_both': dict(require_either=False, require_start=False, require_both=True)}
    import argparse
    sides = {}
    for side, model in (('start', start), ('end', end)):
        if model is not None:
            sides[side] = model.classify_packed(samples, offsets, side, scan_size, score_diff)
    if len(sides) == 2:
        calls = classify.combine_call_numbers(sides['start'][1], sides['end'][1],
                                              argparse.Namespace(**rule[mode]))
    else:
        calls = next(iter(sides.values()))[1]
    return np.asarray(calls, dtype=np.int32), sides


def classify_pair(start, end, samples, offsets, scan_size, score_diff, mode='require_either',
                  want_sides=False, want_probs=False):
    assert not want_sides and not want_probs
    return pair(start, end, samples, offsets, scan_size, score_diff, mode)[0]


def classify_pair_deflated(start, end, comp, streams, offsets, scan_size, score_diff,
                           mode='require_either', want_samples=False, want_stages=False,
                           want_sides=False):
    """hip_backend.classify_pair_deflated with zlib on the host for the device's decoder.  As on
    the device, a stream is decoded up to the bytes asked for: one that cannot give them gets
    status 1 and zeros, and the Adler-32 behind a stream is not looked at"""
    assert not want_stages
    samples = np.zeros(int(offsets[-1]), dtype=np.int16)
    raw = samples.view(np.uint8)
    status = np.zeros(len(streams), dtype=np.int32)
    for k, rec in enumerate(streams):
        chunk = bytes(comp[int(rec['comp_offset']):int(rec['comp_offset'] + rec['comp_bytes'])])
        assert rec['mode'] in (0, 1)
        try:
            data = (zlib.decompressobj().decompress(chunk, int(rec['out_bytes']))
                    if rec['mode'] == 0 else chunk)
            if len(data) < rec['out_bytes']:
                raise zlib.error('stream ends early')
            raw[int(rec['out_offset']):int(rec['out_offset'] + rec['out_bytes'])] = \
                np.frombuffer(data[:int(rec['out_bytes'])], dtype=np.uint8)
        except zlib.error:
            status[k] = 1
    calls, sides = pair(start, end, samples, offsets, scan_size, score_diff, mode)
    out = [calls, status]
    if want_samples:
        out.append(samples)
    if want_sides:
        out.append({'start_calls': sides['start'][1] if 'start' in sides else None,
                    'end_calls': sides['end'][1] if 'end' in sides else None,
                    'start_probs': sides['start'][0] if 'start' in sides else None,
                    'end_probs': sides['end'][0] if 'end' in sides else None})
    return tuple(out)


@pytest.fixture()
def stand_in(monkeypatch):
    made = []
    monkeypatch.setattr(StandInModel, 'clones', [])

    def build(weights):
        made.append(StandInModel(weights))
        return made[-1]
    monkeypatch.setattr(classify, 'build_model', build)
    monkeypatch.setattr(classify, 'set_tensorflow_threads', lambda args: None)
    monkeypatch.setattr(hip_backend, 'classify_pair', classify_pair)
    monkeypatch.setattr(hip_backend, 'classify_pair_deflated', classify_pair_deflated)
    for name in ('DEEPBINNER_HOST_INFLATE_SHARE', 'DEEPBINNER_INFLATE_QUEUES',
                 'DEEPBINNER_INFLATE_CUS', 'DEEPBINNER_VBZ_ZSTD'):
        monkeypatch.delenv(name, raising=False)
    return made


ROUTES = {'raw': {'DEEPBINNER_FAST5_READER': 'native', 'DEEPBINNER_GPU_INFLATE': '1'},
          'packed': {'DEEPBINNER_FAST5_READER': 'native', 'DEEPBINNER_GPU_INFLATE': '0'},
          'lists': {'DEEPBINNER_FAST5_READER': 'python', 'DEEPBINNER_GPU_INFLATE': '0'}}


def run(route, argv, capsys, monkeypatch):
    for name, value in ROUTES[route].items():
        monkeypatch.setenv(name, value)
    capsys.readouterr()
    cli.main(['classify'] + [str(a) for a in argv])
    done = capsys.readouterr()
    lines = done.out.splitlines()
    return lines[0], lines[1:], done.err


@pytest.mark.parametrize('models', [['--native'], ['--rapid'], ['--native', '--require_both']])
@pytest.mark.parametrize('verbose', [[], ['--verbose']])
def test_the_three_routes_print_the_same_rows(models, verbose, stand_in, gold, capsys,
                                              monkeypatch):
    tables = {route: run(route, models + verbose + ['--multi_read', MULTI], capsys, monkeypatch)
              for route in ROUTES}
    header, rows, err = tables['raw']
    assert len(rows) == 30 and 'Classifying fast5s: 3 / 3' in err
    assert tables['packed'][:2] == (header, rows)
    assert tables['lists'][0] == header and sorted(tables['lists'][1]) == sorted(rows)
    if '--rapid' in models and not verbose:
        want = dict(zip(gold['multi_read_ids'], gold['calls']['SQK-RBK004_read_starts/start'][7:]))
        assert {r.split('\t')[0]: r.split('\t')[1] for r in rows} == want


def test_the_queues_of_the_raw_route_get_their_cus_back(stand_in, capsys, monkeypatch):
    run('raw', ['--native', '--multi_read', MULTI], capsys, monkeypatch)
    queue_models = stand_in + StandInModel.clones
    assert len(stand_in) == 2 and len(queue_models) == 6    # three (start, end) pairs on the device
    assert all(m.reserved for m in queue_models)
    assert all(m.reserved[-1] == 0 for m in queue_models)


@pytest.mark.parametrize('verbose', [[], ['--verbose']])
def test_a_stream_both_decoders_refuse_costs_one_row(verbose, stand_in, tmp_path, capsys,
                                                     monkeypatch):
    """a read whose deflate stream is damaged: the stand-in decoder refuses the stream, the
    host's redo refuses the read - no row; its neighbours' rows are those of the intact file"""
    from vbz_fixtures import read_all
    reads = read_all(CONTAINERS[0])
    victim = reads[4][0]
    items = []
    for read_id, signal in reads:
        stream = bytearray(zlib.compress(signal.tobytes(), 1))
        if read_id == victim:
            stream[2] = 0x07                        # BFINAL = 1, BTYPE = 3: the reserved type
        items.append((read_id, signal, None, bytes(stream)))
    damaged = tmp_path / 'damaged.fast5'
    damaged.write_bytes(hdf5_write.multi_read_fast5_bytes(items))
    _, whole, _ = run('raw', ['--native'] + verbose + ['--multi_read', CONTAINERS[0]], capsys,
                      monkeypatch)
    want = [row for row in whole if row.split('\t')[0] != victim]
    assert len(want) == len(reads) - 1
    for route in ('raw', 'packed'):
        _, rows, _ = run(route, ['--native'] + verbose + ['--multi_read', damaged], capsys,
                         monkeypatch)
        assert rows == want, route


@pytest.mark.parametrize('verbose', [[], ['--verbose']])
def test_a_stream_only_the_device_refuses_is_redone_by_the_host(verbose, stand_in, capsys,
                                                                monkeypatch):
    """the device decoder refusing a sound stream (here: the stand-in, told to): the host's
    loader reads that read again and its row is the row of every other route"""
    _, want, _ = run('packed', ['--native'] + verbose + ['--multi_read', CONTAINERS[1]], capsys,
                     monkeypatch)

    def refusing(*args, **kwargs):
        out = classify_pair_deflated(*args, **kwargs)
        read = int(args[3]['read'][3])              # the read that stream 3 belongs to
        out[0][read] = 7 if out[0][read] != 7 else 8    # (a refused stream leaves no call)
        out[1][3] = 1
        return out
    monkeypatch.setattr(hip_backend, 'classify_pair_deflated', refusing)
    _, rows, _ = run('raw', ['--native'] + verbose + ['--multi_read', CONTAINERS[1]], capsys,
                     monkeypatch)
    assert rows == want and len(rows) == 10


def test_realtime_tabulates_the_same_calls_by_every_route(stand_in, tmp_path, capsys, monkeypatch):
    import deepbinner_amd.realtime as realtime
    monkeypatch.setattr(realtime, 'POLL_SECONDS', 0)
    monkeypatch.setattr(shutil, 'which', lambda tool: None)
    monkeypatch.setenv('DEEPBINNER_REALTIME_TABLE_ONLY', '1')
    _, rows, _ = run('packed', ['--native', '--multi_read', MULTI], capsys, monkeypatch)
    want = sorted(row.split('\t') for row in rows)
    for route in ROUTES:
        for name, value in ROUTES[route].items():
            monkeypatch.setenv(name, value)
        out_dir = tmp_path / route
        cli.main(['realtime', '--in_dir', MULTI, '--out_dir', str(out_dir), '--stop',
                  '-s', os.path.join(MODEL_DIR, START + '.dbw'),
                  '-e', os.path.join(MODEL_DIR, END + '.dbw')])
        capsys.readouterr()
        table = [line.split('\t') for line in
                 (out_dir / 'multi_read_classifications.tsv').read_text().splitlines()]
        assert sorted(r[:2] for r in table) == want, route
        assert {r[2] for r in table} == set(CONTAINERS)


# ---- batches of one-read files: containers whose reads happen to live in separate files ---------
SINGLE = os.path.join(GOLD, 'fast5', 'single')
VARIANTS = os.path.join(GOLD, 'fast5', 'h5py_variants')


@pytest.fixture(scope='module')
def one_read(tmp_path_factory):
    """(directory, its files in the order ``classify`` walks them, their read ids): the 7 files of
    golden/fast5/single and the h5py variants the native loader reads, 29 one-read files"""
    from deepbinner_amd.load_fast5s import find_all_fast5s
    sources = sorted(os.path.join(sub, name) for sub in (SINGLE, VARIANTS)
                     for name in os.listdir(sub) if name.endswith('.fast5'))
    sources = [f for f in sources if fast5_native.load_batch([f], None, 1)[3][0] == 0]
    assert len(sources) == 29
    directory = tmp_path_factory.mktemp('one_read')
    for path in sources:
        os.symlink(path, str(directory / os.path.basename(path)))
    files = find_all_fast5s(str(directory))
    return str(directory), files, fast5_native.load_batch(files, None, 1)[0]


def run_one_read(route, argv, directory, capsys, monkeypatch):
    """several batches and a short last one on the packed and lists routes; the raw route on
    however few files"""
    monkeypatch.setenv('DEEPBINNER_RAW_CLASSIFY_MIN_FILES', '1')
    return run(route, list(argv) + ['--batch_size', '4', directory], capsys, monkeypatch)


def last_progress(err):
    import re
    return re.findall(r'Classifying fast5s: (\d+) / (\d+)', err)[-1]


@pytest.mark.parametrize('models', [['--native'], ['--rapid'], ['--native', '--require_both']])
@pytest.mark.parametrize('verbose', [[], ['--verbose']])
def test_the_three_one_read_routes_print_the_same_table(models, verbose, one_read, stand_in, gold,
                                                        capsys, monkeypatch):
    directory, files, ids = one_read
    tables = {route: run_one_read(route, models + verbose, directory, capsys, monkeypatch)
              for route in ROUTES}
    header, rows, err = tables['raw']
    assert [row.split('\t')[0] for row in rows] == ids
    assert tables['packed'][:2] == (header, rows)
    assert tables['lists'][0] == header and sorted(tables['lists'][1]) == sorted(rows)
    for route in ROUTES:
        assert last_progress(tables[route][2]) == ('29', '29'), route
    if '--rapid' in models and not verbose:
        want = dict(zip(gold['read_ids'], gold['calls']['SQK-RBK004_read_starts/start'][:7]))
        got = {r.split('\t')[0]: r.split('\t')[1] for r in rows}
        assert {rid: got[rid] for rid in want} == want


def test_the_queues_of_the_one_read_raw_route_get_their_cus_back(one_read, stand_in, capsys,
                                                                 monkeypatch):
    """the queues are set up once and given back once; a batch of one-read files is not asked
    how many CUs it would leave to the inflate kernels (inflate_cus_for: containers only)"""
    import deepbinner_amd.realtime as realtime
    asked = []
    monkeypatch.setattr(realtime, 'inflate_cus_for',
                        lambda *records: asked.append(records) or realtime.LONG_STREAM_CUS)
    run_one_read('raw', ['--native'], one_read[0], capsys, monkeypatch)
    queue_models = stand_in + StandInModel.clones
    assert len(stand_in) == 2 and len(queue_models) == 6    # three (start, end) pairs on the device
    assert all(m.reserved and m.reserved[-1] == 0 for m in queue_models)
    assert not asked and all(m.reserved == [0, 0] for m in queue_models)


def damaged_one_read_file(path, read_id, signal):
    stream = bytearray(zlib.compress(signal.tobytes(), 1))
    stream[2] = 0x07                                # BFINAL = 1, BTYPE = 3: the reserved type
    with open(path, 'wb') as out:
        out.write(hdf5_write.single_read_fast5_bytes(read_id, signal, packed_signal=bytes(stream)))


@pytest.mark.parametrize('verbose', [[], ['--verbose']])
def test_a_one_read_file_both_decoders_refuse_costs_its_own_row(verbose, one_read, stand_in,
                                                                tmp_path, capsys, monkeypatch):
    """a one-read file whose deflate stream is damaged: the stand-in decoder refuses the stream,
    the host's redo refuses the file - no row; the other files' rows are those of the clean run"""
    from deepbinner_amd.load_fast5s import find_all_fast5s
    directory, files, ids = one_read
    _, clean, _ = run_one_read('raw', ['--native'] + verbose, directory, capsys, monkeypatch)
    row_of = dict(zip((os.path.basename(f) for f in files), clean))
    assert len(row_of) == 29
    for f in files:
        os.symlink(os.path.realpath(f), str(tmp_path / os.path.basename(f)))
    signal = np.arange(5000, dtype=np.int16) % 700
    damaged_one_read_file(str(tmp_path / 'a_damaged.fast5'), 'a-damaged-read', signal)
    walked = [os.path.basename(f) for f in find_all_fast5s(str(tmp_path))]
    assert len(walked) == 30 and fast5_native.load_batch(
        [str(tmp_path / 'a_damaged.fast5')], None, 1)[3][0] != 0
    want = [row_of[name] for name in walked if name != 'a_damaged.fast5']
    for route in ('raw', 'packed'):
        _, rows, err = run_one_read(route, ['--native'] + verbose, str(tmp_path), capsys,
                                    monkeypatch)
        assert rows == want, route


@pytest.mark.parametrize('verbose', [[], ['--verbose']])
def test_a_one_read_stream_only_the_device_refuses_is_redone_by_the_host(verbose, one_read,
                                                                         stand_in, capsys,
                                                                         monkeypatch):
    """the device decoder refusing a sound stream of a one-read batch (the stand-in, told to):
    the host's loader reads that file again - the scanned ends only, on one thread - and its row
    is the row of the packed route"""
    directory, files, ids = one_read
    _, want, _ = run_one_read('packed', ['--native'] + verbose, directory, capsys, monkeypatch)
    refused = []

    def refusing(*args, **kwargs):
        out = classify_pair_deflated(*args, **kwargs)
        read = int(args[3]['read'][3])              # the read that stream 3 belongs to
        out[0][read] = 7 if out[0][read] != 7 else 8    # (a refused stream leaves no call)
        out[1][3] = 1
        refused.append(read)
        return out
    monkeypatch.setattr(hip_backend, 'classify_pair_deflated', refusing)
    reread = []
    load_batch = fast5_native.load_batch

    def spy(fast5_files, keep=None, threads=0):
        reread.append((list(fast5_files), keep, threads))
        return load_batch(fast5_files, keep, threads)
    monkeypatch.setattr(fast5_native, 'load_batch', spy)
    _, rows, _ = run_one_read('raw', ['--native'] + verbose, directory, capsys, monkeypatch)
    assert rows == want and len(rows) == 29
    # (the stand-in's zlib also refuses the two files with chunks missing: three files re-read)
    assert len(refused) == 1 and [files[refused[0]]] in [again[0] for again in reread]
    assert len(reread) == 3 and all(len(again[0]) == 1 for again in reread)
    assert all(again[1:] == (classify.scanned_end_samples(6144, 1024, 1024), 1)
               for again in reread)


def test_a_container_among_one_read_files_on_the_raw_route(one_read, stand_in, tmp_path, capsys,
                                                           monkeypatch):
    """a directory the five sampled files call one-read, with one container in it: the one-read
    batches set it aside and its reads come last (--multi_read), or the run ends with the
    reference's error (without)"""
    from vbz_fixtures import read_all
    directory, files, ids = one_read
    monkeypatch.setattr(classify, 'determine_single_or_multi_fast5s', lambda files, **kw: 'single')
    for f in files:
        os.symlink(os.path.realpath(f), str(tmp_path / os.path.basename(f)))
    os.symlink(CONTAINERS[0], str(tmp_path / os.path.basename(CONTAINERS[0])))
    inside = [rid for rid, _ in read_all(CONTAINERS[0])]
    tables = {route: run_one_read(route, ['--native', '--multi_read'], str(tmp_path), capsys,
                                  monkeypatch) for route in ('raw', 'packed')}
    header, rows, err = tables['raw']
    assert len(rows) == 29 + len(inside)
    assert sorted(row.split('\t')[0] for row in rows[:29]) == sorted(ids)
    assert sorted(row.split('\t')[0] for row in rows[29:]) == sorted(inside)
    assert tables['packed'][:2] == (header, rows)
    for route in tables:
        assert last_progress(tables[route][2]) == ('30', '30'), route
    for route in ('raw', 'packed'):
        with pytest.raises(SystemExit, match=r'does not \(yet\) support multi-read fast5 files'):
            run_one_read(route, ['--native'], str(tmp_path), capsys, monkeypatch)


def test_the_sequence_of_c_abi_calls(one_read, stand_in, capsys, monkeypatch):
    """(function, reads, streams, want_sides) of every call that reaches the device library's
    Python surface - hip_backend.classify_pair / classify_pair_deflated and the models' own
    classify_packed / classify_signals - for a terse raw and a terse packed run over the one-read
    directory and a raw run over the golden containers: recorded on the tree before the one-read
    batches and the containers shared their units, and the same since.  (No file of these runs is
    unreadable.  A packed one-read batch with an unreadable file went to the models as lists of
    signals - one classify_signals call per model - before; since, it is compacted like a
    container with an unreadable read and takes the one classify_pair call of every other batch.)"""
    import threading
    log, inside = [], threading.local()     # (the queues of the raw route are threads)

    def logged(name, function, reads, streams):
        def call(*args, **kwargs):
            if getattr(inside, 'stand_in', False):      # a stand-in calling its models
                return function(*args, **kwargs)
            log.append((name, reads(args), streams(args), bool(kwargs.get('want_sides'))))
            inside.stand_in = True
            try:
                return function(*args, **kwargs)
            finally:
                inside.stand_in = False
        return call

    monkeypatch.setattr(hip_backend, 'classify_pair', logged(
        'classify_pair', classify_pair, lambda a: len(a[3]) - 1, lambda a: None))
    monkeypatch.setattr(hip_backend, 'classify_pair_deflated', logged(
        'classify_pair_deflated', classify_pair_deflated, lambda a: len(a[4]) - 1,
        lambda a: len(a[3])))
    monkeypatch.setattr(StandInModel, 'classify_packed', logged(
        'classify_packed', StandInModel.classify_packed, lambda a: len(a[2]) - 1, lambda a: None))
    monkeypatch.setattr(StandInModel, 'classify_signals', logged(
        'classify_signals', StandInModel.classify_signals, lambda a: len(a[1]), lambda a: None))

    def calls_of(route, argv, directory):
        del log[:]
        run_one_read(route, argv, directory, capsys, monkeypatch)
        return list(log)

    directory = one_read[0]
    # (one batch, the many-chunk variants among it; the stand-in's zlib refuses the two files with
    # chunks missing, which the host then reads and classifies on their own)
    assert calls_of('raw', ['--native'], directory) == \
        [('classify_pair_deflated', 29, 1067, False)] + [('classify_pair', 1, None, False)] * 2
    assert calls_of('packed', ['--native'], directory) == \
        [('classify_pair', 4, None, False)] * 7 + [('classify_pair', 1, None, False)]
    assert calls_of('raw', ['--native', '--multi_read'], MULTI) == \
        [('classify_pair_deflated', 10, 10, False)] * 3
