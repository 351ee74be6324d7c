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
