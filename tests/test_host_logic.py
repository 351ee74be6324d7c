"""
Host-side drop-in surface (CPU only): the reference's own tests restated against
deepbinner_amd — tests/test_classify.py, test_combine_calls.py, test_load_fast5s.py — with the
model object replaced by an oracle-backed double at seam b1 (conftest.oracle_backend), so the
windowing / merge / call / TSV logic of deepbinner_amd.classify is what is under test.
"""
import argparse
import io
import os

import numpy as np
import pytest

from conftest import GOLD, MODEL_DIR
from test_oracle_golden import EXPECTED_START, EXPECTED_END
import deepbinner_amd.classify as classify
import deepbinner_amd.load_fast5s as load_fast5s
import deepbinner_amd.trim_signal as trim_signal
from deepbinner_amd import hdf5_lite

FAST5_DIR = os.path.join(GOLD, 'fast5', 'single')
MULTI_DIR = os.path.join(GOLD, 'fast5', 'multi')
START_MODEL = os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw')
END_MODEL = os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw')
SINGLE = os.path.join(FAST5_DIR, '5210_N128870_20180511_FAH70336_MN20200_sequencing_run_057_'
                                 'Deepbinner_amplicon_43629_read_11206_ch_157_strand.fast5')
ROW = ['0.00', '0.00', '0.00', '1.00'] + ['0.00'] * 9


def make_args(**kw):
    base = dict(verbose=False, batch_size=128, scan_size=6144, score_diff=0.5,
                require_either=False, require_start=False, require_both=False)
    base.update(kw)
    return argparse.Namespace(**base)


# ---- model loading (reference tests/test_classify.py:24-68) -------------------------------
def test_load_2_models(oracle_backend):
    out = io.StringIO()
    sm, si, em, ei, osz, cnt = classify.load_and_check_models(START_MODEL, END_MODEL, 6144,
                                                              out_dest=out)
    assert (si, ei, osz, cnt) == (1024, 1024, 13, 2)
    assert 'Loading' in out.getvalue() and 'done' in out.getvalue()


def test_load_start_only(oracle_backend):
    sm, si, em, ei, osz, cnt = classify.load_and_check_models(START_MODEL, None, 6144,
                                                              out_dest=io.StringIO())
    assert si == 1024 and em is None and ei is None and osz == 13 and cnt == 1


def test_load_end_only(oracle_backend):
    sm, si, em, ei, osz, cnt = classify.load_and_check_models(None, END_MODEL, 6144,
                                                              out_dest=io.StringIO())
    assert ei == 1024 and sm is None and si is None and osz == 13 and cnt == 1


def test_bad_scan_size(oracle_backend):
    with pytest.raises(SystemExit) as e:
        classify.load_and_check_models(START_MODEL, END_MODEL, 6143, out_dest=io.StringIO())
    assert '--scan_size must be a multiple' in str(e.value)


def test_missing_and_invalid_model(oracle_backend, tmp_path):
    with pytest.raises(SystemExit) as e:
        classify.load_trained_model(str(tmp_path / 'nope'), out_dest=io.StringIO())
    assert 'does not exist' in str(e.value)
    bad = tmp_path / 'bad'
    bad.write_bytes(b'not a model file at all' * 10)
    with pytest.raises(SystemExit) as e:
        classify.load_trained_model(str(bad), out_dest=io.StringIO())
    assert 'model input has incorrect shape' in str(e.value)


def test_build_model_has_no_cpu_fallback(monkeypatch, weights):
    """Without a GPU the product path must fail loudly, never compute on the CPU."""
    from deepbinner_amd import hip_backend
    if hip_backend.device_count() > 0:
        pytest.skip('a GPU is visible here')
    with pytest.raises(hip_backend.HipBackendError):
        classify.build_model(weights['EXP-NBD103_read_starts'])


# ---- end-to-end calls (reference tests/test_classify.py:104-180) ---------------------------
@pytest.mark.parametrize('start,end,mode,expected', [
    (True, False, None, EXPECTED_START),
    (False, True, None, EXPECTED_END),
    (True, True, 'require_either', EXPECTED_START),
    (True, True, 'require_both', EXPECTED_END),
])
def test_fast5_classification(oracle_backend, capsys, start, end, mode, expected):
    args = make_args(**({mode: True} if mode else {}))
    fast5s = load_fast5s.find_all_fast5s(FAST5_DIR, verbose=True)
    sm, si, em, ei, osz, _ = classify.load_and_check_models(
        START_MODEL if start else None, END_MODEL if end else None, 6144,
        out_dest=io.StringIO())
    classifications, id_to_file = classify.classify_fast5_files(fast5s, sm, si, em, ei, osz, args,
                                                                full_output=False)
    assert classifications == expected
    assert set(id_to_file) == set(expected)
    out = capsys.readouterr().out
    assert 'Classifying fast5s: 7 / 7 (100.0%)' in out     # full_output=False -> stdout


# ---- exact TSV (reference tests/test_classify.py:182-296) ----------------------------------
@pytest.mark.parametrize('start,end,verbose,header,row', [
    (True, False, False, 'read_ID\tbarcode_call', '177c3867-6812-4476-a6da-9e4d5c43b760\t3'),
    (True, False, True,
     'read_ID\tbarcode_call\tnone\t1\t2\t3\t4\t5\t6\t7\t8\t9\t10\t11\t12',
     '177c3867-6812-4476-a6da-9e4d5c43b760\t3\t' + '\t'.join(ROW)),
    (False, True, True,
     'read_ID\tbarcode_call\tnone\t1\t2\t3\t4\t5\t6\t7\t8\t9\t10\t11\t12',
     '177c3867-6812-4476-a6da-9e4d5c43b760\t3\t' + '\t'.join(ROW)),
    (True, True, False, 'read_ID\tbarcode_call', '177c3867-6812-4476-a6da-9e4d5c43b760\t3'),
    (True, True, True,
     'read_ID\tbarcode_call\t' + '\t'.join(['start_none'] + ['start_%d' % i for i in range(1, 13)]
                                           + ['start_barcode_call', 'end_none']
                                           + ['end_%d' % i for i in range(1, 13)]
                                           + ['end_barcode_call']),
     '177c3867-6812-4476-a6da-9e4d5c43b760\t3\t' + '\t'.join(ROW + ['3'] + ROW + ['3'])),
])
def test_tsv_output(oracle_backend, capsys, start, end, verbose, header, row):
    args = make_args(verbose=verbose, require_either=start and end)
    sm, si, em, ei, osz, _ = classify.load_and_check_models(
        START_MODEL if start else None, END_MODEL if end else None, 6144,
        out_dest=io.StringIO())
    classifications, _ = classify.classify_fast5_files([SINGLE], sm, si, em, ei, osz, args,
                                                       full_output=True, summary_table=False)
    assert classifications['177c3867-6812-4476-a6da-9e4d5c43b760'] == '3'
    lines = capsys.readouterr().out.splitlines()
    assert lines == [header, row]


def test_headers_match_reference(gold, capsys):
    for key, want in gold['calls']['headers'].items():
        verbose, st, en = (c == '1' for c in key)
        classify.print_output_header(verbose, st, en, 13)
        assert capsys.readouterr().out == want


def test_summary_table(capsys):
    from deepbinner_amd.misc import print_summary_table
    import sys
    print_summary_table({'a': '3', 'b': 'none', 'c': '12', 'd': '3'}, output=sys.stderr)
    err = capsys.readouterr().err
    assert err == '\nBarcode     Count\n      3         2\n     12         1\n   none         1\n\n'


# ---- combine_calls (reference tests/test_combine_calls.py:27-51) ---------------------------
def test_combine_calls_truth_table(gold):
    for key, want in gold['calls']['combine_table'].items():
        mode, s, e = key.split('|')
        args = make_args(**{mode: True})
        assert classify.combine_calls(s, e, args) == want
    assert len(gold['calls']['combine_table']) == 15


def test_combine_call_numbers_is_combine_calls(gold):
    """The array form (what dbh_combine_calls_dev computes) against the string form, on the
    reference's truth table and on every pair of calls 0..12 in the three modes."""
    number = lambda name: 0 if name == 'none' else int(name)          # noqa: E731
    for key, want in gold['calls']['combine_table'].items():
        mode, s, e = key.split('|')
        got = classify.combine_call_numbers([number(s)], [number(e)], make_args(**{mode: True}))
        assert int(got[0]) == number(want), key
    grid = np.arange(13)
    starts, ends = np.repeat(grid, 13), np.tile(grid, 13)
    name = lambda c: 'none' if c == 0 else str(int(c))                # noqa: E731
    for mode in ('require_either', 'require_start', 'require_both'):
        args = make_args(**{mode: True})
        got = classify.combine_call_numbers(starts, ends, args)
        assert [name(c) for c in got] == [classify.combine_calls(name(a), name(b), args)
                                          for a, b in zip(starts, ends)]


# ---- small functions ----------------------------------------------------------------------
def test_barcode_call_rule():
    f = classify.get_barcode_call_from_probabilities
    assert f([0.6, 0.4, 0.0], 0.5) == 'none'            # best is class 0
    assert f([0.1, 0.8, 0.1], 0.5) == '1'
    assert f([0.3, 0.7, 0.0], 0.5) == 'none'            # runner-up may be class 0
    assert f([0.2, 0.4, 0.4], 0.1) == 'none'            # tie -> lower index best, diff 0
    assert f([0.25, 0.75, 0.0], 0.5) == '1'             # >= threshold


def test_make_sum_to_one():
    p = classify.make_sum_to_one(np.array([0.2, 0.9, 0.3, 0.4], dtype=np.float32))
    assert p[0] == pytest.approx(0.2, abs=1e-7)
    assert sum(p) == pytest.approx(1.0, abs=1e-7)
    assert p[1] / p[2] == pytest.approx(3.0, rel=1e-6)


def test_check_input_size():
    classify.check_input_size(1024, 512)          # accepted by the reference too
    with pytest.raises(SystemExit) as e:
        classify.check_input_size(1023, 6144)
    assert 'must be even' in str(e.value)
    with pytest.raises(SystemExit) as e:
        classify.check_input_size(1024, 1000)
    assert 'acceptable values for --scan_size are 1024, 1536, 2048, 2560, 3072, 3584, etc' \
        in str(e.value)


def test_normalise_matches_reference_edges(gold):
    edge = gold['calls']['normalise_edge']
    assert list(trim_signal.normalise(np.array([], dtype=np.int16))) == edge['empty']
    assert trim_signal.normalise(np.array([7, 7, 7], dtype=np.int16)).tolist() == edge['flat']
    assert trim_signal.normalise(np.array([1, 2, 3, 4], dtype=np.int16)).tolist() == edge['ramp']


def test_find_signal_start_pos(gold):
    got = [trim_signal.find_signal_start_pos(s) for s in gold['signals']]
    assert got == gold['calls']['trim_start']
    for s, want in zip(gold['multi_signals'], gold['calls']['multi_trim_start']):
        if want < 0:
            with pytest.raises(trim_signal.CannotTrim):
                trim_signal.find_signal_start_pos(s)
        else:
            assert trim_signal.find_signal_start_pos(s) == want
    with pytest.raises(trim_signal.CannotTrim):
        trim_signal.find_signal_start_pos(np.zeros(100, dtype=np.int16))


def test_call_batch_b1_matches_reference(gold, all_signals, weights):
    """Seam-b1 host path of call_batch == the reference's call_batch on the same predict."""
    from conftest import OracleModel
    ids = gold['read_ids'] + gold['multi_read_ids']
    for model_name, side in (('EXP-NBD103_read_starts', 'start'), ('EXP-NBD103_read_ends', 'end')):
        calls, probs = classify.call_batch(1024, 13, ids, all_signals,
                                           OracleModel(weights[model_name]), make_args(), side)
        assert calls == gold['calls']['%s/%s' % (model_name, side)]
        ref = np.load(os.path.join(GOLD, 'merged_%s_%s.npy' % (model_name, side)))
        assert np.abs(np.array(probs) - ref).max() < 1e-6
    assert classify.call_batch(1024, 13, [], [], None, make_args(), 'start') == ([], [])


def test_training_data_path(oracle_backend, gold, tmp_path, capsys):
    path = tmp_path / 'train.txt'
    with open(path, 'w') as f:
        for label, sig in (('3', gold['signals'][0]), ('2', gold['signals'][1])):
            f.write('%s\t%s\n' % (label, ','.join(str(int(v)) for v in sig[:2000])))
    assert classify.determine_input_type(str(path)) == 'training_data'
    sm, si, em, ei, osz, _ = classify.load_and_check_models(START_MODEL, None, 6144,
                                                            out_dest=io.StringIO())
    classify.classify_training_data(str(path), sm, si, em, ei, osz, make_args())
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == 'read_ID\tbarcode_call'
    assert lines[1].startswith('line_1_barcode_3\t') and lines[2].startswith('line_2_barcode_2\t')


# ---- fast5 loading (reference tests/test_load_fast5s.py:32-85) ------------------------------
def test_find_all_fast5s(capsys):
    assert len(load_fast5s.find_all_fast5s(FAST5_DIR)) == 7
    assert len(load_fast5s.find_all_fast5s(FAST5_DIR, verbose=True)) == 7
    err = capsys.readouterr().err
    assert 'Looking for fast5 files' in err and '7 fast5s found' in err


@pytest.mark.parametrize('name,read_id,length,first,idx,val', [
    ('5210_N128870_20180511_FAH70336_MN20200_sequencing_run_057_Deepbinner_amplicon_43629_'
     'read_11206_ch_157_strand.fast5', '177c3867-6812-4476-a6da-9e4d5c43b760', 4971, 714, 4950, 396),
    ('5210_N128870_20180511_FAH70336_MN20200_sequencing_run_057_Deepbinner_amplicon_43629_'
     'read_13863_ch_212_strand.fast5', '9bfcf22c-5654-4b4c-b8f7-d3cebd416338', 4983, 493, 4862, 618),
    ('FAK33493_1336eeb8050cb1ca93d41712cf8e817516306473_1000000.fast5',
     '2fbd86a4-029a-45cf-8f18-411d542572ba', 5395, 505, 5388, 436),
])
def test_get_read_id_and_signal(name, read_id, length, first, idx, val):
    rid, signal = load_fast5s.get_read_id_and_signal(os.path.join(FAST5_DIR, name))
    assert rid == read_id and len(signal) == length
    assert signal[0] == first and signal[idx] == val and signal.dtype == np.int16


def test_missing_fast5():
    assert load_fast5s.get_read_id_and_signal(os.path.join(FAST5_DIR, 'not_a_real_file.fast5')) \
        == (None, None)


def test_loader_pool_matches_serial_loader(monkeypatch):
    monkeypatch.setenv('DEEPBINNER_FAST5_READER', 'python')
    """LoaderPool: same (read_id, signal) as the serial loader, in file order, unreadable files
    reported as (None, None), with more runs than the in-flight window allows at once."""
    files = sorted(load_fast5s.find_all_fast5s(FAST5_DIR))
    files = (files + [os.path.join(FAST5_DIR, 'not_a_real_file.fast5')]) * 4
    want = [load_fast5s.get_read_id_and_signal(f) for f in files]
    with load_fast5s.LoaderPool(2, run=3, ahead=2) as pool:
        got = list(pool.load(files))
    assert [g[0] for g in got] == files
    for (path, read_id, signal), (want_id, want_signal) in zip(got, want):
        assert read_id == want_id
        assert (signal is None and want_signal is None) or np.array_equal(signal, want_signal)
    assert load_fast5s.choose_loader_procs(None, 7) == 1
    assert load_fast5s.choose_loader_procs(0, 100000) >= 1
    assert load_fast5s.choose_loader_procs(5, 7) == 5


@pytest.mark.parametrize('reader', ['python', 'native'])
def test_classification_with_loader_processes(oracle_backend, capsys, monkeypatch, reader):
    """classify_fast5_files gives the same calls, ids and output with --loader_procs 2 (worker
    processes around the Python reader, worker threads inside the native one)."""
    if reader == 'native':
        from deepbinner_amd import fast5_native
        if not fast5_native.available():
            pytest.skip('libdeepbinner_fast5.so not built')
    monkeypatch.setenv('DEEPBINNER_FAST5_READER', reader)
    assert load_fast5s.reader_kind() == reader
    fast5s = sorted(load_fast5s.find_all_fast5s(FAST5_DIR))
    sm, si, em, ei, osz, _ = classify.load_and_check_models(START_MODEL, None, 6144,
                                                            out_dest=io.StringIO())
    outs = []
    for procs in (1, 2):
        args = make_args(loader_procs=procs, batch_size=3)
        result = classify.classify_fast5_files(fast5s, sm, si, em, ei, osz, args)
        outs.append((result, capsys.readouterr().out))
    assert outs[0] == outs[1]
    assert outs[0][0][0] == EXPECTED_START


def test_single_or_multi():
    single = load_fast5s.find_all_fast5s(FAST5_DIR)
    multi = load_fast5s.find_all_fast5s(MULTI_DIR)
    assert load_fast5s.determine_single_or_multi_fast5s(single) == 'single'
    assert load_fast5s.determine_single_or_multi_fast5s(multi) == 'multi'


def test_loader_matches_packed_golden(gold):
    by_file = dict(zip(gold['files'], zip(gold['read_ids'], gold['signals'])))
    for name, (rid, sig) in by_file.items():
        got_id, got = load_fast5s.get_read_id_and_signal(os.path.join(FAST5_DIR, name))
        assert got_id == rid and np.array_equal(got, sig)
    multi = {}
    for path in sorted(load_fast5s.find_all_fast5s(MULTI_DIR)):
        for rid, sig in load_fast5s.iter_reads(path):
            multi[rid] = sig
    assert len(multi) == 30
    for rid, sig in zip(gold['multi_read_ids'], gold['multi_signals']):
        assert np.array_equal(multi[rid], sig)


def test_multi_read_refused_by_classify(oracle_backend):
    sm, si, em, ei, osz, _ = classify.load_and_check_models(START_MODEL, None, 6144,
                                                            out_dest=io.StringIO())
    with pytest.raises(SystemExit) as e:
        classify.classify_fast5_files(load_fast5s.find_all_fast5s(MULTI_DIR), sm, si, em, ei, osz,
                                      make_args())
    assert 'requires one-read-per-file fast5s' in str(e.value)
    with pytest.raises(SystemExit) as e:
        classify.classify_fast5_files([], sm, si, em, ei, osz, make_args())
    assert 'no fast5 files found' in str(e.value)


def test_hdf5_reader_rejects_garbage(tmp_path):
    p = tmp_path / 'x.fast5'
    p.write_bytes(b'\x00' * 4096)
    with pytest.raises(OSError):
        hdf5_lite.File(str(p))
    assert load_fast5s.get_root_level_keys(str(p)) == []
    assert classify.determine_input_type(SINGLE) == 'single_fast5'
    assert classify.determine_input_type(FAST5_DIR) == 'directory'


def test_shipped_weights_are_what_h5py_reads_from_the_reference_models():
    """tests/golden/model_reference.json: every dataset of the reference's three Keras model files
    as the real HDF5 library returns it (oracle/make_model_golden.py, build container).  The .dbw
    blobs that ship - converted through this package's own HDF5 reader - must hold exactly those
    numbers, layer by layer, and nothing else."""
    import hashlib
    import json
    from conftest import GOLD, MODEL_DIR, MODELS
    from deepbinner_amd.model_format import ModelWeights
    with open(os.path.join(GOLD, 'model_reference.json')) as f:
        golden = json.load(f)
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype='<f4').tobytes()).hexdigest()  # noqa: E731
    for name in MODELS:
        want = golden[name]
        assert want['keras_version'] == '2.1.4' and want['backend'] == 'tensorflow'
        weights, _ = ModelWeights.load(os.path.join(MODEL_DIR, name + '.dbw'))
        seen = {}
        for i, (kernel, bias) in enumerate(weights.convs, start=1):
            seen['conv1d_%d/conv1d_%d/kernel:0' % (i, i)] = kernel
            seen['conv1d_%d/conv1d_%d/bias:0' % (i, i)] = bias
        for i, bn in enumerate(weights.bns, start=1):
            for part, values in zip(('gamma:0', 'beta:0', 'moving_mean:0', 'moving_variance:0'), bn):
                seen['batch_normalization_%d/batch_normalization_%d/%s' % (i, i, part)] = values
        assert sorted(seen) == sorted(want['datasets'])
        for path, values in seen.items():
            assert list(values.shape) == want['datasets'][path]['shape'], path
            assert digest(values) == want['datasets'][path]['sha256'], path
        assert weights.flat().size == want['n_parameters'] == 107197


def test_keras_model_file_import(tmp_path):
    """The reference's own Keras model file loads through hdf5_lite (tests/golden/keras/: the
    file with its optimizer state zeroed, gzipped - oracle/make_keras_golden.py)."""
    import gzip
    ref = str(tmp_path / 'EXP-NBD103_read_starts')
    with gzip.open(os.path.join(GOLD, 'keras', 'EXP-NBD103_read_starts.gz'), 'rb') as f:
        with open(ref, 'wb') as out:
            out.write(f.read())
    from deepbinner_amd.model_format import ModelWeights
    w, shape = ModelWeights.load(ref)
    assert shape == [None, 1024, 1] and w.n_classes == 13
    assert np.array_equal(w.flat(), ModelWeights.load(START_MODEL)[0].flat())


def test_dispatch_batches_keeps_order_and_spreads_the_work():
    """The multi-device dispatcher: batches go round the devices, at most `depth` per device in
    flight, results come back in input order whatever the devices' speeds."""
    import threading
    import time
    from deepbinner_amd import classify
    seen, lock, in_flight, peak = [], threading.Lock(), [0], [0]

    def work(batch, start_replica, end_replica):
        with lock:
            in_flight[0] += 1
            peak[0] = max(peak[0], in_flight[0])
        time.sleep(0.02 if start_replica == 's0' else 0.001)      # device 0 is the slow one
        with lock:
            in_flight[0] -= 1
            seen.append((batch, start_replica, end_replica, threading.current_thread().name))
        return batch * 10

    replicas = [('s0', 'e0'), ('s1', 'e1'), ('s2', 'e2')]
    out = list(classify.dispatch_batches(iter(range(20)), replicas, work, depth=2))
    assert out == [b * 10 for b in range(20)]
    for batch, s_rep, e_rep, thread in seen:
        d = batch % 3
        assert (s_rep, e_rep) == replicas[d] and thread.startswith('deepbinner-device-%d' % d)
    assert 1 < peak[0] <= 6
    # one device: no threads at all
    assert list(classify.dispatch_batches(iter(range(3)), [('s', None)],
                                          lambda b, s_rep, e_rep: (b, s_rep))) == \
        [(0, 's'), (1, 's'), (2, 's')]
    # an exception on a device reaches the caller
    def boom(batch, *_):
        if batch == 4:
            raise RuntimeError('device fell over')
        return batch
    try:
        list(classify.dispatch_batches(iter(range(8)), replicas, boom))
        assert False
    except RuntimeError as e:
        assert 'fell over' in str(e)


def test_device_replicas_pairs_the_models_per_device():
    from deepbinner_amd import classify

    class Fake:
        inputs = outputs = n_classes = input_size = predict = None
        classify_signals = classify_packed = None

    a, b, c, d = Fake(), Fake(), Fake(), Fake()
    start, end = classify.ReplicatedModel([a, b]), classify.ReplicatedModel([c, d])
    assert classify.device_replicas(start, end) == [(a, c), (b, d)]
    assert classify.device_replicas(start, None) == [(a, None), (b, None)]
    assert classify.device_replicas(a, None) == [(a, None)]


# ---- bench.py's line (CPU-checkable parts) --------------------------------------------------
def test_bench_workload_string_names_the_configuration():
    """`config.workload` is the one description the driver's record keeps: it must start with the
    BASELINE.json configuration and carry no unformatted placeholder (round-2 verdict)."""
    import bench
    for number, cfg in bench.CONFIGS.items():
        text = bench.workload_string(cfg)
        assert text.startswith('BASELINE.json configs[{}]: {}'.format(number, cfg['models'][0]))
        assert '{' not in text and '}' not in text
        assert 'batch {}'.format(cfg['batch']) in text and str(cfg['reads']) in text
    assert bench.workload_string(bench.CONFIGS[1]).startswith(
        'BASELINE.json configs[1]: EXP-NBD103_read_starts model, 10000 synthetic')
    assert bench.PUBLISHED_CPU == {'value': 15, 'unit': 'reads/s', 'threads': 12,
                                   'source': 'README.md:213'}


def test_bench_dump_outputs_float32_and_a_fixed_sample_above_the_limit(tmp_path, monkeypatch):
    """`--dump-outputs`: every array as float32 .npy; above the size limit the same seeded sample
    of reads for every array (a shorter array keeps the sampled reads it has), its indices in
    read_index.npy, the whole within the limit."""
    import bench
    rng = np.random.default_rng(3)
    calls = rng.integers(0, 13, 1000).astype(np.int32)
    probs = rng.random((1000, 13)).astype(np.float32)
    bench.dump_outputs(str(tmp_path / 'all'), {'calls': calls, 'probs_m': probs})
    got = {n: np.load(str(tmp_path / 'all' / (n + '.npy'))) for n in ('calls', 'probs_m')}
    assert sorted(p.name for p in (tmp_path / 'all').iterdir()) == ['calls.npy', 'probs_m.npy']
    assert got['calls'].dtype == np.float32 and np.array_equal(got['calls'], calls)
    assert np.array_equal(got['probs_m'], probs)
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 20000)
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), {'calls': calls, 'probs_m': probs[:600]})
    a, b = [{p.stem: np.load(str(p)) for p in (tmp_path / run).iterdir()} for run in 'ab']
    assert sorted(a) == ['calls', 'probs_m', 'read_index']
    assert all(np.array_equal(a[k], b[k]) for k in a)
    index = a['read_index'].astype(np.int64)
    assert a['read_index'].dtype == np.float64 and np.all(np.diff(index) > 0)
    assert np.array_equal(a['calls'], calls[index].astype(np.float32))
    assert np.array_equal(a['probs_m'], probs[index[index < 600]])
    assert sum(v.nbytes for v in a.values()) <= 20000


def test_devices_flag_under_a_per_gpu_launcher_is_refused(monkeypatch):
    """`--devices N` (one process driving N GPUs) together with WORLD_SIZE > 1 (a
    launcher that already gave every process its GPU) would put every rank on GPUs 0..N-1."""
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit) as e:
        classify.set_tensorflow_threads(argparse.Namespace(devices=2))
    assert 'one-process-per-GPU launcher' in str(e.value)


def test_usable_cpus_is_a_sane_number():
    from deepbinner_amd import misc
    n = misc.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)


def test_host_inflate_share_follows_the_cores_per_gpu(monkeypatch):
    """How much of the inflating the host keeps (realtime.host_inflate_share): everything when it
    has cores to spare (30 per GPU), nothing otherwise - a split has not paid since round 6's
    kernels; the environment overrides either way."""
    import deepbinner_amd.realtime as realtime
    for name in ('DEEPBINNER_GPU_INFLATE', 'DEEPBINNER_HOST_INFLATE_SHARE'):
        monkeypatch.delenv(name, raising=False)
    shares = []
    for cores in (2, 4, 8, 16, 24, 32, 64, 256):
        monkeypatch.setattr(realtime, 'usable_cpus', lambda cores=cores: cores)
        shares.append(realtime.host_inflate_share(1))
        assert realtime.host_inflate_share(8) <= shares[-1]
    assert shares == sorted(shares) and shares[0] == 0 and shares[-1] == 100
    assert set(shares) == {0, 100} and shares[3] == 0     # 16 cores, one GPU: the box it was measured on
    assert shares[5] == 100                               # 32 cores for one GPU: the host alone
    monkeypatch.setattr(realtime, 'usable_cpus', lambda: 16)
    assert realtime.host_inflate_share(8) == 0       # BASELINE.json configs[4]: one host, eight GPUs
    monkeypatch.setenv('DEEPBINNER_HOST_INFLATE_SHARE', '37')
    assert realtime.host_inflate_share(1) == 37
    monkeypatch.setenv('DEEPBINNER_GPU_INFLATE', '0')
    assert realtime.host_inflate_share(1) == 100
    monkeypatch.setenv('DEEPBINNER_GPU_INFLATE', '1')
    assert realtime.host_inflate_share(1) == 0


def test_queue_clones_hold_no_cycle_and_follow_their_partner():
    """realtime.queue_clones keeps further (start, end) replicas on the pair's first model, keyed
    by weak references to the pair (a strong tuple containing the holder was a
    cycle; clones of a partner that was closed on its own stayed on the GPU)."""
    import gc
    import weakref
    from deepbinner_amd import realtime

    class Fake:
        live = 0

        def __init__(self):
            self.handle = object()
            Fake.live += 1

        def clone(self):
            return Fake()

        def close(self):
            if self.handle is not None:
                self.handle = None
                Fake.live -= 1
            for _pair, more in self.__dict__.pop('_queue_clones', []):
                for group in more:
                    for c in group:
                        if c is not None and c is not self:
                            c.close()

    start, end = Fake(), Fake()
    a = realtime.queue_clones((start, end), 2)
    assert len(a) == 2 and Fake.live == 6
    assert realtime.queue_clones((start, end), 2) == a and Fake.live == 6      # cached by identity
    assert realtime.queue_clones((start, end), 1) == a[:1]
    # another partner: its own clones; the first entry stays
    other = Fake()
    b = realtime.queue_clones((start, other), 1)
    assert b[0][0] is not a[0][0] and Fake.live == 9
    # the partner closed on its own: its clones go at the next call, the other entry is kept
    other.close()
    assert realtime.queue_clones((start, end), 2) == a
    assert Fake.live == 6
    # no cycle through the holder: dropping the last reference frees it without the collector
    gc.disable()
    try:
        ref = weakref.ref(start)
        start.close()
        del start, a, b
        assert ref() is None
    finally:
        gc.enable()
    assert Fake.live == 1       # `end` itself


def test_long_streams_leave_cus_to_the_inflate_kernels(monkeypatch):
    """realtime.inflate_cus_for: a container of long zlib streams takes CUs out of its forward
    launches, an ordinary one none; stored pieces do not count; the environment has the last word."""
    from deepbinner_amd import realtime
    monkeypatch.delenv('DEEPBINNER_INFLATE_CUS', raising=False)
    assert realtime.inflate_cus_for([34000] * 10, [0] * 10) == realtime.INFLATE_CUS
    assert realtime.inflate_cus_for([124000] * 10, [0] * 10) == realtime.LONG_STREAM_CUS
    assert realtime.inflate_cus_for([124000] * 10 + [10 ** 7], [0] * 10 + [1]) == realtime.LONG_STREAM_CUS
    assert realtime.inflate_cus_for([10 ** 7], [1]) == realtime.INFLATE_CUS
    assert realtime.inflate_cus_for([], []) == realtime.INFLATE_CUS
    monkeypatch.setenv('DEEPBINNER_INFLATE_CUS', '16')
    assert realtime.inflate_cus_for([124000] * 10, [0] * 10) is None
