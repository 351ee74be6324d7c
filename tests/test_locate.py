"""``locate`` without a device: the NumPy restatement against the oracle's own logits, the CPU model
of the kernel (``dbh_locate_host``) against the restatement bit for bit, the command against a host
stand-in, and the C ABI's argument checks."""
import argparse
import ctypes
import os

import numpy as np
import pytest

import locate_reference as ref
from conftest import GOLD, MODEL_DIR, REPO, OracleModel
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import hip_backend, locate
from general_fixtures import geometry, golden_signals

STARTS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw')
ENDS = os.path.join(MODEL_DIR, 'EXP-NBD103_read_ends.dbw')
SINGLE = os.path.join(GOLD, 'fast5', 'single')
INVALID, UNSUPPORTED = 1, 5
NEW_SYMBOLS = ['dbh_evidence_floats', 'dbh_evidence_dev', 'dbh_locate_dev', 'dbh_locate_host',
               'dbh_locate_workspace_bytes', 'dbh_locate_i16']


def same_fields(got, want, names=ref.LOCATION.names):
    for name in names:
        assert got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])


# ---- 1: the restatement is a decomposition of the logit ---------------------------------------------
@pytest.mark.parametrize('input_size,n_classes', [(1024, 13), (256, 13), (1000, 5), (96, 2)])
def test_the_mean_of_the_evidence_is_the_logit(input_size, n_classes):
    from oracle import classify_ref
    weights = geometry(input_size, n_classes)
    windows = classify_ref.make_windows(golden_signals()[:3], input_size, input_size, 'start')
    _, evidence, logits = ref.evidence(weights, windows.reshape(-1, input_size))
    assert evidence.dtype == np.float64 and evidence.shape[1:] == (ref.cells_of(input_size), n_classes)
    assert np.array_equal(evidence.mean(axis=1), logits)
    assert (evidence >= 0).all() and evidence.max() > 0


def test_cells_of_every_test_geometry():
    assert [ref.cells_of(L) for L in (96, 98, 160, 256, 1000, 1024, 1502, 2048, 8448, 16384)] == \
        [1, 1, 1, 2, 8, 8, 11, 16, 66, 128]


# ---- 2: the CPU model of the kernel against the restatement ----------------------------------------
@pytest.mark.parametrize('side', ['start', 'end'])
@pytest.mark.parametrize('cells,steps,n_classes,n_reads', ref.RANDOM_CASES)
def test_host_model_matches_the_restatement(cells, steps, n_classes, n_reads, side):
    ev, calls, lengths, input_size = ref.random_case(cells, steps, n_classes, n_reads,
                                                     seed=cells + 1000 * steps)
    got = hip_backend.locate_rule(ev, calls, lengths, input_size, side)
    assert got.dtype == ref.LOCATION
    same_fields(got, ref.locate(ev, calls, lengths, input_size, side))
    called = got['cls'] != 0
    assert np.array_equal(got['cls'], np.where(called, calls, 0))
    assert (got['window'][~called] == -1).all() and (got['end_sample'][~called] == -1).all()
    assert (got['first_sample'][called] <= got['end_sample'][called]).all()
    assert (got['end_sample'][called] <= lengths[called]).all()
    if n_reads >= 64 and cells > 1:
        assert called.any() and (got['first_cell'][called] < got['last_cell'][called]).any()


def test_reads_and_values_are_covered():
    assert {c[0] for c in ref.RANDOM_CASES} == {1, 2, 8, 63, 64, 65, 128}
    assert {c[1] for c in ref.RANDOM_CASES} == {1, 2, 12, 24}
    assert {c[2] for c in ref.RANDOM_CASES} == {2, 13, 256}
    assert {c[3] for c in ref.RANDOM_CASES} >= {1, 64, 65, 1000}


@pytest.mark.parametrize('case', ref.planted_cases(), ids=lambda c: c[0])
def test_planted_cases(case):
    _, ev, c, n, input_size, side, want = case
    got = hip_backend.locate_rule(ev, [c], [n], input_size, side)
    same_fields(got, ref.locate(ev, [c], [n], input_size, side))
    row = got[0]
    assert (row['window'], row['peak_cell'], row['first_cell'], row['last_cell'],
            row['first_sample'], row['end_sample']) == want
    if not ev.any():
        assert row['share'] == 0 and row['peak'] == 0
    # no call, or a call that is no class of the model: no location
    for none in (0, -1, ev.shape[3]):
        empty = hip_backend.locate_rule(ev, [none], [n], input_size, side)
        same_fields(empty, ref.no_location().reshape(1))


def test_share_is_the_fp64_quotient_rounded_once():
    _, ev, c, n, input_size, side, _ = ref.planted_cases()[1]
    below = float(np.nextafter(np.float32(1.5), np.float32(0)))
    got = hip_backend.locate_rule(ev, [c], [n], input_size, side)[0]
    assert got['share'] == np.float32(4.5 / ((1.5 + 3.0) + below)) and got['peak'] == 3


def test_a_nan_never_wins():
    ev = np.zeros((1, 1, 8, 13), dtype=np.float32)
    ev[0, 0, :4, 1] = (np.nan, 1, 1, np.nan)
    got = hip_backend.locate_rule(ev, [1], [2000], 1024, 'start')
    same_fields(got, ref.locate(ev, [1], [2000], 1024, 'start'), ref.INTEGERS + ('peak',))
    assert (got[0]['peak_cell'], got[0]['first_cell'], got[0]['last_cell']) == (1, 1, 2)
    ev[0, 0, :, 1] = np.nan
    got = hip_backend.locate_rule(ev, [1], [2000], 1024, 'start')
    same_fields(got, ref.locate(ev, [1], [2000], 1024, 'start'), ref.INTEGERS + ('peak',))
    assert (got[0]['window'], got[0]['peak_cell'], got[0]['peak']) == (0, 0, 0)


def test_sanitizer_program_is_a_makefile_target():
    text = open(os.path.join(REPO, 'deepbinner_amd', 'csrc', 'Makefile')).read()
    assert 'locate_asan:' in text and 'locate_model_check.cpp' in text
    assert '-fsanitize=address,undefined' in text[text.index('locate_asan:'):]
    source = open(os.path.join(REPO, 'deepbinner_amd', 'csrc', 'locate_model_check.cpp')).read()
    assert 'int main()' in source and 'dbh_locate_core.h' in source


# ---- 4: the command against a host stand-in --------------------------------------------------------
def options(**given):
    base = dict(input=SINGLE, native=False, rapid=False, start_model=STARTS, end_model=ENDS,
                scan_size=1024.0, score_diff=0.5, require_either=True, require_start=False,
                require_both=False, multi_read=False, batch_size=4, loader_procs=0, devices=0)
    base.update(given)
    return argparse.Namespace(**base)


def table(text):
    lines = text.strip('\n').split('\n')
    return lines[0].split('\t'), [line.split('\t') for line in lines[1:]]


@pytest.fixture()
def three_files(tmp_path, gold):
    """The three shortest golden reads as one-read files written by the project's own writer, and a
    short run of noise that no model calls (the stand-in's network is NumPy: keep it small)."""
    from deepbinner_amd import hdf5_write
    order = sorted(range(len(gold['signals'])), key=lambda i: len(gold['signals'][i]))[:3]
    reads = {'read-{}'.format(i): np.asarray(gold['signals'][i], dtype=np.int16) for i in order}
    rng = np.random.default_rng(5)
    reads['noise'] = np.clip(rng.normal(500, 80, 700), -32768, 32767).astype(np.int16)
    for name, signal in reads.items():
        hdf5_write.write_single_read_fast5(str(tmp_path / (name + '.fast5')), name, signal)
    return str(tmp_path), reads


def expected_rows(reads, sides, mode='require_either', scan_size=1024, score_diff=0.5):
    """The table from the restatement: per side the stand-in's calls and locations."""
    from oracle import classify_ref
    from deepbinner_amd.model_format import ModelWeights
    backend = ref.HostBackend()
    names = list(reads)
    samples = np.concatenate([reads[k] for k in names])
    offsets = np.concatenate([[0], np.cumsum([len(reads[k]) for k in names])]).astype(np.int64)
    found = {}
    for side, path in sides:
        model = OracleModel(ModelWeights.load(path)[0])
        _, calls, locations = backend.locate_packed(model, samples, offsets, side, scan_size, score_diff)
        found[side] = (calls, locations)
    rows = {}
    for r, name in enumerate(names):
        each = ['none' if found[s][0][r] == 0 else str(found[s][0][r]) for s, _ in sides]
        final = each[0] if len(each) == 1 else classify_ref.combine_calls(each[0], each[1], mode)
        row = [name, final, str(len(reads[name]))]
        for side, _ in sides:
            loc = found[side][1][r]
            row += ['-'] * 5 if loc['cls'] == 0 else [
                str(loc['cls']), str(loc['first_sample']), str(loc['end_sample']),
                '%.1f' % loc['peak'], '%.2f' % loc['share']]
        rows[name] = row
    return rows


def test_command_rows_and_summary(oracle_backend, three_files, capsys):
    directory, reads = three_files
    backend = ref.HostBackend()
    capsys.readouterr()
    locate.locate(options(input=directory), backend=backend)
    out, err = capsys.readouterr()
    header, lines = table(out)
    assert header == ['read_ID', 'barcode_call', 'samples'] + [
        side + '_' + column for side in ('start', 'end')
        for column in ('class', 'first', 'end', 'peak', 'share')]
    want = expected_rows(reads, (('start', STARTS), ('end', ENDS)))
    assert sorted(lines) == sorted(want.values()) and backend.batches == 2
    assert want['noise'][1] == 'none' and want['noise'][3:] == ['-'] * 10
    called = [row for row in want.values() if row[3] != '-']
    assert called
    for row in called:                       # a located side: a class, a range inside the read
        assert 0 <= int(row[4]) < int(row[5]) <= int(row[2]) and 0 < float(row[7]) <= 1
    assert '4 reads' in err
    shares = [float(row[7]) for row in called]
    assert 'start: {} located, median share '.format(len(called)) in err
    assert abs(float(err.split('start: ')[1].split('median share ')[1].split()[0]) -
               float(np.median(shares))) <= 0.006          # (the rows print two decimals)


def test_command_with_one_model_and_the_require_modes(oracle_backend, three_files, capsys):
    directory, reads = three_files
    capsys.readouterr()
    locate.locate(options(input=directory, start_model=None), backend=ref.HostBackend())
    header, lines = table(capsys.readouterr().out)
    assert header == ['read_ID', 'barcode_call', 'samples', 'end_class', 'end_first', 'end_end',
                      'end_peak', 'end_share']
    assert sorted(lines) == sorted(expected_rows(reads, (('end', ENDS),)).values())
    for mode in ('require_start', 'require_both'):
        given = dict(require_either=False, require_start=False, require_both=False)
        given[mode] = True
        capsys.readouterr()
        locate.locate(options(input=directory, **given), backend=ref.HostBackend())
        _, lines = table(capsys.readouterr().out)
        want = expected_rows(reads, (('start', STARTS), ('end', ENDS)), mode)
        assert sorted(lines) == sorted(want.values())


@pytest.mark.parametrize('given,message', [
    (dict(start_model=None, end_model=None), 'you must provide at least one model'),
    (dict(devices=2), 'a locate runs on one GPU'),
    (dict(input=os.path.join(GOLD, 'training_data.txt')), 'cannot be located'),
    (dict(batch_size=0), '--batch_size must be at least 1'),
    (dict(scan_size=6000.0), '--scan_size must be a multiple of half the model input size'),
])
def test_command_refusals(oracle_backend, given, message):
    with pytest.raises(SystemExit) as e:
        locate.locate(options(**given), backend=ref.HostBackend())
    assert message in str(e.value)
    if 'input' in given:                          # the training-data file: one line
        assert '\n' not in str(e.value)


def test_command_line_entry(monkeypatch):
    seen = {}
    monkeypatch.setattr(locate, 'locate', lambda args: seen.update(vars(args)))
    cli.main(['locate', '--native', 'some_dir'])
    assert seen['scan_size'] == 6144 and seen['score_diff'] == 0.5 and seen['require_either']
    assert os.path.basename(seen['start_model']).startswith('EXP-NBD103_read_starts')
    assert os.path.basename(seen['end_model']).startswith('EXP-NBD103_read_ends')
    assert seen['batch_size'] == 256 and not seen['multi_read'] and seen['devices'] == 0
    cli.main(['locate', '-s', STARTS, '--multi_read', 'some_dir'])
    assert seen['multi_read'] and seen['end_model'] is None
    with pytest.raises(SystemExit) as e:
        cli.main(['locate', 'some_dir'])
    assert 'you must provide at least one model' in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(['locate', '-s', STARTS, '--require_both', 'some_dir'])
    assert 'can only be used with two models' in str(e.value)
    for refused in ('prep', 'train'):
        with pytest.raises(SystemExit) as e:
            cli.main([refused])
        assert 'not part of this build' in str(e.value) and 'scan and locate' in str(e.value)


# ---- 5: the C ABI without a device -----------------------------------------------------------------
def test_symbols_are_exported_and_listed():
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in hip_backend.EXPORTED_SYMBOLS, name
    header = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    section = header[header.index('---- locate:'):header.index('---- compressed input')]
    for cite in ('classify.py:330-357', 'network_architecture.py:91-93', '0.5f * peak'):
        assert cite in section
    assert hip_backend.LOCATION == ref.LOCATION and hip_backend.LOCATION.itemsize == 48


def test_bad_arguments_are_refused_before_any_device_work():
    lib = hip_backend.load_library()
    # the device entry: 1 stands for a device pointer nobody may touch
    good = [1, 1, 1, 4, 12, 8, 13, 1024, 0, 1, None]
    for at, bad in ((0, None), (1, None), (2, None), (3, -1), (4, 0), (4, -3), (5, 7), (5, 9),
                    (6, 1), (6, 257), (7, 1023), (7, 94), (7, 16386), (8, 2), (8, -1), (9, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_locate_dev(*args) == INVALID, (at, bad)
    assert lib.dbh_locate_dev(*(good[:3] + [0] + good[4:])) == 0                 # no read
    # the host entry: the same checks, offsets that run backwards, and buffers untouched
    ev = np.ones((2, 12, 8, 13), np.float32)
    calls = np.array([1, 2], np.int32)
    offsets = np.array([0, 3000, 9000], np.int64)
    out = np.full(2, 7, dtype=ref.LOCATION)
    good = [ev.ctypes.data, calls.ctypes.data, offsets.ctypes.data, 2, 12, 8, 13, 1024, 1,
            out.ctypes.data]
    for at, bad in ((0, None), (1, None), (2, None), (3, -1), (4, 0), (5, 16), (6, 300), (7, 2048),
                    (8, 5), (9, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_locate_host(*args) == INVALID, (at, bad)
    backwards = np.array([0, 3000, 2000], np.int64)
    assert lib.dbh_locate_host(*(good[:2] + [backwards.ctypes.data] + good[3:])) == INVALID
    assert (out['cls'] == 7).all()
    assert lib.dbh_locate_host(*good) == 0 and (out['cls'] == calls).all()
    # the entries that take a model: none given
    n, size = ctypes.c_int64(-7), ctypes.c_size_t(7)
    assert lib.dbh_evidence_floats(None, ctypes.byref(n)) == INVALID and n.value == -7
    assert lib.dbh_evidence_dev(None, 1, 4, 1, 1, None) == INVALID
    assert lib.dbh_locate_workspace_bytes(None, 4, 1024, ctypes.byref(size)) == INVALID
    assert size.value == 7
    assert lib.dbh_locate_i16(None, 1, offsets.ctypes.data, 2, 0, 1024, 0.5, 1, 1, 1) == INVALID
