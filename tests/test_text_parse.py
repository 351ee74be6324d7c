"""Training-data text parsed in blocks, without a device: the CPU model of
the kernel (dbh_text_parse_host, csrc/dbh_text_core.h) against the regular-expression restatement
of tests/text_parse_reference.py; the two facts that make the block route equal to the host's (T1:
a strict line is read by the host's parser with the same label and values; T2: the host raises at
the first line it refuses, from that line alone); read_training_data with the model as its block
parser against parse='host'; and classify on a training-data file on both routes."""
import ctypes
import io
import os
import random

import numpy as np
import pytest

import text_parse_reference as tr
from conftest import GOLD, MODEL_DIR
from deepbinner_amd import hip_backend

model = hip_backend.parse_training_text_host


# ---- the model against the restatement -------------------------------------------------------------
def test_model_equals_the_restatement_on_the_corpus():
    seen = 0
    for name, data, input_size, _ in tr.blocks():
        tr.same_as_restatement(model(data, input_size), data, input_size)
        seen += 1
    assert seen > 16 * 50


def test_the_corpus_meets_every_seam():
    """-32768 begins at each of the seven places around the step seam (six splits and whole), and
    at every place of a 16-byte piece"""
    starts = set()
    for shift in range(16):
        base_rel = shift                     # the line's first byte, from its 16-byte boundary
        starts.update(base_rel + 2 + 7 * i for i in range(tr.SEAM_VALUES))
    assert set(range(1018, 1025)) <= starts and set(range(2042, 2049)) <= starts
    assert {s % 16 for s in starts} == set(range(16))
    kinds = {}
    for _, lines, input_size in tr.corpus():
        for line in lines:
            kinds[tr.line_kind(line, input_size)[0]] = kinds.get(tr.line_kind(line, input_size)[0], 0) + 1
    assert all(kinds.get(k, 0) >= 5 for k in (tr.OK, tr.FORM, tr.COUNT, tr.RANGE))


@pytest.mark.parametrize('refused', tr.MANY_VARIANTS, ids=str)
def test_model_equals_the_restatement_on_more_lines_than_the_grid_has_waves(refused):
    """70,000 lines: the device is held to this model on them (tests/test_gpu_text_parse.py)"""
    data = tr.many_lines(refused)
    got = model(data, tr.MANY_SIZE)
    tr.same_as_restatement(got, data, tr.MANY_SIZE)
    assert len(got[2]) == tr.MANY_LINES and got[3] == refused[0]
    assert np.flatnonzero(got[2]).tolist() == list(refused)
    assert [int(got[2][k]) for k in refused] == [tr.REFUSED[k][0] for k in refused]


@pytest.mark.parametrize('shift', tr.LONG_SHIFTS)
@pytest.mark.parametrize('input_size', tr.LONG_SIZES)
def test_model_equals_the_restatement_on_long_lines(input_size, shift):
    """lines of 100,003 and of 2^20 values - hundreds and thousands of 1,024-byte steps - OK, with
    a value out of range near the end, and a value short.  At shift > 0 the line that block() puts
    in front is itself refused (it is never strict), so first_bad is 0 there and the RANGE line is
    the first refused one behind it."""
    lines, values = tr.long_lines(input_size)
    data, skipped = tr.block(lines, shift)
    assert len(lines[0]) > 4 * input_size > 115 * 1024
    got = model(data, input_size)
    tr.same_as_restatement(got, data, input_size)
    assert got[2][skipped:].tolist() == [tr.OK, tr.RANGE, tr.COUNT]
    assert got[3] == (0 if skipped else 1) and np.flatnonzero(got[2][skipped:])[0] == 1
    assert got[0][skipped].tolist() == values


def test_the_long_lines_meet_every_seam():
    """in each long OK line, at each alignment it is run at, a value begins at every place of a
    1,024-byte step - so at each of the places around the step seam, split every way, and at
    every place of a 16-byte piece - and the value out of range lies in the line's last step"""
    for input_size in tr.LONG_SIZES:
        lines, _ = tr.long_lines(input_size)
        text = np.frombuffer(lines[0], dtype=np.uint8)
        separators = np.flatnonzero((text == ord(',')) | (text == ord('\t')))
        for shift in tr.LONG_SHIFTS:
            starts = shift + separators + 1          # from the 16-byte boundary the walk begins at
            assert np.unique(starts % 1024).size == 1024
            steps = (shift + len(lines[1]) + 1023) // 1024
            assert steps > 115 and (shift + lines[1].rindex(b'40000')) // 1024 == steps - 1


def test_kinds_come_in_order():
    data = b'x\t99999\n1\t99999\n1\t99999,1\n1\t1,2\n'
    samples, labels, kinds, first_bad = model(data, 2)
    assert kinds.tolist() == [tr.FORM, tr.COUNT, tr.RANGE, tr.OK] and first_bad == 0
    assert samples[3].tolist() == [1, 2] and labels[3] == 1
    assert model(b'4\t1,2\n', 2)[3] == -1


def test_max_lines_is_a_bound_not_a_hint():
    data = b'\n' * 9 + b'1\t5\n'
    got = model(data, 1, max_lines=10)
    assert got[2].tolist() == [tr.FORM] * 9 + [tr.OK] and got[3] == 0
    # the wrapper's own bound (strict lines only) is too small here: it asks again with the count
    assert np.array_equal(model(data, 1)[2], got[2])


# ---- T1 and T2 -------------------------------------------------------------------------------------
def test_t1_the_host_reads_strict_lines_the_same(tmp_path):
    rng = random.Random(1)
    lines = [tr.random_strict_line(rng, 24, crlf=rng.random() < 0.2) for _ in range(2000)]
    data = b''.join(line + b'\n' for line in lines)
    samples, labels, kinds, first_bad = model(data, 24)
    assert first_bad == -1 and not kinds.any()
    path = tmp_path / 'strict.txt'
    path.write_bytes(data)
    host_samples, host_labels = hip_backend.read_training_data(str(path), parse='host')
    assert host_samples.dtype == samples.dtype and host_labels.dtype == labels.dtype
    assert np.array_equal(host_samples, samples) and np.array_equal(host_labels, labels)


def outcome(call):
    try:
        samples, labels = call()
    except Exception as e:                      # whatever it is, the other route must raise it too
        return type(e), str(e)
    return samples.dtype, samples.tolist(), labels.dtype, labels.tolist()


def test_t2_the_host_raises_from_the_refused_line_alone(tmp_path):
    good = [b'1\t1,2,3', b'2\t4,5,6', b'0\t7,8,9']
    for k, bad in enumerate((b'1\t2\t3', b'x\t1,2,3', b'1\t1,2', b'1\t1,2,99999', b'1\t1,,3', b'')):
        outcomes = set()
        for front in (good[:1], good, good[1:] + good):
            path = tmp_path / 'same_name.txt'
            path.write_bytes(b''.join(line + b'\n' for line in front + [bad] + good + [b'garbage']))
            kind, text = outcome(lambda: hip_backend.read_training_data(str(path), parse='host'))
            assert kind is hip_backend.TrainingDataError
            outcomes.add(text.replace('line {} of'.format(len(front) + 1), 'line N of'))
        assert len(outcomes) == 1, (k, outcomes)


# ---- the two routes of read_training_data -----------------------------------------------------------
def routes_equal(path, input_size=None, block_bytes=None, messages=None):
    host = outcome(lambda: hip_backend.read_training_data(str(path), input_size, messages,
                                                          parse='host'))
    blocks = outcome(lambda: hip_backend.read_training_data(
        str(path), input_size, messages, parse='gpu', block_parser=model, block_bytes=block_bytes))
    assert host == blocks, (path, host[:2], blocks[:2])
    return host


def row(label, values):
    return ('%s\t%s' % (label, ','.join(str(v) for v in values))).encode()


def write(path, lines, end=b'\n'):
    path.write_bytes(b''.join(line + b'\n' for line in lines[:-1]) + lines[-1] + end)
    return path


def test_routes_equal_on_the_files_of_the_fit_commands_error_texts(tmp_path):
    from deepbinner_amd.fit import MESSAGES
    good = [row(1 + i % 3, range(i, i + 96)) for i in range(20)]
    files = {'train': good, 'a': good + [row('x', range(96))], 'b': [b'1\t2\t3'] + good,
             'c': good[:5] + [row(1, range(98))] + good[5:], 'd': good[:15],
             'f': good[:17] + [row(2, [40000] + list(range(95)))] + good[18:],
             'g': good * 6 + [row(1, range(98))]}
    for name, lines in files.items():
        path = write(tmp_path / (name + '.txt'), lines)
        for block_bytes in (None, 1500):
            for messages in (None, MESSAGES):
                got = routes_equal(path, block_bytes=block_bytes, messages=messages)
                assert (got[0] is hip_backend.TrainingDataError) == (name in 'abcfg')
        routes_equal(path, input_size=98)
    got = routes_equal(tmp_path / 'f.txt')
    assert got[1] == 'line 18 of {} holds signal values outside the int16 range'.format(tmp_path / 'f.txt')


def test_routes_equal_on_the_golden_training_data():
    path = os.path.join(GOLD, 'training_data.txt')
    got = routes_equal(path)
    assert got[0] == np.int16 and len(got[1]) > 0
    routes_equal(path, block_bytes=1 << 16)


@pytest.mark.parametrize('where', ['block 0', 'a later block', 'the last line'])
def test_routes_equal_wherever_the_first_refused_line_is(tmp_path, where):
    good = [row(i % 4, range(i, i + 40)) for i in range(60)]
    at = {'block 0': 1, 'a later block': 41, 'the last line': 59}[where]
    for bad in (b'1\t5,6', b'1\t' + b','.join([b'70000'] * 40), b'q', b'1\t1,2\t3', b''):
        lines = good[:at] + [bad] + good[at + 1:]
        for end in (b'\n', b'', b'\r\n'):
            got = routes_equal(write(tmp_path / 'bad.txt', lines, end), block_bytes=2048)
            if bad or end or at != 59:
                assert got[0] is hip_backend.TrainingDataError, (bad, end, got[:2])
    assert routes_equal(write(tmp_path / 'good.txt', good, b''), block_bytes=2048)[0] == np.int16
    # a block cannot hold a line: the host's route, whatever the file holds
    routes_equal(write(tmp_path / 'good.txt', good), block_bytes=64)
    routes_equal(write(tmp_path / 'bad.txt', good[:7] + [b'x'] + good), block_bytes=64)


def test_routes_equal_where_python_takes_what_the_grammar_refuses(tmp_path):
    good = [row(i % 4, range(i, i + 12)) for i in range(30)]
    values = ','.join(str(v) for v in range(12))
    lenient = ['+1\t' + values, '01\t' + values, ' 5\t' + values, '1\t' + values + ' ',
               '1\t ' + values, '1\t' + values.replace('11', '00000011'), '1\t' + values + '\t',
               '1_0\t' + values, '1\t' + values.replace('10', '1_0'),
               '٣\t' + values, '1\t' + values.replace('7', '٧'),
               '1\t' + values.replace(',', ' ,', 1), '--1\t' + values, '+-1\t' + values]
    for text in lenient:
        for at in (0, 3, 29):
            lines = good[:at] + [text.encode('utf-8')] + good[at + 1:]
            routes_equal(write(tmp_path / 'lenient.txt', lines), block_bytes=512)
    # a lone CR ends a line for Python's reader; bytes that are no UTF-8; a NUL
    for raw in (b'\r'.join(good[:5]) + b'\n', good[0] + b'\n' + good[1] + b'\r' + good[2] + b'\n',
                good[0] + b'\n1\t\xc3,5\n', good[0] + b'\nx\n' + good[1] + b'\n\xc3\x28\n',
                b'\n'.join(good) + b'\nx\n' + b'\n'.join(good * 30) + b'\n\xff\n',
                good[0] + b'\n1\t\x005\n', good[0] + b'\r\r\n' + good[1] + b'\n',
                good[0] + b'\r' + b'x\n', b'\n', b'\r\n', b'\n' + good[0] + b'\n'):
        path = tmp_path / 'raw.txt'
        path.write_bytes(raw)
        routes_equal(path, block_bytes=700)


def test_routes_equal_on_the_empty_file(tmp_path):
    path = tmp_path / 'empty.txt'
    path.write_bytes(b'')
    got = routes_equal(path)
    assert got == (hip_backend.TrainingDataError, 'training signal not formatted correctly')


def test_parse_follows_the_environment(tmp_path, monkeypatch):
    path = write(tmp_path / 'two.txt', [b'1\t1,2', b'2\t3,4'])
    calls = []

    def parser(data, input_size):
        calls.append(len(data))
        return model(data, input_size)

    monkeypatch.setattr(hip_backend._training_file, 'parse_training_text', parser)
    monkeypatch.delenv('DEEPBINNER_TEXT_PARSE', raising=False)
    hip_backend.read_training_data(str(path))
    monkeypatch.setenv('DEEPBINNER_TEXT_PARSE', 'host')
    hip_backend.read_training_data(str(path))
    assert not calls
    monkeypatch.setenv('DEEPBINNER_TEXT_PARSE', 'gpu')
    assert hip_backend.read_training_data(str(path))[0].tolist() == [[1, 2], [3, 4]]
    assert calls == [12]
    hip_backend.read_training_data(str(path), parse='host')
    assert calls == [12]
    monkeypatch.setenv('DEEPBINNER_TEXT_PARSE', 'cpu')
    with pytest.raises(ValueError):
        hip_backend.read_training_data(str(path))


def test_fit_has_the_switch_and_passes_it_on(tmp_path, monkeypatch):
    from deepbinner_amd import deepbinner as cli
    from deepbinner_amd import fit
    argv = ['fit', '--train', 't', '--val', 'v', '--model_out', 'm']
    assert cli.build_parser().parse_args(argv).parse is None
    assert cli.build_parser().parse_args(argv + ['--parse', 'gpu']).parse == 'gpu'
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(argv + ['--parse', 'cpu'])
    seen = []
    monkeypatch.setattr(hip_backend._training_file, 'parse_training_text',
                        lambda data, n: seen.append(n) or model(data, n))
    path = str(write(tmp_path / 'two.txt', [b'1\t1,2', b'2\t3,4']))
    assert fit.load_data(path, parse='gpu')[1].tolist() == [1, 2] and seen == [2]
    assert fit.load_data(path, 2, parse='host')[1].tolist() == [1, 2] and seen == [2]
    with pytest.raises(SystemExit) as e:
        fit.load_data(path, 3, parse='gpu')
    assert str(e.value) == 'Error: inconsistent signal sizes in training data'


# ---- a line's result does not depend on the block it is in -----------------------------------------
def test_split_invariance():
    lines = []
    for name, case, input_size in tr.corpus():
        if input_size in (2, 5):
            lines += case
    rng = random.Random(3)
    lines += [tr.random_strict_line(rng, 2) for _ in range(10)]
    whole = model(b''.join(line + b'\n' for line in lines), 2)
    assert len(whole[2]) == len(lines) and whole[3] == np.flatnonzero(whole[2])[0] > 0
    for cut in range(1, len(lines)):
        parts = [model(b''.join(line + b'\n' for line in piece), 2)
                 for piece in (lines[:cut], lines[cut:])]
        kinds = np.concatenate([p[2] for p in parts])
        assert np.array_equal(kinds, whole[2])
        ok = kinds == tr.OK
        assert np.array_equal(np.concatenate([p[0] for p in parts])[ok], whole[0][ok])
        assert np.array_equal(np.concatenate([p[1] for p in parts])[ok], whole[1][ok])
        bad = [p[3] + at for p, at in zip(parts, (0, cut)) if p[3] >= 0]
        assert bad[0] == whole[3]


# ---- classify on a training-data file ---------------------------------------------------------------
@pytest.mark.parametrize('first_label', ['3', '+1'])
def test_classify_prints_the_same_on_both_routes(oracle_backend, gold, tmp_path, capsys, monkeypatch,
                                                 first_label):
    import argparse
    classify = oracle_backend
    path = tmp_path / 'train.txt'
    with open(path, 'w') as f:
        for label, sig in ((first_label, gold['signals'][0]), ('2', gold['signals'][1]),
                           ('0', gold['signals'][2])):
            f.write('%s\t%s\n' % (label, ','.join(str(int(v)) for v in sig[:1500])))
    models = classify.load_and_check_models(os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw'),
                                            None, 6144, out_dest=io.StringIO())[:5]
    args = argparse.Namespace(verbose=True, batch_size=2, scan_size=6144, score_diff=0.5,
                              require_either=False, require_start=False, require_both=False)
    parsed = []
    monkeypatch.setattr(hip_backend._training_file, 'parse_training_text',
                        lambda data, n: parsed.append(n) or model(data, n))
    printed = {}
    for route in ('host', 'gpu'):
        monkeypatch.setenv('DEEPBINNER_TEXT_PARSE', route)
        capsys.readouterr()
        classify.classify_training_data(str(path), *models, args)
        printed[route] = capsys.readouterr()
    assert parsed == [1500]
    assert printed['host'].out == printed['gpu'].out and printed['host'].err == printed['gpu'].err
    assert printed['host'].out.splitlines()[1].startswith('line_1_barcode_%s\t' % first_label)


# ---- argument errors, before any device work --------------------------------------------------------
@pytest.mark.parametrize('entry', ['dbh_text_parse', 'dbh_text_parse_host'])
def test_argument_errors(entry):
    lib = hip_backend.load_library()
    fn = getattr(lib, entry)
    data = b'1\t5,6\n'
    samples, labels = np.full((4, 2), 77, dtype=np.int16), np.full(4, 77, dtype=np.int32)
    kinds = np.full(4, 77, dtype=np.uint8)
    n_lines, first_bad = ctypes.c_int64(-5), ctypes.c_int64(-5)

    def call(block=data, n_bytes=len(data), input_size=2, max_lines=4, out=None):
        out = out or [samples.ctypes.data, labels.ctypes.data, kinds.ctypes.data,
                      ctypes.byref(n_lines), ctypes.byref(first_bad)]
        return fn(block, n_bytes, input_size, max_lines, *out)

    INVALID, UNSUPPORTED = 1, 5
    assert call(block=None) == INVALID
    full = [samples.ctypes.data, labels.ctypes.data, kinds.ctypes.data, ctypes.byref(n_lines),
            ctypes.byref(first_bad)]
    for missing in range(5):
        assert call(out=full[:missing] + [None] + full[missing + 1:]) == INVALID
    assert call(input_size=0) == INVALID and call(input_size=-3) == INVALID
    assert call(n_bytes=-1) == INVALID and call(max_lines=-1) == INVALID
    assert call(input_size=(1 << 20) + 1) == UNSUPPORTED
    assert call(n_bytes=(1 << 30) + 1) == UNSUPPORTED
    assert call(n_bytes=0) == INVALID
    assert call(n_bytes=len(data) - 1) == INVALID            # the block does not end in a LF
    assert call(block=b'1\t5,6', n_bytes=5) == INVALID
    assert (samples == 77).all() and (labels == 77).all() and (kinds == 77).all()
    assert first_bad.value == -5
    if entry == 'dbh_text_parse_host':
        # more lines than the arrays hold: the count comes back, nothing is written
        assert call(block=data * 5, n_bytes=5 * len(data)) == INVALID
        assert n_lines.value == 5 and (samples == 77).all() and (kinds == 77).all()
        assert call(input_size=1 << 20, max_lines=0) == INVALID and n_lines.value == 1
        assert call() == 0 and n_lines.value == 1 and first_bad.value == -1
        assert samples[0].tolist() == [5, 6] and (samples[1:] == 77).all()
