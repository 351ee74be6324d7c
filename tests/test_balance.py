"""``deepbinner balance`` (deepbinner_amd/balance.py) without a device: the
selection against what the reference wrote (tests/golden/balance, recorded by
tools/make_balance_golden.py with ``--random_signal 0``), byte for byte on stdout and stderr, and
the random signals through the host models of generator and formatter."""
import argparse
import json
import os

import numpy as np
import pytest

from conftest import GOLD
from deepbinner_amd import balance, hip_backend
from deepbinner_amd import deepbinner as cli

BALANCE = os.path.join(GOLD, 'balance')
with open(os.path.join(BALANCE, 'cases.json')) as f:
    CASES = json.load(f)


def host_signals(seed, first, n, size):
    return hip_backend.random_signals(seed, first, n, size, host=True)


def host_formatter(labels, samples):
    return hip_backend.format_training_text(labels, samples, host=True)


def run(capfd, files, seed=0, random_signal=0.0, barcodes=None):
    args = argparse.Namespace(training_data=files, barcodes=barcodes, random_signal=random_signal,
                              seed=seed)
    capfd.readouterr()
    balance.balance(args, signals=host_signals, formatter=host_formatter)
    return capfd.readouterr()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_the_selection_is_the_references(case, capfd, monkeypatch):
    monkeypatch.chdir(BALANCE)
    argv = ['balance'] + case['files'] + ['--random_signal', '0', '--seed', str(case['seed'])]
    if case['barcodes'] is not None:
        argv += ['--barcodes', case['barcodes']]
    capfd.readouterr()
    cli.main(argv)                                        # no random signals: no device is touched
    got = capfd.readouterr()
    assert got.out == case['stdout'] and got.err == case['stderr']


def test_the_golden_cases_cover_what_they_should():
    by_name = {c['name']: c for c in CASES}
    assert len({c['seed'] for c in CASES}) == 3
    assert {len(c['files']) for c in CASES} == {2, 3}
    assert 'barcode 03: 0' in by_name['three files, seed 1']['stderr']          # c.txt has none
    nothing = by_name['a barcode that no file has']
    assert nothing['stdout'] == '' and 'Smallest count = 0 (barcode 07)' in nothing['stderr']


def test_barcodes_are_split_at_commas(capfd, monkeypatch):
    monkeypatch.chdir(BALANCE)
    got = run(capfd, ['a.txt', 'b.txt'], barcodes='1,2')
    assert 'Including user-specified barcodes in output: 0, 1, 2\n' in got.err
    assert 'Smallest count = 9 (no barcode)' in got.err
    labels = [line.split('\t')[0] for line in got.out.splitlines()]
    assert sorted(labels) == ['0'] * 9 + ['1'] * 9 + ['2'] * 9
    with pytest.raises(SystemExit) as e:
        run(capfd, ['a.txt'], barcodes='1,x')
    assert '--barcodes' in str(e.value)


def test_an_empty_file_and_mixed_sizes_are_errors(capfd, tmp_path, monkeypatch):
    monkeypatch.chdir(BALANCE)
    empty = tmp_path / 'empty.txt'
    empty.write_bytes(b'')
    with pytest.raises(SystemExit) as e:
        run(capfd, ['a.txt', str(empty)])
    assert 'is empty' in str(e.value)
    other = tmp_path / 'other.txt'
    other.write_bytes(b'1\t1,2,3\n')
    with pytest.raises(SystemExit) as e:
        run(capfd, ['a.txt', str(other)])
    assert str(e.value) == 'Error: multiple signal sizes detected: [3, 12]'


def test_random_signals_are_appended_as_no_barcode_lines(capfd, monkeypatch):
    monkeypatch.chdir(BALANCE)
    plain = run(capfd, ['a.txt', 'b.txt'], seed=4)
    got = run(capfd, ['a.txt', 'b.txt'], seed=4, random_signal=1.0)
    assert 'Adding 9 random signals as no-barcode training samples\n' in got.err
    assert got.out.startswith(plain.out)
    added = got.out[len(plain.out):].splitlines()
    assert len(added) == 9
    for line in added:
        label, values = line.split('\t')
        assert label == '0' and len(values.split(',')) == 12
    samples, labels, kinds, first_bad = hip_backend.parse_training_text_host(got.out.encode(), 12)
    assert first_bad == -1 and not kinds.any() and len(labels) == 4 * 9 + 9
    assert np.array_equal(samples[-9:], host_signals(4, 0, 9, 12))
    assert run(capfd, ['a.txt', 'b.txt'], seed=4, random_signal=1.0).out == got.out
    assert run(capfd, ['a.txt', 'b.txt'], seed=5, random_signal=1.0).out[-200:] != got.out[-200:]
    assert 'Adding 14 random signals' in run(capfd, ['a.txt', 'b.txt'], random_signal=1.5).err   # round(13.5)


def test_chunks_do_not_show_in_the_output(capfd, monkeypatch):
    monkeypatch.chdir(BALANCE)
    whole = run(capfd, ['a.txt', 'b.txt'], seed=2, random_signal=1.0).out
    monkeypatch.setattr(balance, 'TEXT_CHUNK_BYTES', 4 * (12 + 7 * 12))      # four signals a chunk
    assert balance.chunk_signals(12) == 4
    assert run(capfd, ['a.txt', 'b.txt'], seed=2, random_signal=1.0).out == whole
    monkeypatch.undo()
    assert balance.chunk_signals(1024) == (256 << 20) // 7180
    assert balance.chunk_signals(1) == (256 << 20) // 19 and balance.chunk_signals(2 ** 20) == 36
