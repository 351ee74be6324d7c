"""``deepbinner refine`` (deepbinner_amd/refine.py) without a device: the
reference's form against what the reference wrote (tests/golden/refine, recorded by
tools/make_balance_golden.py), and the fused ``--model`` form against the two-step form, with the
network run by the NumPy oracle."""
import json
import os

import pytest

from deepbinner_amd import deepbinner as cli
from refine_fixtures import REFINE, START_MODEL, fused_equals_two_step


def test_the_references_form_is_the_references_bytes(capfd, monkeypatch):
    with open(os.path.join(REFINE, 'case.json')) as f:
        want = json.load(f)
    monkeypatch.chdir(REFINE)
    capfd.readouterr()
    cli.main(['refine', 'training.txt', 'classes.tsv'])
    got = capfd.readouterr()
    assert got.out == want['stdout'] and len(got.out.splitlines()) == 5
    # stderr: the reference's bytes with the progress states between heading and final state left out
    states = want['stderr'].split('\r')
    assert states[0] == '\nRefining training data\n' and states[-1] == 'Matches: 5 / 8 (62.50%)\n\n'
    assert got.err == states[0] + '\r' + states[-1]


def test_misaligned_files_name_the_line(capfd, tmp_path, monkeypatch):
    monkeypatch.chdir(REFINE)
    with open('classes.tsv') as f:
        rows = f.read().splitlines()
    rows[3], rows[4] = rows[4], rows[3]                   # lines 3 and 4 of the data swapped
    table = tmp_path / 'swapped.tsv'
    table.write_text('\n'.join(rows) + '\n')
    with pytest.raises(SystemExit) as e:
        cli.main(['refine', 'training.txt', str(table)])
    assert 'line 3 of the training data' in str(e.value) and 'line_4_barcode_3' in str(e.value)
    assert len(capfd.readouterr().out.splitlines()) == 1          # what matched in front of it


def test_a_table_or_a_model_but_not_both(capfd, monkeypatch):
    monkeypatch.chdir(REFINE)
    for argv in (['refine', 'training.txt'],
                 ['refine', 'training.txt', 'classes.tsv', '--model', START_MODEL]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert 'either a classification file or --model' in str(e.value)
    assert capfd.readouterr().out == ''


def test_the_fused_form_equals_the_two_step_form(oracle_backend, gold, tmp_path, capfd):
    fused_equals_two_step(gold, tmp_path, capfd)
