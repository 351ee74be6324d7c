#!/usr/bin/env python3
"""
Records what the reference's ``balance`` and ``refine`` write, for tests/test_balance.py and
tests/test_refine.py:    python tools/make_balance_golden.py /path/to/reference

The reference's ``deepbinner/balance.py`` and ``deepbinner/refine.py`` run as they are, on small
inputs that this script writes: ``random.seed(k)`` in front of each run, ``--random_signal 0``
(the random signals are this package's own law), and an empty stand-in module
named ``noise``, which balance.py imports and, without random signals, never calls.  The runs
happen inside the fixture directory with relative file names, so that the recorded stderr names no
place.  Output, data only: tests/golden/balance/{a,b,c}.txt and cases.json,
tests/golden/refine/{training.txt,classes.tsv} and case.json.
"""
import argparse
import contextlib
import importlib
import io
import json
import os
import random
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALANCE = os.path.join(REPO, 'tests', 'golden', 'balance')
REFINE = os.path.join(REPO, 'tests', 'golden', 'refine')
SIGNAL_SIZE = 12

# name -> the labels of its lines, in order
INPUTS = {
    'a.txt': [1, 2, 0, 3, 1, 1, 2, 0, 3, 3, 1, 2, 2, 0, 1, 3, 2, 1, 0, 3, 1, 2, 3, 1, 0, 2, 1, 3, 1, 2],
    'b.txt': [3, 3, 2, 1, 0, 0, 2, 3, 1, 2, 3, 3, 0, 1, 2, 3, 2, 0, 1, 3, 3, 2],
    'c.txt': [2, 0, 1, 1, 2, 0, 0, 1, 2, 1, 0, 2, 1, 1, 0, 2],           # no barcode 3
}
CASES = [
    {'name': 'two files, seed 0', 'files': ['a.txt', 'b.txt'], 'barcodes': None, 'seed': 0},
    {'name': 'three files, seed 1', 'files': ['a.txt', 'b.txt', 'c.txt'], 'barcodes': None, 'seed': 1},
    {'name': 'three files in another order, seed 2', 'files': ['c.txt', 'a.txt', 'b.txt'],
     'barcodes': None, 'seed': 2},
    {'name': 'a barcode that no file has', 'files': ['a.txt', 'b.txt'], 'barcodes': '7', 'seed': 0},
    {'name': 'one barcode asked for', 'files': ['b.txt', 'c.txt'], 'barcodes': '2', 'seed': 1},
]
# refine: (label, the table's call); the table names its reads as classify does
REFINE_LINES = [(1, '1'), (2, 'none'), (0, 'none'), (3, '2'), (3, '3'), (0, '1'), (12, '12'), (2, '2')]


def write_inputs():
    rng = np.random.RandomState(20181)
    os.makedirs(BALANCE, exist_ok=True)
    os.makedirs(REFINE, exist_ok=True)
    for name, labels in INPUTS.items():
        with open(os.path.join(BALANCE, name), 'w') as out:
            for label in labels:
                values = rng.randint(-40, 1200, size=SIGNAL_SIZE)
                out.write('{}\t{}\n'.format(label, ','.join(str(v) for v in values)))
    with open(os.path.join(REFINE, 'training.txt'), 'w') as out, \
            open(os.path.join(REFINE, 'classes.tsv'), 'w') as table:
        table.write('read_ID\tbarcode_call\n')
        for k, (label, call) in enumerate(REFINE_LINES, 1):
            values = rng.randint(-40, 1200, size=SIGNAL_SIZE)
            out.write('{}\t{}\n'.format(label, ','.join(str(v) for v in values)))
            table.write('line_{}_barcode_{}\t{}\n'.format(k, label, call))


def captured(run, where):
    out, err = io.StringIO(), io.StringIO()
    here = os.getcwd()
    os.chdir(where)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            run()
    finally:
        os.chdir(here)
    return out.getvalue(), err.getvalue()


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[1])
    parser.add_argument('reference', help="the reference's source tree (holds deepbinner/balance.py)")
    reference = os.path.abspath(parser.parse_args().reference)
    sys.modules['noise'] = types.ModuleType('noise')
    sys.path.insert(0, reference)
    balance = importlib.import_module('deepbinner.balance')
    refine = importlib.import_module('deepbinner.refine')
    write_inputs()

    cases = []
    for case in CASES:
        args = argparse.Namespace(training_data=case['files'], barcodes=case['barcodes'],
                                  random_signal=0.0)
        random.seed(case['seed'])
        stdout, stderr = captured(lambda: balance.balance_training_samples(args), BALANCE)
        cases.append(dict(case, stdout=stdout, stderr=stderr))
    with open(os.path.join(BALANCE, 'cases.json'), 'w') as out:
        json.dump(cases, out, indent=1)

    args = argparse.Namespace(training_data='training.txt', classification_data='classes.tsv')
    stdout, stderr = captured(lambda: refine.refine_training_samples(args), REFINE)
    with open(os.path.join(REFINE, 'case.json'), 'w') as out:
        json.dump({'stdout': stdout, 'stderr': stderr}, out, indent=1)
    print('wrote {} balance cases and one refine case'.format(len(cases)))


if __name__ == '__main__':
    main()
