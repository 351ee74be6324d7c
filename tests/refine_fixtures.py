"""A helper, not a test: what tests/test_refine.py and tests/test_gpu_balance.py share."""
import os

from conftest import GOLD, MODEL_DIR
from deepbinner_amd import deepbinner as cli

REFINE = os.path.join(GOLD, 'refine')
START_MODEL = os.path.join(MODEL_DIR, 'EXP-NBD103_read_starts.dbw')


def fused_equals_two_step(gold, tmp_path, capfd):
    """classify, refine with its table, refine --model: the same lines kept, some and not all
    (tests/test_gpu_balance.py runs this on the device as well)"""
    calls = gold['calls']['EXP-NBD103_read_starts/start']
    # the label of every second line is its read's call, the others' one beside it
    lines = []
    for k in range(4):
        call = 0 if calls[k] == 'none' else int(calls[k])
        label = call if k % 2 == 0 else call % 12 + 1
        lines.append('%d\t%s\n' % (label, ','.join(str(int(v)) for v in gold['signals'][k][:2000])))
    training = tmp_path / 'training.txt'
    training.write_text(''.join(lines))

    capfd.readouterr()
    cli.main(['classify', '-s', START_MODEL, str(training)])
    table = tmp_path / 'calls.tsv'
    table.write_text(capfd.readouterr().out)
    cli.main(['refine', str(training), str(table)])
    two_step = capfd.readouterr()
    cli.main(['refine', '--model', START_MODEL, str(training)])
    fused = capfd.readouterr()
    assert fused.out == two_step.out
    kept = fused.out.splitlines(keepends=True)
    assert 0 < len(kept) < 4 and all(line in lines for line in kept)
    assert fused.err.split('\r')[-1] == two_step.err.split('\r')[-1]
    assert 'Classifying training data' in fused.err and 'Refining training data' in fused.err
