"""``balance`` and ``refine --model`` through the real device route: the
random signals generated and formatted on the GPU, chunk by chunk, equal the same command on the
host models byte for byte; the fused refine equals the two-step form."""
import argparse

import numpy as np
import pytest

from deepbinner_amd import balance
from refine_fixtures import fused_equals_two_step

pytestmark = pytest.mark.gpu


def test_balance_on_the_device_equals_the_host_models(hip, tmp_path, capfd, monkeypatch):
    # two files of 1,024-value samples, 25 and 15 of each of three labels: 40 is the smallest count
    filler = hip.random_signals(21, 0, 120, 1024, host=True)
    names = []
    for name, rows, per_label in (('one.txt', filler[:75], 25), ('two.txt', filler[75:], 15)):
        labels = np.arange(3 * per_label, dtype=np.int32) % 3
        hip.write_training_data(str(tmp_path / name), labels, rows, host=True)
        names.append(str(tmp_path / name))
    monkeypatch.setattr(balance, 'TEXT_CHUNK_BYTES', 16 * (12 + 7 * 1024))
    assert balance.chunk_signals(1024) == 16               # 40 signals: chunks of 16, 16 and 8
    args = argparse.Namespace(training_data=names, barcodes=None, random_signal=1.0, seed=6)

    chunks = []
    made = hip.ResidentText.random_signals

    def counted(self, seed, first, n, size=None):
        chunks.append(n)
        return made(self, seed, first, n, size)

    monkeypatch.setattr(hip.ResidentText, 'random_signals', counted)
    capfd.readouterr()
    balance.balance(args)                                  # the command's own device route
    device = capfd.readouterr()
    assert chunks == [16, 16, 8]
    balance.balance(args, signals=lambda *a: hip.random_signals(*a, host=True),
                    formatter=lambda l, s: hip.format_training_text(l, s, host=True))
    host = capfd.readouterr()
    assert device.out == host.out and device.err == host.err
    lines = device.out.splitlines()
    assert len(lines) == 160 and 'Adding 40 random signals' in device.err
    assert all(line.startswith('0\t') for line in lines[120:])
    monkeypatch.undo()
    capfd.readouterr()
    balance.balance(args)                                   # one chunk
    assert capfd.readouterr().out == host.out


def test_refine_with_a_model_equals_the_two_step_form(hip, gold, tmp_path, capfd):
    fused_equals_two_step(gold, tmp_path, capfd)
