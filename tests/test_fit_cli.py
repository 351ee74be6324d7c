"""The ``fit`` command on the CPU: its flags and defaults (the reference's ``train``,
deepbinner.py:246-269), the reference's error texts (train_network.py:28-124), the checkpoint policy
(Keras's ModelCheckpoint(monitor='val_acc', save_best_only=True, mode='max'),
train_network.py:62-63), and the whole loop against the fp64 NumPy stand-ins of
tests/feed_reference.py on the task tests/test_gpu_feed.py gives the device.
"""
import os

import numpy as np
import pytest

import feed_reference as fr
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import fit as fit_module
from deepbinner_amd import hip_backend
from deepbinner_amd.model_format import ModelWeights

def parse(argv):
    return cli.build_parser().parse_args(argv)


def write(path, lines):
    path.write_text(''.join(line + '\n' for line in lines))
    return str(path)


def row(label, values):
    return '{}\t{}'.format(label, ','.join(str(v) for v in values))


def host_fit(args, trainer_factory=fr.HostTrainer):
    fit_module.fit(args, trainer_factory=trainer_factory, dataset_factory=fr.HostDataset,
                   epoch_order=fr.epoch_order)


# ---- the command line ------------------------------------------------------------------------------
def test_flags_and_defaults():
    args = parse(['fit', '--train', 't', '--val', 'v', '--model_out', 'm'])
    assert (args.train, args.val, args.model_out, args.model_in) == ('t', 'v', 'm', None)
    assert (args.epochs, args.aug, args.batch_size, args.batches_per_epoch, args.seed) == \
        (100, 2.0, 20, 5000, 0)
    assert isinstance(args.aug, float)
    args = parse(['fit', '--train', 't', '--val', 'v', '--model_out', 'm', '--model_in', 'i',
                  '--epochs', '3', '--aug', '1', '--batch_size', '16', '--batches_per_epoch', '7',
                  '--seed', '5'])
    assert (args.model_in, args.epochs, args.aug, args.batch_size, args.batches_per_epoch,
            args.seed) == ('i', 3, 1.0, 16, 7, 5)
    for missing in ('--train', '--val', '--model_out'):
        argv = ['fit', '--train', 't', '--val', 'v', '--model_out', 'm']
        at = argv.index(missing)
        with pytest.raises(SystemExit):
            parse(argv[:at] + argv[at + 2:])


def test_train_is_still_refused_and_fit_is_dispatched(monkeypatch):
    with pytest.raises(SystemExit) as e:
        cli.main(['train', '--train', 't', '--val', 'v', '--model_out', 'm'])
    assert 'not part of this build' in str(e.value)
    seen = {}
    monkeypatch.setattr(fit_module, 'fit', lambda args: seen.update(vars(args)))
    cli.main(['fit', '--train', 't', '--val', 'v', '--model_out', 'm'])
    assert seen['train'] == 't' and seen['epochs'] == 100


def test_error_texts(tmp_path):
    good = [row(1 + i % 3, range(i, i + 96)) for i in range(20)]
    train = write(tmp_path / 'train.txt', good)
    out = str(tmp_path / 'out.dbw')

    def fails(message, train=train, val=train, extra=()):
        with pytest.raises(SystemExit) as e:
            host_fit(parse(['fit', '--train', train, '--val', val, '--model_out', out,
                            '--batch_size', '16', '--epochs', '1'] + list(extra)))
        assert message in str(e.value), str(e.value)
        assert not os.path.exists(out)

    fails('Error: a non-integer barcode class was encountered in ',
          train=write(tmp_path / 'a.txt', good + [row('x', range(96))]))
    fails('Error: training signal not formatted correctly',
          train=write(tmp_path / 'b.txt', ['1\t2\t3'] + good))
    fails('Error: inconsistent signal sizes in training data',
          train=write(tmp_path / 'c.txt', good[:5] + [row(1, range(98))] + good[5:]))
    fails('Error: the number of training samples is smaller than the batch size',
          train=write(tmp_path / 'd.txt', good[:15]))
    fails('Error: the number of validation samples is smaller than the batch size',
          val=write(tmp_path / 'e.txt', good[:15]))
    bad = write(tmp_path / 'f.txt', good[:17] + [row(2, [40000] + list(range(95)))] + good[18:])
    fails('Error: line 18 of {} holds signal values outside the int16 range'.format(bad), train=bad)
    fails('Error: line 18 of {} holds signal values outside the int16 range'.format(bad), val=bad)
    # beyond the first hundred lines the reference asserts; here it is the same message
    late = write(tmp_path / 'g.txt', good * 6 + [row(1, range(98))])
    fails('Error: inconsistent signal sizes in training data', train=late)

    other_size = str(tmp_path / 'size.dbw')
    ModelWeights.fresh(4, 130).save(other_size)
    fails('Error: the provided model\'s input size (130) is not equal to the training data\'s '
          'size (96)', extra=['--model_in', other_size])
    other_classes = str(tmp_path / 'classes.dbw')
    ModelWeights.fresh(5, 96).save(other_classes)
    fails('Error: the provided model\'s output classes (5) are not equal to the training data\'s '
          'classes (4)', extra=['--model_in', other_classes])
    fails('does not exist', extra=['--model_in', str(tmp_path / 'nothing.dbw')])
    # what the device entries would refuse, said before anything is loaded
    fails('Error: --aug must be 1 or more', extra=['--aug', '0.5'])
    fails('Error: --aug must be 1 or more', extra=['--aug', 'nan'])
    fails('Error: --epochs must be a positive integer', extra=['--epochs', '0'])
    fails('Error: --batches_per_epoch must be a positive integer', extra=['--batches_per_epoch', '0'])


# ---- the checkpoint policy -------------------------------------------------------------------------
class Scripted(fr.HostTrainer):
    """A trainer whose validation results are given; every step moves its weights a little, so
    that the epoch a file was saved in can be read off its first weight."""
    saved = []

    def run_epoch(self, dataset, indices, batch_size, augmentation):
        steps = len(indices) // batch_size
        self.state.iterations += steps
        self.state.flat = self.state.flat.copy()
        self.state.flat[0] = np.float32(self.state.iterations)
        return np.full(steps, 1.0), np.full(steps, batch_size // 2)

    def save_checkpoint(self, path):
        Scripted.saved.append(self.state.iterations)
        super().save_checkpoint(path)


def test_model_out_is_written_only_on_strict_improvement(tmp_path, capsys):
    lines = [row(1 + i % 3, range(i, i + 96)) for i in range(32)]
    train = write(tmp_path / 'train.txt', lines)
    out = str(tmp_path / 'out.dbw')
    rights = [10, 10, 12, 11, 12, 13]
    epochs_seen = []
    Scripted.saved = []

    class Counting(Scripted):
        def evaluate(self, dataset, first=0, count=None, window_losses=False):
            result = 10.0, rights[len(epochs_seen)]
            epochs_seen.append(self.state.iterations)
            return result

    host_fit(parse(['fit', '--train', train, '--val', train, '--model_out', out, '--batch_size',
                    '16', '--epochs', str(len(rights))]), trainer_factory=Counting)
    # 2 steps per epoch: saved after epochs 1, 3 and 6 - not on the ties at 2 and 5, not on the drop
    assert Scripted.saved == [2, 6, 12]
    text = capsys.readouterr().out.splitlines()
    epoch_lines = [fr.EPOCH_LINE.match(line) for line in text if line.startswith('Epoch ')]
    assert len(epoch_lines) == len(rights) and all(epoch_lines)
    assert [bool(m.group(8)) for m in epoch_lines] == [True, False, True, False, False, True]
    assert [float(m.group(6)) for m in epoch_lines] == [round(r / 32, 4) for r in rights]
    assert epoch_lines[0].group(8) == out
    saved, _ = ModelWeights.load(out)
    assert saved.flat()[0] == 12.0                                  # the file of epoch 6


# ---- the whole loop on the task of tests/test_gpu_feed.py -------------------------------------------
def test_host_fit_learns_the_motif_task_and_classify_loads_the_result(tmp_path, capsys):
    """The condition of the device test: the fp64 restatement of the same run ends its last epoch
    under a quarter of ln 4 and calls 64 of 64 validation windows right with the saved model."""
    (train_x, train_l), (val_x, val_l) = fr.fit_sets()
    train = str(tmp_path / 'train.txt')
    val = str(tmp_path / 'val.txt')
    fr.write_training_file(train, train_x, train_l)
    fr.write_training_file(val, val_x, val_l)
    out = str(tmp_path / 'model.dbw')
    host_fit(parse(['fit', '--train', train, '--val', val, '--model_out', out, '--batch_size',
                    str(fr.FIT_BATCH), '--epochs', str(fr.FIT_EPOCHS), '--aug', '2', '--seed',
                    str(fr.FIT_SEED)]))
    text = capsys.readouterr().out
    assert 'Number of possible barcode classifications = 4' in text
    assert 'Training data signal length = 96' in text
    assert '    training samples: {}'.format(fr.FIT_TRAIN) in text
    epochs = [fr.EPOCH_LINE.match(line) for line in text.splitlines() if line.startswith('Epoch ')]
    assert len(epochs) == fr.FIT_EPOCHS and all(epochs)
    for m in epochs:
        print(m.group(0))
    assert float(epochs[-1].group(3)) < np.log(4) / 4
    assert os.path.isfile(out) and os.path.isfile(out + '.state.npz')

    from conftest import OracleModel
    import deepbinner_amd.classify as classify
    saved_build = classify.build_model
    classify.build_model = lambda w: OracleModel(w, dtype=np.float64)
    try:
        model, input_size, output_size = classify.load_trained_model(out)
    finally:
        classify.build_model = saved_build
    assert (input_size, output_size) == (96, 4)
    probs = model.predict(fr.normalise(val_x)[:, :, None])
    assert int((probs.argmax(axis=1) == val_l).sum()) == 64
    assert hip_backend.read_training_data(val)[0].dtype == np.int16
