"""Fine-tuning behind frozen blocks, the parts that need no GPU: ``fit``'s
``--freeze`` and ``--fresh_head`` and their refusals, ``ModelWeights.with_fresh_head``, the loop
against the host stand-ins of tests/feed_reference.py, the new symbols of the C ABI and what they
refuse before any device work, and the fp64 reference's run that chose the step count of the
device's head-only learning test (tests/finetune_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import feed_reference as fr
import finetune_cases as fc
import train_reference as tr
import train_step_reference as ts
from conftest import REPO
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import fit as fit_module
from deepbinner_amd import hip_backend
from deepbinner_amd.model_format import (FROZEN_CONVS, ModelWeights, conv_shapes, param_count,
                                         trainable_count)

NEW_SYMBOLS = ['dbh_gradients_frozen', 'dbh_gradients_frozen_dev', 'dbh_nadam_update_frozen',
               'dbh_nadam_update_frozen_dev', 'dbh_trainer_set_frozen', 'dbh_trainer_get_frozen']
BASE = ['fit', '--train', 't', '--val', 'v', '--model_out', 'm']


def parse(argv):
    return cli.build_parser().parse_args(argv)


def row(label, values):
    return '{}\t{}'.format(label, ','.join(str(v) for v in values))


def write(path, lines):
    path.write_text(''.join(line + '\n' for line in lines))
    return str(path)


# ---- the command line ------------------------------------------------------------------------------
def test_options_and_defaults():
    args = parse(BASE)
    assert args.freeze is None and args.fresh_head is False
    args = parse(BASE + ['--model_in', 'i', '--freeze', '4', '--fresh_head'])
    assert (args.model_in, args.freeze, args.fresh_head) == ('i', 4, True)
    for bad in ('two', '2.5', ''):
        with pytest.raises(SystemExit):
            parse(BASE + ['--model_in', 'i', '--freeze', bad])


class Recording(fr.HostTrainer):
    """HostTrainer that notes what fit() hands it and trains nothing."""
    seen = []

    def __init__(self, weights, max_windows, device=None, **options):
        Recording.seen.append((weights, dict(options)))
        options.pop('frozen_blocks', None)
        super().__init__(weights, max_windows, device=device, **options)

    def run_epoch(self, dataset, indices, batch_size, augmentation):
        steps = len(indices) // batch_size
        self.state.iterations += steps
        return np.full(steps, 1.0), np.full(steps, batch_size // 2)


def host_fit(argv):
    Recording.seen = []
    fit_module.fit(parse(argv), trainer_factory=Recording, dataset_factory=fr.HostDataset,
                   epoch_order=fr.epoch_order)
    return Recording.seen


@pytest.fixture()
def files(tmp_path):
    """a training file of four classes at 96 samples, and starting models of 4 and of 5 classes"""
    train = write(tmp_path / 'train.txt', [row(i % 4, range(i, i + 96)) for i in range(20)])
    four, five = str(tmp_path / 'four.dbw'), str(tmp_path / 'five.dbw')
    ModelWeights.fresh(4, 96, seed=1).save(four)
    ModelWeights.fresh(5, 96, seed=2).save(five)
    out = str(tmp_path / 'out.dbw')
    return {'argv': ['fit', '--train', train, '--val', train, '--model_out', out, '--batch_size',
                     '16', '--epochs', '1', '--seed', '9'], 'four': four, 'five': five, 'out': out}


def test_refusals(files):
    def fails(message, extra):
        with pytest.raises(SystemExit) as e:
            host_fit(files['argv'] + extra)
        assert message in str(e.value), str(e.value)
        assert not os.path.exists(files['out']) and not Recording.seen

    for n in ('0', '8', '-1'):
        fails('Error: --freeze must be a number of blocks from 1 to 7', ['--model_in', files['four'],
                                                                        '--freeze', n])
    fails('Error: --freeze needs --model_in', ['--freeze', '3'])
    fails('Error: --fresh_head needs --model_in', ['--fresh_head'])
    # without --fresh_head the class counts must match, in the words they always had
    for extra in ([], ['--freeze', '7']):
        fails('Error: the provided model\'s output classes (5) are not equal to the training data\'s '
              'classes (4)', ['--model_in', files['five']] + extra)
    # --fresh_head does not lift the input-size check
    other = files['out'] + '.130.dbw'
    ModelWeights.fresh(4, 130).save(other)
    fails('Error: the provided model\'s input size (130) is not equal to the training data\'s size '
          '(96)', ['--model_in', other, '--fresh_head'])


def test_fit_hands_frozen_blocks_and_the_new_head_to_the_trainer(files, capsys):
    (weights, options), = host_fit(files['argv'] + ['--model_in', files['five'], '--fresh_head',
                                                    '--freeze', '6'])
    assert options == {'seed': 9, 'frozen_blocks': 6}
    source = ModelWeights.load(files['five'])[0]
    want = source.with_fresh_head(4, seed=9)
    assert weights.n_classes == 4 and weights.flat().tobytes() == want.flat().tobytes()
    lines = capsys.readouterr().out.splitlines()
    loaded = [i for i, line in enumerate(lines) if line.startswith('Loading ') and line.endswith('done')]
    assert len(loaded) == 1
    assert lines[loaded[0] + 1] == 'Frozen blocks: 6 of 7 - training {:,} of {:,} parameters'.format(
        trainable_count(4, 6), param_count(4)) == \
        'Frozen blocks: 6 of 7 - training 14,212 of 106,756 parameters'
    assert ModelWeights.load(files['out'])[0].n_classes == 4

    # --freeze alone: the starting model as it is
    (weights, options), = host_fit(files['argv'] + ['--model_in', files['four'], '--freeze', '1'])
    assert options == {'seed': 9, 'frozen_blocks': 1}
    assert weights.flat().tobytes() == ModelWeights.load(files['four'])[0].flat().tobytes()
    assert 'Frozen blocks: 1 of 7 - ' in capsys.readouterr().out

    # neither option: what fit did before - no frozen_blocks keyword, no new line
    (weights, options), = host_fit(files['argv'] + ['--model_in', files['four']])
    assert options == {'seed': 9}
    assert 'Frozen' not in capsys.readouterr().out
    (weights, options), = host_fit(files['argv'])
    assert options == {'seed': 9}
    assert weights.flat().tobytes() == ModelWeights.fresh(4, 96, seed=9).flat().tobytes()


# ---- the model -------------------------------------------------------------------------------------
def test_with_fresh_head_changes_the_head_alone():
    source = ModelWeights.fresh(13, 130, seed=4)
    for bn in source.bns:                       # (fresh statistics are all 0 and 1: make them tell)
        for a in bn:
            a += np.random.default_rng(a.size).standard_normal(a.size).astype(np.float32)
    before = source.flat().copy()
    for classes, seed in ((5, 0), (13, 7), (256, 1)):
        made = source.with_fresh_head(classes, seed=seed)
        fresh = ModelWeights.fresh(classes, 130, seed=seed)
        assert (made.n_classes, made.input_size) == (classes, 130)
        for i, ((kernel, bias), (k0, b0)) in enumerate(zip(made.convs[:-1], source.convs[:-1])):
            assert kernel.tobytes() == k0.tobytes() and bias.tobytes() == b0.tobytes(), i
            assert kernel is not k0 and bias is not b0
        for got, want in zip(made.bns, source.bns):
            assert all(a.tobytes() == b.tobytes() and a is not b for a, b in zip(got, want))
        assert made.convs[-1][0].shape == (1, 48, classes)
        assert made.convs[-1][0].tobytes() == fresh.convs[-1][0].tobytes()
        assert made.convs[-1][1].tobytes() == fresh.convs[-1][1].tobytes()
        assert made.flat().size == param_count(classes)
    assert source.flat().tobytes() == before.tobytes()
    assert source.with_fresh_head(13, seed=7).convs[-1][0].tobytes() != source.convs[-1][0].tobytes()


def test_blocks_follow_the_header_s_table():
    """model_format's FROZEN_CONVS and trainable_count against the table as tests/finetune_cases.py
    restates it from the header."""
    assert [FROZEN_CONVS[f] for f in range(8)] == [fc.LAST_FROZEN_CONV[f] for f in range(8)]
    text = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    for f, first in ((1, 'conv1d_2'), (2, 'conv1d_5'), (3, 'conv1d_8'), (4, 'conv1d_10, 11, 12, 14'),
                     (5, 'conv1d_17'), (6, 'conv1d_18'), (7, 'conv1d_20')):
        assert re.search(r'\* +{} +conv1d_\S+.*bn_{} +{} '.format(f, f, first), text), f
    for classes in (2, 13, 256):
        slices, moving = tr.tensor_slices(classes)
        moving_all = np.logical_or(*fc.moving_masks(classes, 3))
        assert moving_all.sum() == 2 * 480
        for f in range(8):
            mask = fc.frozen_mask(classes, f)
            assert trainable_count(classes, f) == int((~mask & ~moving_all).sum())
            frozen, trainable = fc.tensor_names(f)
            assert len(frozen) + len(trainable) == 54 and 'conv1d_20/kernel' in trainable
            # the frozen convolutions are the blob's first floats: one offset decides them
            first = sum(k * cin * cout + cout for _, k, cin, cout, _, _ in conv_shapes(classes)[:FROZEN_CONVS[f]])
            assert mask[:first].all() and not mask[first:slices['bn_1/gamma'].start].any()
        assert trainable_count(classes, 0) == param_count(classes) - 2 * 480


# ---- the C ABI -------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint {}\s*\('.format(name), text), name
        assert name in hip_backend.SIGNATURES and name in hip_backend.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    for name in ('dbh_gradients_frozen', 'dbh_gradients_frozen_dev', 'dbh_nadam_update_frozen',
                 'dbh_nadam_update_frozen_dev'):
        plain = hip_backend.SIGNATURES[name.replace('_frozen', '')]
        assert hip_backend.SIGNATURES[name] == (plain[0], plain[1] + [ctypes.c_int]), name
    assert hip_backend.MAX_FROZEN_BLOCKS == fc.MAX_FROZEN == 7


def test_refused_before_any_device_work():
    """frozen_blocks outside 0..7 is DBH_ERR_INVALID_ARGUMENT, with nothing written, on a box
    without a GPU too: the check stands in front of every device call."""
    lib = hip_backend.load_library()
    weights = ModelWeights.fresh(2, 96)
    flat = weights.flat()
    x = np.zeros((3, 96), dtype=np.float32)
    labels = np.zeros(3, dtype=np.int32)
    grads = np.full(flat.size, 7.0, dtype=np.float32)
    stats = np.full(960, 7.0, dtype=np.float32)
    loss, correct = ctypes.c_double(7.0), ctypes.c_int64(7)
    k = hip_backend.NadamCoefficients(**hip_backend.nadam_schedule(0))
    for f in (-1, 8, 1 << 20):
        assert lib.dbh_gradients_frozen(flat, flat.size, 2, 96, x, labels, 3, 0.15, 0,
                                        ctypes.byref(loss), ctypes.byref(correct), grads, stats, f) == 1
        assert lib.dbh_gradients_frozen_dev(16, flat.size, 2, 96, 16, 16, 3, 0.15, 0, 16, 16, 16, 16,
                                            16, None, f) == 1
        assert lib.dbh_nadam_update_frozen(grads.ctypes.data, grads.ctypes.data, grads.ctypes.data,
                                           grads.ctypes.data, stats.ctypes.data, flat.size, 2,
                                           ctypes.byref(k), f) == 1
        assert lib.dbh_nadam_update_frozen_dev(16, 16, 16, 16, 16, flat.size, 2, ctypes.byref(k), None,
                                               f) == 1
    assert (grads == 7.0).all() and (stats == 7.0).all() and (loss.value, correct.value) == (7.0, 7)
    assert lib.dbh_trainer_set_frozen(None, 3) == 1
    assert lib.dbh_trainer_get_frozen(None, ctypes.byref(ctypes.c_int(0))) == 1
    with pytest.raises(hip_backend.HipBackendError):
        hip_backend.loss_and_gradients(weights, x, labels, frozen_blocks=9)
    for f in (-1, 8):                           # a trainer refuses before it allocates anything
        with pytest.raises(ValueError):
            hip_backend.Trainer(weights, 3, frozen_blocks=f)


# ---- the reference's own head-only run -------------------------------------------------------------
def test_the_reference_halves_its_loss_with_the_head_alone():
    """What chose HEAD_STEPS for tests/test_gpu_finetune.py: the fp64 reference, a five-class
    source of its own training, the head re-drawn for three classes and trained alone."""
    losses = fc.head_only_reference()
    print('head only, fp64: first loss {:.4f}, loss of step {} {:.4f}, mean of the last five {:.4f}'
          .format(losses[0], len(losses), losses[-1], float(np.mean(losses[-5:]))))
    assert len(losses) == fc.HEAD_STEPS == 75
    assert abs(losses[0] - 0.953) < 5e-4 and abs(losses[-1] - 0.250) < 5e-4
    assert losses[-1] <= losses[0] / 2 and float(np.mean(losses[-5:])) <= losses[0] / 2
    # and the update at f = 7 in NumPy leaves everything but the head where it was
    state = ts.State(ModelWeights.fresh(fc.HEAD_SOURCE_CLASSES, ts.LEARN_INPUT)
                     .with_fresh_head(ts.LEARN_CLASSES, seed=fc.HEAD_SEED))
    x, labels = ts.learning_batches()[0][0]
    loss, _, grads, stats = fc.head_only_gradients(state.weights(), x, labels, 0.15, 1)
    mask = fc.frozen_mask(ts.LEARN_CLASSES, 7)
    assert not grads[mask].any() and grads[~mask].any()
    m = np.full(state.flat.size, 0.5, dtype=np.float32)
    p, m2, v2 = fc.frozen_update(state.flat, grads, m, m, stats, ts.LEARN_CLASSES,
                                 ts.nadam_coefficients(0), 7)
    assert p[mask].tobytes() == state.flat[mask].tobytes() and m2[mask].tobytes() == m[mask].tobytes()
    assert (p[~mask] != state.flat[~mask]).all() and v2[mask].tobytes() == m[mask].tobytes()
