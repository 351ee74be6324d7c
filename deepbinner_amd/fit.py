"""
The ``fit`` command: what the reference's ``train`` does (``deepbinner/train_network.py:28-124``)
on the resident trainer.  The same conditions checked, under the reference's messages, and the
same options; the data stay on the device as the int16 samples the files hold, batches are
assembled there (``hip_backend.Dataset``), an epoch is queued whole and synchronised once, and ``--model_out`` is
written when - and only when - the validation accuracy is strictly above the best so far, which is
Keras's ``ModelCheckpoint(monitor='val_acc', save_best_only=True, mode='max')``
(train_network.py:62-63).

Two deliberate differences.  The random stream is this package's stateless hash, seeded by
``--seed``: the reference's law (a shuffled pass over the samples, a uniform quarter of the positions
doubled and a quarter dropped with chance 1 - 1/aug), not its draws.  And every epoch validates ALL
validation windows in file order, where the reference validates a rolling ``val_count //
batch_size`` batches of a shuffled generator.

Fine-tuning, with ``--model_in``: ``--freeze N`` leaves the first N blocks of
the starting model as they are (``Trainer(frozen_blocks=N)``), ``--fresh_head`` re-draws conv1d_20
for the data's class count with ``--seed`` (``ModelWeights.with_fresh_head``), which is how a model
is reused on another barcode set.

``fit`` takes its device classes as parameters, so that the loop and the checkpoint policy also run
against host stand-ins (tests/feed_reference.py).
"""
import pathlib
import sys

import numpy as np

from .model_format import ModelWeights, param_count, trainable_count


# an evaluation runs in chunks of the trainer's max_windows; a step takes batch_size of them
EVALUATION_WINDOWS = 256
MAX_BATCH_SAMPLES = 1 << 20          # dbh_gradients_max_windows: windows * input size of one call


def fit(args, trainer_factory=None, dataset_factory=None, epoch_order=None):
    from . import hip_backend
    trainer_factory = trainer_factory or hip_backend.Trainer
    dataset_factory = dataset_factory or hip_backend.Dataset.from_arrays
    epoch_order = epoch_order or hip_backend.epoch_order
    check_options(args)

    print()
    parse = getattr(args, 'parse', None)
    train_samples, train_labels = load_data(args.train, parse=parse)
    class_count = int(train_labels.max()) + 1
    signal_size = train_samples.shape[1]
    val_samples, val_labels = load_data(args.val, signal_size, parse=parse)
    report(MESSAGES['classes'], class_count, class_count - 1)
    report(MESSAGES['size'], signal_size)
    for which, count in (('training', len(train_labels)), ('validation', len(val_labels))):
        if count < args.batch_size:
            sys.exit(MESSAGES['few'].format(which))
    report(MESSAGES['summary'], len(train_labels), len(val_labels), args.batch_size)
    for name, labels in ((args.train, train_labels), (args.val, val_labels)):
        if labels.min() < 0 or labels.max() >= class_count:
            sys.exit('Error: {} holds a barcode class outside 0-{}'.format(name, class_count - 1))

    freeze = getattr(args, 'freeze', None) or 0
    if args.model_in:
        weights = load_starting_model(args.model_in)
        if weights.input_size != signal_size:
            sys.exit(MESSAGES['model size'].format(weights.input_size, signal_size))
        if getattr(args, 'fresh_head', False):
            weights = weights.with_fresh_head(class_count, seed=args.seed)
        if weights.n_classes != class_count:
            sys.exit(MESSAGES['model classes'].format(weights.n_classes, class_count))
        if freeze:
            print(MESSAGES['frozen'].format(freeze, trainable_count(class_count, freeze),
                                            param_count(class_count)))
    else:
        weights = ModelWeights.fresh(class_count, signal_size, seed=args.seed)
    frozen = {'frozen_blocks': freeze} if freeze else {}

    batch = args.batch_size
    steps = min(len(train_labels) // batch, args.batches_per_epoch)
    max_windows = max(batch, min(EVALUATION_WINDOWS, MAX_BATCH_SAMPLES // signal_size))
    best = None
    with dataset_factory(train_samples, train_labels, class_count) as train_set, \
            dataset_factory(val_samples, val_labels, class_count) as val_set, \
            trainer_factory(weights, max_windows, seed=args.seed, **frozen) as trainer:
        n_train, n_val = len(train_set), len(val_set)
        for epoch in range(args.epochs):
            indices = stream_indices(epoch_order, args.seed, n_train, epoch * steps * batch,
                                     steps * batch)
            losses, counts = trainer.run_epoch(train_set, indices, batch, args.aug)
            loss = float(np.mean(np.asarray(losses, dtype=np.float64)))
            acc = int(np.sum(counts)) / (steps * batch)
            val_loss_sum, val_right = trainer.evaluate(val_set)
            line = ('Epoch {}/{} - loss: {:.4f} - acc: {:.4f} - val_loss: {:.4f} - val_acc: {:.4f}'
                    .format(epoch + 1, args.epochs, loss, acc, val_loss_sum / n_val,
                            val_right / n_val))
            if best is None or val_right > best:      # the same n_val every epoch: exact
                was = '-inf' if best is None else '{:.5f}'.format(best / n_val)
                trainer.save_checkpoint(args.model_out)
                best = val_right
                line += ' - val_acc improved from {} to {:.5f}, saved {}'.format(
                    was, val_right / n_val, args.model_out)
            else:
                line += ' - val_acc did not improve from {:.5f}'.format(best / n_val)
            print(line, flush=True)


def stream_indices(epoch_order, seed, n, first, count):
    """Positions [first, first + count) of the sample stream: pass 0's order, then pass 1's, ...;
    a batch may span two passes, as the reference's does (train_network.py:151-158)."""
    parts = []
    for p in range(first // n, (first + count - 1) // n + 1):
        order = np.asarray(epoch_order(seed, p, n), dtype=np.int64)
        lo, hi = max(first, p * n), min(first + count, (p + 1) * n)
        parts.append(order[lo - p * n:hi - p * n])
    return np.concatenate(parts)


# the reference's texts (train_network.py:36-42, 79-84, 95, 103-105, 116-122), which its users
# and their scripts know; what finds the conditions is this module's own single pass over a file
MESSAGES = {
    'label': 'a non-integer barcode class was encountered in {}',
    'line': 'training signal not formatted correctly',
    'sizes': 'inconsistent signal sizes in training data',
    'few': 'Error: the number of {} samples is smaller than the batch size',
    'classes': ('Number of possible barcode classifications = {}', '  (1-{} plus a no-barcode class)'),
    'size': ('Training data signal length = {}',),
    'summary': ('Data summary:', '    training samples: {}', '  validation samples: {}',
                '          batch_size: {}'),
    'model size': 'Error: the provided model\'s input size ({}) is not equal to the training '
                  'data\'s size ({})',
    'model classes': 'Error: the provided model\'s output classes ({}) are not equal to the '
                     'training data\'s classes ({})',
    # this build's own
    'frozen': 'Frozen blocks: {} of 7 - training {:,} of {:,} parameters',
    'needs model': 'Error: --{} needs --model_in (a starting model to fine-tune)',
    'freeze range': 'Error: --freeze must be a number of blocks from 1 to 7',
}


def report(lines, *values):
    """Print the lines of one block, each ``{}`` taking the next value, then an empty line."""
    values = list(values)
    for line in lines:
        print(line.format(*[values.pop(0) for _ in range(line.count('{}'))]))
    print()


def check_options(args):
    """What the device entries would refuse later, said before any file is read."""
    if not args.aug >= 1.0:
        sys.exit('Error: --aug must be 1 or more (1 = no augmentation)')
    for name in ('epochs', 'batch_size', 'batches_per_epoch'):
        if getattr(args, name) < 1:
            sys.exit('Error: --{} must be a positive integer'.format(name))
    freeze = getattr(args, 'freeze', None)
    if freeze is not None and not 1 <= freeze <= 7:
        sys.exit(MESSAGES['freeze range'])
    for name in ('freeze', 'fresh_head'):
        if getattr(args, name, None) and not args.model_in:
            sys.exit(MESSAGES['needs model'].format(name))


def load_starting_model(model_file):
    """classify.load_trained_model's messages, without building an inference model"""
    if not pathlib.Path(model_file).is_file():
        sys.exit('Error: {} does not exist'.format(model_file))
    print('Loading {}... '.format(model_file), end='', flush=True)
    try:
        weights, _ = ModelWeights.load(str(model_file))
    except Exception:       # whatever a damaged or foreign file trips inside the readers
        sys.exit('Error: model input has incorrect shape - are you sure that {} is a valid '
                 'model file?'.format(model_file))
    print('done')
    return weights


def load_data(filename, signal_size=None, parse=None):
    """(int16 samples [n, L], int32 labels [n]) of a training-data file, read in one pass
    (hip_backend.read_training_data); whatever is wrong with a line is an ``Error:`` with the
    reference's text where it has one.  The reference takes the signal size from the first hundred
    lines and asserts it for the rest; here every line is held to it, under the same message.
    ``parse``: 'host', 'gpu' (the text parsed on the device) or None for DEEPBINNER_TEXT_PARSE;
    either route gives the same arrays and the same errors."""
    from .hip_backend import TrainingDataError, read_training_data
    try:
        return read_training_data(filename, signal_size, MESSAGES, parse=parse)
    except TrainingDataError as e:
        sys.exit('Error: {}'.format(e))
