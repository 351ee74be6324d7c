"""
The ``refine`` command (reference ``deepbinner/refine.py``): keep the training samples that a
trained model calls as their own label.

Two forms.  The reference's, ``refine training_data classification_data``: the table that
``classify`` wrote for the training file is read beside it, line for line, and a training line is
written to stdout when its label equals the table's call (``none`` = 0).  stdout is the reference's,
byte for byte; stderr has its heading and the final ``Matches: a / b (p%)`` state, the progress in
between updated every few thousand lines.  A pair of files whose lines do not belong together is an
``Error:`` naming the line, where the reference has a bare ``assert``.

The fused form, ``refine --model FILE training_data``, classifies the file first, in this process,
through ``classify``'s own training-data route - the device parse of DESIGN.md section 22 included
where DEEPBINNER_TEXT_PARSE=gpu - and filters by the calls it made, with no table in between.  Its
stdout equals what the two-step form gives from the table of ``classify -s FILE training_data``.
"""
import argparse
import contextlib
import io
import sys

from .balance import write_bytes

PROGRESS_EVERY = 4096


def refine(args):
    if (args.model is None) == (args.classification_data is None):
        sys.exit('Error: refine takes either a classification file or --model (one of the two)')
    if args.model is not None:
        table = classify_in_process(args)
    else:
        with open(args.classification_data, 'rt') as classes:
            table = classes.read()
    print('\nRefining training data', file=sys.stderr)
    with open(args.training_data, 'rb') as raw:
        training_lines = raw.read().splitlines(keepends=True)
    class_lines = table.splitlines()[1:]                   # the first is the header
    matches = total = 0
    kept = []
    for training_line, class_line in zip(training_lines, class_lines):
        parts = class_line.rstrip().split('\t')
        label = training_line.split(b'\t')[0].decode('ascii', errors='replace')
        if len(parts) < 2 or parts[0].split('_')[-1] != label:
            write_bytes(b''.join(kept))                    # what matched in front of it
            sys.exit('Error: line {} of {} ({}) does not belong to line {} of the training data '
                     '(barcode {})'.format(total + 2, args.classification_data or 'the calls',
                                           parts[0], total + 1, label))
        try:
            call = 0 if parts[1] == 'none' else int(parts[1])
            same = int(label) == call
        except ValueError:
            sys.exit('Error: line {} of the training data or its call is not an integer barcode '
                     'class'.format(total + 1))
        if same:
            kept.append(training_line)
            matches += 1
        total += 1
        if total % PROGRESS_EVERY == 0:
            write_bytes(b''.join(kept))
            kept = []
            report(matches, total)
    write_bytes(b''.join(kept))
    if total:
        report(matches, total)
    print('\n', file=sys.stderr)


def report(matches, total):
    print('\rMatches: {} / {} ({:.2f}%)'.format(matches, total, 100.0 * matches / total),
          file=sys.stderr, end='')


def classify_in_process(args):
    """The table ``classify -s MODEL training_data`` writes, as text, made here."""
    from . import classify
    if classify.determine_input_type(args.training_data) != 'training_data':
        sys.exit('Error: {} is not a file of training data'.format(args.training_data))
    if not 0.0 < args.score_diff <= 1.0:
        sys.exit('Error: --score_diff must be in the range (0, 1] (greater than 0 and less than or '
                 'equal to 1)')
    options = argparse.Namespace(input=args.training_data, start_model=args.model, end_model=None,
                                 scan_size=args.scan_size, score_diff=args.score_diff,
                                 batch_size=args.batch_size, verbose=False, devices=0)
    table = io.StringIO()
    with contextlib.redirect_stdout(table):
        classify.classify(options)
    return table.getvalue()
