"""
Command line of the classify path: the ``classify`` and ``realtime`` sub-commands with the flags,
defaults, validation and error messages of the reference's ``deepbinner/deepbinner.py``
(:90-156 options, :283-345 checks and preset resolution), so that existing command lines keep
working, plus ``bin`` (:159-176), the consumer of the table ``classify`` writes.  The options are
declared as data (``OPTIONS``) and turned into argparse calls by one loop.  The training side:
``balance`` (:228-243, plus ``--seed``) and ``refine`` (:272-280, plus the fused ``--model`` form)
are the reference's commands, and ``fit`` is its ``train`` (:246-269: the same options and
defaults, plus ``--seed``) on the resident trainer - under another name, because ``train`` and
``prep`` answer with a one-line refusal.  ``sweep`` is not the reference's: the calls of every scan
size and score difference counted in one pass (sweep.py).  Nor is ``scan``: every window of a read
through the network, and the places inside it where a barcode class leads (scan.py).  Nor is
``locate``: where in the signal each side's call comes from, read out of the network's last layers
(locate.py).
"""

import argparse
import pathlib
import sys

from .version import __version__

NOT_PROVIDED = ('prep', 'train')
PRESETS = {'native': ('EXP-NBD103_read_starts', 'EXP-NBD103_read_ends'),
           'rapid': ('SQK-RBK004_read_starts', None)}
TWO_MODEL_FLAGS = ('require_either', 'require_start', 'require_both')
_IGNORED = 'Accepted for compatibility with the TensorFlow build (ignored)'
_HELP = (('-h', '--help'), dict(action='help', default=argparse.SUPPRESS,
                                help='Show this help message and exit'))

# (group title, [(flags, argparse keywords)]) shared by classify and realtime
OPTIONS = [
    ('Model presets', [
        (('--native',), dict(action='store_true',
                             help='Preset for EXP-NBD103 read start and end models')),
        (('--rapid',), dict(action='store_true', help='Preset for SQK-RBK004 read start model')),
    ]),
    ('Models (at least one is required if not using a preset)', [
        (('-s', '--start_model'), dict(type=str, help='Model trained on the starts of reads')),
        (('-e', '--end_model'), dict(type=str, help='Model trained on the ends of reads')),
    ]),
    ('Barcoding', [
        (('--scan_size',), dict(type=float, default=6144,
                                help="This much of a read's start/end signal will examined for "
                                     "barcode signals")),
        (('--score_diff',), dict(type=float, default=0.5,
                                 help='For a read to be classified, there must be this much '
                                      'difference between the best and second-best barcode '
                                      'scores')),
    ]),
    ('Two model (read start and read end) behaviour', [
        (('--require_either',), dict(action='store_true',
                                     help='Most lenient approach: a barcode call on either the '
                                          'start or end is sufficient to classify a read, as long '
                                          'as they do not disagree on the barcode (default '
                                          'behaviour)')),
        (('--require_start',), dict(action='store_true',
                                    help='Moderate approach: a start barcode is required to '
                                         'classify a read but an end barcode is optional')),
        (('--require_both',), dict(action='store_true',
                                   help='Most stringent approach: both start and end barcodes '
                                        'must be present and agree to classify a read')),
    ]),
    ('Performance', [
        (('--batch_size',), dict(type=int, default=256,
                                 help='Number of reads handed to the GPU per call')),
        (('--loader_procs',), dict(type=int, default=0,
                                   help='Threads (native reader) or processes (Python reader) '
                                        'that load and decompress fast5 files ahead of the GPU '
                                        '(0 = automatic)')),
        (('--devices',), dict(type=int, default=0,
                              help='GPUs to spread the batches over, one model replica each '
                                   '(0 = DEEPBINNER_DEVICES or one)')),
        # TensorFlow knobs of the reference
        (('--intra_op_parallelism_threads',), dict(type=int, default=12, help=_IGNORED)),
        (('--inter_op_parallelism_threads',), dict(type=int, default=1, help=_IGNORED)),
        (('--device_count',), dict(type=int, default=1, help=_IGNORED)),
        (('--omp_num_threads',), dict(type=int, default=12, help=_IGNORED)),
    ]),
]

# per sub-command: description, groups in front of the shared ones (None in that list: no shared
# ones), the 'Other' group behind them
COMMANDS = {
    'classify': ('Classify fast5 reads',
                 [('Positional', [
                     (('input',), dict(type=str,
                                       help='One of the following: a single fast5 file, a '
                                            'directory of fast5 files (will be searched '
                                            'recursively) or a tab-delimited file of training '
                                            'data'))])],
                 [(('--verbose',), dict(action='store_true',
                                        help='Include the output probabilities for all barcodes '
                                             'in the results (default: just show the final '
                                             'barcode call)')),
                  (('--multi_read',), dict(action='store_true',
                                           help='Classify the reads of multi-read fast5 files '
                                                'where they are (one-read files may be mixed '
                                                'in)')), _HELP]),
    'realtime': ('Sort fast5 files during sequencing',
                 [('Required', [
                     (('--in_dir',), dict(type=str, required=True,
                                          help='Directory where sequencer deposits fast5 files')),
                     (('--out_dir',), dict(type=str, required=True,
                                           help='Directory to output binned fast5 files'))])],
                 [(('--stop',), dict(action='store_true',
                                     help='Automatically stop when there are no more input reads '
                                          '(default: continue to run and wait for more reads)')),
                  _HELP]),
    'bin': ('Bin fasta/q reads',
            [('Required', [
                (('--classes',), dict(type=str, required=True,
                                      help='Deepbinner classification file (made with the '
                                           'deepbinner classify command)')),
                (('--reads',), dict(type=str, required=True, help='FASTA or FASTQ reads')),
                (('--out_dir',), dict(type=str, required=True,
                                      help='Directory to output binned read files'))]),
             None],
            [(('--threads',), dict(type=int, default=0,
                                   help='Threads that compress the output (0 = automatic)')),
             _HELP]),
    'fit': ('Train the neural network (the reference\'s train command)',
            [('Required', [
                (('--train',), dict(type=str, required=True,
                                    help='Balanced training data produced by the balance command')),
                (('--val',), dict(type=str, required=True,
                                  help='Validation data used to assess the training')),
                (('--model_out',), dict(type=str, required=True,
                                        help='Filename for the trained model'))]),
             None],
            [(('--model_in',), dict(type=str,
                                    help='An existing model to use as a starting point for '
                                         'training')),
             (('--freeze',), dict(type=int, default=None, metavar='N',
                                  help='With --model_in: keep the first N blocks (1-7) of the '
                                       'starting model as they are and train only what is behind '
                                       'them (a block ends at a batch normalisation; the last '
                                       'convolution is never frozen)')),
             (('--fresh_head',), dict(action='store_true',
                                      help='With --model_in: draw a new last convolution for the '
                                           'number of classes in the training data (with --seed), '
                                           'so that a model of another barcode set can be the '
                                           'starting point')),
             (('--epochs',), dict(type=int, default=100, help='Number of training epochs')),
             (('--aug',), dict(type=float, default=2.0,
                               help='Data augmentation factor (1 = no augmentation)')),
             (('--batch_size',), dict(type=int, default=20, help='Training batch size')),
             (('--batches_per_epoch',), dict(type=int, default=5000,
                                             help='The number of samples per epoch will be this '
                                                  'times the batch size')),
             (('--seed',), dict(type=int, default=0,
                                help='Seed of the epoch order, augmentation, noise and dropout '
                                     '(the same seed gives the same model, bit for bit)')),
             (('--parse',), dict(type=str, choices=['host', 'gpu'], default=None,
                                 help='Where the training-data text is parsed: host, or gpu for '
                                      'whole blocks on the device with the same result (default: '
                                      'DEEPBINNER_TEXT_PARSE, else host)')),
             _HELP]),
    'balance': ('Select balanced training set',
                [('Positional', [
                    (('training_data',), dict(type=str, nargs='+',
                                              help='Files of raw training data produced by the '
                                                   'prep command'))]),
                 None],
                [(('--barcodes',), dict(type=str,
                                        help='A comma-delimited list of which barcodes to include '
                                             '(default: include all barcodes)')),
                 (('--random_signal',), dict(type=float, default=1.0,
                                             help='This many random signals will be added to the '
                                                  'output as no-barcode training samples '
                                                  '(expressed as a multiple of the balanced '
                                                  'per-barcode count, default: 1.0)')),
                 (('--seed',), dict(type=int, default=0,
                                    help='Seed of the selection and of the random signals (the '
                                         'same seed gives the same output, byte for byte)')),
                 _HELP]),
    'refine': ('Refine the training set',
               [('Positional', [
                   (('training_data',), dict(type=str,
                                             help='Balanced training data produced by the balance '
                                                  'command')),
                   (('classification_data',), dict(type=str, nargs='?', default=None,
                                                   help='Training data barcode calls produced by '
                                                        'the classify command (or give --model)'))]),
                None],
               [(('--model',), dict(type=str, default=None,
                                    help='Classify the training data with this model here, '
                                         'instead of reading a classification file')),
                (('--scan_size',), dict(type=float, default=6144,
                                        help="With --model: this much of a sample's signal will "
                                             "be examined for barcode signals")),
                (('--score_diff',), dict(type=float, default=0.5,
                                         help='With --model: the difference between the best and '
                                              'second-best barcode scores that a call needs')),
                (('--batch_size',), dict(type=int, default=256,
                                         help='With --model: samples handed to the GPU per call')),
                _HELP]),
    'sweep': ('Count the calls of every scan size and score difference in one pass',
              [('Positional', [
                  (('input',), dict(type=str,
                                    help='One of the following: a single fast5 file, a directory '
                                         'of fast5 files (will be searched recursively) or a '
                                         'tab-delimited file of training data (whose labels are '
                                         'then the labels)'))]),
               OPTIONS[0], OPTIONS[1],
               ('Sweep', [
                   (('--max_scan_size',), dict(type=float, default=12288,
                                               help='The largest scan size: every multiple of half '
                                                    'the model input size up to it is counted')),
                   (('--score_diffs',), dict(type=str, default='0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9',
                                             help='Comma-delimited score differences to count, '
                                                  'each in (0, 1]')),
                   (('--labels',), dict(type=str, default=None,
                                        help='Known barcodes of the reads: a sequencing summary '
                                             '(read_id, barcode_arrangement) or a table made '
                                             'with the deepbinner classify command; adds the '
                                             'right, wrong and missed columns')),
                   (('--live',), dict(action='store_true',
                                      help='Count instead what replay --stop_on_decision would '
                                           'decide early at every --min_windows and score '
                                           'difference')),
                   (('--chunk_samples',), dict(type=int, default=None,
                                               help='With --live: samples of a read per push '
                                                    '(default: 1600, 0.4 s at 4 kHz)'))]),
               ('Performance', [
                   (('--batch_size',), dict(type=int, default=256,
                                            help='Number of reads handed to the GPU per call')),
                   (('--loader_procs',), dict(type=int, default=0,
                                              help='Threads (native reader) or processes (Python '
                                                   'reader) that load fast5 files ahead of the GPU '
                                                   '(0 = automatic)')),
                   (('--devices',), dict(type=int, default=0,
                                         help='A sweep runs on one GPU: more than 1 is refused'))]),
               None],
              [(('--multi_read',), dict(action='store_true',
                                        help='Take the reads of multi-read fast5 files where '
                                             'they are (one-read files may be mixed in)')), _HELP]),
    'scan': ('Flag reads with barcode signal inside the read (chimeras)',
             [('Positional', [
                 (('input',), dict(type=str,
                                   help='One of the following: a single fast5 file or a directory '
                                        'of fast5 files (will be searched recursively)'))])],
             [(('--min_windows',), dict(type=int, default=1,
                                        help='An event is this many consecutive windows of one '
                                             'barcode class at least')),
              (('--multi_read',), dict(action='store_true',
                                       help='Take the reads of multi-read fast5 files where '
                                            'they are (one-read files may be mixed in)')), _HELP]),
    'locate': ('Report where in the signal each barcode call comes from',
               [('Positional', [
                   (('input',), dict(type=str,
                                     help='One of the following: a single fast5 file or a directory '
                                          'of fast5 files (will be searched recursively)'))])],
               [(('--multi_read',), dict(action='store_true',
                                         help='Take the reads of multi-read fast5 files where '
                                              'they are (one-read files may be mixed in)')),
                (('--occlude',), dict(action='store_true',
                                      help='Call each located side again with the located samples '
                                           'blanked, with everything else blanked and with a '
                                           'control stretch blanked (six more columns per side)')),
                _HELP]),
    'replay': ('Play reads back as a sequencer delivers them and call each while it arrives',
               [('Positional', [
                   (('input',), dict(type=str,
                                     help='One of the following: a single fast5 file or a directory '
                                          'of fast5 files (will be searched recursively)'))])],
               [(('--channels',), dict(type=int, default=512,
                                       help='Reads in flight at a time, one per sequencer channel')),
                (('--chunk_samples',), dict(type=int, default=1600,
                                            help='Samples of every open read per round (1600: 0.4 s '
                                                 'at 4 kHz)')),
                (('--min_windows',), dict(type=int, default=1,
                                          help='A read is decided no earlier than at this many '
                                               'windows')),
                (('--stop_on_decision',), dict(action='store_true',
                                               help='Run no further window of a read once it is '
                                                    'decided')),
                (('--multi_read',), dict(action='store_true',
                                         help='Take the reads of multi-read fast5 files where '
                                              'they are (one-read files may be mixed in)')),
                (('--both_ends',), dict(action='store_true',
                                        help='Also call each read\'s end barcode when the read '
                                             'ends, and combine the two calls as classify does '
                                             '(needs both models)')),
                (('--balance',), dict(type=str, default=None, metavar='LIST',
                                      help='Barcodes to balance: eject a read whose barcode is ahead '
                                           'of the one that has yielded least (1,2,5; 1:2,2:1 sets '
                                           'integer shares)')),
                (('--deplete',), dict(type=str, default=None, metavar='LIST',
                                      help='Barcodes whose reads are always ejected')),
                (('--keep',), dict(type=str, default=None, metavar='LIST',
                                   help='Keep these barcodes and eject every other one')),
                (('--slack_samples',), dict(type=int, default=0,
                                            help='How many samples a balanced barcode may be ahead '
                                                 'before its reads are ejected')),
                (('--eject_undecided',), dict(action='store_true',
                                              help='Eject a read that ends without a decision')),
                (('--eject_samples',), dict(type=int, default=None,
                                            help='Simulated ejection delay: samples an ejected read '
                                                 'still delivers (default: one --chunk_samples)')),
                _HELP]),
}
USES_MODELS = ('classify', 'realtime', 'scan', 'locate', 'replay')


def _add_groups(parser, groups):
    for title, options in groups:
        group = parser.add_argument_group(title)
        for flags, keywords in options:
            group.add_argument(*flags, **keywords)


def build_parser():
    parser = argparse.ArgumentParser(
        prog='deepbinner',
        description='Deepbinner: a deep convolutional neural network barcode demultiplexer for '
                    'Oxford Nanopore reads (MI355X / HIP implementation of the classify path)',
        add_help=False)
    subparsers = parser.add_subparsers(title='Commands', dest='subparser_name')
    for name, (description, leading, other) in COMMANDS.items():
        sub = subparsers.add_parser(name, description=description, add_help=False)
        shared = [] if None in leading else OPTIONS
        _add_groups(sub, [g for g in leading if g] + shared + [('Other', other)])
    _add_groups(parser, [('Help', [
        _HELP, (('--version',), dict(action='version', version=__version__,
                                     help="Show program's version number and exit"))])])
    return parser


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    parser = build_parser()
    if not argv:
        parser.print_help(file=sys.stderr)
        sys.exit(1)
    if argv[0] in NOT_PROVIDED:
        sys.exit('Error: the {} command is not part of this build - it covers the classify, '
                 'realtime, bin, balance, fit, refine, replay, sweep, scan and locate commands only'
                 .format(argv[0]))
    args = parser.parse_args(argv)
    if args.subparser_name in USES_MODELS:
        check_classify_and_realtime_arguments(args)
    if args.subparser_name == 'classify':
        from .classify import classify as run
    elif args.subparser_name == 'realtime':
        from .realtime import realtime as run
    elif args.subparser_name == 'bin':
        from .bin import bin_reads as run
    elif args.subparser_name == 'fit':
        from .fit import fit as run
    elif args.subparser_name == 'balance':
        from .balance import balance as run
    elif args.subparser_name == 'refine':
        from .refine import refine as run
    elif args.subparser_name == 'sweep':
        if resolve_presets(args) == 0:
            sys.exit('Error: you must provide at least one model')
        from .sweep import sweep as run
    elif args.subparser_name == 'scan':
        from .scan import scan as run
    elif args.subparser_name == 'locate':
        from .locate import locate as run
    elif args.subparser_name == 'replay':
        from .replay import replay as run
    else:
        return
    run(args)


def check_classify_and_realtime_arguments(args):
    """Preset resolution and option checks with the reference's messages (deepbinner.py:283-317);
    with two models and no mode given the mode is require_either (:315-316)."""
    n_models = resolve_presets(args)
    if n_models == 0:
        sys.exit('Error: you must provide at least one model')
    if not 0.0 < args.score_diff <= 1.0:
        sys.exit('Error: --score_diff must be in the range (0, 1] (greater than 0 and less than or '
                 'equal to 1)')
    given = [flag for flag in TWO_MODEL_FLAGS if getattr(args, flag)]
    if given and n_models < 2:
        sys.exit('Error: --{} can only be used with two models (start and end)'.format(given[0]))
    if len(given) > 1:
        sys.exit('Error: only one of the following options can be used: --require_either, '
                 '--require_start, --require_both')
    if not given:
        args.require_either = True
    assert two_model_args_used(args) == 1


def resolve_presets(args):
    """--native / --rapid -> args.start_model, args.end_model (deepbinner.py:283-300, same
    messages) -> how many models the run has."""
    chosen = [name for name in PRESETS if getattr(args, name)]
    if len(chosen) > 1:
        sys.exit('Error: you can only use one model preset (--native or --rapid)')
    if chosen:
        if args.start_model is not None or args.end_model is not None:
            sys.exit('Error: you cannot explicitly specify a model and '
                     'also use a model preset (--{})'.format(chosen[0]))
        start, end = PRESETS[chosen[0]]
        args.start_model = find_model(start)
        args.end_model = find_model(end) if end else None
    return sum(m is not None for m in (args.start_model, args.end_model))


def two_model_args_used(args):
    return sum(bool(getattr(args, flag)) for flag in TWO_MODEL_FLAGS)


def find_model(model_name):
    """Where the reference looks - ``models/`` beside or inside the package (deepbinner.py:332-345)
    - first for the Keras file, then for this package's converted ``.dbw``."""
    here = pathlib.Path(__file__).resolve()
    candidates = [base / name
                  for base in (here.parents[1] / 'models', here.parents[0] / 'models')
                  for name in (model_name, model_name + '.dbw')]
    for path in candidates:
        if path.is_file():
            return str(path)
    sys.exit('Error: could not find {} - did Deepbinner install correctly?'.format(model_name))


if __name__ == '__main__':
    main()
