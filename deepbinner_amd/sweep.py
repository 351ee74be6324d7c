"""
The ``sweep`` command: what ``classify`` would call at EVERY scan size up to ``--max_scan_size`` and
at every ``--score_diffs`` threshold, out of one pass over the reads.  Not a command of the
reference, whose two numbers (``--scan_size`` 6144, ``--score_diff`` 0.5; deepbinner.py:106-113)
were chosen for its three models on its authors' data; with models of one's own the way to choose
them was one ``classify`` run per setting.

Window s of a read is the same samples whatever the scan size (classify.py:337-349) and the merge
over windows is a running min / max (classify.py:368-374), so the window pass at the largest scan
size holds every smaller one's merged vector; the device folds the prefixes
(``hip_backend.sweep_pair``: per read and scan size the best class and its lead over the runner-up)
and counts the outcomes of every (scan size, threshold, two-model rule) there
(``hip_backend.sweep_tally``).  Python sees whole arrays only, and prints one table at the end.

``sweep(args, backend=None)`` takes its device entries as a parameter, so that the loop, the checks
and the table also run against a host stand-in (tests/sweep_reference.py).

``--devices``: a sweep runs on one GPU; a value above 1 is refused.

``--live`` asks the other question the same pass answers: what ``replay --stop_on_decision`` would
decide EARLY, while the read arrives in chunks of ``--chunk_samples``, at every ``--min_windows``
from 1 to the windows of ``--max_scan_size`` and every threshold.  A live session's track is the
sweep's fold, and its decision is integers and comparisons over that track and the read's length
(include/deepbinner_hip.h, "early tally"), so the device counts every setting from the one window
pass (``hip_backend.sweep_early_tally``) where ``replay`` takes one run per setting.  One row per
(min_windows, score_diff, mode): how many reads were decided, never decided, agree with the call of
the whole scan, changed, lost it, were decided later than ``min_windows``; the sums of the deciding
window numbers, of the samples received at the decision and of those reads' lengths; ``push_median``,
the smallest push by which half of the decided reads were decided (0: none were); then the calls as
the sweep's table counts them - with two models the read call of a pair session stopped on its
decision.  The start model is required (``-e`` alone is refused as ``replay`` refuses it) and a
training-data file is refused.  Recorded reads, as ever: nothing here is checked on a sequencer.
"""
import sys

import numpy as np

MAX_PUSHES = 4096               # dbh_sweep_early_pushes refuses more

THRESHOLD_RANGE = ('Error: every --score_diffs value must be in the range (0, 1] (greater than 0 '
                   'and less than or equal to 1)')
DIFFERENT_SIZES = ('Error: the two models of a sweep must have the same input size (they have {} '
                   'and {})')


def parse_score_diffs(text):
    """'0.1,0.2,...' -> ascending thresholds without repeats, each in (0, 1]."""
    try:
        values = sorted({float(v) for v in str(text).split(',') if v.strip()})
    except ValueError:
        sys.exit('Error: --score_diffs must be a comma-delimited list of numbers')
    if not values:
        sys.exit('Error: --score_diffs must name at least one threshold')
    if not all(0.0 < v <= 1.0 for v in values):
        sys.exit(THRESHOLD_RANGE)
    return values


def load_models(args, classify):
    """-> (start model, end model, input size, class count) by ``classify``'s own loader and
    messages; two models must agree on the class count and - one fold serves both - the input
    size, of which half must divide ``--max_scan_size`` (check_input_size's message)."""
    loaded = []
    for filename in (args.start_model, args.end_model):
        loaded.append((None, None, None) if filename is None
                      else classify.load_trained_model(filename))
    sizes = [size for _, size, _ in loaded if size is not None]
    classes = [n for _, _, n in loaded if n is not None]
    if not sizes:
        sys.exit('Error: you must provide at least one model')
    if len(set(classes)) > 1:
        sys.exit('Error: two models have different number of barcode classes')
    if len(set(sizes)) > 1:
        sys.exit(DIFFERENT_SIZES.format(*sizes))
    classify.check_input_size(sizes[0], args.max_scan_size)
    if args.max_scan_size < sizes[0] // 2:
        sys.exit('Error: --max_scan_size must be at least half the model input size')
    return loaded[0][0], loaded[1][0], sizes[0], classes[0]


def pack(signals, keep):
    """Lists of signals -> (samples int16, offsets int64) as the C ABI takes them, the middle of
    a long read dropped as the native loader drops it: no window reaches past ``keep`` samples
    from either end."""
    parts = []
    for signal in signals:
        signal = np.asarray(signal)
        if signal.dtype != np.int16 and len(signal) and (signal.min() < -32768 or signal.max() > 32767):
            sys.exit('Error: signal values do not fit int16')
        if len(signal) > 2 * keep:
            signal = np.concatenate([signal[:keep], signal[len(signal) - keep:]])
        parts.append(np.asarray(signal, dtype=np.int16))
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)), offsets


def fast5_units(fast5_files, args, classify, keep, sizes, n_classes, command='sweep'):
    """The units of ``classify``'s loaders (containers.py): batches of one-read files, then - with
    ``--multi_read`` - the containers among them."""
    from . import containers
    from .load_fast5s import determine_single_or_multi_fast5s, reader_kind
    if not fast5_files:
        sys.exit('Error: no fast5 files found')
    multi_read = bool(getattr(args, 'multi_read', False))
    if not multi_read and determine_single_or_multi_fast5s(fast5_files) == 'multi':
        sys.exit('Error: deepbinner {} requires one-read-per-file fast5s - convert with '
                 'multi_to_single_fast5 before running, or give --multi_read'.format(command))
    units = containers.Units(args, sizes[0], sizes[1], n_classes, keep=keep,
                             threads=int(getattr(args, 'loader_procs', 0) or 0), skip_damaged=True)
    later = [] if multi_read else None
    if multi_read and determine_single_or_multi_fast5s(fast5_files, mixed_ok=True) == 'multi':
        later = fast5_files
    else:
        singles = fast5_files
        if multi_read and reader_kind() == 'python':
            later = [f for f in fast5_files if classify._python_holds_several_reads(f)]
            singles = [f for f in fast5_files if f not in set(later)]
        yield from classify.load_in_batches(singles, args, keep, later)
    if later:
        if reader_kind() == 'native':
            yield from containers.files_done(containers.packed_containers(later, units))
        else:
            yield from containers.files_done(containers.read_chunks(later, units))


def fast5_batches(fast5_files, args, classify, keep, sizes, n_classes, labels):
    """(samples, offsets, labels or None, files finished) per unit of ``fast5_units``."""
    for unit in fast5_units(fast5_files, args, classify, keep, sizes, n_classes):
        if hasattr(unit, 'samples'):
            samples, offsets = unit.samples, unit.offsets
        else:
            samples, offsets = pack(unit.signals, keep)
        known = None
        if labels is not None:
            known = np.array([-1 if labels.get(rid) is None else labels[rid] for rid in unit.ids],
                             dtype=np.int32).reshape(-1)
        yield samples, offsets, known, unit.n_files


def training_batches(path, args, keep):
    """The same for a training-data file (``label<TAB>v1,v2,...``): its labels are the labels."""
    with open(path, 'rt') as text:
        records = [line.rstrip().split('\t') for line in text if line.strip()]
    for first in range(0, len(records), args.batch_size):
        batch = records[first:first + args.batch_size]
        signals = [np.array([int(v) for v in values.split(',')]) for _, values in batch]
        for k, signal in enumerate(signals):
            if len(signal) and (signal.min() < -32768 or signal.max() > 32767):
                sys.exit('Error: line {} of {} holds signal values outside the int16 range'
                         .format(first + k + 1, path))
        samples, offsets = pack(signals, keep)
        yield samples, offsets, np.array([int(label) for label, _ in batch], dtype=np.int32), len(batch)


def live_batches(fast5_files, args, classify, keep, sizes, n_classes, labels):
    """``fast5_batches`` for ``--live``: the loaders keep every read whole, so that its length is
    known, and the pack clips it here; a fifth value, the lengths (int64), follows."""
    from .replay import KEEP_ALL
    for unit in fast5_units(fast5_files, args, classify, KEEP_ALL, sizes, n_classes):
        if hasattr(unit, 'samples'):
            signals = [unit.samples[unit.offsets[i]:unit.offsets[i + 1]]
                       for i in range(len(unit.offsets) - 1)]
        else:
            signals = unit.signals
        lengths = np.array([len(signal) for signal in signals], dtype=np.int64)
        samples, offsets = pack(signals, keep)
        known = None
        if labels is not None:
            known = np.array([-1 if labels.get(rid) is None else labels[rid] for rid in unit.ids],
                             dtype=np.int32).reshape(-1)
        yield samples, offsets, known, unit.n_files, lengths


def check_live(args, backend, input_size, max_scan_size, kind):
    """``--live`` and ``--chunk_samples`` -> chunk_samples (None: not live) and P, or a one-line error."""
    from .replay import NO_START_MODEL
    chunk = getattr(args, 'chunk_samples', None)
    if not getattr(args, 'live', False):
        if chunk is not None:
            sys.exit('Error: --chunk_samples needs --live')
        return None, None
    chunk = 1600 if chunk is None else int(chunk)
    if chunk < 1:
        sys.exit('Error: --chunk_samples must be at least 1')
    if args.start_model is None:
        sys.exit(NO_START_MODEL)
    if kind == 'training_data':
        sys.exit('Error: a training-data file cannot be swept with --live - its samples are one '
                 'window long, not reads that arrive')
    cap = max_scan_size + input_size // 2
    if -(-cap // chunk) > MAX_PUSHES:
        sys.exit('Error: --chunk_samples {} takes more than {} pushes to deliver the {} samples a '
                 'read is called from'.format(chunk, MAX_PUSHES, cap))
    return chunk, backend.sweep_early_pushes(input_size, max_scan_size, chunk)


def sweep(args, backend=None):
    from . import classify
    if backend is None:
        from . import hip_backend as backend
    classify.refuse_pod5(args.input, 'sweep')
    thresholds = parse_score_diffs(args.score_diffs)
    if int(getattr(args, 'devices', 0) or 0) > 1:
        sys.exit('Error: a sweep runs on one GPU (--devices {} is not supported)'.format(args.devices))
    if args.batch_size < 1:
        sys.exit('Error: --batch_size must be at least 1')
    classify.set_tensorflow_threads(args)
    start_model, end_model, input_size, n_classes = load_models(args, classify)
    half = input_size // 2
    max_scan_size = int(args.max_scan_size)
    steps = max_scan_size // half
    keep = classify.scanned_end_samples(max_scan_size, input_size)

    kind = classify.determine_input_type(args.input)
    chunk_samples, pushes = check_live(args, backend, input_size, max_scan_size, kind)
    labels = None
    if kind == 'training_data':
        if start_model is not None and end_model is not None:
            sys.exit('Error: training data can only be classified using a single model')
        # as classify does (classify.py:223-224): windows from the start of each signal,
        # whichever model was given
        start_model, end_model = (start_model if start_model is not None else end_model), None
        with open(args.input, 'rt') as text:
            total = sum(1 for line in text if line.strip())
        batches, what = training_batches(args.input, args, keep), 'training data'
    else:
        if getattr(args, 'labels', None):
            from .samples import read_labels
            labels = read_labels(args.labels)
        fast5s = (classify.find_all_fast5s(args.input, verbose=True) if kind == 'directory'
                  else [args.input])
        total = len(fast5s)
        sizes = (input_size if start_model is not None else None,
                 input_size if end_model is not None else None)
        batches = (live_batches if chunk_samples else fast5_batches)(
            fast5s, args, classify, keep, sizes, n_classes, labels)
        what = 'fast5s'
    labelled = kind == 'training_data' or labels is not None
    both = start_model is not None and end_model is not None

    print('', file=sys.stderr)
    if chunk_samples:
        counts = backend.sweep_early_counts(steps, len(thresholds), both, n_classes, pushes)
    else:
        counts = backend.sweep_counts(steps, len(thresholds), both, n_classes)
    done = reads = 0
    classify.print_classification_progress(0, max(total, 1), what)
    for samples, offsets, known, n_files, *lengths in batches:
        n = len(offsets) - 1
        if n > 0:
            start, end = backend.sweep_pair(start_model, end_model, samples, offsets, max_scan_size)
            known = known if labelled else None
            if chunk_samples:
                backend.sweep_early_tally(start, end, thresholds, n_classes, known, lengths[0],
                                          input_size, chunk_samples, counts)
            else:
                backend.sweep_tally(start, end, thresholds, n_classes, known, counts)
            reads += n
        done += n_files
        classify.print_classification_progress(min(done, total), max(total, 1), what)
    print('', file=sys.stderr)
    modes = backend.SWEEP_MODES if both else ('-',)
    if chunk_samples:
        print_live_table(counts, thresholds, modes, reads, n_classes, labelled)
    else:
        print_table(counts, [half * k for k in range(1, steps + 1)], thresholds, modes, reads,
                    n_classes, labelled)


def print_live_table(counts, thresholds, modes, reads, n_classes, labelled):
    """``--live``: one row per (min_windows, threshold, mode), nested and ordered as ``print_table``'s;
    the columns of the start side's early decision repeat in each mode's rows."""
    calls, early, _, pushes = counts
    columns = ['min_windows', 'score_diff', 'mode', 'reads', 'decided', 'never', 'agree', 'changed',
               'lost', 'late', 'windows_sum', 'push_median', 'samples_sum', 'length_sum',
               'classified', 'none']
    if labelled:
        columns += ['right', 'wrong', 'missed']
    print('\t'.join(columns + [str(c) for c in range(1, n_classes)]))
    for m in range(calls.shape[0]):
        for t, threshold in enumerate(thresholds):
            decided, agree, changed, lost, late, windows, samples, length = (
                int(v) for v in early[m, t])
            by_push, median = np.cumsum(pushes[m, t]), 0
            if decided:                 # the smallest push by which half of the decided reads were
                median = int(np.argmax(2 * by_push >= decided)) + 1
            for j, mode in enumerate(modes):
                cell = [int(v) for v in calls[m, t, j]]
                row = [m + 1, repr(float(threshold)), mode, reads, decided, reads - decided, agree,
                       changed, lost, late, windows, median, samples, length,
                       sum(cell[1:n_classes]), cell[0]]
                if labelled:
                    row += cell[n_classes:n_classes + 3]
                print('\t'.join(str(v) for v in row + cell[1:n_classes]))


def print_table(counts, scan_sizes, thresholds, modes, reads, n_classes, labelled):
    """One row per (scan size, threshold, mode), in that order of nesting, all ascending and the
    modes either, start, both."""
    columns = ['scan_size', 'score_diff', 'mode', 'reads', 'classified', 'none']
    if labelled:
        columns += ['right', 'wrong', 'missed']
    print('\t'.join(columns + [str(c) for c in range(1, n_classes)]))
    for k, scan_size in enumerate(scan_sizes):
        for t, threshold in enumerate(thresholds):
            for j, mode in enumerate(modes):
                cell = [int(v) for v in counts[k, t, j]]
                row = [scan_size, repr(float(threshold)), mode, reads, sum(cell[1:n_classes]), cell[0]]
                if labelled:
                    row += cell[n_classes:n_classes + 3]
                print('\t'.join(str(v) for v in row + cell[1:n_classes]))
