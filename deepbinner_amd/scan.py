"""
The ``scan`` command: flag reads that carry barcode signal INSIDE the read.  Not a command of the
reference, whose ``classify`` looks at the first and last ``--scan_size`` samples of a read and
nothing else (classify.py:337-357): a chimeric read - two molecules in one signal, the second one's
adapter and barcode somewhere in the middle - is called by whichever barcode sits at its ends, and
lands in a bin with the other molecule's sequence attached.  The reference's own evaluation
(scripts/assign_reads_to_reference.py) has a ``chimera`` verdict, but only after basecalling and
alignment.

Here every window of the read goes through the network - the same windows, one every half input
size, carried on to the read's other end (``HipModel.scan_packed``: ``dbh_scan_i16``) - and a run
of consecutive windows whose best class is one barcode, leading the runner-up by ``--score_diff``,
is an EVENT.  An event whose first window lies behind the ``--scan_size`` samples ``classify``
itself looks at is INTERIOR.  The models were trained with mid-read windows as the no-barcode class
(prep_native_start.py:217-219), so a barcode class leading there means something - but what has
been checked are synthetic junctions only (reads packed end to end); nothing has been validated on
real chimeric reads.

One row per read: ``read_ID``, ``barcode_call`` - ``classify``'s call for the same batch, to the
byte -, ``samples``, ``interior_events`` and ``events``: every event of the read, the start
model's then the end model's, as ``side:class:first_sample-end_sample:peak`` with absolute sample
positions [first, end) on both sides, or ``-``.  A summary goes to stderr.

``scan(args, backend=None)`` takes its device entries as a parameter, so that the loop, the checks
and the table also run against a host stand-in (tests/scan_reference.py).

``--devices``: a scan runs on one GPU; a value above 1 is refused.
"""
import sys

import numpy as np

KEEP_ALL = 1 << 40              # samples per read end the loaders keep: every read whole
NO_INTERIOR = ('Error: a training-data file cannot be scanned - its samples are one window long and '
               'have no interior')


def event_samples(side, first, last, n_samples, input_size):
    """[first sample, end sample) of the windows first .. last of a read (include/deepbinner_hip.h,
    "scan": window k of side start begins at k h, of side end it ends at n - k h)."""
    half = input_size // 2
    if side == 'start':
        return min(first * half, n_samples), min(last * half + input_size, n_samples)
    return max(n_samples - last * half - input_size, 0), max(n_samples - first * half, 0)


def event_text(side, event, n_samples, input_size):
    lo, hi = event_samples(side, int(event['first']), int(event['last']), n_samples, input_size)
    return '{}:{}:{}-{}:{:.3f}'.format(side, int(event['cls']), lo, hi, float(event['peak']))


def scan(args, backend=None):
    from . import classify, sweep
    if backend is None:
        from . import hip_backend as backend
    if int(getattr(args, 'devices', 0) or 0) > 1:
        sys.exit('Error: a scan runs on one GPU (--devices {} is not supported)'.format(args.devices))
    if args.batch_size < 1:
        sys.exit('Error: --batch_size must be at least 1')
    if args.min_windows < 1:
        sys.exit('Error: --min_windows must be at least 1')
    if args.start_model is None and args.end_model is None:
        sys.exit('Error: you must provide at least one model')
    classify.refuse_pod5(args.input, 'scan')
    kind = classify.determine_input_type(args.input)
    if kind == 'training_data':
        sys.exit(NO_INTERIOR)
    classify.set_tensorflow_threads(args)
    start_model, start_size, end_model, end_size, n_classes, _ = classify.load_and_check_models(
        args.start_model, args.end_model, args.scan_size)
    sides = [(side, model, size) for side, model, size in
             (('start', start_model, start_size), ('end', end_model, end_size)) if model is not None]
    scan_size = int(args.scan_size)
    mode = classify.combine_mode(args) if len(sides) == 2 else 'require_either'

    fast5s = (classify.find_all_fast5s(args.input, verbose=True) if kind == 'directory'
              else [args.input])
    units = sweep.fast5_units(fast5s, args, classify, KEEP_ALL, (start_size, end_size), n_classes,
                              command='scan')
    print('', file=sys.stderr)
    print('\t'.join(['read_ID', 'barcode_call', 'samples', 'interior_events', 'events']))
    reads = flagged = done = 0
    per_class = np.zeros(n_classes, dtype=np.int64)
    total = len(fast5s)
    classify.print_classification_progress(0, max(total, 1), 'fast5s')
    for unit in units:
        if hasattr(unit, 'samples'):
            samples, offsets = unit.samples, unit.offsets
        else:
            samples, offsets = sweep.pack(unit.signals, KEEP_ALL)
        n = len(offsets) - 1
        if n > 0:
            calls = backend.classify_pair(start_model, end_model, samples, offsets, scan_size,
                                          args.score_diff, mode)
            lengths = np.diff(offsets)
            texts = [[] for _ in range(n)]
            interior = np.zeros(n, dtype=np.int64)
            for side, model, size in sides:
                skip = scan_size // (size // 2)
                events = backend.scan_packed(model, samples, offsets, side, args.score_diff,
                                             args.min_windows, skip)
                for event in events:
                    r = int(event['read'])
                    texts[r].append(event_text(side, event, int(lengths[r]), size))
                    if event['first'] >= skip:
                        interior[r] += 1
                        per_class[int(event['cls'])] += 1
            for r, read_id in enumerate(unit.ids):
                print('\t'.join([read_id, classify.call_name(int(calls[r])), str(int(lengths[r])),
                                 str(int(interior[r])), ','.join(texts[r]) or '-']))
            reads += n
            flagged += int((interior > 0).sum())
        done += unit.n_files
        classify.print_classification_progress(min(done, total), max(total, 1), 'fast5s')
    print('', file=sys.stderr)
    print('{} reads, {} with at least one interior event'.format(reads, flagged), file=sys.stderr)
    for cls in np.flatnonzero(per_class):
        print('  barcode {}: {} interior events'.format(cls, int(per_class[cls])), file=sys.stderr)
