"""
The ``locate`` command: where in the signal each barcode call comes from.  Not a command of the
reference, whose ``classify`` says which barcode a read carries and nothing about where.

The network already knows: it ends in ``conv1d_20 (1x1) -> ReLU -> global average -> softmax``
(network_architecture.py:91-93), so a class's logit is exactly the mean, over the positions of the
last stage, of that class's post-ReLU ``conv1d_20`` output - and each position is one cell of 128
samples.  That per-cell value is the class's EVIDENCE: a decomposition of the logit, not a
heuristic.  For the call of each side the command reports the window whose evidence peaks highest,
the run of cells around the peak at half its height or more, as samples [first, end) of the read,
the peak and the share of the window's evidence the run holds (include/deepbinner_hip.h, "locate").

This says where the NETWORK sees the barcode.  It has no ground truth: like ``scan`` it is checked
on what the network says, not on where the barcode is.

One row per read: ``read_ID``, ``barcode_call``, ``samples``, then per loaded model
``<side>_class``, ``<side>_first``, ``<side>_end``, ``<side>_peak`` and ``<side>_share``; a side
without a call prints ``-``.  ``barcode_call`` is ``combine_calls`` of the two side calls of this
same pass, which runs on the GENERAL path (the evidence is read there): it is the general path's
call, equal to ``classify``'s except where a read sits within rounding of a threshold.  A summary
goes to stderr.

``--occlude`` tests each location against the model (include/deepbinner_hip.h, "occlude"): the side
is called again with the located samples blanked to 0.0 - the value of a short window's zero pad -
(``out``), with everything BUT them blanked (``only``), and with an equally long control stretch at
the other end of the scanned region blanked (``ctrl``).  Six more columns per loaded side:
``<side>_out_call``, ``<side>_out_p``, ``<side>_only_call``, ``<side>_only_p``, ``<side>_ctrl_call``
and ``<side>_ctrl_p``, the call and the probability of the ORIGINAL class under each; ``-`` where
there is no result (no location, a span wholly in the padding, a control that would overlap the
span).  The summary then counts, among the located sides, how many lost their call under ``out``,
kept it under ``only`` and kept it under ``ctrl``.  Still no ground truth: the test is against the
network, not against where the barcode is.

``locate(args, backend=None)`` takes its device entries as a parameter, so that the loop, the checks
and the table also run against a host stand-in (tests/locate_reference.py).

``--devices``: a locate runs on one GPU; a value above 1 is refused.
"""
import sys

import numpy as np

KEEP_ALL = 1 << 40              # samples per read end the loaders keep: every read whole
NO_POSITIONS = ('Error: a training-data file cannot be located - its samples are one window long '
                'and have no position in a read')
COLUMNS = ('class', 'first', 'end', 'peak', 'share')
VARIANTS = ('out', 'only', 'ctrl')
OCCLUDE_COLUMNS = tuple(v + field for v in VARIANTS for field in ('_call', '_p'))


def location_fields(location):
    """The five columns of one side of a row."""
    if int(location['cls']) == 0:
        return ['-'] * len(COLUMNS)
    return [str(int(location['cls'])), str(int(location['first_sample'])),
            str(int(location['end_sample'])), '{:.1f}'.format(float(location['peak'])),
            '{:.2f}'.format(float(location['share']))]


def occlusion_fields(occlusion):
    """The six ``--occlude`` columns of one side of a row."""
    fields = []
    for v in VARIANTS:
        call = int(occlusion[v + '_call'])
        fields += ['-', '-'] if call < 0 else [str(call), '{:.4f}'.format(float(occlusion[v + '_p']))]
    return fields


def locate(args, backend=None):
    from . import classify, sweep
    if backend is None:
        from . import hip_backend as backend
    if int(getattr(args, 'devices', 0) or 0) > 1:
        sys.exit('Error: a locate runs on one GPU (--devices {} is not supported)'.format(args.devices))
    if args.batch_size < 1:
        sys.exit('Error: --batch_size must be at least 1')
    if args.start_model is None and args.end_model is None:
        sys.exit('Error: you must provide at least one model')
    classify.refuse_pod5(args.input, 'locate')
    kind = classify.determine_input_type(args.input)
    if kind == 'training_data':
        sys.exit(NO_POSITIONS)
    classify.set_tensorflow_threads(args)
    start_model, start_size, end_model, end_size, n_classes, _ = classify.load_and_check_models(
        args.start_model, args.end_model, args.scan_size)
    # the evidence is read on the general path: a general-kind model, whatever the geometry
    sides = [(side, backend.general_model(model)) for side, model in
             (('start', start_model), ('end', end_model)) if model is not None]
    scan_size = int(args.scan_size)
    occlude = bool(getattr(args, 'occlude', False))
    columns = COLUMNS + (OCCLUDE_COLUMNS if occlude else ())

    fast5s = (classify.find_all_fast5s(args.input, verbose=True) if kind == 'directory'
              else [args.input])
    units = sweep.fast5_units(fast5s, args, classify, KEEP_ALL, (start_size, end_size), n_classes,
                              command='locate')
    print('', file=sys.stderr)
    print('\t'.join(['read_ID', 'barcode_call', 'samples'] +
                    ['{}_{}'.format(side, column) for side, _ in sides for column in columns]))
    reads = done = 0
    shares = {side: [] for side, _ in sides}
    # per side: [located with a result, call gone under out], [.., kept under only], [.., under ctrl]
    tested = {side: {v: [0, 0] for v in VARIANTS} for side, _ in sides}
    total = len(fast5s)
    classify.print_classification_progress(0, max(total, 1), 'fast5s')
    for unit in units:
        if hasattr(unit, 'samples'):
            samples, offsets = unit.samples, unit.offsets
        else:
            samples, offsets = sweep.pack(unit.signals, KEEP_ALL)
        n = len(offsets) - 1
        if n > 0:
            lengths = np.diff(offsets)
            found = {}
            for side, model in sides:
                if occlude:
                    _, calls, locations, occlusions = backend.locate_occluded_packed(
                        model, samples, offsets, side, scan_size, args.score_diff)
                    for v in VARIANTS:
                        has = (occlusions['cls'] != 0) & (occlusions[v + '_call'] >= 0)
                        same = occlusions[v + '_call'][has] == occlusions['cls'][has]
                        tested[side][v][0] += int(has.sum())
                        tested[side][v][1] += int((~same).sum() if v == 'out' else same.sum())
                else:
                    _, calls, locations = backend.locate_packed(model, samples, offsets, side,
                                                                scan_size, args.score_diff)
                    occlusions = None
                found[side] = (calls, locations, occlusions)
                shares[side].extend(float(s) for s in locations['share'][locations['cls'] != 0])
            if len(sides) == 2:
                final = classify.combine_call_numbers(found['start'][0], found['end'][0], args)
            else:
                final = found[sides[0][0]][0]
            for r, read_id in enumerate(unit.ids):
                row = [read_id, classify.call_name(int(final[r])), str(int(lengths[r]))]
                for side, _ in sides:
                    row += location_fields(found[side][1][r])
                    if occlude:
                        row += occlusion_fields(found[side][2][r])
                print('\t'.join(row))
            reads += n
        done += unit.n_files
        classify.print_classification_progress(min(done, total), max(total, 1), 'fast5s')
    print('', file=sys.stderr)
    print('{} reads'.format(reads), file=sys.stderr)
    for side, _ in sides:
        if shares[side]:
            print('  {}: {} located, median share {:.2f}'.format(
                side, len(shares[side]), float(np.median(shares[side]))), file=sys.stderr)
        else:
            print('  {}: 0 located'.format(side), file=sys.stderr)
        if occlude:
            counts = tested[side]
            print('  {}: occluded: call lost under out {} of {}, kept under only {} of {}, kept '
                  'under ctrl {} of {}'.format(side, counts['out'][1], counts['out'][0],
                                               counts['only'][1], counts['only'][0],
                                               counts['ctrl'][1], counts['ctrl'][0]), file=sys.stderr)
