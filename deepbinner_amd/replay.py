"""
The ``replay`` command: play recorded reads back as a sequencer would deliver them and call each
read's barcode WHILE its signal arrives.  Not a command of the reference, whose every entry takes
whole reads: ``classify`` starts when the read has left the pore and its file is written.  Barcode-
aware adaptive sampling - eject a read, balance a barcode - has to decide from the first second of
signal, while the molecule is still in the pore.

``--channels`` reads are in flight at a time, one per channel of a live session
(``hip_backend.LiveSession``: include/deepbinner_hip.h, "live").  Each round pushes the next
``--chunk_samples`` samples (1600: 0.4 s at 4 kHz) of every open read; a read's last chunk carries
END, and the channel then begins the next read in file order.  The session runs every window that
became complete through the start model and folds it; a read is DECIDED at the first window, from
``--min_windows`` on, whose best class is a barcode leading by ``--score_diff``, and FINAL when all
``--scan_size`` samples' windows are in - what ``classify`` with the start model alone calls.

One row per read, in file order: ``read_ID``, ``live_call``, ``decided_windows``,
``decided_samples`` (how much of the read had arrived at the push that decided; ``-`` where nothing
decided), ``final_call`` (``-`` under ``--stop_on_decision`` when the read never became FINAL),
``samples`` and ``agree`` (``yes`` / ``no``; ``-`` where either call is missing).  A summary goes to
stderr.  An early call can differ from the final one by construction - a later window may raise
another barcode - and ``agree`` is there to choose ``--min_windows`` and ``--score_diff`` by.  All of
this is what the network says on prefixes of recorded reads; nothing has been checked on a
sequencer.

Without ``--both_ends`` only the start model is used: the end of a read is not known while it
arrives.  ``-e`` alone is refused, a preset's end model is ignored.  With ``--both_ends`` the session
is a pair session (both models: ``-s`` and ``-e``, or a preset): the push that carries a read's END
also runs the end model over the read's last ``--scan_size`` samples and combines the two sides as
``classify`` does, under ``--require_either`` / ``--require_start`` / ``--require_both``.  Two columns
follow ``agree``: ``end_call``, and ``read_call`` = ``combine_calls`` of the start side and
``end_call``.  The start side is ``final_call`` where the read became FINAL; under
``--stop_on_decision`` a read stops at its decision, and ``read_call`` is then combined from the
early start call (``live_call``), not from a final one.  The summary gains one line: how many
reads were called from the start only, the end only, both sides in agreement, and how many had both
sides disagree.  ``replay(args, backend=None)`` takes its device entries as a parameter, so that the loop and the table also run against a host stand-in
(tests/live_reference.py).  ``--devices``: a replay runs on one GPU; a value above 1 is refused.

A yield policy (include/deepbinner_hip.h, "Yield policies") makes the replay a simulation of
barcode-aware adaptive sampling.  ``--balance 1,2,5`` balances those barcodes (``1:2,2:1`` gives
integer shares): a decided read is ejected while its barcode's yield, divided by its share, is more
than ``--slack_samples`` ahead of the balanced barcode that has yielded least.  ``--deplete LIST``
always ejects those barcodes; ``--keep LIST`` keeps those and ejects every other barcode; a barcode
named nowhere is kept.  ``--eject_undecided`` ejects a read that ends without a decision.  After
the push that returns EJECT a read delivers ``--eject_samples`` more samples (default: one
``--chunk_samples``; at most what it has left) in the usual chunks and ends there - with 0 an empty
END chunk goes in the next round - and the channel begins the next read.  That delay is a parameter
of the simulation, not a measurement.  Two columns are added at the end: ``action`` (``keep`` /
``eject`` / ``-``) and ``delivered``, the samples pushed; ``samples`` stays what the recorded read
holds.  A table on stderr gives, per barcode that occurred, the reads, the reads ejected, the samples
delivered and the samples the recorded reads hold - the yield without a policy - then the number of
rounds.  Recorded reads and an assumed ejection delay: nothing of this is checked on a sequencer.
"""
import sys

import numpy as np

KEEP_ALL = 1 << 40              # samples per read end the loaders keep: every read whole
NO_TRAINING_DATA = ('Error: a training-data file cannot be replayed - its samples are one window '
                    'long, not reads that arrive')
NO_START_MODEL = ('Error: replay needs a start model (-s, --native or --rapid) - the end of a read '
                  'is not known while it arrives')
NO_PAIR = ('Error: replay --both_ends needs a start model and an end model (-s and -e, --native or '
           '--rapid)')
HEADER = ['read_ID', 'live_call', 'decided_windows', 'decided_samples', 'final_call', 'samples',
          'agree']
PAIR_HEADER = HEADER + ['end_call', 'read_call']
POLICY_COLUMNS = ['action', 'delivered']
MAX_WEIGHT = 1 << 20            # DBH_LIVE_MAX_WEIGHT


def parse_barcode_list(text, flag, n_classes, shares=False):
    """``1,2,5`` (with ``shares``: also ``1:2,2:1``) -> {barcode: share}; one-line errors."""
    out = {}
    for item in (part.strip() for part in text.split(',')):
        name, _, share = item.partition(':')
        if not name.isdigit() or (share and not (shares and share.isdigit())) or \
                (':' in item and not share):
            sys.exit('Error: {} takes barcode numbers separated by commas{} (got {!r})'.format(
                flag, ', each with an optional :share' if shares else '', item))
        barcode, share = int(name), int(share) if share else 1
        if barcode < 1 or barcode >= n_classes:
            sys.exit('Error: {} names barcode {}, but the model has barcodes 1 to {}'.format(
                flag, barcode, n_classes - 1))
        if share < 1 or share > MAX_WEIGHT:
            sys.exit('Error: {} share of barcode {} must be from 1 to {}'.format(
                flag, barcode, MAX_WEIGHT))
        if barcode in out:
            sys.exit('Error: {} names barcode {} twice'.format(flag, barcode))
        out[barcode] = share
    return out


def parse_policy(args, n_classes):
    """The policy flags as ``LiveSession``'s ``policy`` -> (dict or None, eject_samples)."""
    lists = {flag: getattr(args, flag, None) for flag in ('balance', 'deplete', 'keep')}
    slack = int(getattr(args, 'slack_samples', 0) or 0)
    eject_undecided = bool(getattr(args, 'eject_undecided', False))
    eject_samples = getattr(args, 'eject_samples', None)
    given = {flag: parse_barcode_list(text, '--' + flag, n_classes, shares=flag == 'balance')
             for flag, text in lists.items() if text is not None}
    if not given and not eject_undecided:
        if slack or eject_samples is not None:
            sys.exit('Error: --slack_samples and --eject_samples need a policy (--balance, '
                     '--deplete, --keep or --eject_undecided)')
        return None, 0
    if slack < 0:
        sys.exit('Error: --slack_samples cannot be negative')
    if eject_samples is not None and eject_samples < 0:
        sys.exit('Error: --eject_samples cannot be negative')
    if slack and 'balance' not in given:
        sys.exit('Error: --slack_samples needs --balance')
    names = list(given)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            both = sorted(set(given[a]) & set(given[b]))
            if both:
                sys.exit('Error: barcode {} is named by --{} and by --{}'.format(both[0], a, b))
    weights = np.full(n_classes, 0 if 'keep' in given else -1, dtype=np.int32)
    weights[0] = -1
    for barcode in given.get('keep', {}):
        weights[barcode] = -1
    for barcode in given.get('deplete', {}):
        weights[barcode] = 0
    for barcode, share in given.get('balance', {}).items():
        weights[barcode] = share
    policy = dict(weights=weights, slack_samples=slack,
                  undecided='eject' if eject_undecided else 'keep')
    return policy, int(args.chunk_samples if eject_samples is None else eject_samples)


def reads_in_file_order(units, sweep):
    """(read id, int16 signal) of every read of every unit, as the loaders give them."""
    for unit in units:
        if hasattr(unit, 'samples'):
            samples, offsets = unit.samples, unit.offsets
        else:
            samples, offsets = sweep.pack(unit.signals, KEEP_ALL)
        for r, read_id in enumerate(unit.ids):
            yield read_id, np.asarray(samples[offsets[r]:offsets[r + 1]], dtype=np.int16)


def result_row(read_id, result, backend, call_name):
    """A read's last record as the table's row, and (decided, agrees or None) for the summary."""
    decided = int(result['decided_windows']) > 0
    final = int(result['status']) == backend.LIVE_FINAL
    agree = (int(result['call']) == int(result['final_call'])) if decided and final else None
    row = [read_id,
           call_name(int(result['call'])) if decided else 'none',
           str(int(result['decided_windows'])) if decided else '-',
           str(int(result['decided_samples'])) if decided else '-',
           call_name(int(result['final_call'])) if final else '-',
           str(int(result['samples'])),
           '-' if agree is None else ('yes' if agree else 'no')]
    return row, decided, agree


def replay(args, backend=None):
    from . import classify, sweep
    if backend is None:
        from . import hip_backend as backend
    if int(getattr(args, 'devices', 0) or 0) > 1:
        sys.exit('Error: a replay runs on one GPU (--devices {} is not supported)'
                 .format(args.devices))
    both_ends = bool(getattr(args, 'both_ends', False))
    if both_ends and (args.start_model is None or getattr(args, 'end_model', None) is None):
        sys.exit(NO_PAIR)
    if args.start_model is None:
        sys.exit(NO_START_MODEL)
    if args.channels < 1 or args.channels > 16384:
        sys.exit('Error: --channels must be from 1 to 16384')
    if args.chunk_samples < 1:
        sys.exit('Error: --chunk_samples must be at least 1')
    if args.min_windows < 1:
        sys.exit('Error: --min_windows must be at least 1')
    classify.refuse_pod5(args.input, 'replay')
    kind = classify.determine_input_type(args.input)
    if kind == 'training_data':
        sys.exit(NO_TRAINING_DATA)
    classify.set_tensorflow_threads(args)
    model, size, end_model, end_size, n_classes, _ = classify.load_and_check_models(
        args.start_model, args.end_model if both_ends else None, args.scan_size)
    scan_size = int(args.scan_size)
    if args.min_windows > scan_size // (size // 2):
        sys.exit('Error: --min_windows cannot be more than the {} windows of --scan_size'
                 .format(scan_size // (size // 2)))
    fast5s = (classify.find_all_fast5s(args.input, verbose=True) if kind == 'directory'
              else [args.input])
    units = sweep.fast5_units(fast5s, args, classify, KEEP_ALL, (size, end_size), n_classes,
                              command='replay')
    policy, eject_samples = parse_policy(args, n_classes)
    reads = enumerate(reads_in_file_order(units, sweep))
    print('', file=sys.stderr)
    print('\t'.join((PAIR_HEADER if both_ends else HEADER) + (POLICY_COLUMNS if policy else [])))

    pair = dict(end_model=end_model, combine=classify.combine_mode(args)) if both_ends else {}
    if policy:
        pair['policy'] = policy
    session = backend.LiveSession(model, args.channels, scan_size=scan_size,
                                  score_diff=args.score_diff, min_windows=args.min_windows,
                                  stop_on_decision=bool(args.stop_on_decision), **pair)
    sides = {'start only': 0, 'end only': 0, 'both agree': 0, 'both disagree': 0}
    # per channel: [read number, id, signal, position] and, under a policy, the action taken and
    # how many samples the read delivers (all of them, until it is ejected)
    slots = [None] * args.channels
    by_barcode, rounds = {}, 0          # call -> [reads, ejected, delivered, recorded samples]
    rows, printed = {}, 0                       # finished rows that wait for their turn
    decided_samples, n_reads, n_agree, n_compared, n_late, n_never = [], 0, 0, 0, 0, 0
    exhausted = False
    try:
        while True:
            for ch in range(args.channels):
                if slots[ch] is None and not exhausted:
                    nxt = next(reads, None)
                    if nxt is None:
                        exhausted = True
                    else:
                        slots[ch] = [nxt[0], nxt[1][0], nxt[1][1], 0, None, len(nxt[1][1])]
            active = [ch for ch in range(args.channels) if slots[ch] is not None]
            if not active:
                break
            chunks, begin, end = [], [], []
            for ch in active:
                _, _, signal, at, _, limit = slots[ch]
                chunks.append(signal[at:min(at + args.chunk_samples, limit)])
                begin.append(at == 0)
                end.append(at + args.chunk_samples >= limit)
                slots[ch][3] = min(at + args.chunk_samples, limit)
            rounds += 1
            if policy:
                results, end_results, actions = session.push_policy(active, chunks, begin=begin,
                                                                    end=end)
            elif both_ends:
                results, end_results = session.push_pair(active, chunks, begin=begin, end=end)
            else:
                results = session.push(active, chunks, begin=begin, end=end)
            for i, (ch, result, last) in enumerate(zip(active, results, end)):
                if policy and slots[ch][4] is None and \
                        int(actions[i]['action']) != backend.LIVE_NO_ACTION:
                    ejected = int(actions[i]['action']) == backend.LIVE_EJECT
                    slots[ch][4] = 'eject' if ejected else 'keep'
                    if ejected:                 # the read goes on for the ejection delay
                        slots[ch][5] = min(slots[ch][5], slots[ch][3] + eject_samples)
                if not last:
                    continue
                number, read_id = slots[ch][0], slots[ch][1]
                row, decided, agree = result_row(read_id, result, backend, classify.call_name)
                if both_ends:
                    ended = end_results[i]
                    start_call, end_call = int(ended['start_call']), int(ended['end_call'])
                    row += [classify.call_name(end_call),
                            classify.call_name(int(ended['read_call']))]
                    if start_call and end_call:
                        sides['both agree' if start_call == end_call else 'both disagree'] += 1
                    elif start_call or end_call:
                        sides['start only' if start_call else 'end only'] += 1
                if policy:
                    recorded = len(slots[ch][2])
                    row[5] = str(recorded)
                    row += [slots[ch][4] or '-', str(int(result['samples']))]
                    tally = by_barcode.setdefault(int(result['call']), [0, 0, 0, 0])
                    tally[0] += 1
                    tally[1] += slots[ch][4] == 'eject'
                    tally[2] += int(result['samples'])
                    tally[3] += recorded
                rows[number] = row
                slots[ch] = None
                n_reads += 1
                if decided:
                    decided_samples.append(int(result['decided_samples']))
                    n_late += int(result['decided_windows']) > args.min_windows
                else:
                    n_never += 1
                if agree is not None:
                    n_compared += 1
                    n_agree += bool(agree)
            while printed in rows:
                print('\t'.join(rows.pop(printed)))
                printed += 1
    finally:
        session.close()
    print('{} reads, {} decided'.format(n_reads, len(decided_samples)), file=sys.stderr)
    if decided_samples:
        print('  decided_samples: median {}, maximum {}'.format(
            int(np.median(decided_samples)), max(decided_samples)), file=sys.stderr)
    print('  live call agrees with the final call: {} of {}'.format(n_agree, n_compared),
          file=sys.stderr)
    print('  decided later than window {}: {}, never: {}'.format(args.min_windows, n_late, n_never),
          file=sys.stderr)
    if both_ends:
        print('  barcode on: ' + ', '.join('{} {}'.format(name, count)
                                           for name, count in sides.items()), file=sys.stderr)
    if policy:
        print('  barcode\treads\tejected\tdelivered\trecorded', file=sys.stderr)
        for call in sorted(by_barcode):
            print('  ' + '\t'.join([classify.call_name(call)] + [str(v) for v in by_barcode[call]]),
                  file=sys.stderr)
        print('  rounds: {}'.format(rounds), file=sys.stderr)
