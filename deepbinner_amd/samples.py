"""
Host rules for cutting training samples out of raw reads by signal alone: what the reference's
``prep`` does behind its sequence stage, as functions with nothing of the device in them.

  ``parse_label``, ``read_labels``      which barcode a read carries, from a table: a sequencing
                                        summary as ``prep.py:81-104`` loads one (its rules and its
                                        two error messages), or the table ``classify`` writes
  ``around_signal``, ``from_middle``,   the cutting rules of ``prep_functions.py:156-233`` with the
  ``before_signal``, ``after_signal``,  generator passed in; each returns the slice's (start, end)
  ``cut``                               or None, and ``cut`` takes the slice as Python does
  ``oddly_spaced``                      ``signal_elements_oddly_spaced`` of either side
  ``barcoded_samples``,                 the sample counts and order of ``prep_native_start.py:
  ``plain_samples``                     169-222`` and ``prep_native_end.py:172-225``

A ``samples`` command on top of them - trim, adapter scan, barcode ranking and the text on the
device - is NOT in the package: its first run inside the whole GPU suite hung, the cause is not
known, and everything that run executed on or around the device is left out (DESIGN.md
section 24).  ``prep`` stays a refused command.
"""
import sys

# per side: samples around the barcode, beside the adapter, from the middle; samples of a read
# without a barcode; the bounds of the barcode-adapter gap (prep_native_start.py:30-40,
# prep_native_end.py:30-40)
COUNTS = {'start': dict(barcoded=2, beside=1, middle=1, plain=2, gap=(15, 90)),
          'end': dict(barcoded=4, beside=2, middle=2, plain=4, gap=(-100, -20))}
MIDDLE_MARGIN = 25000                              # prep_functions.py:189

TOO_LONG = 'skipping due to too-long barcode signal'
ODD_GAP = 'skipping due to odd adapter-barcode arrangement'


# ---- the label table -------------------------------------------------------------------------
def parse_label(text):
    """A table's barcode entry -> 0 (known to carry none), a barcode number, or None (no label:
    ``none``, ``unclassified``).  ``barcodeNN`` is NN (prep.py:102)."""
    text = text.strip().replace('barcode', '')
    if text in ('none', 'unclassified', ''):
        return None
    try:
        label = int(text)
    except ValueError:
        label = -1
    if label < 0:
        sys.exit('Error: {!r} is not a barcode label (a number, barcodeNN, none or unclassified)'
                 .format(text))
    return label


def read_labels(path):
    """{read id: label} from a tab-separated table with a header.  The table ``classify`` writes
    (header ``read_ID<TAB>barcode_call``): its first two columns, the first line passed over, as
    ``refine`` reads it.  Anything else is taken as a sequencing summary, with the reference's
    rules and its two error messages (prep.py:81-104)."""
    labels = {}
    read_id_column = barcode_column = None
    with open(path, 'rt') as table:
        for line in table:
            parts = line.strip().split('\t')
            if read_id_column is None:
                if parts[:2] == ['read_ID', 'barcode_call']:
                    read_id_column, barcode_column = 0, 1
                    continue
                try:
                    read_id_column = parts.index('read_id')
                except ValueError:
                    sys.exit('Error: {} does not have a read_id column'.format(path))
                try:
                    barcode_column = parts.index('barcode_arrangement')
                except ValueError:
                    sys.exit('Error: {} does not have a barcode_arrangement column'.format(path))
            if len(parts) <= max(read_id_column, barcode_column):
                continue
            if parts[read_id_column] != 'read_id':         # a header line, wherever it comes
                labels[parts[read_id_column]] = parse_label(parts[barcode_column])
    return labels


# ---- the cutting rules (each returns (start, end) of the slice, or None) -----------------------
def around_signal(rng, length, include_start, include_end, size):
    """prep_functions.py:156-181.  A ``randint`` over an empty range (an include range that
    begins before sample 0) drops the sample."""
    include_size = include_end - include_start
    min_start = max(0, include_start + include_size - size)
    try:
        start = rng.randint(min_start, include_start)
    except ValueError:
        return None
    end = start + size
    if end > length:
        end = length
        start = end - size
    return start, end


def from_middle(rng, length, size):
    """prep_functions.py:184-195"""
    try:
        start = rng.randint(MIDDLE_MARGIN, length - MIDDLE_MARGIN - size)
    except ValueError:
        return None
    return start, start + size


def before_signal(rng, before_point, size):
    """prep_functions.py:198-214"""
    try:
        start = rng.randint(0, before_point - size)
    except ValueError:
        return None
    return start, start + size


def after_signal(rng, length, after_point, size):
    """prep_functions.py:217-233"""
    try:
        end = rng.randint(after_point + size, length)
    except ValueError:
        return None
    return end - size, end


def cut(signal, span, size):
    """The slice as Python takes it (a start below 0 counts from the end), or None where it does
    not come out ``size`` long - the reference's ``len(training_sample) == signal_size``."""
    if span is None:
        return None
    piece = signal[span[0]:span[1]]
    return piece if len(piece) == size else None


def oddly_spaced(side, adapter, barcode, size, say):
    """signal_elements_oddly_spaced of the side (prep_native_start.py:152-166,
    prep_native_end.py:155-169) -> a verdict, or None."""
    if barcode[1] - barcode[0] >= size:
        return TOO_LONG
    if side == 'start':
        gap = barcode[0] - adapter[1]
        say('    adapter-barcode signal gap: {}'.format(gap))
    else:
        gap = adapter[0] - barcode[1]
        say('    barcode-adapter signal gap: {}'.format(gap))
    say('    barcode signal size: {}'.format(barcode[1] - barcode[0]))
    low, high = COUNTS[side]['gap']
    return ODD_GAP if gap < low or gap > high else None


def barcoded_samples(rng, signal, side, adapter, barcode, label, size, say):
    """make_barcoded_training_samples of the side -> [(label, int16 sample)]"""
    counts, name, rows = COUNTS[side], '{:02d}'.format(label), []
    for _ in range(counts['barcoded']):
        span = around_signal(rng, len(signal), barcode[0], barcode[1], size)
        if span is not None:
            say('    barcode {} sample taken from trimmed signal: {}-{}'.format(name, *span))
        rows.append((label, cut(signal, span, size)))
    for _ in range(counts['beside']):
        if side == 'start':
            span = before_signal(rng, adapter[1] - 50, size)
            what = 'trimmed signal start'
        else:
            span = after_signal(rng, len(signal), adapter[1] + 50, size)
            what = 'signal end'
        if span is not None:
            say('    no-barcode sample taken from {}: {}-{}'.format(what, *span))
        rows.append((0, cut(signal, span, size)))
    for _ in range(counts['middle']):
        span = from_middle(rng, len(signal), size)
        if span is not None:
            say('    no-barcode sample taken from middle of signal: {}-{}'.format(*span))
        rows.append((0, cut(signal, span, size)))
    return [(l, s) for l, s in rows if s is not None]


def plain_samples(rng, signal, side, adapter, size, say):
    """make_non_barcoded_training_samples of the side"""
    point = adapter[1] if side == 'start' else adapter[0]
    rows = []
    for _ in range(COUNTS[side]['plain']):
        span = around_signal(rng, len(signal), point - 10, point + 10, size)
        if span is not None:
            say('    no-barcode sample taken from trimmed signal: {}-{}'.format(*span))
        rows.append((0, cut(signal, span, size)))
    return [(l, s) for l, s in rows if s is not None]
