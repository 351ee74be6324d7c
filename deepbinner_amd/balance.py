"""
The ``balance`` command (reference ``deepbinner/balance.py``): from one or more training-data
files, as many samples of every barcode as the rarest barcode has, taken round-robin from the
files, and behind them synthetic no-barcode signals (``--random_signal`` times that many).

What is counted, which quotas follow and what is said on stderr are the reference's, byte for
byte (balance.py:31-129).  Each file is read once, as bytes: where its lines start and what their
labels are is kept, and a selected line is written as the slice of the file it is.  The selection
shuffles with Python's ``random.Random(seed)`` in the reference's order of calls - per file, each
barcode's list in the order barcodes first appear there; a shuffle depends on the list's length
alone, so shuffling indices gives the reference's permutation.  With ``--random_signal 0``, stdout
and stderr are what the reference writes after ``random.seed(seed)``.

Three deliberate differences.  ``--barcodes`` is split at commas, as its help says (the reference
walks the string's characters and raises ValueError at the first comma).  An empty input file is an
``Error:`` of ours (the reference raises TypeError, or reports a size of None).  And the random
signals follow the reference's law, not its Mersenne-Twister stream: value i of signal s is a
stateless function of (seed, s, i, signal size) (include/deepbinner_hip.h, "random signals"), with
gradient noise of hashed gradients where the reference calls ``noise.pnoise1``.  DESIGN.md
section 23.

The random signals are made and turned into text on the device, a chunk at a time
(``hip_backend.ResidentText``): generator and formatter queued on one stream, one synchronisation,
and only text comes down - the int16 values never visit the host; stream and buffers are made
once and kept from chunk to chunk.  ``balance`` takes the two device functions as parameters, so
that the whole command also runs on their host models (``hip_backend.random_signals(...,
host=True)`` and ``format_training_text(..., host=True)``).
"""
import random
import sys

import numpy as np

# a chunk of random signals is sized so that its text stays below this
TEXT_CHUNK_BYTES = 256 << 20
MAX_CHUNK_VALUES = 1 << 30          # dbh_random_signals: n_signals * input_size of one call


def barcode_name(barcode):
    return 'no barcode' if barcode == 0 else 'barcode {:02d}'.format(barcode)


def say(text=''):
    print(text, file=sys.stderr)


def write_bytes(data):
    out = sys.stdout
    out.flush()
    if hasattr(out, 'buffer'):
        out.buffer.write(data)
        out.buffer.flush()
    else:
        out.write(bytes(data).decode('utf-8', errors='surrogateescape'))


class TrainingFile:
    """One input file, read once: its bytes, where each line starts, each line's label."""

    def __init__(self, name):
        self.name = name
        with open(name, 'rb') as raw:
            self.data = raw.read()
        if not self.data:
            sys.exit('Error: {} is empty'.format(name))
        ends = np.flatnonzero(np.frombuffer(self.data, dtype=np.uint8) == 0x0a) + 1
        if not len(ends) or ends[-1] != len(self.data):
            ends = np.append(ends, len(self.data))       # a last line without a LF
        self.starts = np.concatenate(([0], ends)).astype(np.int64)
        self.labels = []
        for k in range(len(ends)):
            start, end = int(self.starts[k]), int(self.starts[k + 1])
            tab = self.data.find(b'\t', start, end)
            try:
                self.labels.append(int(self.data[start:tab if tab >= 0 else end]))
            except ValueError:
                sys.exit('Error: line {} of {} does not begin with an integer barcode class'
                         .format(k + 1, name))
        first = self.data[:self.starts[1]].strip().split(b'\t')
        if len(first) < 2:
            sys.exit('Error: line 1 of {} holds no signal'.format(name))
        self.signal_size = len(first[1].split(b','))
        self.counts = {}
        for label in self.labels:
            self.counts[label] = self.counts.get(label, 0) + 1

    def line(self, k):
        return self.data[self.starts[k]:self.starts[k + 1]]


def balance(args, signals=None, formatter=None):
    """``signals(seed, first, n, size)`` and ``formatter(labels, samples)``: both, or neither for
    the device's (a ResidentText made for this run's chunk size)."""
    if (signals is None) != (formatter is None):
        raise ValueError('balance takes both device functions or neither')
    if not args.random_signal >= 0.0:
        sys.exit('Error: --random_signal must be 0 or more')
    wanted = parse_barcodes(args.barcodes)
    seed = getattr(args, 'seed', 0)

    files = {}
    for name in args.training_data:
        if name not in files:
            files[name] = TrainingFile(name)
    signal_size = get_signal_size(files)
    counts = count_samples(args.training_data, files)
    barcodes = get_barcodes(counts, wanted)
    smallest_count = get_smallest_count(barcodes, counts)
    quotas = get_quotas(barcodes, counts, smallest_count)
    select_samples(args.training_data, files, quotas, random.Random(seed))
    add_random_signals(args.random_signal, smallest_count, signal_size, seed, signals, formatter)
    say()


def parse_barcodes(text):
    if text is None:
        return None
    try:
        return [int(part) for part in text.split(',')]
    except ValueError:
        sys.exit('Error: --barcodes takes a comma-delimited list of barcode numbers')


def get_signal_size(files):
    sizes = sorted({f.signal_size for f in files.values()})
    if len(sizes) != 1:
        sys.exit('Error: multiple signal sizes detected: {}'.format(sizes))
    say('\nSignal size detected as {}'.format(sizes[0]))
    return sizes[0]


def count_samples(names, files):
    say('\nCounting samples in input files:')
    for name in names:                                   # a file given twice is reported twice
        f = files[name]
        say('  {}'.format(name))
        for barcode in sorted(f.counts):
            say('    {}: {}'.format(barcode_name(barcode), f.counts[barcode]))
    return {name: f.counts for name, f in files.items()}


def get_barcodes(counts, wanted):
    if wanted is None:
        barcodes = sorted({barcode for c in counts.values() for barcode in c})
        say('\nIncluding all barcodes in output: {}'.format(', '.join(str(b) for b in barcodes)))
        return barcodes
    barcodes = sorted(wanted if 0 in wanted else wanted + [0])
    say('\nIncluding user-specified barcodes in output: {}'
        .format(', '.join(str(b) for b in barcodes)))
    return barcodes


def get_smallest_count(barcodes, counts):
    totals = [(barcode, sum(c.get(barcode, 0) for c in counts.values())) for barcode in barcodes]
    barcode, smallest = min(totals, key=lambda pair: pair[1])
    say('\nSmallest count = {} ({})'.format(smallest, barcode_name(barcode)))
    say('  all barcodes will be limited to this many samples')
    return smallest


def get_quotas(barcodes, counts, smallest_count):
    """{barcode: {file: samples to take}}: one sample from each file in turn, for as long as it has
    one, until the smallest count is reached; a file that the round never came to is not listed."""
    say('\nDetermining how many samples to take from each file:')
    quotas = {}
    for barcode in barcodes:
        say('  {}: '.format(barcode_name(barcode)))
        used, total = {}, 0
        while total < smallest_count:
            for name, c in counts.items():
                used.setdefault(name, 0)
                if used[name] < c.get(barcode, 0):
                    used[name] += 1
                    total += 1
                    if total == smallest_count:
                        break
        for name, count in used.items():
            say('    {}: {}'.format(name, count))
        quotas[barcode] = used
    return quotas


def select_samples(names, files, quotas, rng):
    say('\nSelecting samples and printing to stdout:')
    for name in names:
        f = files[name]
        say('  {}'.format(name))
        lines_of = {}
        for k, label in enumerate(f.labels):
            lines_of.setdefault(label, []).append(k)
        for label in lines_of:                         # the order barcodes first appear in the file
            rng.shuffle(lines_of[label])
        for barcode in sorted(quotas):
            number = quotas[barcode].get(name, 0)
            say('    {}: {}'.format(barcode_name(barcode), number))
            chosen = lines_of.get(barcode, [])[:number]
            if chosen:
                write_bytes(b''.join(f.line(k) for k in chosen))


def chunk_signals(signal_size, chunk_bytes=None):
    """how many random signals make one chunk: its text below chunk_bytes, its values within one call"""
    chunk_bytes = chunk_bytes or TEXT_CHUNK_BYTES
    by_text = chunk_bytes // (12 + 7 * signal_size)      # dbh_text_format_bound per line
    return max(1, min(by_text, MAX_CHUNK_VALUES // signal_size))


def add_random_signals(random_amount, smallest_count, signal_size, seed, signals, formatter):
    random_count = int(round(random_amount * smallest_count))
    say('\nAdding {} random signals as no-barcode training samples'.format(random_count))
    if random_count == 0:
        return
    per_chunk = min(chunk_signals(signal_size), random_count)
    resident = None
    if signals is None:
        from . import hip_backend
        resident = hip_backend.ResidentText(per_chunk, signal_size)
        signals, formatter = resident.random_signals, resident.format_training_text
    try:
        for first in range(0, random_count, per_chunk):
            n = min(per_chunk, random_count - first)
            samples = signals(seed, first, n, signal_size)
            text = formatter(np.zeros(n, dtype=np.int32), samples)
            write_bytes(text)
            del text                                     # a view of the resident buffer
    finally:
        if resident is not None:
            resident.close()
