"""The strict grammar of training-data text (include/deepbinner_hip.h, "training-data text";
DESIGN.md section 22) restated with regular expressions, and the corpus that the CPU model
(dbh_text_parse_host) and the device entry (dbh_text_parse) are both held to.  Nothing here looks
at how the parser walks a line; the corpus is built so that its 1,024-byte steps and 16-byte
pieces fall everywhere."""
import functools
import random
import re

import numpy as np

OK, FORM, COUNT, RANGE = 0, 1, 2, 3
LINE = re.compile(rb'(0|-?[1-9][0-9]{0,8})\t([+-]?[0-9]{1,7}(?:,[+-]?[0-9]{1,7})*)\r?')


def line_kind(line, input_size):
    """A line without its LF -> (kind, label, values); label and values None unless OK."""
    m = LINE.fullmatch(line)
    if not m:
        return FORM, None, None
    values = [int(v) for v in m.group(2).split(b',')]
    if len(values) != input_size:
        return COUNT, None, None
    if min(values) < -32768 or max(values) > 32767:
        return RANGE, None, None
    return OK, int(m.group(1)), values


def parse_block(data, input_size):
    """What both entries return for a block: (rows {line: values}, labels {line: label}, kinds,
    first_bad_line); rows and labels of OK lines only."""
    assert data.endswith(b'\n')
    rows, labels, kinds = {}, {}, []
    for k, line in enumerate(data[:-1].split(b'\n')):
        kind, label, values = line_kind(line, input_size)
        kinds.append(kind)
        if kind == OK:
            rows[k], labels[k] = values, label
    bad = [k for k, kind in enumerate(kinds) if kind != OK]
    return rows, labels, kinds, (bad[0] if bad else -1)


def same_as_restatement(result, data, input_size):
    samples, labels, kinds, first_bad = result
    rows, want_labels, want_kinds, want_bad = parse_block(data, input_size)
    assert kinds.tolist() == want_kinds
    assert first_bad == want_bad
    assert samples.shape == (len(want_kinds), input_size) and samples.dtype == np.int16
    for k, values in rows.items():
        assert samples[k].tolist() == values, k
        assert int(labels[k]) == want_labels[k], k


def same_results(a, b):
    """two entries' results on one block: kinds, first bad line, rows and labels of OK lines"""
    assert np.array_equal(a[2], b[2]) and a[3] == b[3]
    ok = a[2] == OK
    assert np.array_equal(a[0][ok], b[0][ok]) and np.array_equal(a[1][ok], b[1][ok])


# ---- the corpus ------------------------------------------------------------------------------------
def line_of_length(n, label=b'7'):
    """a line of exactly n bytes, strict from 3 bytes on: label, TAB, values of 1 to 7 digits"""
    if n <= len(label):
        return label[:n]
    body, widths, k = b'', (1, 2, 7, 3, 5, 4, 6), 0
    room = n - len(label) - 1
    while len(body) < room:
        width = widths[k % 7]                       # wide ones with zeros in front: all in range
        body += b'%0*d,' % (width, (k * 37 + 5) % 10 ** min(width, 4))
        k += 1
    body = body[:room]
    if body.endswith(b','):
        body = body[:-1] + b'3'
    return label + b'\t' + body


SEAM_VALUES = 300      # '-32768,' is 7 bytes: over 2,100 bytes its start meets every place of a step


def corpus():
    """[(name, [lines without LF], input_size)]; every case is also run at all 16 alignments."""
    cases = []
    for n in list(range(1, 41)) + [1023, 1024, 1025, 2048, 2049]:
        line = line_of_length(n)
        cases.append(('length %d' % n, [line], max(line.count(b',') + 1, 1)))
    lengths = [line_of_length(n, b'-12') for n in range(1, 41)]
    cases.append(('lengths, 5 values', lengths, 5))
    seam = b'1\t' + b','.join([b'-32768'] * SEAM_VALUES)
    cases.append(('seams -32768', [seam, b'2\t' + b','.join([b'+32767'] * SEAM_VALUES), seam + b'\r'],
                  SEAM_VALUES))
    two = [b'1\t0000012,5', b'1\t00000123,5', b'1\t12345678,5', b'1\t+5,-0', b'1\t--5,1', b'1\t,5',
           b'1\t5,', b'1\t5,,5', b'1\t\t5,5', b'1\t5\t5', b'1 5,5', b'', b'1\t5,5\r', b'1\t5\r,5',
           b'1\t5,5\r\r', b'\r', b'1\t5,\x005', b'1\t5,\xc35', b'1\t5,5\xc3', b'01\t5,5', b'+1\t5,5',
           b'-0\t5,5', b'1234567890\t5,5', b'x\t5,5', b'-\t5,5', b'0\t5,5', b'-7\t5,5', b'00\t5,5',
           b'999999999\t5,5', b'-999999999\t1,2', b'2147483648\t1,2', b'1\t32768,0', b'1\t-32769,0',
           b'1\t32767,-32768', b'1\t9999999,1', b'1\t-9999999,+9999999', b'1\t5', b'1\t5,5,5',
           b'1\t99999,5,5', b'1\t99999', b'1\t+,5', b'1\t5,+', b'1\t5,-', b'1\t5,5,', b'\t5,5', b'1\t',
           b'1', b'1\t5 ,5', b' 1\t5,5', b'1\t5, 5', b'1_0\t5,5', b'1\t1_0,5', b'1\t5,5 ', b'1\t5;5',
           b'1\t0x5,5', b'1\t5.0,5', b'1\t1e3,5', b'12\t-0000001,+0000002', b'1\t+-5,5', b'1,2\t5,5',
           b'1\t5,5\t', b'-1-\t5,5', b'1-\t5,5', b'1\t5-,5', b'1\t5+5,5']
    cases.append(('two values', two, 2))
    cases.append(('one value', [b'3\t7', b'3\t-32768', b'3\t7,8', b'3\t', b'0\t+0', b'3\t70000',
                                b'3\t1234567', b'3\t12345678'], 1))
    rng = random.Random(22)
    wide = [random_strict_line(rng, 96) for _ in range(12)]
    wide.insert(7, wide[3].replace(b',', b',,', 1))
    wide.append(wide[0][:-1])
    cases.append(('96 values', wide, 96))
    long_lines = [b'11\t' + b','.join([b'-12345'] * 16384),
                  b'0\t' + b','.join(b'%d' % (i % 10) for i in range(16384)),
                  random_strict_line(rng, 16384),
                  b'5\t' + b','.join([b'-12345'] * 16383),
                  b'5\t' + b','.join([b'-12345'] * 8000 + [b'40000'] + [b'1'] * 8383)]
    cases.append(('16,384 values', long_lines, 16384))
    cases.append(('one line', [random_strict_line(rng, 96)], 96))
    return cases


def random_strict_line(rng, n_values, crlf=False):
    label = rng.choice([b'0', b'%d' % rng.randrange(1, 13), b'-%d' % rng.randrange(1, 10 ** 9),
                        b'%d' % rng.randrange(1, 10 ** 9)])
    values = []
    for _ in range(n_values):
        v = rng.choice([rng.randrange(-32768, 32768), rng.randrange(-9, 10), rng.randrange(300, 900)])
        text = b'%d' % abs(v)
        text = text.rjust(rng.randrange(len(text), 8), b'0') if rng.random() < 0.1 else text
        sign = b'-' if v < 0 else rng.choice([b'', b'', b'', b'+'])
        values.append(sign + text)
    return label + b'\t' + b','.join(values) + (b'\r' if crlf else b'')


# ---- beyond the corpus: more lines than the grid has waves, and lines past 16,384 values ------------
# 70,000 lines of 7 values: the parse kernel's 8,192 workgroups hold 32,768 waves, a line each, so
# lines 32,768.. are a wave's second and lines 65,536.. its third.  A variant names the lines it
# has refused: one each of FORM, COUNT and RANGE.
MANY_LINES, MANY_SIZE = 70000, 7
REFUSED = {0: (FORM, b'1\t5,,6,1,2,3,4'), 40000: (COUNT, b'1\t5,6,1,2,3,4'),
           69999: (RANGE, b'1\t5,6,1,40000,2,3,4')}
MANY_VARIANTS = [(0, 40000, 69999), (40000, 69999), (69999,)]
LONG_SIZES = [100003, 2 ** 20]
LONG_SHIFTS = (0, 1, 15)


@functools.lru_cache(maxsize=None)
def _many_strict_lines():
    # 2,003 lines of random_strict_line, every one used 34 or 35 times: 2,003 is prime, so line k
    # and line k + 32,768 (one wave's first and second) are never the same text
    rng = random.Random(70)
    pool = [random_strict_line(rng, MANY_SIZE, crlf=rng.random() < 0.1) for _ in range(2003)]
    return [pool[(5 * k) % 2003] for k in range(MANY_LINES)]


def many_lines(refused):
    """the block of MANY_LINES lines with REFUSED's lines at the indices `refused`"""
    lines = list(_many_strict_lines())
    for k in refused:
        lines[k] = REFUSED[k][1]
    return b''.join(line + b'\n' for line in lines)


@functools.lru_cache(maxsize=None)
def long_lines(input_size):
    """(lines, the OK line's values): an OK line of `input_size` values, the same with a value out
    of range three from its end, and the same a value short - kinds OK, RANGE, COUNT.  The OK
    line's values are those of one random_strict_line of 10,007 values, over and over: its text is
    no multiple of 16 bytes long, so every round falls elsewhere in the pieces and steps."""
    rng = random.Random(input_size)
    label, values = random_strict_line(rng, 10007).split(b'\t')
    values = values.split(b',')
    values = (values * (input_size // len(values) + 1))[:input_size]
    out_of_range = values[:-3] + [b'40000'] + values[-2:]
    lines = [label + b'\t' + b','.join(v) for v in (values, out_of_range, values[:-1])]
    return lines, [int(v) for v in values]


def block(lines, shift=0):
    """the lines as one block whose first line starts `shift` bytes behind a 16-byte boundary: a
    line of shift - 1 bytes (never a strict one) goes in front"""
    head = [b'#' * (shift - 1)] if shift else []
    return b''.join(line + b'\n' for line in head + list(lines)), len(head)


def blocks(shifts=range(16)):
    """(name, block, input_size, lines in front) over the corpus at every alignment; the three
    cases of long lines at four alignments"""
    for name, lines, input_size in corpus():
        for shift in shifts:
            if input_size == 16384 and shift not in (0, 1, 9, 15):
                continue
            data, skipped = block(lines, shift)
            yield '%s, shift %d' % (name, shift), data, input_size, skipped
