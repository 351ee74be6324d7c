"""A helper, not a test: training-data text as Python itself writes it - the contract of
``include/deepbinner_hip.h``, "training-data text, written"  - and the rows
that the formatter's tests, with and without a device, share."""
import functools

import numpy as np

MAX_LABEL = 10 ** 9 - 1
LABELS = [0, 7, 10, 255, -1, 999999999]
SIZES = [1, 2, 63, 64, 65, 1024, 16384]


def text(labels, samples):
    return b''.join('{}\t{}\n'.format(label, ','.join(map(str, row))).encode('ascii')
                    for label, row in zip(np.asarray(labels).tolist(), np.asarray(samples).tolist()))


def bound(n_lines, input_size):
    return n_lines * (12 + 7 * input_size)


def rows(input_size, seed=0):
    """int16 [6, input_size]: all -32768, all 0, alternating -32768 / 7, two full-range draws, and
    one of every width; with LABELS as their labels"""
    rng = np.random.RandomState(seed + input_size)
    widths = np.array([0, -1, 9, -9, 10, -10, 99, 100, -100, 999, 1000, -1000, 9999, 10000, -10000,
                       32767, -32768, -32767])
    out = np.zeros((6, input_size), dtype=np.int16)
    out[0] = -32768
    out[2] = np.where(np.arange(input_size) % 2 == 0, -32768, 7)
    out[3] = rng.randint(-32768, 32768, size=input_size)
    out[4] = rng.randint(-32768, 32768, size=input_size)
    out[5] = widths[np.arange(input_size) % len(widths)]
    return np.array(LABELS, dtype=np.int32), out


def many_short_lines(n, seed=3):
    """n lines of one value: the scan over lines gets more lines than it has threads"""
    rng = np.random.RandomState(seed)
    labels = rng.choice(LABELS, size=n).astype(np.int32)
    return labels, rng.randint(-32768, 32768, size=(n, 1)).astype(np.int16)


# Rows of more than 16,384 values, kept out of SIZES (which the tests multiply by other
# parameters): 100,003 is no multiple of 64, so a wave's last step of 64 values is a partial one,
# and 2^20 is the longest row the entries take (16,384 steps; several million bytes carried).
LONG_SIZES = [100003, 2 ** 20]
# More lines than the scan over tiles of 1,024 lines has threads: 1,075 tiles, two to a thread,
# the last busy thread with one.  SPLIT is no multiple of 1,024.
MANY_LINES, SPLIT = 1100000, 500003


@functools.lru_cache(maxsize=None)
def long_rows(input_size):
    """(labels, samples [2, input_size], Python's text of them), once per size: the row of every
    width in turn and a full-range draw, under the widest label and -1"""
    _, samples = rows(input_size)
    labels, samples = np.array([999999999, -1], dtype=np.int32), samples[[5, 3]].copy()
    samples.setflags(write=False)
    labels.setflags(write=False)
    return labels, samples, text(labels, samples)


@functools.lru_cache(maxsize=None)
def many_lines():
    """(labels, samples, Python's text) of many_short_lines(MANY_LINES), once"""
    labels, samples = many_short_lines(MANY_LINES)
    samples.setflags(write=False)
    labels.setflags(write=False)
    return labels, samples, text(labels, samples)
