"""A helper, not a test: training-data text as Python itself writes it - the contract of
``include/deepbinner_hip.h``, "training-data text, written"  - and the rows
that the formatter's tests, with and without a device, share."""
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
