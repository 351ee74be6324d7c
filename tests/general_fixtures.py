"""Models of other geometries than the shipped ones, made at test time from the shipped weights
(no committed fixtures): the convolution and batch-norm weights do not depend on the input size,
so a shipped model reloaded with another ``input_size`` is a valid model with realistic outputs;
other class counts widen (or narrow) ``conv1d_20`` from its 13 real columns with seeded ~1 %
perturbations."""
import os

import numpy as np

from conftest import GOLD, MODEL_DIR
from deepbinner_amd.model_format import ModelWeights

STARTS = 'EXP-NBD103_read_starts'
ENDS = 'EXP-NBD103_read_ends'

# (input size, class count) of the general path's log-space tests: every stage length len[1..7]
# is odd at one of these sizes and even at another (tests/test_log_space_compare.py checks it).
# 98: len[1] = 49; 112: len[4] = 7; 160: len[6] = 3; 1502: len[5] = 46, len[6] = 23;
# 16382: len[1..5] = 8191, 4095, 2047, 1023, 511
PARITY_GEOMETRIES = [(96, 2), (98, 13), (112, 33), (160, 256), (1502, 17), (16382, 97)]


def shipped(name=STARTS):
    return ModelWeights.load(os.path.join(MODEL_DIR, name + '.dbw'))[0]


def geometry(input_size=1024, n_classes=13, name=STARTS, seed=0):
    """The shipped model ``name`` with another input size and / or class count."""
    w = shipped(name)
    convs = list(w.convs)
    if n_classes != w.n_classes:
        rng = np.random.default_rng(seed + 1000 * n_classes)
        kernel, bias = convs[-1]
        # class 0 stays class 0; barcode j takes a real barcode column, perturbed
        cols = [0] + [1 + (j - 1) % (w.n_classes - 1) for j in range(1, n_classes)]
        scale = 1.0 + 0.01 * rng.standard_normal(n_classes)
        k2 = (kernel[:, :, cols] * scale[None, None, :]).astype(np.float32)
        b2 = (bias[cols] * scale).astype(np.float32)
        convs[-1] = (np.ascontiguousarray(k2), np.ascontiguousarray(b2))
    return ModelWeights(n_classes, convs, w.bns, input_size=input_size)


def golden_signals():
    """The seven reads of the golden single-read files."""
    reads = np.load(os.path.join(GOLD, 'reads.npz'))
    offsets = reads['offsets']
    return [reads['samples'][offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


def synthetic_reads(input_size, scan_size, seed):
    """Lengths 0, below one window, about one window, and longer than twice the scan."""
    rng = np.random.default_rng(seed)
    lengths = [0, 1, input_size // 3, input_size - 1, input_size, input_size + 17,
               scan_size + input_size // 2, 2 * scan_size + input_size + 5]
    return [np.clip(rng.normal(500, 80, n), -32768, 32767).astype(np.int16) for n in lengths]


def save(weights, path):
    weights.save(str(path))
    return str(path)
