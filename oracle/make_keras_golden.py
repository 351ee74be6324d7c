#!/usr/bin/env python3
"""
ORACLE tooling - a Keras model file of the reference as a fixture,
``tests/golden/keras/EXP-NBD103_read_starts.gz``, for ``test_keras_model_file_import``.

The reference's ``models/EXP-NBD103_read_starts`` (Keras 2.1.4 HDF5, 1.4 MB) holds the model's
weights, its ``model_config`` / ``training_config`` attributes and the optimizer's state (two thirds
of the file).  The importer reads ``model_weights`` and ``model_config`` only, so the optimizer's
datasets keep their place in the file and their values are zeroed: the file stays the same HDF5
structure byte for byte elsewhere, and compresses to ~0.4 MB (gzip, no timestamp).  Data only.

    python oracle/make_keras_golden.py REFERENCE_CHECKOUT
"""
import gzip
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from deepbinner_amd import hdf5_lite             # noqa: E402
from deepbinner_amd.hdf5_lite import _u          # noqa: E402

NAME = 'EXP-NBD103_read_starts'


def optimizer_spans(f):
    """(file offset, bytes) of every dataset under /optimizer_weights (contiguous layout)."""
    spans = []

    def walk(group):
        for key in group.keys():
            obj = group[key]
            if isinstance(obj, hdf5_lite.Group):
                walk(obj)
                continue
            lay = obj._first(0x0008)
            version, kind = f._buf[lay.off], f._buf[lay.off + 1]
            if (version, kind) != (3, 1):
                raise SystemExit('%s: not a contiguous v3 layout' % obj.name)
            count = int(np.prod(obj.shape)) if obj.shape else 1
            spans.append((f._base + _u(f._buf, lay.off + 2, f._O), count * obj.dtype.itemsize))

    walk(f['optimizer_weights'])
    return spans


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    src = os.path.join(sys.argv[1], 'models', NAME)
    data = bytearray(open(src, 'rb').read())
    with hdf5_lite.File(src) as f:
        spans = optimizer_spans(f)
    for start, size in spans:
        data[start:start + size] = bytes(size)
    out_dir = os.path.join(REPO, 'tests', 'golden', 'keras')
    os.makedirs(out_dir, exist_ok=True)
    with gzip.GzipFile(os.path.join(out_dir, NAME + '.gz'), 'wb', compresslevel=9, mtime=0) as g:
        g.write(bytes(data))
    print('%d optimizer datasets zeroed (%d bytes)' % (len(spans), sum(s for _, s in spans)))


if __name__ == '__main__':
    main()
