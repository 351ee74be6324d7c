#!/usr/bin/env python3
"""
Writes a directory of fast5 files for oracle/_build/loader_host_test beyond tests/golden/fast5:
what the loader's tests build in their temporary directories, side by side.

    python tools/loader_spot_inputs.py DIR
    oracle/_build/loader_host_test $(find tests/golden/fast5 DIR -name '*.fast5')

- vbz_*: a VBZ copy of every golden file (tests/test_vbz.py's copies: with and without a zstd
  stage, one chunk and several, a chunk stored raw)
- the shuffled one-read copies of tests/test_shuffle.py (with and without deflate and fletcher32,
  and plain deflate) and a shuffled container of 40 reads
- deflated_50: a container of 50 deflated reads of 2,000 to 9,000 samples
- long_streams: a container whose deflate streams are all above 64 KiB
- truncated: deflated_50 cut short;  flipped: a container with a byte changed inside a stream
Nothing here is committed; the files are the same from run to run.
"""
import os
import pathlib
import sys
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

import shuffle_fixtures as sf      # noqa: E402
import test_shuffle                # noqa: E402
import vbz_fixtures as vf          # noqa: E402
from deepbinner_amd import hdf5_write      # noqa: E402


def container(path, lengths, seed):
    rng = np.random.default_rng(seed)
    reads = []
    for i, n in enumerate(lengths):
        signal = sf.squiggle(rng, int(n))
        reads.append(('%08x-0000-4000-8000-%012x' % (seed, i), signal, None,
                      zlib.compress(signal.tobytes(), 1)))
    with open(path, 'wb') as f:
        f.write(hdf5_write.multi_read_fast5_bytes(reads))
    return reads


def main(out):
    os.makedirs(out, exist_ok=True)
    for k, path in enumerate(vf.golden_fast5()):
        vf.write_vbz_copy(vf.read_all(path), os.path.join(out, 'vbz_%02d_%s' % (k, os.path.basename(path))),
                          vf.VARIANTS[k % len(vf.VARIANTS)])
    test_shuffle.copies(pathlib.Path(out))
    sf.small_container(os.path.join(out, 'shuffled_40.fast5'), n_reads=40)

    rng = np.random.default_rng(50)
    container(os.path.join(out, 'deflated_50.fast5'), rng.integers(2000, 9001, 50), 50)
    long_reads = container(os.path.join(out, 'long_streams.fast5'), [120000, 150000, 131072, 200000], 64)
    assert all(len(r[3]) > 64 * 1024 for r in long_reads)

    whole = open(os.path.join(out, 'deflated_50.fast5'), 'rb').read()
    with open(os.path.join(out, 'truncated.fast5'), 'wb') as f:
        f.write(whole[:len(whole) * 3 // 5])
    path = os.path.join(out, 'flipped.fast5')
    stream = container(path, [3000, 5000, 8000, 4000], 7)[2][3]
    image = bytearray(open(path, 'rb').read())
    at = image.index(stream)
    image[at + len(stream) // 2] ^= 0x10
    with open(path, 'wb') as f:
        f.write(image)
    print('%d files in %s' % (len([n for n in os.listdir(out) if n.endswith('.fast5')]), out))


if __name__ == '__main__':
    main(sys.argv[1])
