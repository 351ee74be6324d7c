#!/usr/bin/env python3
"""Shuffled containers (HDF5's shuffle filter + deflate) beside their unshuffled deflate twins
(the same reads), one GPU, on both routes of the raw loader:

    python tools/shuffle_rate.py [--reads 4000] [--mean-length 27000 100000] [--containers 2]
                                 [--threads 4 16] [--runs 3] [--out FILE]

Containers are written into a temporary directory through hdf5_write's ``signal_filter``
(tests/shuffle_fixtures.py): shuffle + deflate level 1, once as one chunk per read and once in
chunks of 3,125 samples (what h5py's automatic chunking gives a 50 k-sample read; a read of more
than 200 k samples in 64 chunks, the most the writer puts into a dataset; the last chunk of a read
is then partial and stays the host's on either route).  Per row - `deflate` (the twin),
`shuffle host` (the default: the loader's threads inflate and unshuffle), `shuffle gpu`
(shuffle='gpu': modes 4 / 5) - it reports
  - the GPU decode time per container: dbh_inflate over the container's raw streams, HIP events
    around the kernels.  For `shuffle gpu` also the same streams sent as plain zlib streams (the
    pair's own time on the shuffled bytes: their high-byte planes are long runs, which the twin
    never shows the resolver); the difference is the de-interleave's device time;
  - the share of the streams, and of the output bytes, that the loader left to the host (mode 1);
  - per size of the loader's team: host CPU us per read on the raw route (process CPU time over
    the stream divided by reads), the loader's reads/s, and end-to-end reads/s of one caller
    (raw stream -> dbh_classify_pair_deflated, both models).
--runs repeats every row (the spread between runs is what a difference has to exceed).
"""
import argparse
import os
import resource
import sys
import tempfile
import time
import uuid

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

CHUNK = 3125


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def chunk_of(index, n_samples):
    """CHUNK samples - more for a read beyond 64 chunks of them (200 k samples), which is as many
    as hdf5_write puts into a dataset's one B-tree node: then a 64th of the read."""
    return max(CHUNK, -(-n_samples // 64))


def write_set(directory, n_containers, n_reads, mean_length, seed):
    """-> {(kind, layout): paths}: kind 'deflate' | 'shuffle', layout 'one_chunk' | 'chunked'"""
    import shuffle_fixtures as sf
    rng = np.random.default_rng(seed)
    out = {}
    for c in range(n_containers):
        reads = []
        for _ in range(n_reads):
            n = int(np.clip(rng.lognormal(np.log(mean_length), 0.25), 2000, 400000))
            levels = np.repeat(rng.normal(450, 80, n // 8 + 1), 8)[:n]
            signal = np.clip(np.rint(levels + rng.normal(0, 8, n)), 0, 2047).astype(np.int16)
            reads.append((str(uuid.UUID(bytes=rng.bytes(16), version=4)), signal))
        for kind, pipeline in (('deflate', 'deflate'), ('shuffle', 'shuffle_deflate')):
            for layout, chunk in (('one_chunk', None), ('chunked', chunk_of)):
                path = os.path.join(directory, '%s_%s_%d_%02d.fast5' % (kind, layout, mean_length, c))
                sf.write_copy(reads, path, pipeline, chunk, level=1, multi=True)
                out.setdefault((kind, layout), []).append(path)
    return out


def as_plain_zlib(records):
    """mode-4 records as the zlib streams behind their prefixes, wanted N (= out_bytes here)"""
    from deepbinner_amd import fast5_native
    plain = records.copy()
    four = plain['mode'] == fast5_native.RAW_ZLIB_SHUFFLE
    plain['comp_offset'][four] += 4
    plain['comp_bytes'][four] -= 4
    plain['mode'][four] = fast5_native.RAW_ZLIB
    return plain


def decode_times(paths, shuffle):
    """-> (ms per container, ms per container with mode 4 sent as plain zlib or None, share of the
    streams left to the host, share of the output bytes)"""
    from deepbinner_amd import fast5_native, hip_backend
    decode_ms, plain_ms = [], []
    host_streams = streams = host_bytes = all_bytes = 0
    for _, ids, offsets, status, comp, records in fast5_native.stream_raw(paths, threads=16, shuffle=shuffle):
        out_bytes = int(offsets[-1]) * 2
        hip_backend.inflate(comp, records, out_bytes)              # (warm)
        decode_ms.append(min(hip_backend.inflate(comp, records, out_bytes)[2] for _ in range(3)))
        if shuffle == 'gpu':
            plain = as_plain_zlib(records)
            hip_backend.inflate(comp, plain, out_bytes)
            plain_ms.append(min(hip_backend.inflate(comp, plain, out_bytes)[2] for _ in range(3)))
        stored = records['mode'] == fast5_native.RAW_STORED
        host_streams += int(stored.sum())
        streams += len(records)
        host_bytes += int(records['out_bytes'][stored].sum())
        all_bytes += int(records['out_bytes'].sum())
    return (float(np.median(decode_ms)), float(np.median(plain_ms)) if plain_ms else None,
            host_streams / max(streams, 1), host_bytes / max(all_bytes, 1))


def loader_and_end_to_end(paths, start, end, threads, shuffle):
    from deepbinner_amd import fast5_native, hip_backend
    cpu0, t0, reads = cpu_seconds(), time.perf_counter(), 0
    for _, ids, offsets, status, comp, records in fast5_native.stream_raw(paths, threads=threads, shuffle=shuffle):
        reads += len(ids)
    loader_s, loader_cpu = time.perf_counter() - t0, cpu_seconds() - cpu0
    t0, calls, refused = time.perf_counter(), 0, 0
    for _, ids, offsets, status, comp, records in fast5_native.stream_raw(paths, threads=threads, shuffle=shuffle):
        got = hip_backend.classify_pair_deflated(start, end, comp, records, offsets, 6144, 0.5)
        calls += len(got[0])
        refused += int(np.count_nonzero(got[1]))
    e2e = time.perf_counter() - t0
    assert refused == 0, refused
    return 1e6 * loader_cpu / max(reads, 1), reads / loader_s, calls / e2e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--mean-length', type=int, nargs='+', default=[27000, 100000])
    ap.add_argument('--containers', type=int, default=2)
    ap.add_argument('--threads', type=int, nargs='+', default=[4, 16],
                    help="sizes of the loader's team (4: what the raw route takes per GPU by default)")
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    opts = ap.parse_args()
    from deepbinner_amd import hip_backend
    from deepbinner_amd.model_format import ModelWeights
    models = os.path.join(REPO, 'deepbinner_amd', 'models')
    start = hip_backend.HipModel(ModelWeights.load(os.path.join(models, 'EXP-NBD103_read_starts.dbw'))[0])
    end = hip_backend.HipModel(ModelWeights.load(os.path.join(models, 'EXP-NBD103_read_ends.dbw'))[0])
    lines = ['device: ' + hip_backend.device_name(0)]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    with tempfile.TemporaryDirectory() as d:
        for length in opts.mean_length:
            n_reads = opts.reads if length < 50000 else max(opts.reads // 4, 1)
            sets = write_set(d, opts.containers, n_reads, length, 2 + length)
            for layout in ('one_chunk', 'chunked'):
                for run in range(opts.runs):
                    for name, kind, route in (('deflate', 'deflate', 'host'), ('shuffle host', 'shuffle', 'host'),
                                              ('shuffle gpu', 'shuffle', 'gpu')):
                        paths = sets[(kind, layout)]
                        size = sum(os.path.getsize(p) for p in paths) / len(paths) / 2 ** 20
                        decode, plain, host_streams, host_bytes = decode_times(paths, route)
                        split = ''
                        if plain is not None:
                            split = ' (zlib pair on the shuffled bytes %.3f, de-interleave %.3f)' % (
                                plain, decode - plain)
                        say('run %d %-12s %5d reads x ~%6d samples, %-9s: %.1f MiB/container, GPU decode '
                            '%.3f ms/container%s, left to the host %.1f %% of the streams = %.1f %% of the bytes'
                            % (run + 1, name, n_reads, length, layout, size, decode, split,
                               100 * host_streams, 100 * host_bytes))
                        for threads in opts.threads:
                            cpu, loader, e2e = loader_and_end_to_end(paths, start, end, threads, route)
                            say('run %d %-12s %5d reads x ~%6d samples, %-9s, %2d loader threads: '
                                '%.1f us host CPU/read (loader alone %.0f reads/s), end to end %.0f reads/s'
                                % (run + 1, name, n_reads, length, layout, threads, cpu, loader, e2e))
    start.close()
    end.close()
    if opts.out:
        with open(opts.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
