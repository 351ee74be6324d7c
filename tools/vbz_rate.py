#!/usr/bin/env python3
"""VBZ containers beside their deflate twins (the same reads), one GPU:

    python tools/vbz_rate.py [--reads 4000] [--mean-length 27000] [--containers 4] [--runs 3] [--out FILE]

Per container set it reports
  - the GPU decode time per container: dbh_inflate over the container's raw streams (zlib pair for
    the twin, the streamvbyte kernel for VBZ), HIP events around the kernels;
  - host CPU us per read on the raw route (f5_stream_open_raw: parsing, preads, and for VBZ the
    zstd stage, which is host work), split as tools/gpu_inflate_split.py splits it: process CPU
    time over the stream divided by reads;
  - end-to-end reads/s of raw stream -> dbh_classify_pair_deflated (both models), the path
    `deepbinner classify --native` / `realtime` take over multi-read containers.
The VBZ containers are measured on both routes in the same process: `vbz host` (the loader's
threads undo the zstd stage, the GPU gets mode 2) and `vbz gpu` (vbz_zstd='gpu': the chunks go out
as stored, mode 3, and dbh_zstd.hip undoes the zstd stage in front of the streamvbyte kernel).  For
the gpu route the GPU decode time is zstd + streamvbyte together; the zstd stage's own share is
that minus the host route's streamvbyte-only time over the same container.  --runs repeats every
row (the spread between runs is what a difference has to exceed).
Containers are written into a temporary directory with the package's writer and the VBZ encoder
of tests/vbz_fixtures.py (zstd level 1, one chunk per read, as MinKNOW writes).
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


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def write_set(directory, n_containers, n_reads, mean_length, seed):
    import vbz_fixtures as vf
    from deepbinner_amd import hdf5_write
    rng = np.random.default_rng(seed)
    twins, vbzs = [], []
    for c in range(n_containers):
        reads = []
        for _ in range(n_reads):
            n = int(np.clip(rng.lognormal(np.log(mean_length), 0.25), 2000, 400000))
            levels = np.repeat(rng.normal(450, 80, n // 8 + 1), 8)[:n]
            signal = np.clip(np.rint(levels + rng.normal(0, 8, n)), 0, 2047).astype(np.int16)
            reads.append((str(uuid.UUID(bytes=rng.bytes(16), version=4)), signal))
        twin = os.path.join(directory, 'deflate_%d_%02d.fast5' % (mean_length, c))
        with open(twin, 'wb') as f:
            f.write(hdf5_write.multi_read_fast5_bytes(reads))
        vbz = os.path.join(directory, 'vbz_%d_%02d.fast5' % (mean_length, c))
        vf.write_vbz_copy(reads, vbz, vf.VARIANTS[0], multi=True)
        twins.append(twin)
        vbzs.append(vbz)
    return twins, vbzs


def measure(paths, start, end, threads, vbz_zstd='host'):
    from deepbinner_amd import fast5_native, hip_backend
    # the GPU decode alone, per container
    decode_ms = []
    for _, ids, offsets, status, comp, records in fast5_native.stream_raw(paths, threads=threads, vbz_zstd=vbz_zstd):
        out_bytes = int(offsets[-1]) * 2
        hip_backend.inflate(comp, records, out_bytes)              # (warm)
        times = [hip_backend.inflate(comp, records, out_bytes)[2] for _ in range(3)]
        decode_ms.append(min(times))
    # host CPU per read on the raw route (the loader alone)
    cpu0, t0, reads = cpu_seconds(), time.perf_counter(), 0
    for _, ids, offsets, status, comp, records in fast5_native.stream_raw(paths, threads=threads, vbz_zstd=vbz_zstd):
        reads += len(ids)
    loader_s, loader_cpu = time.perf_counter() - t0, cpu_seconds() - cpu0
    # end to end: raw stream -> classify_pair_deflated
    t0, calls = time.perf_counter(), 0
    for _, ids, offsets, status, comp, records in fast5_native.stream_raw(paths, threads=threads, vbz_zstd=vbz_zstd):
        got = hip_backend.classify_pair_deflated(start, end, comp, records, offsets, 6144, 0.5)
        calls += len(got[0])
    e2e = time.perf_counter() - t0
    return {'containers': len(paths), 'reads': reads,
            'gpu_decode_ms_per_container': float(np.median(decode_ms)),
            'loader_host_cpu_us_per_read': 1e6 * loader_cpu / max(reads, 1),
            'loader_reads_per_s': reads / loader_s,
            'end_to_end_reads_per_s': calls / e2e}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--mean-length', type=int, nargs='+', default=[27000, 100000])
    ap.add_argument('--containers', type=int, default=4)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    opts = ap.parse_args()
    from deepbinner_amd import hip_backend
    from deepbinner_amd.model_format import ModelWeights
    models = os.path.join(REPO, 'deepbinner_amd', 'models')
    start = hip_backend.HipModel(ModelWeights.load(os.path.join(models, 'EXP-NBD103_read_starts.dbw'))[0])
    end = hip_backend.HipModel(ModelWeights.load(os.path.join(models, 'EXP-NBD103_read_ends.dbw'))[0])
    lines = ['device: ' + hip_backend.device_name(0)]
    with tempfile.TemporaryDirectory() as d:
        for length in opts.mean_length:
            n_reads = opts.reads if length < 50000 else max(opts.reads // 4, 1)
            twins, vbzs = write_set(d, opts.containers, n_reads, length, 32020 + length)
            for run in range(opts.runs):
                svb_only = None
                for name, paths, route in (('deflate', twins, 'host'), ('vbz host', vbzs, 'host'),
                                           ('vbz gpu', vbzs, 'gpu')):
                    r = measure(paths, start, end, opts.threads, route)
                    sizes = sum(os.path.getsize(p) for p in paths) / len(paths) / 2 ** 20
                    decode = r['gpu_decode_ms_per_container']
                    if name == 'vbz host':
                        svb_only = decode
                    stage = ' (zstd stage %.3f)' % (decode - svb_only) if name == 'vbz gpu' else ''
                    lines.append('run %d %-8s %6d reads x ~%6d samples: %.1f MiB/container, GPU decode '
                                 '%.3f ms/container%s, loader %.1f us CPU/read (%.0f reads/s), '
                                 'end to end %.0f reads/s' % (
                                     run + 1, name, n_reads, length, sizes, decode, stage,
                                     r['loader_host_cpu_us_per_read'], r['loader_reads_per_s'],
                                     r['end_to_end_reads_per_s']))
                    print(lines[-1], flush=True)
    start.close()
    end.close()
    if opts.out:
        with open(opts.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
