#!/usr/bin/env python3
"""`deepbinner classify --multi_read` (start + end models) over multi-read containers written on
the spot the way tools/realtime_rate.py writes its own (tools/multi_read_rate.py: log-normal read
lengths, gzip 1; or VBZ with --vbz): reads/s and process CPU per read of the containers by which
a small and a large run differ (the process's start and the model loading cancel).

    python tools/classify_multi_read_rate.py [--reads 4000] [--mean-length 27000] [--runs 3]
        [--small 4] [--large 24] [--distinct 4] [--vbz] [--verbose] [--loader-procs 16]
        [--command classify|realtime] [--dir DIR] [--package CHECKOUT]

--distinct containers are written (in parallel processes) and linked over and over up to --large.
--command realtime times `realtime --stop` with DEEPBINNER_REALTIME_TABLE_ONLY=1 over the same
containers instead: the figure `classify --multi_read` is compared with.  --dir keeps the
containers for the next invocation; --package imports deepbinner_amd from another checkout (the
same containers through two commits).  Prints one JSON line per run and a summary line.
"""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_container(job):
    path, reads, mean, seed, vbz = job
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import multi_read_rate
    if not vbz:
        multi_read_rate.write_with_own_writer(path, reads, mean, seed)
        return path
    # the same reads as VBZ chunks (ONT's filter 32020: streamvbyte + zstd), by the encoder the
    # tests write their VBZ fixtures with
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import vbz_fixtures
    from deepbinner_amd import load_fast5s
    plain = path + '.deflate'
    multi_read_rate.write_with_own_writer(plain, reads, mean, seed)
    vbz_fixtures.write_vbz_copy(list(load_fast5s._python_iter_reads(plain)), path,
                                vbz_fixtures.VARIANTS[0], multi=True)
    os.unlink(plain)
    return path


def containers(opts, root):
    """-> {'small': dir, 'large': dir} of links to the --distinct containers under ``root``"""
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing
    kind = 'vbz' if opts.vbz else 'deflate'
    base = os.path.join(root, '%s_%d_%d' % (kind, opts.reads, opts.mean_length))
    os.makedirs(base, exist_ok=True)
    jobs = [(os.path.join(base, 'distinct_%02d.fast5' % k), opts.reads, opts.mean_length, 100 + k,
             opts.vbz) for k in range(opts.distinct)]
    todo = [job for job in jobs if not os.path.exists(job[0])]
    if todo:
        with ProcessPoolExecutor(min(len(todo), 8),
                                 mp_context=multiprocessing.get_context('spawn')) as pool:
            list(pool.map(write_container, todo))
    dirs = {}
    for name, count in (('small', opts.small), ('large', opts.large)):
        dirs[name] = os.path.join(base, name)
        shutil.rmtree(dirs[name], ignore_errors=True)
        os.makedirs(dirs[name])
        for k in range(count):
            os.symlink(jobs[k % opts.distinct][0], os.path.join(dirs[name], 'c%03d.fast5' % k))
    return dirs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--reads', type=int, default=4000, help='reads per container')
    ap.add_argument('--mean-length', type=int, default=27000, help='mean samples per read')
    ap.add_argument('--distinct', type=int, default=4)
    ap.add_argument('--small', type=int, default=4)
    ap.add_argument('--large', type=int, default=24)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--vbz', action='store_true')
    ap.add_argument('--verbose', action='store_true', help='time the --verbose table')
    ap.add_argument('--loader-procs', type=int, default=16)
    ap.add_argument('--command', choices=('classify', 'realtime'), default='classify')
    ap.add_argument('--dir', help='keep the containers here (default: a temporary directory)')
    ap.add_argument('--package', help='import deepbinner_amd from this checkout')
    opts = ap.parse_args()

    root = opts.dir or tempfile.mkdtemp(prefix='classify_multi_read_rate_')
    os.makedirs(root, exist_ok=True)
    dirs = containers(opts, root)
    sys.path.insert(0, os.path.abspath(opts.package) if opts.package else REPO)
    from deepbinner_amd import deepbinner as cli
    import deepbinner_amd.realtime as realtime
    models = os.path.join(os.path.dirname(os.path.abspath(realtime.__file__)), 'models')
    model_args = ['-s', os.path.join(models, 'EXP-NBD103_read_starts.dbw'),
                  '-e', os.path.join(models, 'EXP-NBD103_read_ends.dbw'),
                  '--loader_procs', str(opts.loader_procs)]
    if opts.command == 'realtime':
        realtime.POLL_SECONDS = 0
        shutil.which = lambda tool: None            # (no multi_to_single_fast5: in place)
        os.environ['DEEPBINNER_REALTIME_TABLE_ONLY'] = '1'

    def once(name):
        out = os.path.join(root, 'out_' + name)
        shutil.rmtree(out, ignore_errors=True)
        if opts.command == 'realtime':
            argv = ['realtime', '--in_dir', dirs[name], '--out_dir', out, '--stop'] + model_args
        else:
            argv = (['classify', '--multi_read'] + (['--verbose'] if opts.verbose else []) +
                    model_args + [dirs[name]])
        table = io.StringIO()
        t0, c0 = time.perf_counter(), time.process_time()
        with contextlib.redirect_stdout(table), contextlib.redirect_stderr(io.StringIO()):
            cli.main(argv)
        seconds, cpu = time.perf_counter() - t0, time.process_time() - c0
        if opts.command == 'realtime':
            with open(os.path.join(out, 'multi_read_classifications.tsv')) as f:
                rows = sum(1 for _ in f)
        else:
            rows = table.getvalue().count('\n') - 1
        return seconds, cpu, rows

    once('small')                                   # (page cache, code objects, pinned pools)
    n = (opts.large - opts.small) * opts.reads
    rates, cpus = [], []
    for run in range(opts.runs):
        small, large = once('small'), once('large')
        assert small[2] == opts.small * opts.reads and large[2] == opts.large * opts.reads, \
            (small[2], large[2])
        rates.append(round(n / (large[0] - small[0])))
        cpus.append(round((large[1] - small[1]) / n * 1e6, 1))
        print(json.dumps({'run': run, 'reads_per_s': rates[-1], 'cpu_us_per_read': cpus[-1],
                          'seconds': [round(small[0], 3), round(large[0], 3)]}), flush=True)
    print(json.dumps({
        'command': opts.command + (' --multi_read' if opts.command == 'classify' else ' --stop') +
        (' --verbose' if opts.verbose and opts.command == 'classify' else ''),
        'package': os.path.abspath(opts.package) if opts.package else REPO,
        'containers': 'vbz' if opts.vbz else 'deflate', 'reads_per_container': opts.reads,
        'mean_samples': opts.mean_length, 'small_large': [opts.small, opts.large],
        'loader_procs': opts.loader_procs, 'vbz_zstd': os.environ.get('DEEPBINNER_VBZ_ZSTD', 'host'),
        'reads_per_s': rates, 'median_reads_per_s': sorted(rates)[len(rates) // 2],
        'spread_reads_per_s': max(rates) - min(rates), 'cpu_us_per_read': cpus,
        'host_share_percent': realtime.host_inflate_share(1)}), flush=True)
    if not opts.dir:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
