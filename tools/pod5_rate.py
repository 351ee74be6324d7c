#!/usr/bin/env python3
"""`classify` on a POD5 file beside its VBZ multi-read fast5 twin, one GPU:

    python tools/pod5_rate.py [--reads 4000] [--runs 3] [--row-samples 102400] [--out FILE]
                              [--parent-tree DIR]

Input: `--reads` synthetic reads of 6,000 to 20,000 samples - the recipe of tools/live_rate.py:
cut from the seven golden reads, a little noise on top - written once as a POD5 file (the writer of
tests/pod5_fixtures.py, which needs pyarrow; zstd level 1, rows of `--row-samples` samples) and
once as a VBZ multi-read fast5 container (tests/vbz_fixtures.py, one chunk per read), into a
temporary directory.  Reported, as JSON:

  classify_wall_s   the wall time of `deepbinner classify --native` on each file, in this process,
                    stdout discarded: one warm-up run (library load, first launches), then `--runs`
                    runs - all of them, their median and their range; for POD5 with the rows' zstd
                    frames undone on the host (the default) and on the GPU (DEEPBINNER_VBZ_ZSTD=gpu)
  decode_ms         the inflate stage of `dbh_classify_pair_deflated` (the `stage_ms` the entry
                    returns, HIP events) on the whole file as one unit: the svb16 kernel on the
                    POD5 file's rows (mode 6; mode 7: zstd + svb16) beside dbh_vbz.hip's on the
                    fast5 twin's chunks (mode 2; mode 3) - the same samples; minimum of three
  pod5_split_s      where the POD5 time goes: `pod5_lite.open`, `raw_unit` (the Python reader: row
                    lists, zstd through ctypes, the copy into the unit's buffer) and the device
                    call, each the median of `--runs`

`--parent-tree DIR` (a built checkout of the commit before POD5 came in, which has neither this
tool nor the POD5 writer): the fast5 twin's figures once more, twice on that checkout and twice on
this tree, alternating, each in a child process of its own that imports the package from the
checkout it is given (`--tree`, the child's mode: the fast5 container alone - `classify` wall time
and the VBZ kernel's inflate stage, modes 2 and 3) -> `fast5_twin_by_tree`.  What the difference
between the trees has to exceed is the difference between the two runs of one tree.

A record, not a bound.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import uuid

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def use_tree(tree):
    """the package and the test helpers of the checkout at ``tree`` (this one, unless --tree)"""
    sys.path.insert(0, os.path.join(tree, 'tests'))
    sys.path.insert(0, tree)


def synthetic_reads(n_reads, seed=36):
    reads = np.load(os.path.join(REPO, 'tests', 'golden', 'reads.npz'))
    offsets = reads['offsets']
    bases = [np.resize(reads['samples'][offsets[k]:offsets[k + 1]], 20000).astype(np.int16)
             for k in range(len(offsets) - 1)]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_reads):
        n = int(rng.integers(6000, 20001))
        signal = bases[int(rng.integers(0, len(bases)))][:n] + rng.integers(-3, 4, n).astype(np.int16)
        out.append((str(uuid.UUID(bytes=rng.bytes(16), version=4)), signal.astype(np.int16)))
    return out


def classify_wall(path, flags, runs, env=None):
    from deepbinner_amd import deepbinner as cli
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    times = []
    try:
        for k in range(runs + 1):
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()) as out, contextlib.redirect_stderr(io.StringIO()):
                cli.main(['classify', '--native'] + flags + [path])
            if k:
                times.append(time.perf_counter() - t0)
            rows = len(out.getvalue().splitlines()) - 1
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return {'runs_s': times, 'median_s': statistics.median(times), 'range_s': [min(times), max(times)],
            'rows': rows, 'reads_per_s': rows / statistics.median(times)}


def inflate_ms(models, comp, records, offsets):
    from deepbinner_amd import hip_backend
    best = None
    for _ in range(4):          # (the first one warms)
        stages = hip_backend.classify_pair_deflated(*models, comp, records, offsets, 6144, 0.5,
                                                    want_stages=True)[2]
        best = stages[1] if best is None else min(best, stages[1])
    return best


def fast5_twin(opts):
    """--tree: the fast5 container alone, with the package of the checkout at opts.tree"""
    use_tree(opts.tree)
    import vbz_fixtures as vf
    import deepbinner_amd
    from deepbinner_amd import fast5_native, hip_backend
    from deepbinner_amd.model_format import ModelWeights
    assert os.path.dirname(os.path.abspath(deepbinner_amd.__file__)).startswith(os.path.abspath(opts.tree))
    result = {'tree': os.path.abspath(opts.tree), 'reads': opts.reads}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'reads_vbz.fast5')
        vf.write_vbz_copy(synthetic_reads(opts.reads), path, vf.VARIANTS[0], multi=True)
        result['classify_wall_s'] = classify_wall(path, ['--multi_read'], opts.runs)
        models_dir = os.path.join(opts.tree, 'deepbinner_amd', 'models')
        models = [hip_backend.HipModel(ModelWeights.load(os.path.join(models_dir, name + '.dbw'))[0])
                  for name in ('EXP-NBD103_read_starts', 'EXP-NBD103_read_ends')]
        result['decode_ms'] = {}
        for zstd, name in (('host', 'vbz_mode2'), ('gpu', 'vbz_zstd_mode3')):
            for _, ids, offsets, status, comp, records in fast5_native.stream_raw([path], vbz_zstd=zstd):
                result['decode_ms'][name] = inflate_ms(models, comp, records, offsets)
        for model in models:
            model.close()
    text = json.dumps(result, indent=1)
    print(text)
    if opts.out:
        with open(opts.out, 'w') as f:
            f.write(text + '\n')


def by_tree(opts):
    """--parent-tree: children on the parent's checkout and on this one, alternating"""
    out = {'parent_commit': [], 'this_tree': []}
    with tempfile.TemporaryDirectory() as d:
        for k in range(2):
            for name, tree in (('parent_commit', opts.parent_tree), ('this_tree', REPO)):
                target = os.path.join(d, '%s_%d.json' % (name, k))
                subprocess.run([sys.executable, os.path.abspath(__file__), '--tree', tree, '--reads',
                                str(opts.reads), '--runs', str(opts.runs), '--out', target],
                               check=True, stdout=subprocess.DEVNULL, timeout=600)
                with open(target) as f:
                    got = json.load(f)
                out[name].append({'classify_wall_median_s': got['classify_wall_s']['median_s'],
                                  'classify_wall_range_s': got['classify_wall_s']['range_s'],
                                  'decode_ms': got['decode_ms']})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--row-samples', type=int, default=102400)
    ap.add_argument('--out', default=None)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--tree', default=None, help=argparse.SUPPRESS)
    opts = ap.parse_args()
    if opts.tree:
        return fast5_twin(opts)
    use_tree(REPO)
    import pod5_fixtures as pf
    import vbz_fixtures as vf
    from deepbinner_amd import fast5_native, hip_backend, pod5_lite
    from deepbinner_amd.model_format import ModelWeights
    result = {'device': hip_backend.device_name(0), 'reads': opts.reads, 'row_samples': opts.row_samples}
    with tempfile.TemporaryDirectory() as d:
        reads = synthetic_reads(opts.reads)
        result['samples'] = int(sum(len(s) for _, s in reads))
        pod5_path, fast5_path = os.path.join(d, 'reads.pod5'), os.path.join(d, 'reads_vbz.fast5')
        with open(pod5_path, 'wb') as f:
            f.write(pf.pod5_bytes(reads, level=1, row_samples=opts.row_samples))
        vf.write_vbz_copy(reads, fast5_path, vf.VARIANTS[0], multi=True)
        result['file_bytes'] = {'pod5': os.path.getsize(pod5_path), 'fast5_vbz': os.path.getsize(fast5_path)}

        wall = result['classify_wall_s'] = {}
        wall['fast5_vbz'] = classify_wall(fast5_path, ['--multi_read'], opts.runs)
        wall['pod5_zstd_host'] = classify_wall(pod5_path, [], opts.runs, {'DEEPBINNER_VBZ_ZSTD': 'host'})
        wall['pod5_zstd_gpu'] = classify_wall(pod5_path, [], opts.runs, {'DEEPBINNER_VBZ_ZSTD': 'gpu'})
        print(json.dumps(wall), flush=True)

        models_dir = os.path.join(REPO, 'deepbinner_amd', 'models')
        models = [hip_backend.HipModel(ModelWeights.load(os.path.join(models_dir, name + '.dbw'))[0])
                  for name in ('EXP-NBD103_read_starts', 'EXP-NBD103_read_ends')]
        decode = result['decode_ms'] = {}
        for zstd, svb, vbz in (('host', 'svb16_mode6', 'vbz_mode2'), ('gpu', 'svb16_zstd_mode7', 'vbz_zstd_mode3')):
            _, offsets, comp, records = pod5_lite.raw_unit(pod5_path, zstd=zstd)
            decode[svb] = inflate_ms(models, comp, records, offsets)
            for _, ids, offsets, status, comp, records in fast5_native.stream_raw([fast5_path], vbz_zstd=zstd):
                decode[vbz] = inflate_ms(models, comp, records, offsets)
        split = {'open': [], 'raw_unit': [], 'device_call': []}
        for _ in range(opts.runs):
            t0 = time.perf_counter()
            pod5 = pod5_lite.open(pod5_path)
            t1 = time.perf_counter()
            _, offsets, comp, records = pod5_lite.raw_unit(pod5)
            t2 = time.perf_counter()
            hip_backend.classify_pair_deflated(*models, comp, records, offsets, 6144, 0.5)
            t3 = time.perf_counter()
            for name, value in zip(('open', 'raw_unit', 'device_call'), (t1 - t0, t2 - t1, t3 - t2)):
                split[name].append(value)
        result['pod5_split_s'] = {name: statistics.median(values) for name, values in split.items()}
        for model in models:
            model.close()
    if opts.parent_tree:
        result['fast5_twin_by_tree'] = by_tree(opts)
    text = json.dumps(result, indent=1)
    print(text)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
