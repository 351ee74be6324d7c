"""200 queued dbh_trainer_step_dev calls against 200 queued dbh_gradients_dev calls at (1024, 13)
for batches of 20 (the reference's default, deepbinner.py:265) and 256: what noise and update add
to the gradient pass.  Host clock around queued work that ends in a synchronise; the two alternate,
five runs each after a warm-up run, so the gradient call's own run-to-run spread is beside the
difference.  A first measurement: no threshold.

    python tools/train_step_rate.py > profiles/train_step/steps_gpu.txt

With ``--frozen`` the same step at frozen blocks, as JSON:

    python tools/train_step_rate.py --frozen 0,2,4,6,7 [--parent-tree DIR] [--runs 3]
                                    [--out profiles/train_step/frozen_rate.json]

Every figure is one child process of its own (``--tree``, the child's mode: it imports the package
of the checkout it is given, warms up with one run of 200 queued steps and times the next), the
configurations alternating, ``--runs`` children each.  ``--parent-tree DIR``: a built checkout of the
commit before frozen blocks came in, whose trainer has no such option - its step beside this tree's.
A record; the two conditions it evaluates are those of the change that brought it.  f = 0 through
the new code lies within the spread of the parent's own runs - read one-sidedly: its median is at
most the slowest of the parent's runs; being faster than the parent's fastest is no failure, and the
ranges of both are in the record.  And no step at f >= 1 is slower than the step at f = 0, median
against median.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLS, RUNS = 200, 5
BATCHES = (20, 256)


def main():
    sys.path.insert(0, REPO)
    from deepbinner_amd import hip_backend as hip
    from deepbinner_amd.model_format import ModelWeights
    weights, _ = ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models',
                                                'EXP-NBD103_read_starts.dbw'))
    flat = weights.flat()
    print('# L = 1024, C = 13, dropout 0.15, noise 0.02; one MI355X ({}), one session; {} queued calls '
          'per run, then one synchronise; {} alternating runs after one warm-up run each'.format(
              hip.device_name(0), CALLS, RUNS))
    for n in BATCHES:
        rng = np.random.default_rng(n)
        x = hip.DeviceBuffer.from_array(rng.standard_normal((n, 1024)).astype(np.float32))
        labels = hip.DeviceBuffer.from_array(rng.integers(13, size=n).astype(np.int32))
        w = hip.DeviceBuffer.from_array(flat)
        loss, correct = hip.DeviceBuffer(8), hip.DeviceBuffer(8)
        grads, stats = hip.DeviceBuffer(flat.nbytes), hip.DeviceBuffer(960 * 4)
        work = hip.DeviceBuffer(hip.gradients_workspace_bytes(13, 1024, n))
        trainer = hip.Trainer(weights, n, seed=1)
        stream = hip.Stream()

        def gradients():
            hip.gradients_dev(w.ptr, flat.size, 13, 1024, x.ptr, labels.ptr, n, 0.15, 1, loss.ptr,
                              correct.ptr, grads.ptr, stats.ptr, work.ptr, stream.ptr)

        def step():
            trainer.step_dev(x.ptr, labels.ptr, n, loss.ptr, correct.ptr, stream.ptr)

        def run(fn):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            stream.synchronize()
            return (time.perf_counter() - t0) / CALLS

        run(gradients), run(step)
        times = {'gradients': [], 'step': []}
        for _ in range(RUNS):
            times['gradients'].append(run(gradients))
            times['step'].append(run(step))
        for name in ('gradients', 'step'):
            t = times[name]
            print('batch {:3d}  {:9s} ms per call: {}   median {:.3f}  ({:.1f} calls/s, {:.0f} windows/s)'
                  .format(n, name, '  '.join('{:.3f}'.format(v * 1e3) for v in t),
                          np.median(t) * 1e3, 1 / np.median(t), n / np.median(t)))
        g, s = np.median(times['gradients']), np.median(times['step'])
        spread = (max(times['gradients']) - min(times['gradients'])) / g
        print('batch {:3d}  step / gradients = {:.4f}; the gradient call\'s own spread over its runs: '
              '{:.4f} of its median'.format(n, s / g, spread))
        final = float(loss.download(1, np.float64)[0])
        print('batch {:3d}  loss of the last step {:.4f} after {} steps on one batch'.format(
            n, final, trainer.iterations))
        trainer.close()
        stream.close()


def one_configuration(opts):
    """--tree: ms per queued step at each batch size, with the package of the checkout at
    opts.tree; opts.one is the number of frozen blocks, or 'parent' for a trainer without them"""
    sys.path.insert(0, opts.tree)
    import deepbinner_amd
    from deepbinner_amd import hip_backend as hip
    from deepbinner_amd.model_format import ModelWeights
    assert os.path.dirname(os.path.abspath(deepbinner_amd.__file__)).startswith(os.path.abspath(opts.tree))
    # (the package and its library come from --tree; the model file is always this checkout's, so
    # every configuration steps the same weights)
    weights, _ = ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models',
                                                'EXP-NBD103_read_starts.dbw'))
    frozen = {} if opts.one == 'parent' else {'frozen_blocks': int(opts.one)}
    result = {'tree': os.path.abspath(opts.tree), 'configuration': opts.one, 'ms_per_step': {}}
    for n in BATCHES:
        rng = np.random.default_rng(n)
        x = hip.DeviceBuffer.from_array(rng.standard_normal((n, 1024)).astype(np.float32))
        labels = hip.DeviceBuffer.from_array(rng.integers(13, size=n).astype(np.int32))
        loss, correct = hip.DeviceBuffer(8), hip.DeviceBuffer(8)
        trainer = hip.Trainer(weights, n, seed=1, **frozen)
        stream = hip.Stream()
        for timed in (False, True):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                trainer.step_dev(x.ptr, labels.ptr, n, loss.ptr, correct.ptr, stream.ptr)
            stream.synchronize()
            if timed:
                result['ms_per_step'][str(n)] = (time.perf_counter() - t0) / CALLS * 1e3
        trainer.close()
        stream.close()
    with open(opts.out, 'w') as f:
        json.dump(result, f)


def frozen_record(opts):
    import tempfile
    configurations = [('parent', opts.parent_tree)] if opts.parent_tree else []
    configurations += [(str(int(f)), REPO) for f in opts.frozen.split(',')]
    runs = {name: {str(n): [] for n in BATCHES} for name, _ in configurations}
    with tempfile.TemporaryDirectory() as d:
        for k in range(opts.runs):
            for name, tree in configurations:
                target = os.path.join(d, '{}_{}.json'.format(name, k))
                subprocess.run([sys.executable, os.path.abspath(__file__), '--tree', tree, '--one',
                                name, '--out', target], check=True, stdout=subprocess.DEVNULL,
                               timeout=300)
                with open(target) as f:
                    got = json.load(f)['ms_per_step']
                for n, ms in got.items():
                    runs[name][n].append(ms)
    sys.path.insert(0, REPO)
    from deepbinner_amd import hip_backend as hip
    result = {'device': hip.device_name(0), 'shape': 'L = 1024, C = 13, dropout 0.15, noise 0.02',
              'queued_steps_per_run': CALLS, 'runs_per_configuration': opts.runs,
              'order': 'alternating, one child process per figure, one warm-up run in each',
              'ms_per_step': {}, 'conditions': {}}
    for name, by_batch in runs.items():
        key = 'parent_commit' if name == 'parent' else 'frozen_' + name
        result['ms_per_step'][key] = {n: {'runs': t, 'median': statistics.median(t),
                                          'range': [min(t), max(t)]} for n, t in by_batch.items()}
    table = result['ms_per_step']
    for n in (str(b) for b in BATCHES):
        checks = {}
        if 'parent_commit' in table and 'frozen_0' in table:
            checks['frozen_0_median_within_parent_range'] = \
                table['frozen_0'][n]['median'] <= table['parent_commit'][n]['range'][1]
        if 'frozen_0' in table:
            checks['frozen_steps_not_slower_than_frozen_0'] = all(
                v[n]['median'] <= table['frozen_0'][n]['median']
                for key, v in table.items() if key.startswith('frozen_') and key != 'frozen_0')
            checks['median_over_frozen_0'] = {
                key: v[n]['median'] / table['frozen_0'][n]['median']
                for key, v in table.items() if key.startswith('frozen_')}
        result['conditions']['batch_' + n] = checks
    text = json.dumps(result, indent=1)
    print(text)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--frozen', default=None, help='comma-separated numbers of frozen blocks')
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--tree', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--one', default=None, help=argparse.SUPPRESS)
    options = ap.parse_args()
    if options.tree:
        one_configuration(options)
    elif options.frozen:
        frozen_record(options)
    else:
        main()
