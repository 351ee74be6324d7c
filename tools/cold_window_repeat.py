#!/usr/bin/env python3
"""How often a grouped sweep differs from the same sweep in one group, and in which window.

    python tools/cold_window_repeat.py 60 [--reads-per-group 50 7 1] [--memory pageable pinned]

The set-up of tests/test_gpu_sweep.py::test_native_pair_end_to_end: the two shipped EXP-NBD103
models, the 300 reads of its fixture; the sweep in one group once, then REPEATS sweeps per row at
the stated group size in this process.  A repeat is bad when any cell of best or margin differs;
every bad repeat names its read, scan step and window (tests/cold_window.py).  Needs an MI355X.
The method of profiles/host_groups/grouped_sweep_repeat.txt, kept as a tool."""
import argparse
import contextlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import cold_window                                         # noqa: E402
from test_gpu_sweep import pinned_copy, random_reads       # noqa: E402


def golden_signals():
    reads = np.load(os.path.join(REPO, 'tests', 'golden', 'reads.npz'))
    out = []
    for samples, offsets in (('samples', 'offsets'), ('multi_samples', 'multi_offsets')):
        s, o = reads[samples], reads[offsets]
        out += [s[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('repeats', type=int)
    parser.add_argument('--reads-per-group', type=int, nargs='+', default=[50])
    parser.add_argument('--memory', nargs='+', default=['pageable', 'pinned'],
                        choices=['pageable', 'pinned'])
    args = parser.parse_args()

    from deepbinner_amd import hip_backend as hip
    from deepbinner_amd.model_format import ModelWeights
    models = [hip.HipModel(ModelWeights.load(os.path.join(REPO, 'deepbinner_amd', 'models',
                                                          name + '.dbw'))[0], device=0)
              for name in (cold_window.STARTS, cold_window.ENDS)]
    samples, offsets = random_reads(1024, cold_window.K, 11, golden_signals())
    whole = hip.sweep_pair(models[0], models[1], samples, offsets, cold_window.K * 512)
    print('library {}'.format(hip.library_path()))
    print('{:>15}  {:>8}  {:>9}'.format('reads per group', 'memory', 'bad runs'))
    for reads_per_group in args.reads_per_group:
        for memory in args.memory:
            with pinned_copy(hip, samples) if memory == 'pinned' \
                    else contextlib.nullcontext(samples) as held:
                bad = cold_window.repeat_grouped(hip, models[0], models[1], held, offsets, whole,
                                                 reads_per_group, args.repeats)
            print('{:>15}  {:>8}  {:>4} / {}'.format(reads_per_group, memory,
                                                     len({row[0] for row in bad}), args.repeats))
            if bad:
                print(cold_window.describe(bad))
            sys.stdout.flush()
    for model in models:
        model.close()


if __name__ == '__main__':
    main()
