"""A grouped sweep repeated and held to the sweep in one group, to the bit (no test of its own: what
tests/test_gpu_cold_window.py and tools/cold_window_repeat.py share).

The persistent forward kernel's COLD path - the first window (k = 0) of a workgroup's first group,
which fetches its samples itself instead of finding them staged in LDS - has returned wrong
probabilities for one window in 12 to 24 of 100 sweeps at 50 reads per group
(profiles/host_groups/grouped_sweep_repeat.txt).  A mismatch is named by read, scan step and the
window index read * K + step, so that a failure says which window of which workgroup it was."""
import numpy as np

K = 12
STARTS, ENDS = 'EXP-NBD103_read_starts', 'EXP-NBD103_read_ends'


def mismatches(got, want, reads_per_group):
    """[(side, read, first scan step that differs, window index, window in its group, what)]: the
    fold is a running min / max, so a window's probabilities carry into every later step - the first
    step that differs is the window that was wrong."""
    found = []
    for j, side in enumerate(('start', 'end')):
        best, margin = got[j]
        want_best, want_margin = want[j]
        if best is None:
            continue
        differs = (best != want_best) | (margin.view(np.uint64) != want_margin.view(np.uint64))
        for read in np.flatnonzero(differs.any(axis=1)):
            step = int(np.argmax(differs[read]))
            window = int(read) * K + step
            in_group = (int(read) % reads_per_group) * K + step if reads_per_group else window
            found.append((side, int(read), step, window, in_group,
                          'best {} for {}, margin {!r} for {!r}'.format(
                              best[read, step], want_best[read, step], float(margin[read, step]),
                              float(want_margin[read, step]))))
    return found


def repeat_grouped(hip, start, end, samples, offsets, whole, reads_per_group, repeats):
    """``repeats`` sweeps at ``reads_per_group`` reads per host group (0: one group) in this process
    -> [(repeat, *mismatch)] against ``whole``, the sweep in one group."""
    bad = []
    start.set_host_group(reads_per_group * K)
    try:
        for repeat in range(repeats):
            got = hip.sweep_pair(start, end, samples, offsets, K * 512)
            bad += [(repeat,) + found for found in mismatches(got, whole, reads_per_group)]
    finally:
        start.set_host_group(0)
    return bad


def describe(bad):
    return '\n'.join('repeat {}: {} model, read {}, scan step {}: window {} ({} of its group): {}'
                     .format(*row) for row in bad)
