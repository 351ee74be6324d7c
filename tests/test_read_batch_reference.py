"""What a resident read batch has to compute, held to the reference's own
code on the host: the restated trim rule against ``find_signal_start_pos``, the tie at a standard
deviation of exactly 20, the moments of a read whose D passes 2^64, the scan's windows."""
import os

import numpy as np
import pytest

import read_batch_reference as R
from conftest import REPO
from deepbinner_amd import prep_signal
from deepbinner_amd.trim_signal import CannotTrim, find_signal_start_pos

DESIGN = os.path.join(REPO, 'DESIGN.md')


def reference_trim(signal):
    try:
        return find_signal_start_pos(signal)
    except CannotTrim:
        return -1


def synthetic_read(rng):
    """Quiet open pore of random length with a few isolated noisy windows in it, then signal."""
    quiet = int(rng.integers(0, 1500))
    loud = int(rng.integers(0, 600))
    signal = np.concatenate([rng.normal(520, 4, quiet), rng.normal(500, 80, loud)])
    for _ in range(int(rng.integers(0, 4))):
        if quiet > 60:
            at = int(rng.integers(0, quiet - 50))
            burst = slice(at, at + int(rng.integers(10, 60)))
            signal[burst] = rng.normal(520, 70, len(signal[burst]))
    return np.round(signal).astype(np.int16)


def test_trim_rule_equals_find_signal_start_pos(gold):
    got = [R.trim_position(s) for s in gold['signals']]
    assert got == [110, 235, 660, 85, 60, 285, 310]
    assert got == [reference_trim(s) for s in gold['signals']]
    rng = np.random.default_rng(21)
    reads = list(gold['signals']) + [synthetic_read(rng) for _ in range(3000)]
    reads += [np.round(rng.normal(500, 60, length)).astype(np.int16) for length in range(201)]
    reads += [np.full(length, 500, dtype=np.int16) for length in (0, 34, 35, 134, 135, 160)]
    outcomes = set()
    for k, read in enumerate(reads):
        margins = R.window_margins(read)
        # the comparison cannot hide the tie: no window of these inputs sits on the bound
        assert not np.any(margins == R.BOUND), k
        want = reference_trim(read)
        assert R.trim_position(read) == want, (k, len(read))
        outcomes.add('cannot' if want < 0 else 'first' if want == R.SKIP else 'later')
        if want >= 0:
            assert want + R.AHEAD * R.STEP <= len(read) and len(read) >= R.SHORTEST_TRIMMABLE
    assert outcomes == {'cannot', 'first', 'later'}
    positions = [R.trim_position(read) for read in reads[7:3007]]
    assert sum(1 for p in positions if p < 0) > 100 and len(set(positions)) > 30
    # a high window whose look-ahead runs off the end is case (b) even behind four high ones
    loud = np.round(rng.normal(500, 80, 10 + 25 * 8)).astype(np.int16)
    quiet_then_loud = np.concatenate([np.full(10 + 25 * 4, 500, dtype=np.int16), loud[:25 * 4]])
    assert R.trim_position(quiet_then_loud) == reference_trim(quiet_then_loud) == -1
    assert R.trim_position(loud) == reference_trim(loud) == 10


def tie_windows(rng, rounds):
    """int16 windows with 25 Q - S^2 == 250000 exactly: random windows of a spread near 20 at
    levels all over the int16 range."""
    found = []
    for _ in range(rounds):
        x = np.round(rng.normal(0, 20.0, size=(200000, R.STEP))).astype(np.int64) + \
            rng.integers(-32600, 32600, size=(200000, 1))
        s, q = x.sum(axis=1), (x * x).sum(axis=1)
        found += [w.astype(np.int16) for w in x[R.STEP * q - s * s == R.BOUND]]
    return found


def test_the_tie_at_exactly_twenty(capsys):
    """Windows whose standard deviation is exactly 20 are not high by the integer rule.  The
    reference's ``np.std(window) > 20`` could call one high only by returning more than 20.0,
    which takes a variance two units in the last place above 400.  What np.std does on the
    windows found here is recorded, and section 21's sentences are held to it."""
    windows = tie_windows(np.random.default_rng(2), 8)
    multiples = [w for w in windows if int(w.astype(np.int64).sum()) % 25 == 0]
    others = [w for w in windows if int(w.astype(np.int64).sum()) % 25 != 0]
    assert len(multiples) >= 10 and len(others) >= 50
    above = [w for w in windows if np.std(w) > 20]
    below = [w for w in windows if np.std(w) < 20]
    variances = [float(np.var(w)) for w in windows]
    ulp = np.spacing(400.0)
    with capsys.disabled():
        print('{} windows with 25 Q - S^2 == 250000 ({} with S no multiple of 25): np.std above '
              '20 on {}, below on {}; np.var within {:.0f} .. {:.0f} units of 400'.format(
                  len(windows), len(others), len(above), len(below),
                  (min(variances) - 400.0) / ulp, (max(variances) - 400.0) / ulp))
    for w in windows:
        padded = np.concatenate([np.zeros(10, dtype=np.int16), w])
        assert R.window_margins(padded)[0] == R.BOUND
    # with S a multiple of 25 the mean is exact; np.std is still only as exact as its sum
    for w in multiples:
        assert np.std(w) == 20.0
    # what section 21 says about the others
    text = ' '.join(open(DESIGN).read().split())
    if above:
        assert 'np.std == 20.0 on every one' not in text
    else:
        assert 'np.std == 20.0 on every one' in text
        assert 'no window is known on which the rules part' in text
        assert all(np.std(w) == 20.0 for w in others)
        assert all(abs(v - 400.0) <= ulp for v in variances)
    assert 'The search is not exhaustive' in text


def test_moments_of_a_read_whose_d_passes_two_to_the_64():
    extreme = np.tile(np.array([-32768, 32767], dtype=np.int16), 100000)
    moved = extreme.copy()
    moved[12344] += 1
    for signal in (extreme, moved, moved[:199999]):
        n = len(signal)
        s, q = R.sums(signal)
        assert n * q - s * s > 2 ** 64
        assert R.moments(signal) == prep_signal.signal_moments(signal)
    # the conversion of D rounds once: D's exact square root is not what a double holds
    s, q = R.sums(moved)
    d = len(moved) * q - s * s
    assert float(d) != d or d.bit_length() <= 53
    assert R.moments(np.zeros(0, dtype=np.int16)) == prep_signal.signal_moments([]) == (0.0, 0.0)
    assert R.moments(np.full(300, -7, dtype=np.int16)) == (-7.0, 0.0)
    rng = np.random.default_rng(4)
    x = rng.integers(-300, 1500, size=5000).astype(np.int16)
    assert R.moments(x) == prep_signal.signal_moments(x)


@pytest.mark.parametrize('length', [0, 1, 499, 1500, 1501, 2000, 14999, 16000, 40000])
@pytest.mark.parametrize('side', ['start', 'end'])
def test_scan_windows_equal_adapter_windows(length, side):
    windows = R.adapter_windows(length, side)
    assert windows == prep_signal.adapter_windows(length, side)
    first, last = prep_signal.adapter_region(length, side)
    assert all(first <= a <= b <= last for a, b in windows) and len(windows) <= R.WINDOWS
