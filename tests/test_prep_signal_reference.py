"""prep's signal stage without a device: the NumPy restatement of the contract
(tests/prep_signal_reference.py) against the reference's own method, the window construction against
the reference's loops, the first-hit rules, and what the library must do where there is no GPU."""
import ctypes

import numpy as np
import pytest

import prep_signal_reference as P
from deepbinner_amd import dtw_semi_global as dtw
from deepbinner_amd import prep_signal

# The largest relative difference between the restatement's distance (normal equations in the
# header's summation order, mean and std from exact integer sums) and the reference method's
# (lstsq, np.mean / np.std) measured on the 40 cases below: 1.6e-14 (printed by the test).  Allowed:
# 16 times that - two more passes of fp64 rounding of the same size on larger cases, nothing more.
MEASURED = 1.6e-14
BOUND = 16 * MEASURED
THRESHOLD = 50.0


def make_case(k):
    """A read of some 150 levels as int16 with a noisy copy of a 20-30 level query inside, and
    that query at a scale of 0.85 .. 1.15 with an offset."""
    rng = np.random.default_rng(1000 + k)
    query = P.squiggle(rng, int(rng.integers(20, 31)))
    before, after = P.squiggle(rng, 60), P.squiggle(rng, 60)
    signal = np.concatenate([before, query + rng.normal(0, 0.05, len(query)), after])
    raw = np.round(signal * 80.0 + 500.0).astype(np.int16)
    scale = 0.85 + 0.30 * k / 39
    return raw, scale * query + 0.1 * (k % 5 - 2), len(before)


CASES = [make_case(k) for k in range(40)]


def relative(a, b):
    if a == b:
        return 0.0
    return abs(a - b) / abs(b)


def test_restatement_against_the_reference_method(capsys):
    worst = 0.0
    for k, (raw, query, _) in enumerate(CASES):
        ours = P.rescaled(P.normalised(raw, *P.moments(raw)), query)
        theirs = P.reference_rescaled(P.reference_normalise(raw.astype(np.float64)), query)
        assert ours[1:3] == theirs[1:3], k
        assert np.array_equal(ours[4], theirs[4]), k
        assert np.isfinite(theirs[0]), k
        worst = max(worst, relative(ours[0], theirs[0]))
        assert relative(ours[0], theirs[0]) <= BOUND, (k, ours[0], theirs[0])
        assert relative(ours[3], theirs[3]) <= BOUND, (k, ours[3], theirs[3])
        # the condition on the inputs: no distance within the bound of the threshold
        assert abs(theirs[0] - THRESHOLD) > BOUND * THRESHOLD, (k, theirs[0])
    with capsys.disabled():
        print('largest relative difference of the distance on {} cases: {:.3e} (bound {:.3e})'
              .format(len(CASES), worst, BOUND))


def test_first_hit_of_a_group_as_the_reference_method_has_it():
    """Windows of 600 samples every 200 over ten of the reads: the same window is the first hit by
    both methods, and no window's distance is within the bound of the threshold."""
    seen = set()
    for k, (raw, query, at) in enumerate(CASES[:10]):
        ours_signal = P.normalised(raw, *P.moments(raw))
        theirs_signal = P.reference_normalise(raw.astype(np.float64))
        ours, theirs = [], []
        for first in range(0, len(raw) - 600, 200):
            ours.append(P.rescaled(ours_signal[first:first + 600], query)[0])
            theirs.append(P.reference_rescaled(theirs_signal[first:first + 600], query)[0])
        for a, b in zip(ours, theirs):
            assert relative(a, b) <= BOUND
            assert b == P.INF or abs(b - THRESHOLD) > BOUND * THRESHOLD
        hit = P.first_hit(ours, THRESHOLD)
        assert hit == P.first_hit(theirs, THRESHOLD)
        assert hit >= 0 and hit * 200 <= at < hit * 200 + 600, (k, hit, at)
        seen.add(hit)
    assert len(seen) > 1


def test_moments_are_exact_and_close_to_numpy():
    rng = np.random.default_rng(3)
    for length in (1, 2, 1000, 40000):
        x = rng.integers(-300, 1500, size=length).astype(np.int16)
        mean, std = P.moments(x)
        assert (mean, std) == prep_signal.signal_moments(x)
        assert abs(mean - np.mean(x)) <= 1e-12 * max(1.0, abs(mean))
        assert abs(std - np.std(x)) <= 1e-12 * max(1.0, std)
    assert prep_signal.signal_moments(np.full(77, 431, dtype=np.int16)) == (431.0, 0.0)
    flat = P.normalised(np.full(5, 431, dtype=np.int16), 431.0, 0.0)
    assert np.array_equal(flat, np.zeros(5))


@pytest.mark.parametrize('length', [0, 1, 499, 1500, 1501, 2000, 14999, 16000, 40000])
def test_window_construction_equals_the_reference_loops(length):
    start = [w for w in prep_signal.adapter_windows(length, 'start') if w[1] > w[0]]
    assert start == P.reference_start_windows(length)
    listed = prep_signal.adapter_windows(length, 'start')
    assert len(listed) == 30 and all(a == b == length for a, b in listed if a == b)
    end = prep_signal.adapter_windows(length, 'end')
    assert end == P.reference_end_windows(length)
    for side, windows in (('start', listed), ('end', end)):
        first, last = prep_signal.adapter_region(length, side)
        assert 0 <= first <= last <= length and last - first <= 16000
        assert all(first <= a <= b <= last for a, b in windows)
    # the barcode's window (prep_native_start.py:90-92, prep_native_end.py:91-92)
    signal = range(length)
    for adapter in ((120, 300), (50, 99), (length - 400, length - 1), (1000, 1200)):
        if not 0 <= adapter[0] <= adapter[1] < length:
            continue
        got = prep_signal.barcode_window(length, adapter, 'start')
        at = adapter[1] - 100
        want = signal[at:adapter[1] + 1000] if at >= 0 else None
        assert got == (None if want is None else (want[0], want[-1] + 1))
        got = prep_signal.barcode_window(length, adapter, 'end')
        at = adapter[0] - 1000
        want = signal[at:] if at >= 0 else None
        assert got == (None if want is None else (want[0], want[-1] + 1))
    assert prep_signal.barcode_window(length, (None, None), 'start') is None


def test_first_hit_rules():
    inf, nan = P.INF, float('nan')
    assert P.first_hit([50.0], 50.0) == 0                       # <=, not <
    assert P.first_hit([np.nextafter(50.0, 51.0), 50.0], 50.0) == 1
    assert P.first_hit([inf, nan, 12.0], 50.0) == 2
    assert P.first_hit([inf, nan], 50.0) == -1
    assert P.first_hit([inf], inf) == -1
    assert P.first_hit([], 50.0) == -1


def test_slope_bounds_and_the_constant_query_fall_through():
    """Queries whose fitted slope lies just outside 0.75 .. 1.333 get +inf and the group falls
    through to its next window; so does a constant query; just inside the bounds they hit."""
    raw, _, at = CASES[0]
    signal = P.normalised(raw, *P.moments(raw))
    piece = signal[at:at + 160].copy()
    window = (at - 20, at + 180)
    low_in, low_out = P.queries_beside_a_slope_bound(signal[slice(*window)], piece, 0.75)
    high_in, high_out = P.queries_beside_a_slope_bound(signal[slice(*window)], piece, 1.333)
    regions, mean_std = [raw], [P.moments(raw)]
    queries = [low_out, high_out, np.full(160, 0.25), low_in, high_in]
    jobs = [(0,) + window + (q,) for q in range(5)]
    distances, positions, slopes, hits = P.locate(regions, mean_std, queries, jobs, [0, 3, 4, 5],
                                                  THRESHOLD)
    assert 0.7499 < slopes[0] < 0.75 <= slopes[3] < 0.7501
    assert 1.3331 > slopes[1] > 1.333 >= slopes[4] > 1.3329
    assert np.isnan(slopes[2])
    assert list(distances[:3]) == [P.INF] * 3 and list(hits) == [-1, 3, 4]
    assert distances[3] < THRESHOLD and distances[4] < THRESHOLD
    # one group: the three that cannot hit, then one that does
    assert list(P.locate(regions, mean_std, queries, jobs[:4], [0, 4], THRESHOLD)[3]) == [3]
    # an empty window is skipped and never the hit
    empty = P.locate(regions, mean_std, queries, [(0, 7, 7, 3), jobs[3]], [0, 2], THRESHOLD)
    assert empty[0][0] == P.INF and tuple(empty[1][0]) == (-1, -1) and list(empty[3]) == [1]
    # a distance exactly equal to the threshold hits
    assert list(P.locate(regions, mean_std, queries, jobs[3:4], [0, 1], distances[3])[3]) == [0]
    below = np.nextafter(distances[3], 0.0)
    assert list(P.locate(regions, mean_std, queries, jobs[3:4], [0, 1], below)[3]) == [-1]


def test_a_reference_of_one_sample():
    """dtw.cpp finds no end row among rows 1 .. ref_len-1: DBL_MAX, positions 0, 0, the path along
    row 0.  The rescaled DTW then fits a constant y: slope 0 or so, distance +inf."""
    query = np.array([0.5, -1.0, 2.0])
    distance, start, end, pairs = P.dtw_ref.semi_global_dtw(np.array([0.3]), query)
    assert distance == np.finfo(np.float64).max and (start, end) == (0, 0)
    assert pairs == [(0, 0), (0, 1), (0, 2)]
    got = P.rescaled(np.array([0.3]), query)
    assert got[0] == P.INF and got[1:3] == (0, 0) and abs(got[3]) < 1e-12


# ------------------------------------------------------------------------ the library, no device
needs_library = pytest.mark.skipif(not dtw.available(), reason='libdeepbinner_dtw.so not built')


@needs_library
def test_new_symbols_are_exported():
    assert {'dtw_rescaled_batch', 'dtw_locate_batch'} <= set(dtw.EXPORTED_SYMBOLS)
    lib = ctypes.CDLL(dtw.library_path())
    assert hasattr(lib, 'dtw_rescaled_batch') and hasattr(lib, 'dtw_locate_batch')


def good_locate_arguments():
    return dict(samples=np.arange(100, dtype=np.int16), region_offsets=[0, 60, 100],
                mean_std=[[49.5, 28.0], [80.0, 0.0]], queries=np.linspace(-1, 1, 12),
                query_offsets=[0, 5, 12], jobs=[[0, 0, 60, 0], [1, 10, 10, 1], [1, 0, 40, 1]],
                group_offsets=[0, 1, 3], threshold=50.0)


BAD_LOCATE = {
    'region offsets not ascending': dict(region_offsets=[0, 120, 100]),
    'negative region offset': dict(region_offsets=[-1, 60, 100]),
    'query offsets not ascending': dict(query_offsets=[0, 13, 12]),
    'an empty query': dict(query_offsets=[0, 0, 12]),
    'window past its region': dict(jobs=[[0, 0, 61, 0]], group_offsets=[0, 1]),
    'window before its region': dict(jobs=[[0, -1, 10, 0]], group_offsets=[0, 1]),
    'window backwards': dict(jobs=[[0, 20, 10, 0]], group_offsets=[0, 1]),
    'read out of range': dict(jobs=[[2, 0, 10, 0]], group_offsets=[0, 1]),
    'query out of range': dict(jobs=[[0, 0, 10, 2]], group_offsets=[0, 1]),
    'negative query': dict(jobs=[[0, 0, 10, -1]], group_offsets=[0, 1]),
    'std not finite': dict(mean_std=[[49.5, float('inf')], [80.0, 0.0]]),
    'std not a number': dict(mean_std=[[49.5, float('nan')], [80.0, 0.0]]),
    'std negative': dict(mean_std=[[49.5, -1.0], [80.0, 0.0]]),
    'mean not finite': dict(mean_std=[[float('nan'), 1.0], [80.0, 0.0]]),
    'groups do not cover the jobs': dict(group_offsets=[0, 1, 2]),
    'groups not from zero': dict(group_offsets=[1, 1, 3]),
    'groups not ascending': dict(group_offsets=[0, 4, 3]),
    'threshold not a number': dict(threshold=float('nan')),
}


@needs_library
@pytest.mark.parametrize('what', sorted(BAD_LOCATE))
def test_locate_argument_errors_need_no_device(what):
    arguments = good_locate_arguments()
    arguments.update(BAD_LOCATE[what])
    with pytest.raises(RuntimeError, match='invalid argument'):
        dtw.locate_batch(**arguments)


@needs_library
def test_rescaled_argument_errors_need_no_device():
    lib = dtw.load_library()
    with pytest.raises(RuntimeError, match='invalid argument'):
        dtw.rescaled_batch([np.zeros(5), np.zeros(0)], [np.zeros(4), np.zeros(4)])
    with pytest.raises(RuntimeError, match='invalid argument'):
        dtw.rescaled_batch([np.zeros(5)], [np.zeros(0)])
    with pytest.raises(ValueError):
        dtw.rescaled_batch([np.zeros(5)], [])
    assert dtw.rescaled_batch([], []) == []
    # straight at the C ABI: offsets that go down, a null output, an alignment without lengths;
    # nothing is written on error
    f64, i64 = np.zeros(8), np.array([0, 5, 3], dtype=np.int64)
    fine = np.array([0, 2, 4], dtype=np.int64)
    distances, slopes = np.full(2, 7.0), np.full(2, 7.0)
    positions = np.full(4, 7, dtype=np.int32)
    alignment = np.full(64, 7, dtype=np.int32)
    assert lib.dtw_rescaled_batch(f64, i64, f64, fine, 2, distances, positions, slopes, None,
                                  None, None) == 1
    assert lib.dtw_rescaled_batch(f64, fine, f64, fine, 2, distances, positions, slopes, None,
                                  None, alignment.ctypes.data) == 1
    assert lib.dtw_rescaled_batch(f64, fine, f64, fine, -1, distances, positions, slopes, None,
                                  None, None) == 1
    assert np.all(distances == 7.0) and np.all(slopes == 7.0) and np.all(positions == 7)
    assert np.all(alignment == 7)


def no_device():
    from deepbinner_amd import hip_backend
    try:
        return hip_backend.device_count() < 1
    except Exception:
        return True


@needs_library
def test_no_device_is_an_error_not_a_fallback():
    if not no_device():
        pytest.skip('a GPU is present')
    raw, query, _ = CASES[0]
    signal = P.normalised(raw, *P.moments(raw))
    with pytest.raises(RuntimeError, match='no gfx950 device'):
        dtw.rescaled_batch([signal], [query])
    with pytest.raises(RuntimeError, match='no gfx950 device'):
        dtw.semi_global_dtw_with_rescaling_batch([signal], [query], resident=True)
    with pytest.raises(RuntimeError, match='no gfx950 device'):
        dtw.locate_batch(**good_locate_arguments())
    with pytest.raises(RuntimeError):
        prep_signal.locate_adapters([raw], query, 'start')
    with pytest.raises(RuntimeError):
        prep_signal.align_adapter_to_read_start_dtw(signal, query)
    # nothing to look at, nothing to run: no device needed
    assert prep_signal.locate_adapters([], query, 'start') == []
    assert prep_signal.locate_adapters([np.zeros(30, dtype=np.int16)], query, 'end') == \
        [(None, None)]


def test_the_default_path_is_unchanged(monkeypatch):
    """resident=False is the host loop it was: two batched passes with an lstsq fit between them,
    and never the new entry."""
    calls = []

    def batch(refs, queries, alignments=True):
        calls.append([q.copy() for q in queries])
        out = []
        for ref, query in zip(refs, queries):
            d, s, e, pairs = P.dtw_ref.semi_global_dtw(ref, query)
            out.append((d, s, e, np.array(pairs, dtype=np.int32).reshape(-1, 2)))
        return out

    def never(*args, **kwargs):
        raise AssertionError('the default path went to the resident entry')

    monkeypatch.setattr(dtw, 'semi_global_dtw_batch', batch)
    monkeypatch.setattr(dtw, 'rescaled_batch', never)
    for k in (0, 7, 39):
        raw, query, _ = CASES[k]
        signal = P.reference_normalise(raw.astype(np.float64))
        want = P.reference_rescaled(signal, query)
        for got in (dtw.semi_global_dtw_with_rescaling(signal, query),
                    dtw.semi_global_dtw_with_rescaling_batch([signal], [query])[0]):
            assert got[:3] == want[:3]
            assert got[3] == [(signal[i], want[5][j]) for i, j in want[4]]
    assert len(calls) == 12 and np.array_equal(calls[1][0], P.reference_rescaled(
        P.reference_normalise(CASES[0][0].astype(np.float64)), CASES[0][1])[5])


def test_trim_signal_keeps_the_reference_quirk(capsys):
    rng = np.random.default_rng(9)
    quiet = np.full(2500, 500, dtype=np.int16)
    loud = rng.integers(300, 700, size=3000).astype(np.int16)
    signal = np.concatenate([quiet, loud])
    trimmed = prep_signal.trim_signal(signal)
    err = capsys.readouterr().err
    assert 'excessive trimming' in err and trimmed is not None      # a verdict, yet no skip
    assert len(signal) - len(trimmed) > 2000 and np.array_equal(trimmed, signal[-len(trimmed):])
    assert prep_signal.trim_signal(quiet) is None
    assert 'failed signal trimming' in capsys.readouterr().err
    assert prep_signal.align_barcode_to_read_dtw(np.zeros(10), -1, '01', {}) == (None, None)
