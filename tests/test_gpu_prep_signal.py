"""prep's signal stage on the GPU: ``dtw_rescaled_batch`` and ``dtw_locate_batch`` against the NumPy
restatement of their contract (tests/prep_signal_reference.py), bit for bit, at the smallest shapes
that can still go wrong; ``prep_signal``'s batch forms on top."""
import numpy as np
import pytest

import prep_signal_reference as P
from deepbinner_amd import dtw_semi_global as dtw
from deepbinner_amd import prep_signal

pytestmark = pytest.mark.gpu


def bits(values):
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)


def same_result(got, want):
    """(distance, start, end, slope, pairs, query') - the floating-point ones by their bits, a
    NaN slope as a NaN."""
    assert bits(got[0]) == bits(want[0]) and got[1:3] == want[1:3], (got[:4], want[:4])
    assert (np.isnan(got[3]) and np.isnan(want[3])) or bits(got[3]) == bits(want[3]), \
        (got[3], want[3])
    assert np.array_equal(got[4], want[4])
    assert np.array_equal(bits(got[5]), bits(want[5]))


def planted(rng, query, levels_before, levels_after, scale=1.0, offset=0.0, noise=0.05):
    ref = np.concatenate([P.squiggle(rng, levels_before),
                          query + rng.normal(0, noise, len(query)), P.squiggle(rng, levels_after)])
    return ref, scale * query + offset


def pair_with_path_length(target):
    """A pair whose pass-1 alignment has exactly ``target`` entries (the fit's lane striding)."""
    for seed in range(400):
        rng = np.random.default_rng(5000 + 7 * target + seed)
        query = P.squiggle(rng, target // 6 + 2)[:max(1, target - seed % 6)]
        ref, query = planted(rng, query, 6, 6, scale=0.9 + 0.01 * (seed % 20), offset=0.2)
        if len(P.dtw_ref.semi_global_dtw(ref, query)[3]) == target:
            return ref, query
    raise AssertionError('no pair with a path of {}'.format(target))


def build_pairs():
    rng = np.random.default_rng(77)
    pairs = {}
    for n in (1, 63, 64, 65, 128, 129):
        pairs['path %d' % n] = pair_with_path_length(n)
    # the multi-panel variant of dtw_kernel: more than 64 * 16 query samples
    levels = rng.normal(0.0, 1.0, size=40)
    long_query = np.repeat(levels[3:-3], rng.integers(33, 38, size=34))[:1100]
    pairs['multi-panel'] = (np.repeat(levels, rng.integers(6, 10, size=40))[:300],
                            1.1 * long_query + 0.1 + rng.normal(0, 0.05, 1100))
    query = P.squiggle(rng, 5)
    pairs['reference of 1'] = (np.array([0.3]), query)
    pairs['reference of 2'] = (np.array([0.3, -0.8]), query)
    pairs['query of 1, reference of 1'] = (np.array([0.3]), np.array([1.5]))
    ref, query = planted(rng, P.squiggle(rng, 20), 8, 8)
    pairs['constant query'] = (ref, np.full(90, 0.25))
    for seed in range(100):      # the first pair whose slope can be walked over both bounds
        rng = np.random.default_rng(6000 + seed)
        ref, query = planted(rng, P.squiggle(rng, 20), 3, 3, noise=0.0)
        try:
            for bound in (0.75, 1.333):
                inside, outside = P.queries_beside_a_slope_bound(ref, query, bound)
                pairs['slope inside %g' % bound] = (ref, inside)
                pairs['slope outside %g' % bound] = (ref, outside)
            break
        except AssertionError:
            continue
    return pairs


def build_mixed_batch():
    """70 pairs of all three lane widths (queries up to 256, up to 512, longer)."""
    rng = np.random.default_rng(78)
    refs, queries = [], []
    for k in range(70):
        q = int(rng.choice([30, 200, 256, 257, 400, 512, 513, 700]))
        query = P.squiggle(rng, q // 6 + 2)[:q]
        ref, query = planted(rng, query, int(rng.integers(2, 30)), int(rng.integers(2, 30)),
                             scale=float(rng.uniform(0.8, 1.25)), offset=float(rng.normal(0, .3)))
        refs.append(ref)
        queries.append(query)
    return refs, queries


@pytest.fixture(scope='module')
def named_pairs():
    pairs = build_pairs()
    return pairs, {name: P.rescaled(ref, query) for name, (ref, query) in pairs.items()}


@pytest.fixture(scope='module')
def mixed_batch():
    refs, queries = build_mixed_batch()
    return refs, queries, [P.rescaled(ref, query) for ref, query in zip(refs, queries)]


def test_gpu_rescaled_cases_bit_for_bit(named_pairs):
    pairs, want = named_pairs
    names = sorted(pairs)
    got = dtw.rescaled_batch([pairs[n][0] for n in names], [pairs[n][1] for n in names])
    for name, result in zip(names, got):
        same_result(result, want[name])
    by_name = dict(zip(names, got))
    # what the cases are there for
    inf = float('inf')
    assert by_name['constant query'][0] == inf and np.isnan(by_name['constant query'][3])
    assert by_name['path 1'][0] == inf and len(by_name['path 1'][4]) == 1
    assert by_name['reference of 1'][0] == inf and by_name['reference of 1'][1:3] == (0, 0)
    assert by_name['slope outside 0.75'][0] == inf and by_name['slope outside 1.333'][0] == inf
    assert by_name['slope inside 0.75'][0] < inf and by_name['slope inside 1.333'][0] < inf
    assert 0.7499 < by_name['slope outside 0.75'][3] < 0.75 <= by_name['slope inside 0.75'][3]
    assert 1.3331 > by_name['slope outside 1.333'][3] > 1.333 >= by_name['slope inside 1.333'][3]
    assert len(pairs['multi-panel'][1]) == 1100 and by_name['multi-panel'][0] < inf
    # one pair alone gives what it gives in the batch
    for name in ('path 65', 'multi-panel', 'reference of 2'):
        same_result(dtw.rescaled_batch([pairs[name][0]], [pairs[name][1]])[0], want[name])
    # without the alignment: the same numbers
    without = dtw.rescaled_batch([pairs[n][0] for n in names], [pairs[n][1] for n in names],
                                 alignments=False)
    for a, b in zip(without, got):
        assert a[4] is None and bits(a[0]) == bits(b[0]) and a[1:3] == b[1:3]


def test_gpu_rescaled_mixed_batch_split_and_twice(mixed_batch, monkeypatch):
    """70 pairs of mixed lane widths in one call; the same under a direction-word budget that cuts
    every width's pairs into several parts (a pair's pass 1, fit and pass 2 stay together); the
    same call twice."""
    refs, queries, want = mixed_batch
    whole = dtw.rescaled_batch(refs, queries)
    for got, expected in zip(whole, want):
        same_result(got, expected)
    assert sum(1 for w in want if np.isfinite(w[0])) > 40
    milliseconds, cells = dtw.last_kernel_time()          # both passes of every pair
    assert milliseconds > 0.0 and cells == 2 * sum(len(r) * len(q) for r, q in zip(refs, queries))
    again = dtw.rescaled_batch(refs, queries)
    monkeypatch.setenv('DEEPBINNER_DTW_PATH_BYTES', str(300 * 1024))
    split = dtw.rescaled_batch(refs, queries)
    for other in (again, split):
        for got, expected in zip(other, whole):
            same_result(got, expected)


def test_gpu_resident_through_python(named_pairs, mixed_batch):
    pairs, want = named_pairs
    for name in ('path 129', 'slope outside 0.75', 'constant query'):
        ref, query = pairs[name]
        distance, start, end, values = dtw.semi_global_dtw_with_rescaling(ref, query,
                                                                          resident=True)
        w = want[name]
        assert bits(distance) == bits(w[0]) and (start, end) == w[1:3]
        assert values == [(ref[i], w[5][j]) for i, j in w[4]]
    refs, queries, want = mixed_batch
    for got, w, ref in zip(dtw.semi_global_dtw_with_rescaling_batch(refs[:8], queries[:8],
                                                                    resident=True), want, refs):
        assert bits(got[0]) == bits(w[0]) and got[1:3] == w[1:3]
        assert got[3] == [(ref[i], w[5][j]) for i, j in w[4]]


# --------------------------------------------------------------------------------------- locate
LENGTHS = [16000, 16000, 4000, 4000, 1500, 1500, 1501, 1501, 700, 700, 1, 1]
PLANTS = [15600, 100, 2450, 1250, 600, None, 1100, None, 200, 'flat', None, 'flat']
SEED = 80         # with it every read that can be trimmed is trimmed at PREFIX exactly
PREFIX = 60          # open-pore samples in front of a read: 10 + two quiet windows of 25


def build_reads(seed=SEED):
    """12 trimmed int16 reads; a scaled, noisy copy of the adapter planted so that the first hit
    is window 0, window 3, the last window and nowhere, for both sides; two reads with D == 0."""
    rng = np.random.default_rng(seed)
    adapter = P.squiggle(rng, 45)[:300]
    reads = []
    for length, plant in zip(LENGTHS, PLANTS):
        signal = P.squiggle(rng, length // 6 + 2)[:length]
        if plant == 'flat':
            reads.append(np.full(length, 431, dtype=np.int16))
            continue
        if plant is not None:
            signal[plant:plant + 300] = adapter + rng.normal(0, 0.05, 300)
        reads.append(np.round(signal * 80.0 + 500.0).astype(np.int16))
    return reads, 1.1 * adapter + 0.2


def restated_scan(reads, windows_of, queries_of):
    """The restatement's answer for one group per read."""
    regions, mean_std, jobs, group_offsets, table = [], [], [], [0], []
    for r, read in enumerate(reads):
        regions.append(read)
        mean_std.append(P.moments(read))
        for a, b in windows_of(r):
            table.append(queries_of(r))
            jobs.append((r, a, b, len(table) - 1))
        group_offsets.append(len(jobs))
    return jobs, group_offsets, P.locate(regions, mean_std, table, jobs, group_offsets, 50.0)


@pytest.fixture(scope='module')
def scans():
    reads, adapter = build_reads()
    out = {'reads': reads, 'adapter': adapter}
    for side in ('start', 'end'):
        out[side] = restated_scan(reads, lambda r: prep_signal.adapter_windows(len(reads[r]), side),
                                  lambda r: adapter)
    return out


def window_of_hit(jobs, group_offsets, hits, r):
    return -1 if hits[r] < 0 else int(hits[r]) - group_offsets[r]


def absolute(jobs, positions, hits, r):
    if hits[r] < 0:
        return None, None
    return (int(positions[hits[r], 0]) + jobs[hits[r]][1],
            int(positions[hits[r], 1]) + jobs[hits[r]][1])


@pytest.mark.parametrize('side', ['start', 'end'])
def test_gpu_locate_bit_for_bit(scans, side):
    reads, adapter = scans['reads'], scans['adapter']
    jobs, group_offsets, (distances, positions, slopes, hits) = scans[side]
    # the inputs are what the test is after
    found = [window_of_hit(jobs, group_offsets, hits, r) for r in range(len(reads))]
    assert found[:4] == ([29, 0, 3, 0] if side == 'start' else [0, 29, 1, 3]), found
    assert {0, 3, 29, -1} <= set(found) and found[9:] == [-1, -1, -1], found
    assert any(a == b for _, a, b, _ in jobs) == (side == 'start')          # empty windows
    assert any(b - a == 1 for _, a, b, _ in jobs) == (side == 'start')      # one-sample windows
    assert P.moments(reads[9])[1] == 0.0
    finite = distances[np.isfinite(distances)]
    assert np.all(np.abs(finite - 50.0) > 1e-6)       # no verdict hangs on the last bits

    got = prep_signal.locate(
        reads, [prep_signal.adapter_region(len(read), side) for read in reads],
        [[(a, b, adapter) for a, b in prep_signal.adapter_windows(len(read), side)]
         for read in reads])
    first = [prep_signal.adapter_region(len(read), side)[0] for read in reads]
    assert [(r, a - first[r], b - first[r]) for r, a, b, _ in jobs] == \
        [job[:3] for job in got['jobs']]
    assert list(got['group_offsets']) == group_offsets
    assert np.array_equal(got['hits'], hits)
    assert np.array_equal(bits(got['distances']), bits(distances))
    assert np.array_equal(got['job_positions'], positions)
    nan = np.isnan(slopes)
    assert np.array_equal(np.isnan(got['slopes']), nan)
    assert np.array_equal(bits(got['slopes'][~nan]), bits(slopes[~nan]))
    want_positions = [absolute(jobs, positions, hits, r) for r in range(len(reads))]
    assert got['positions'] == want_positions
    # the same call twice: the same bits
    again = prep_signal.locate(
        reads, [prep_signal.adapter_region(len(read), side) for read in reads],
        [[(a, b, adapter) for a, b in prep_signal.adapter_windows(len(read), side)]
         for read in reads])
    for key in ('distances', 'slopes'):
        assert np.array_equal(bits(again[key]), bits(got[key]))
    assert np.array_equal(again['job_positions'], got['job_positions'])
    assert np.array_equal(again['hits'], got['hits'])

    # through locate_adapters, from raw reads with open-pore signal in front: the reads that can
    # be trimmed give the same positions, the others (one sample, flat) none
    raw = [np.concatenate([np.full(PREFIX, 520, dtype=np.int16), read]) for read in reads]
    trimmed = [prep_signal.trim_signal(signal, out=None) for signal in raw]
    for r, t in enumerate(trimmed):
        if len(reads[r]) > 1 and PLANTS[r] != 'flat':
            assert t is not None and np.array_equal(t, reads[r]), r
        else:
            assert t is None, r
    located = prep_signal.locate_adapters(raw, adapter, side)
    assert located == [p if trimmed[r] is not None else (None, None)
                       for r, p in enumerate(want_positions)]
    assert sum(1 for p in located if p[0] is not None) >= 4


@pytest.mark.parametrize('side', ['start', 'end'])
def test_gpu_locate_barcodes_on_top(scans, side):
    """The barcode scan behind the adapter scan: a scaled piece of each read beside its adapter
    as that read's barcode squiggle; search windows as the reference cuts them."""
    reads, adapter = scans['reads'], scans['adapter']
    jobs, group_offsets, (_, positions, _, hits) = scans[side]
    adapters = [absolute(jobs, positions, hits, r) for r in range(len(reads))]
    signals = [P.normalised(read, *P.moments(read)) for read in reads]
    barcodes, want = [], []
    for r, (a_start, a_end) in enumerate(adapters):
        if a_start is None:
            barcodes.append(None)
            want.append((None, None))
            continue
        at = a_end + 30 if side == 'start' else a_start - 330
        piece = signals[r][max(at, 0):max(at, 0) + 200]
        barcodes.append(1.1 * piece + 0.1 if len(piece) > 10 else np.array([0.5, -0.5, 1.0]))
        # prep_native_start.py:90-95, prep_native_end.py:91-95, prep_functions.py:138-153
        search_start = a_end - 100 if side == 'start' else a_start - 1000
        search = signals[r][search_start:a_end + 1000] if side == 'start' \
            else signals[r][search_start:]
        if search_start < 0:
            want.append((None, None))
            continue
        distance, start, end = P.rescaled(search, barcodes[-1])[:3]
        want.append((None, None) if distance > 50.0
                    else (start + search_start, end + search_start))
    assert sum(1 for w in want if w[0] is not None) >= 2, want
    if side == 'end':       # the refusal of a search window that starts before the signal
        assert any(w[0] is None and b is not None for w, b in zip(want, barcodes)), want
    raw = [np.concatenate([np.full(PREFIX, 520, dtype=np.int16), read]) for read in reads]
    assert prep_signal.locate_barcodes(raw, adapters, barcodes, side) == want
    # the reference's one-read names on the normalised signal: the same positions
    r = next(r for r, w in enumerate(want) if w[0] is not None)
    one = prep_signal.align_adapter_to_read_start_dtw if side == 'start' \
        else prep_signal.align_adapter_to_read_end_dtw
    assert one(signals[r], adapter) == adapters[r]
    assert one(reads[r], adapter) == adapters[r]
    search_start = adapters[r][1] - 100 if side == 'start' else adapters[r][0] - 1000
    search = signals[r][search_start:adapters[r][1] + 1000] if side == 'start' \
        else signals[r][search_start:]
    assert prep_signal.align_barcode_to_read_dtw(search, search_start, '07',
                                                 {'07': barcodes[r]}) == want[r]
