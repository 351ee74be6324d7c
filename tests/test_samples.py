"""``prep_signal.trim_positions``, the squiggle files, and the host rules of
``deepbinner_amd.samples`` (label tables, cutting rules, spacing verdicts) against their
restatements (tests/samples_reference.py, tests/read_batch_reference.py).  No device."""
import os
import random

import numpy as np
import pytest

import read_batch_reference as B
import samples_reference as S
from deepbinner_amd import prep_signal, samples
from deepbinner_amd.trim_signal import CannotTrim, find_signal_start_pos

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float('inf'), float('nan')


# ------------------------------------------------------------------------------- trim_positions
def reference_trim(signal):
    try:
        return find_signal_start_pos(signal)
    except CannotTrim:
        return -1


def test_trim_positions_on_synthetic_reads_and_every_short_length():
    rng = np.random.default_rng(21)
    reads = [S.synthetic_raw(rng) for _ in range(300)]
    base = S.synthetic_raw(rng)
    while len(base) < 200:
        base = S.synthetic_raw(rng)
    noisy = np.round(rng.normal(500, 60, 200)).astype(np.int16)
    reads += [base[len(base) - n:] for n in range(201)] + [noisy[:n] for n in range(201)]
    got = prep_signal.trim_positions(reads)
    assert got.dtype == np.int64 and len(got) == len(reads)
    assert list(got) == [B.trim_position(read) for read in reads]
    assert list(got) == [reference_trim(read) for read in reads]
    assert (got[:300] >= 0).sum() > 100 and (got[:300] < 0).sum() > 5
    assert (got[300:] >= 0).any() and got[300 + 134] == -1 and got[501 + 134] == -1
    assert list(prep_signal.trim_positions([])) == []


def test_trim_positions_on_the_golden_reads():
    gold = np.load(os.path.join(REPO, 'tests', 'golden', 'reads.npz'))
    offsets = gold['offsets']
    reads = [gold['samples'][offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
    assert len(reads) == 7
    got = prep_signal.trim_positions(reads)
    assert list(got) == [reference_trim(read) for read in reads]
    assert list(got) == [B.trim_position(read) for read in reads]


# ------------------------------------------------------------------------------ the cutting rules
SIGNAL = np.arange(60000, dtype=np.int32) % 30011          # every slice names where it came from


def both(ours, theirs, seeds=range(40)):
    """The same generator state into both: our (span) against the restated (sample)."""
    seen = set()
    for seed in seeds:
        a, b = random.Random('cut:{}'.format(seed)), random.Random('cut:{}'.format(seed))
        got, want = ours(a), theirs(b)
        assert (got is None) == (want is None)
        if got is not None:
            assert np.array_equal(got, want)
            seen.add(int(got[0]))
        assert a.random() == b.random()                    # as many draws in both
    return seen


@pytest.mark.parametrize('length,include,size,some', [
    (5000, (0, 20), 96, True),              # an include range at sample 0: only start 0 is left
    (5000, (-10, 10), 96, False),           # beginning before the read: randint over nothing
    (5000, (4950, 4990), 96, True),         # a sample shifted back at the read's end
    (80, (30, 50), 96, False),              # a read shorter than signal_size: start goes negative
    (96, (30, 50), 96, True),
    (97, (1, 96), 96, True),                # a span of size - 1
    (5000, (300, 395), 96, True),
    (5000, (300, 500), 1024, True),
])
def test_sample_around_a_signal(length, include, size, some):
    signal = SIGNAL[:length]
    seen = both(lambda rng: samples.cut(signal, samples.around_signal(rng, length, *include, size), size),
                lambda rng: S.reference_around(rng, signal, *include, size))
    assert bool(seen) == some
    if include == (0, 20):
        assert seen == {0}
    if include == (4950, 4990):
        # starts are drawn from 4894 .. 4950; those above 4904 are moved back to it
        assert max(seen) == length - size and min(seen) >= 4990 - size and len(seen) > 3


@pytest.mark.parametrize('size', [96, 1024])
def test_sample_from_the_middle_at_its_boundary(size):
    for length, some in ((50000 + size - 1, False), (50000 + size, True), (50000 + size + 7, True),
                         (3000, False)):
        signal = SIGNAL[:length]
        seen = both(lambda rng: samples.cut(signal, samples.from_middle(rng, length, size), size),
                    lambda rng: S.reference_middle(rng, signal, size))
        assert bool(seen) == some
        if length == 50000 + size:
            assert seen == {int(signal[25000])}


@pytest.mark.parametrize('point,some', [(95, False), (96, True), (97, True), (400, True), (-5, False)])
def test_sample_before_a_point(point, some):
    signal = SIGNAL[:5000]
    seen = both(lambda rng: samples.cut(signal, samples.before_signal(rng, point, 96), 96),
                lambda rng: S.reference_before(rng, signal, point, 96))
    assert bool(seen) == some
    if point == 96:
        assert seen == {0}


@pytest.mark.parametrize('point,some', [(4905, False), (4904, True), (4000, True), (-200, True),
                                        (-96, True)])
def test_sample_after_a_point(point, some):
    # (a point below -size lets the generator draw an end in front of `size`: the slice comes out
    # short, or empty, and is dropped - in both)
    signal = SIGNAL[:5000]
    seen = both(lambda rng: samples.cut(signal, samples.after_signal(rng, 5000, point, 96), 96),
                lambda rng: S.reference_after(rng, signal, point, 96), seeds=range(60))
    assert bool(seen) == some
    if point == 4904:
        assert seen == {int(signal[4904])}


@pytest.mark.parametrize('side,gaps', [('start', {14: 'gap', 15: None, 90: None, 91: 'gap'}),
                                       ('end', {-101: 'gap', -100: None, -20: None, -19: 'gap'})])
def test_spacing_verdicts_at_their_bounds(side, gaps):
    text = {None: None, 'gap': samples.ODD_GAP, 'long': samples.TOO_LONG}
    for gap, want in gaps.items():
        for span, long_ in ((95, None), (96, 'long'), (97, 'long')):
            if side == 'start':
                adapter, barcode = (400, 640), (640 + gap, 640 + gap + span)
            else:
                adapter, barcode = (3000, 3240), (3000 - gap - span, 3000 - gap)
            said = []
            got = samples.oddly_spaced(side, adapter, barcode, 96, said.append)
            assert S.reference_oddly_spaced(side, adapter, barcode, 96) == (long_ or want)
            assert got == text[long_ or want]
            # the too-long verdict comes before the gap is printed (prep_native_start.py:154-158)
            assert len(said) == (0 if long_ else 2)
            if not long_:
                assert said[0].endswith('signal gap: {}'.format(gap))
                assert said[1] == '    barcode signal size: {}'.format(span)


# ------------------------------------------------------------------------------------ the tables
def test_label_tables_in_both_forms(tmp_path):
    summary = tmp_path / 'summary.txt'
    summary.write_text('filename\tread_id\tx\tbarcode_arrangement\n'
                       'a.fast5\tr-zero\t1\t0\n'
                       'a.fast5\tr-none\t1\tnone\n'
                       'a.fast5\tr-unc\t1\tunclassified\n'
                       'filename\tread_id\tx\tbarcode_arrangement\n'          # summaries concatenated
                       'a.fast5\tr-seven\t1\tbarcode07\n'
                       'a.fast5\tr-twelve\t1\t12\n')
    want = {'r-zero': 0, 'r-none': None, 'r-unc': None, 'r-seven': 7, 'r-twelve': 12}
    assert samples.read_labels(str(summary)) == want
    table = tmp_path / 'classes.txt'
    table.write_text('read_ID\tbarcode_call\tstart_none\n'
                     'r-zero\t0\t0.1\nr-none\tnone\t0.9\nr-unc\tunclassified\t0.9\n'
                     'r-seven\t7\t0.0\nr-twelve\t12\t0.0\n')
    assert samples.read_labels(str(table)) == want
    assert [samples.parse_label(t) for t in ('0', 'none', 'unclassified', 'barcode07', '07', '7')] \
        == [0, None, None, 7, 7, 7]
    with pytest.raises(SystemExit) as e:
        samples.parse_label('barcodeX')
    assert 'not a barcode label' in str(e.value)


def test_summary_without_its_columns(tmp_path):
    for header, missing in (('filename\tbarcode_arrangement', 'read_id'),
                            ('filename\tread_id', 'barcode_arrangement')):
        path = tmp_path / (missing + '.txt')
        path.write_text(header + '\na\tb\n')
        with pytest.raises(SystemExit) as e:
            samples.read_labels(str(path))
        assert str(e.value) == 'Error: {} does not have a {} column'.format(path, missing)


# --------------------------------------------------------------------------------- squiggle files
def test_squiggle_files_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    table = {'adapter': rng.normal(size=40), 12: rng.normal(size=25) * 1e-7, 1: rng.normal(size=31),
             3: np.array([0.1, -2.5e300, 1 / 3])}
    path = str(tmp_path / 'squiggles.txt')
    prep_signal.write_squiggles(path, table)
    lines = open(path).read().splitlines()
    assert [line.split('\t')[0] for line in lines] == ['adapter', '01', '03', '12']
    back = prep_signal.read_squiggles(path)
    assert set(back) == set(table)
    for key in table:
        assert back[key].dtype == np.float64 and np.array_equal(back[key], table[key])
    # names as people write them
    (tmp_path / 'short.txt').write_text('1\t0.5,1\n\nadapter\t1e-3,2,-3.25\n')
    short = prep_signal.read_squiggles(str(tmp_path / 'short.txt'))
    assert list(short[1]) == [0.5, 1.0] and list(short['adapter']) == [0.001, 2.0, -3.25]


@pytest.mark.parametrize('text,said', [
    ('adapter\t1,2\n01\t1,2\n1\t3,4\n', 'second squiggle named 1'),
    ('adapter\t1,2\nadapter\t1,2\n', 'second squiggle named adapter'),
    ('01\t1,2\n', 'no squiggle named adapter'),
    ('adapter\t1,,2\n', 'empty or non-numeric'),
    ('adapter\t\n', 'empty or non-numeric'),
    ('adapter\t1,x\n', 'empty or non-numeric'),
    ('adapter\t1,inf\n', 'not finite'),
    ('adapter\t1,nan\n', 'not finite'),
    ('adapter\t1,2\nbc1\t1,2\n', 'barcode number'),
    ('adapter 1,2\n', 'name<TAB>'),
])
def test_squiggle_file_errors(tmp_path, text, said):
    path = tmp_path / 'bad.txt'
    path.write_text(text)
    with pytest.raises(ValueError) as e:
        prep_signal.read_squiggles(str(path))
    assert said in str(e.value)
    with pytest.raises(ValueError):
        prep_signal.write_squiggles(str(tmp_path / 'out.txt'), {1: [1.0]})
    with pytest.raises(ValueError):
        prep_signal.write_squiggles(str(tmp_path / 'out.txt'), {'adapter': [1.0, INF]})
