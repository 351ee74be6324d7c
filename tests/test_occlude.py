"""``locate --occlude`` without a device: the CPU models of the kernels (``dbh_occlude_plan_host``,
``dbh_occlude_windows_host``) against the NumPy restatement bit for bit - they are copies and zeros,
no tolerance - the identities of the rule, how often the fp64 oracle alone sits within rounding of a
threshold, the command against a host stand-in, and the C ABI's argument checks."""
import ctypes
import os

import numpy as np
import pytest

import locate_reference as loc_ref
import occlude_reference as ref
from conftest import REPO
from deepbinner_amd import deepbinner as cli
from deepbinner_amd import hip_backend, locate
from test_locate import ENDS, STARTS, expected_rows, options, table, three_files  # noqa: F401

INVALID, UNSUPPORTED = 1, 5
NEW_SYMBOLS = ['dbh_occlude_plan_dev', 'dbh_occlude_plan_host', 'dbh_occlude_windows_dev',
               'dbh_occlude_windows_host', 'dbh_locate_occluded_workspace_bytes',
               'dbh_locate_occluded_i16']
SIDES = ['start', 'end']


def same_records(got, want):
    assert got.dtype == want.dtype
    for name in want.dtype.names:
        assert got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert got.tobytes() == want.tobytes()


# ---- 1: the CPU models against the restatement ------------------------------------------------------
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('input_size,steps,n_reads', ref.GEOMETRIES)
def test_host_models_match_the_restatement(input_size, steps, n_reads, side):
    x, lengths, locations = ref.random_case(input_size, steps, n_reads, side,
                                            seed=input_size + 100 * steps + n_reads)
    plans, occlusions = hip_backend.occlude_plan(locations, lengths, steps, input_size, side)
    want_plans, want_occlusions = ref.plan(locations, lengths, steps, input_size, side)
    same_records(plans, want_plans)
    same_records(occlusions, want_occlusions)
    variants = hip_backend.occlude_windows(x, lengths, plans, side)
    same_bits(variants, ref.blank(x, lengths, want_plans, side))

    # the identities: OUT and ONLY partition R; nothing outside R or in the pad moves; idempotent
    for r in range(n_reads):
        n = int(lengths[r])
        lo, hi = ref.scanned(n, steps, input_size, side)
        out = ref.blank_mask(plans[r], ref.OUT, n, steps, input_size, side)
        only = ref.blank_mask(plans[r], ref.ONLY, n, steps, input_size, side)
        ctrl = ref.blank_mask(plans[r], ref.CTRL, n, steps, input_size, side)
        t = np.array([ref.origin(n, s, input_size, side) + np.arange(input_size)
                      for s in range(steps)])
        in_r = (t >= lo) & (t < hi)
        assert np.array_equal(in_r, (t >= 0) & (t < n))         # a window's read samples lie in R
        if plans[r]['valid'] & 1:
            assert np.array_equal(out ^ only, in_r) and not (out & only).any()
        else:
            assert not out.any() and not only.any() and not ctrl.any()
            assert plans[r]['valid'] == 0 and occlusions[r]['ctrl_first'] == -1
        if plans[r]['valid'] & 4:
            assert not (ctrl & out).any()
            assert occlusions[r]['ctrl_end'] - occlusions[r]['ctrl_first'] == \
                plans[r]['end'][0] - plans[r]['first'][0]
            assert lo <= occlusions[r]['ctrl_first'] and occlusions[r]['ctrl_end'] <= hi
        for v, mask in enumerate((out, only, ctrl)):
            kept = variants[v, r][~mask]
            assert kept.tobytes() == x[r][~mask].tobytes()
            assert not variants[v, r][mask].any()
    again = [hip_backend.occlude_windows(variants[v], lengths, plans, side)[v] for v in range(3)]
    same_bits(np.stack(again), variants)


def test_shapes_and_planted_kinds_are_covered():
    assert {g[0] for g in ref.GEOMETRIES} == {96, 98, 160, 1024}
    assert {g[1] for g in ref.GEOMETRIES} == {1, 2, 12}
    assert {g[2] for g in ref.GEOMETRIES} == {1, 64, 65}
    touching = overlapping = whole = padded = clipped = midpoint = 0
    for input_size, steps, n_reads in ref.GEOMETRIES:
        for side in SIDES:
            _, lengths, locations = ref.random_case(input_size, steps, n_reads, side,
                                                    seed=input_size + 100 * steps + n_reads)
            L, h = input_size, input_size // 2
            if n_reads >= 5:
                assert list(lengths[:4]) == [L // 3, L, L + h - 1, L + h] and lengths[4] > steps * h + L
            plans, occlusions = ref.plan(locations, lengths, steps, input_size, side)
            for r in range(n_reads):
                lo, hi = ref.scanned(int(lengths[r]), steps, input_size, side)
                first, end = plans[r]['first'][0], plans[r]['end'][0]
                ctrl = (plans[r]['first'][2], plans[r]['end'][2])
                valid = int(plans[r]['valid'])
                whole += valid & 1 and (first, end) == (lo, hi)
                touching += valid == 7 and (ctrl[0] == end or ctrl[1] == first)
                overlapping += valid == 3 and hi - (end - first) == end - 1
                padded += locations[r]['cls'] > 0 and valid == 0
                clipped += valid & 1 and locations[r]['first_sample'] < lo
                midpoint += valid & 1 and first + end == lo + hi
    assert min(touching, overlapping, whole, padded, clipped, midpoint) >= 3, \
        (touching, overlapping, whole, padded, clipped, midpoint)


def planted(side, steps, input_size, n, cls, first, end):
    location = ref.location_of(cls, first, end).reshape(1)
    plans, occlusions = hip_backend.occlude_plan(location, [n], steps, input_size, side)
    same_records(plans, ref.plan(location, [n], steps, input_size, side)[0])
    return plans[0], occlusions[0]


def test_planted_locations():
    # start side, 2 steps of 1024: R = [0, 1536)
    plan, occ = planted('start', 2, 1024, 5000, 3, 0, 128)                 # the read's first sample
    assert (plan['valid'], occ['ctrl_first'], occ['ctrl_end']) == (7, 1408, 1536)
    plan, occ = planted('end', 2, 1024, 5000, 3, 4872, 5000)               # the read's last sample
    assert (plan['valid'], occ['ctrl_first'], occ['ctrl_end']) == (7, 3464, 3592)
    plan, occ = planted('end', 1, 1024, 300, 2, 0, 44)                     # partly in the padding
    assert (plan['valid'], plan['first'][0], plan['end'][0]) == (7, 0, 44)
    assert (occ['ctrl_first'], occ['ctrl_end']) == (256, 300)
    plan, occ = planted('end', 1, 1024, 300, 2, 0, 0)                      # wholly in the padding
    assert plan['valid'] == 0 and occ['cls'] == 2 and occ['out_call'] == -1 and np.isnan(occ['out_p'])
    assert (occ['ctrl_first'], occ['ctrl_end']) == (-1, -1) and np.isnan(occ['p'])
    plan, occ = planted('start', 2, 1024, 5000, 3, 512, 1024)              # midpoint on R's: the first m
    assert (plan['valid'], occ['ctrl_first'], occ['ctrl_end']) == (7, 0, 512)
    plan, occ = planted('start', 2, 1024, 5000, 3, 511, 1023)              # below it: the last m
    assert (plan['valid'], occ['ctrl_first'], occ['ctrl_end']) == (7, 1024, 1536)
    plan, occ = planted('start', 2, 1024, 5000, 3, 0, 768)                 # control touches the span
    assert (plan['valid'], occ['ctrl_first'], occ['ctrl_end']) == (7, 768, 1536)
    plan, occ = planted('start', 2, 1024, 1535, 3, 0, 768)                 # ... overlaps it by one
    assert (plan['valid'], occ['ctrl_first'], occ['ctrl_end']) == (3, -1, -1)
    assert occ['ctrl_call'] == -1 and np.isnan(occ['ctrl_p'])
    plan, occ = planted('start', 2, 1024, 5000, 0, -1, -1)                 # no call
    assert plan['valid'] == 0 and occ['cls'] == 0 and np.isnan(occ['p'])
    plan, occ = planted('start', 2, 1024, 5000, 3, 0, 1536)                # all of R
    assert plan['valid'] == 3 and (plan['first'][0], plan['end'][0]) == (0, 1536)


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('input_size', [98, 1024])
def test_a_span_of_all_of_r(input_size, side):
    """ONLY leaves the windows bit-identical to the input and OUT makes them all zero."""
    steps, rng = 2, np.random.default_rng(input_size)
    lengths = np.array([input_size // 3, input_size, 4 * input_size + 3], dtype=np.int64)
    x = rng.standard_normal((3, steps, input_size)).astype(np.float32)
    locations = []
    for r, n in enumerate(lengths):
        lo, hi = ref.scanned(int(n), steps, input_size, side)
        locations.append(ref.location_of(1, lo, hi))
        for s in range(steps):
            t = ref.origin(int(n), s, input_size, side) + np.arange(input_size)
            x[r, s][(t < 0) | (t >= n)] = 0
    plans, _ = hip_backend.occlude_plan(np.array(locations, dtype=loc_ref.LOCATION), lengths,
                                        steps, input_size, side)
    variants = hip_backend.occlude_windows(x, lengths, plans, side)
    assert variants[ref.ONLY].tobytes() == x.tobytes()
    assert not variants[ref.OUT].any() and x.any()


def test_unaligned_buffers_take_the_same_values():
    """The 16-byte path at every offset of the input and of the variants from a 16-byte boundary."""
    lib = hip_backend.load_library()
    input_size, steps, n_reads = 98, 2, 3
    x, lengths, locations = ref.random_case(input_size, steps, n_reads, 'end', seed=3)
    plans, _ = ref.plan(locations, lengths, steps, input_size, 'end')
    want = ref.blank(x, lengths, plans, 'end')
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    for shift_in in range(4):
        for shift_out in range(4):
            raw_in = np.zeros(x.size + 8, np.float32)
            raw_out = np.full(3 * x.size + 8, 7, np.float32)
            at = (-raw_in.ctypes.data // 4) % 4 + shift_in            # floats to boundary + shift
            to = (-raw_out.ctypes.data // 4) % 4 + shift_out
            raw_in[at:at + x.size] = x.ravel()
            assert lib.dbh_occlude_windows_host(
                raw_in[at:].ctypes.data, offsets.ctypes.data, plans.ctypes.data, n_reads, steps,
                input_size, 1, raw_out[to:].ctypes.data) == 0
            assert raw_out[to:to + 3 * x.size].tobytes() == want.tobytes(), (shift_in, shift_out)
            assert (raw_out[:to] == 7).all() and (raw_out[to + 3 * x.size:] == 7).all()


# ---- 2: the fp64 oracle alone --------------------------------------------------------------------------
def test_route_cases_cover_the_sizes_and_class_counts():
    assert {(c[0], c[1]) for c in ref.ROUTE_CASES} == {(L, C) for L in (96, 160, 1024)
                                                       for C in (2, 13)}
    assert {c[2].split('-')[0] for c in ref.ROUTE_CASES} == {'flipped', 'random'}


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('input_size,n_classes,model,steps,score_diff', ref.ROUTE_CASES)
def test_the_oracle_is_seldom_within_rounding_of_a_threshold(input_size, n_classes, model, steps,
                                                             score_diff, side):
    """The device test leaves a read's call out where the oracle's lead over score_diff is below
    1e-4: with these reads, weights and score_diff the oracle alone leaves out fewer than 1 in 20,
    and calls some of the reads."""
    signals, calls, locations, occlusions, v_probs, leads = ref.oracle_route(
        input_size, n_classes, model, steps, score_diff, side)
    assert len(signals) == 32 and v_probs.shape == (3, 32, n_classes)
    near = int((np.abs(leads) < 1e-4).any(axis=0).sum())
    has = occlusions['out_call'] >= 0
    print('occlude oracle: L {} C {} {} side {}: {} located, {} with a control, {} near a threshold; '
          'out flips {}, only keeps {}, ctrl keeps {}'.format(
              input_size, n_classes, model, side, int(has.sum()),
              int((occlusions['ctrl_call'] >= 0).sum()), near,
              int((occlusions['out_call'][has] != occlusions['cls'][has]).sum()),
              int((occlusions['only_call'] == occlusions['cls']).sum()),
              int((occlusions['ctrl_call'] == occlusions['cls']).sum())))
    assert near * 20 < len(signals)
    assert has.sum() >= 2
    assert np.array_equal(has, (locations['cls'] > 0) &
                          (locations['end_sample'] > locations['first_sample']))
    assert np.isnan(occlusions['out_p'][~has]).all() and np.isfinite(occlusions['out_p'][has]).all()
    lengths = {len(s) for s in signals}
    h = input_size // 2
    assert {input_size // 3, input_size, input_size + h - 1, input_size + h} <= lengths
    assert max(lengths) > steps * h + input_size


# ---- 3: the command against a host stand-in ----------------------------------------------------------
def test_command_with_occlude(oracle_backend, three_files, capsys):
    directory, reads = three_files
    backend = ref.HostBackend()
    capsys.readouterr()
    locate.locate(options(input=directory, occlude=True), backend=backend)
    out, err = capsys.readouterr()
    header, lines = table(out)
    per_side = ['class', 'first', 'end', 'peak', 'share', 'out_call', 'out_p', 'only_call', 'only_p',
                'ctrl_call', 'ctrl_p']
    assert header == ['read_ID', 'barcode_call', 'samples'] + [
        side + '_' + column for side in ('start', 'end') for column in per_side]
    assert backend.occluded == 2 and backend.batches == 2
    plain = expected_rows(reads, (('start', STARTS), ('end', ENDS)))
    rows = {line[0]: line for line in lines}
    assert sorted(rows) == sorted(plain)
    counts = {side: {v: [0, 0] for v in ref.VARIANTS} for side in ('start', 'end')}
    for name, row in rows.items():
        assert row[:3] == plain[name][:3]
        for k, side in enumerate(('start', 'end')):
            fields = row[3 + 11 * k:14 + 11 * k]
            assert fields[:5] == plain[name][3 + 5 * k:8 + 5 * k]
            if fields[0] == '-':
                assert fields[5:] == ['-'] * 6
                continue
            assert fields[5] != '-' and fields[7] != '-'         # a span with samples: OUT and ONLY
            for j, v in enumerate(ref.VARIANTS):
                call, p = fields[5 + 2 * j], fields[6 + 2 * j]
                assert (call == '-') == (p == '-')
                if call == '-':
                    continue
                assert 0 <= int(call) < 13 and 0 <= float(p) <= 1 and len(p.split('.')[1]) == 4
                counts[side][v][0] += 1
                counts[side][v][1] += (call != fields[0]) if v == 'out' else (call == fields[0])
    assert rows['noise'][3:] == ['-'] * 22
    assert sum(counts[side]['out'][0] for side in counts) > 0
    for side in ('start', 'end'):
        c = counts[side]
        assert ('{}: occluded: call lost under out {} of {}, kept under only {} of {}, kept under '
                'ctrl {} of {}'.format(side, c['out'][1], c['out'][0], c['only'][1], c['only'][0],
                                       c['ctrl'][1], c['ctrl'][0])) in err
    assert '4 reads' in err and 'located, median share' in err


def test_command_without_the_flag_is_byte_identical(oracle_backend, three_files, capsys):
    """No flag: the output of today and the entry of today (the stand-in without the new entry)."""
    directory, reads = three_files
    capsys.readouterr()
    locate.locate(options(input=directory), backend=loc_ref.HostBackend())
    before = capsys.readouterr()
    backend = ref.HostBackend()
    locate.locate(options(input=directory, occlude=False), backend=backend)
    after = capsys.readouterr()
    assert after.out == before.out and after.err == before.err and 'occluded' not in after.err
    assert backend.occluded == 0 and backend.batches == 2
    header, lines = table(after.out)
    assert len(header) == 13
    assert sorted(lines) == sorted(expected_rows(reads, (('start', STARTS), ('end', ENDS))).values())


@pytest.mark.parametrize('given,message', [
    (dict(start_model=None, end_model=None), 'you must provide at least one model'),
    (dict(devices=2), 'a locate runs on one GPU'),
    (dict(batch_size=0), '--batch_size must be at least 1'),
    (dict(scan_size=6000.0), '--scan_size must be a multiple of half the model input size'),
])
def test_command_refusals_with_occlude(oracle_backend, given, message):
    with pytest.raises(SystemExit) as e:
        locate.locate(options(occlude=True, **given), backend=ref.HostBackend())
    assert message in str(e.value)


def test_command_line_entry(monkeypatch):
    seen = {}
    monkeypatch.setattr(locate, 'locate', lambda args: seen.update(vars(args)))
    cli.main(['locate', '--native', 'some_dir'])
    assert seen['occlude'] is False and seen['scan_size'] == 6144
    cli.main(['locate', '--native', '--occlude', 'some_dir'])
    assert seen['occlude'] is True and seen['scan_size'] == 6144 and seen['score_diff'] == 0.5
    for other in ('classify', 'scan'):
        with pytest.raises(SystemExit):
            cli.main([other, '--native', '--occlude', 'some_dir'])
    for refused in ('prep', 'train'):
        with pytest.raises(SystemExit) as e:
            cli.main([refused, '--occlude'])
        assert 'not part of this build' in str(e.value) and 'scan and locate' in str(e.value)


# ---- 4: the C ABI without a device -------------------------------------------------------------------
def test_symbols_records_and_documents():
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in hip_backend.EXPORTED_SYMBOLS, name
    assert hip_backend.OCCLUSION == ref.OCCLUSION and hip_backend.OCCLUSION.itemsize == 64
    assert hip_backend.OCCLUDE_PLAN == ref.PLAN and hip_backend.OCCLUDE_PLAN.itemsize == 64
    header = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    section = header[header.index('---- occlude:'):header.index('---- compressed input')]
    assert header.index('---- locate:') < header.index('---- occlude:')
    for words in ('DBH_OCCLUDE_OUT', 'DBH_OCCLUDE_ONLY', 'DBH_OCCLUDE_CTRL', 'Nothing is renormalised',
                  'the doubled integers', 'not the variant', 'DBH_ERR_UNSUPPORTED'):
        assert words in section, words
    for name in ('locate_occluded_signals', 'locate_occluded_packed'):
        assert callable(getattr(hip_backend.HipModel, name))
    makefile = open(os.path.join(REPO, 'deepbinner_amd', 'csrc', 'Makefile')).read()
    assert 'occlude_asan:' in makefile and 'dbh_occlude.hip' in makefile
    assert '-fsanitize=address,undefined' in makefile[makefile.index('occlude_asan:'):]
    source = open(os.path.join(REPO, 'deepbinner_amd', 'csrc', 'occlude_model_check.cpp')).read()
    assert 'int main()' in source and 'dbh_occlude_core.h' in source


def test_bad_arguments_are_refused_before_any_device_work():
    lib = hip_backend.load_library()
    # the device entries: 1 stands for a device pointer nobody may touch
    good = [1, 1, 4, 12, 1024, 0, 1, 1, None]
    for at, bad in ((0, None), (1, None), (2, -1), (3, 0), (3, -2), (3, 1 << 21), (4, 1023),
                    (4, 94), (4, 16386), (5, 2), (5, -1), (6, None), (7, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_occlude_plan_dev(*args) == INVALID, (at, bad)
    assert lib.dbh_occlude_plan_dev(*(good[:2] + [0] + good[3:])) == 0           # no read
    good = [1, 1, 1, 4, 12, 1024, 1, 1, None]
    for at, bad in ((0, None), (1, None), (2, None), (3, -1), (4, 0), (5, 97), (5, 20000), (6, 3),
                    (7, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_occlude_windows_dev(*args) == INVALID, (at, bad)
    assert lib.dbh_occlude_windows_dev(*(good[:3] + [0] + good[4:])) == 0
    # the host entries: the same checks, offsets that run backwards, and buffers untouched
    locations = np.array([ref.location_of(2, 10, 300), ref.location_of(0, 0, 0)],
                         dtype=loc_ref.LOCATION)
    offsets = np.array([0, 3000, 9000], np.int64)
    backwards = np.array([0, 3000, 2000], np.int64)
    plans, occlusions = np.full(128, 7, np.uint8), np.full(128, 7, np.uint8)
    good = [locations.ctypes.data, offsets.ctypes.data, 2, 12, 1024, 1, plans.ctypes.data,
            occlusions.ctypes.data]
    for at, bad in ((0, None), (1, None), (1, backwards.ctypes.data), (2, -1), (3, 0), (4, 1023),
                    (5, 5), (6, None), (7, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_occlude_plan_host(*args) == INVALID, (at, bad)
    assert (plans == 7).all() and (occlusions == 7).all()
    assert lib.dbh_occlude_plan_host(*good) == 0
    assert occlusions.view(ref.OCCLUSION)['cls'].tolist() == [2, 0]
    x = np.ones((2, 12, 1024), np.float32)
    out = np.full((3, 2, 12, 1024), 7, np.float32)
    good = [x.ctypes.data, offsets.ctypes.data, plans.ctypes.data, 2, 12, 1024, 1, out.ctypes.data]
    for at, bad in ((0, None), (1, None), (1, backwards.ctypes.data), (2, None), (3, -1), (4, 0),
                    (5, 95), (6, 2), (7, None)):
        args = list(good)
        args[at] = bad
        assert lib.dbh_occlude_windows_host(*args) == INVALID, (at, bad)
    assert (out == 7).all()
    assert lib.dbh_occlude_windows_host(*good) == 0 and not (out == 7).any()
    # the entries that take a model: none given
    size = ctypes.c_size_t(7)
    assert lib.dbh_locate_occluded_workspace_bytes(None, 4, 1024, ctypes.byref(size)) == INVALID
    assert size.value == 7
    assert lib.dbh_locate_occluded_i16(None, 1, offsets.ctypes.data, 2, 0, 1024, 0.5, 1, 1, 1,
                                       1) == INVALID
