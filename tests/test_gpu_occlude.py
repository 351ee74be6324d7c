"""``locate --occlude`` on the device: the plan's and the windows' kernels against their CPU models bit
for bit, the whole route beside ``locate`` (the same bits, whatever the grouping), two exact anchors
on a read whose span is everything its windows cover, the variants' results against the fp64 oracle
on the restatement's blanked windows, the golden reads through the shipped models, and the command.

Against fp64 the probabilities hold the project's tolerance for probabilities, 1e-4; a call is left
out of the comparison where the oracle's own lead over score_diff is below 1e-4, in at most 1 read
in 20 (tests/test_occlude.py asserts that the oracle alone stays below that on these cases)."""
import ctypes
import os

import numpy as np
import pytest

import locate_reference as loc_ref
import occlude_reference as ref
from conftest import GOLD
from general_fixtures import ENDS, STARTS, geometry, golden_signals

pytestmark = pytest.mark.gpu

SIDES = ['start', 'end']
TOLERANCE = 1e-4


def same_records(got, want, names=None):
    assert got.dtype == want.dtype
    for name in names or want.dtype.names:
        assert got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])


@pytest.fixture(scope='module')
def models(hip):
    out = {}

    def get(key, build):
        if key not in out:
            out[key] = hip.HipModel(build(), device=0, general=True)
        return out[key]
    yield get
    for m in out.values():
        m.close()


# ---- 1: the kernels against their CPU models -----------------------------------------------------------
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('input_size,steps,n_reads', ref.GEOMETRIES)
def test_kernels_match_the_host_models(hip, input_size, steps, n_reads, side):
    x, lengths, locations = ref.random_case(input_size, steps, n_reads, side,
                                            seed=input_size + 100 * steps + n_reads)
    plans, occlusions = hip.occlude_plan(locations, lengths, steps, input_size, side)
    d_plans, d_occlusions = hip.occlude_plan(locations, lengths, steps, input_size, side,
                                             device=True)
    same_records(d_plans, plans)
    same_records(d_occlusions, occlusions)
    got = hip.occlude_windows(x, lengths, plans, side, device=True)
    want = hip.occlude_windows(x, lengths, plans, side)
    assert got.shape == want.shape == (3, n_reads, steps, input_size)
    assert got.tobytes() == want.tobytes()
    assert want.tobytes() == ref.blank(x, lengths, plans, side).tobytes()


# ---- 2: the route beside locate, and against the fp64 oracle ---------------------------------------
def check_against_the_plan(occlusions, calls, probs, locations, lengths, steps, input_size, side):
    """What of a record follows from the location alone, and from the unblanked pass."""
    plans, want = ref.plan(locations, lengths, steps, input_size, side)
    same_records(occlusions, want, ('cls', 'ctrl_first', 'ctrl_end', 'reserved'))
    for r in range(len(calls)):
        c = int(calls[r])
        assert occlusions[r]['cls'] == c
        if c == 0:
            assert np.isnan(occlusions[r]['p'])
        else:
            assert occlusions[r]['p'].tobytes() == probs[r, c].tobytes()
        for v, name in enumerate(ref.VARIANTS):
            if (int(plans[r]['valid']) >> v) & 1:
                assert occlusions[r][name + '_call'] >= 0 and np.isfinite(occlusions[r][name + '_p'])
            else:                                             # a stated reason for no result
                assert occlusions[r][name + '_call'] == -1 and np.isnan(occlusions[r][name + '_p'])
                span = locations[r]['end_sample'] - locations[r]['first_sample']
                assert c == 0 or span == 0 or (v == ref.CTRL and occlusions[r]['ctrl_first'] == -1)
    return plans


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('input_size,n_classes,model,steps,score_diff', ref.ROUTE_CASES)
def test_route_beside_locate_and_against_the_oracle(models, monkeypatch, input_size, n_classes, model,
                                                    steps, score_diff, side):
    weights = ref.route_model(input_size, n_classes, model)
    device = models((input_size, n_classes, model), lambda: weights)
    signals = ref.route_reads(input_size, steps)
    lengths = [len(s) for s in signals]
    scan = steps * (input_size // 2)
    monkeypatch.delenv('DEEPBINNER_LOCATE_GROUP', raising=False)
    base = device.locate_signals(signals, side, scan, score_diff)
    probs, calls, locations, occlusions = device.locate_occluded_signals(signals, side, scan,
                                                                         score_diff)
    # locate's own results to the bit, and no grouping of the reads shows in any result
    assert probs.tobytes() == base[0].tobytes() and calls.tobytes() == base[1].tobytes()
    same_records(locations, base[2])
    for group in (1, 7, 256):
        monkeypatch.setenv('DEEPBINNER_LOCATE_GROUP', str(group))
        g = device.locate_occluded_signals(signals, side, scan, score_diff)
        assert g[0].tobytes() == probs.tobytes() and g[1].tobytes() == calls.tobytes()
        same_records(g[2], locations)
        same_records(g[3], occlusions)
    monkeypatch.delenv('DEEPBINNER_LOCATE_GROUP')
    plans = check_against_the_plan(occlusions, calls, probs, locations, lengths, steps, input_size,
                                   side)

    # the variants: the oracle's forward, merge and call in fp64 on the restatement's blanked
    # windows, from the device's own locations on
    want, v_probs, leads = ref.variant_results(weights, signals, locations, side, scan, score_diff)
    worst, compared, skipped = 0.0, 0, set()
    for r in range(len(signals)):
        for v, name in enumerate(ref.VARIANTS):
            if not (int(plans[r]['valid']) >> v) & 1:
                continue
            compared += 1
            err = abs(float(occlusions[r][name + '_p']) - v_probs[v, r, calls[r]])
            worst = max(worst, err)
            assert err <= TOLERANCE, (r, name, err)
            if abs(leads[v, r]) < TOLERANCE:
                skipped.add(r)
            else:
                assert occlusions[r][name + '_call'] == want[r][name + '_call'], (r, name)
    print('occlude route: L {} C {} {} side {}: {} reads, {} results compared, worst p error {:.3e}, '
          '{} reads near a threshold'.format(input_size, n_classes, model, side, len(signals),
                                             compared, worst, len(skipped)))
    assert len(signals) == 32 and len(skipped) * 20 <= len(signals)
    assert compared >= 4


# ---- 3: two exact anchors -------------------------------------------------------------------------------
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('n_classes,model,score_diff', [(2, 'random-2', 0.5), (13, 'random-0', 0.1)])
def test_a_span_of_everything_the_windows_cover(models, n_classes, model, score_diff, side):
    """L = 96 at one step: the one cell of the one window is all of R.  ONLY then blanks nothing and
    gives the unblanked pass back bit for bit, and OUT is a read of zeros - which ``classify_signals``
    slices inside the layer chain, where the route slices with the kernel of its own unit."""
    device = models((96, n_classes, model), lambda: ref.route_model(96, n_classes, model))
    signals = ref.route_reads(96, 1)
    probs, calls, locations, occlusions = device.locate_occluded_signals(signals, side, 48, score_diff)
    zeros = [np.zeros(len(s), dtype=np.int16) for s in signals]
    z_probs, z_calls = device.classify_signals(zeros, side, 48, score_diff)
    anchored = 0
    for r, signal in enumerate(signals):
        c = int(calls[r])
        if c == 0 or len(signal) == 0:
            continue
        lo, hi = ref.scanned(len(signal), 1, 96, side)
        assert (locations[r]['first_sample'], locations[r]['end_sample']) == (lo, hi)
        anchored += 1
        assert occlusions[r]['only_call'] == c
        assert occlusions[r]['only_p'].tobytes() == probs[r, c].tobytes() == \
            occlusions[r]['p'].tobytes()
        assert occlusions[r]['out_p'].tobytes() == z_probs[r, c].tobytes()
        assert occlusions[r]['out_call'] == z_calls[r]
        assert occlusions[r]['ctrl_call'] == -1               # the control would be the span itself
    assert anchored >= 4


# ---- 4: the golden reads through the shipped models ---------------------------------------------------
def test_golden_reads_at_the_shipped_scan_size(models):
    signals = golden_signals()
    lengths = [len(s) for s in signals]
    located = 0
    for name, side in ((STARTS, 'start'), (ENDS, 'end')):
        device = models((1024, 13, name), lambda: geometry(1024, 13, name=name))
        base = device.locate_signals(signals, side, 6144, 0.5)
        probs, calls, locations, occlusions = device.locate_occluded_signals(signals, side, 6144, 0.5)
        assert probs.tobytes() == base[0].tobytes() and calls.tobytes() == base[1].tobytes()
        same_records(locations, base[2])
        check_against_the_plan(occlusions, calls, probs, locations, lengths, 12, 1024, side)
        located += int((occlusions['out_call'] >= 0).sum())
        for r in range(len(signals)):
            print('occlude golden: {} read {} cls {} p {:.4f} span [{}, {}) out {} {:.4f} only {} '
                  '{:.4f} ctrl {} {:.4f}'.format(
                      side, r, occlusions[r]['cls'], occlusions[r]['p'], locations[r]['first_sample'],
                      locations[r]['end_sample'], occlusions[r]['out_call'], occlusions[r]['out_p'],
                      occlusions[r]['only_call'], occlusions[r]['only_p'],
                      occlusions[r]['ctrl_call'], occlusions[r]['ctrl_p']))
    assert located >= 5                         # the golden reads carry barcodes


# ---- 5: refusals and the command ---------------------------------------------------------------------
def test_a_persistent_model_is_refused(hip, hip_models):
    model = hip_models[STARTS]
    assert model.kind == 0
    with pytest.raises(hip.HipBackendError):
        model.locate_occluded_signals([np.zeros(2000, np.int16)], 'start', 1024, 0.5)
    lib, size = hip.load_library(), ctypes.c_size_t(7)
    assert lib.dbh_locate_occluded_workspace_bytes(model.handle, 4, 1024, ctypes.byref(size)) == 5
    assert size.value == 7
    samples, offsets = np.zeros(2000, np.int16), np.array([0, 2000], np.int64)
    occlusions = np.full(64, 7, np.uint8)
    assert lib.dbh_locate_occluded_i16(
        model.handle, samples.ctypes.data, offsets.ctypes.data, 1, 0, 1024, 0.5,
        np.zeros(13, np.float32).ctypes.data, np.zeros(1, np.int32).ctypes.data,
        np.zeros(1, loc_ref.LOCATION).ctypes.data, occlusions.ctypes.data) == 5
    assert (occlusions == 7).all()


def test_workspace_covers_the_group(hip, models):
    device = models((1024, 13, STARTS), lambda: geometry(1024, 13, name=STARTS))
    plain = hip.locate_workspace_bytes(device, 10, 6144)
    more = hip.locate_occluded_workspace_bytes(device, 10, 6144)
    # four sets of 120 windows; three sets of probabilities and of calls and the plans, each region
    # a multiple of 256 bytes
    assert more - plain == 4 * 120 * 1024 * 4 + 1792 + 256 + 768


def command_rows(capsys, argv):
    from deepbinner_amd import deepbinner as cli
    capsys.readouterr()
    cli.main(argv)
    out, err = capsys.readouterr()
    lines = [line.split('\t') for line in out.strip().split('\n')]
    return lines[0], {row[0]: row[1:] for row in lines[1:]}, err


def test_command_with_and_without_the_flag(hip, gold, capsys):
    directory = os.path.join(GOLD, 'fast5', 'single')
    header, plain, plain_err = command_rows(capsys, ['locate', '--native', '--batch_size', '3',
                                                     directory])
    o_header, rows, err = command_rows(capsys, ['locate', '--native', '--batch_size', '3',
                                                '--occlude', directory])
    per_side = ['class', 'first', 'end', 'peak', 'share', 'out_call', 'out_p', 'only_call', 'only_p',
                'ctrl_call', 'ctrl_p']
    assert len(header) == 13 and 'occluded' not in plain_err
    assert o_header == ['read_ID', 'barcode_call', 'samples'] + [
        side + '_' + column for side in ('start', 'end') for column in per_side]
    assert sorted(rows) == sorted(plain) == sorted(gold['read_ids'])
    tested = 0
    for read_id, row in rows.items():
        assert row[:2] == plain[read_id][:2]
        for k in range(2):
            fields = row[2 + 11 * k:13 + 11 * k]
            assert fields[:5] == plain[read_id][2 + 5 * k:7 + 5 * k]
            if fields[0] == '-':
                assert fields[5:] == ['-'] * 6
            else:
                tested += fields[5] != '-'
                assert all(f == '-' or 0 <= float(f) <= 1 for f in fields[6::2])
    assert tested >= 5
    for side in ('start', 'end'):
        assert '{}: occluded: call lost under out '.format(side) in err
    assert set(line for line in plain_err.split('\n') if 'located' in line or 'reads' in line) <= \
        set(err.split('\n'))
