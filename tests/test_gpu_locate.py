"""``locate`` on the device: the evidence the general path's head stores against the fp64 oracle, the
rule's kernel against its CPU model, the whole route against the restatement on the oracle's
evidence, and the command beside ``classify``.

The evidence bound is the project's rule for stage activations (tests/test_gpu_parity.py:
test_stage_activations): 2e-5 of scale, scale = max(1, |e64|.max()).  Measured on the device per
geometry: profiles/locate/parity.json."""
import functools
import os

import numpy as np
import pytest

import locate_reference as ref
from conftest import GOLD
from general_fixtures import ENDS, STARTS, geometry, golden_signals, synthetic_reads

pytestmark = pytest.mark.gpu

BOUND = 2e-5
# (input size, classes, shipped model): one cell; odd len1 / len6 and 256 class threads; two cells;
# odd len3 and len5; the shipped geometry, forced general; 11 cells; 66 cells - past one trip of a
# wave's lanes; 128 cells
EVIDENCE_GEOMETRIES = [(96, 2, STARTS), (98, 13, STARTS), (160, 256, STARTS), (256, 13, STARTS),
                       (1000, 13, STARTS), (1024, 13, STARTS), (1024, 13, ENDS), (1502, 17, STARTS),
                       (8448, 4, STARTS), (16384, 256, STARTS)]
ROUTE_GEOMETRIES = [(1024, 13, STARTS), (1024, 13, ENDS), (256, 13, STARTS), (1000, 5, STARTS),
                    (2048, 13, ENDS)]


@pytest.fixture(scope='module')
def models(hip):
    out = {}

    def get(input_size, n_classes, name=STARTS):
        key = (input_size, n_classes, name)
        if key not in out:
            out[key] = hip.HipModel(geometry(input_size, n_classes, name=name), device=0,
                                    general=True)
        return out[key]
    yield get
    for m in out.values():
        m.close()


def same_fields(got, want, names=ref.LOCATION.names):
    for name in names:
        assert got[name].tobytes() == want[name].tobytes(), (name, got[name], want[name])


# ---- 6: the evidence against the fp64 oracle --------------------------------------------------------
@pytest.mark.parametrize('input_size,n_classes,name', EVIDENCE_GEOMETRIES)
def test_evidence_matches_the_oracle(models, input_size, n_classes, name):
    from oracle import classify_ref
    model = models(input_size, n_classes, name)
    assert model.kind == 1
    windows = classify_ref.make_windows(golden_signals(), input_size, 3 * (input_size // 2),
                                        'start').reshape(-1, input_size)
    rng = np.random.default_rng(input_size + n_classes)
    windows = np.concatenate([windows, rng.standard_normal((6, input_size))]).astype(np.float32)
    if input_size >= 8448:
        windows = np.ascontiguousarray(windows[[0, 8, 16, -1]])
    probs, evidence = model.evidence(windows)
    _, e64, _ = ref.evidence(model.weights, windows)
    cells = ref.cells_of(input_size)
    assert evidence.shape == (len(windows), cells, n_classes) == e64.shape
    assert evidence.dtype == np.float32
    scale = max(1.0, float(np.abs(e64).max()))
    err = float(np.abs(evidence - e64).max())
    print('locate parity: L {} C {} model {} windows {} max error {:.3e} scale {:.4f} '
          'of scale {:.3e}'.format(input_size, n_classes, name, len(windows), err, scale, err / scale))
    assert err <= BOUND * scale
    assert (evidence >= 0).all()
    assert np.array_equal(probs, model.predict(windows))


def test_evidence_across_the_chunk_seam(models, hip):
    model = models(16384, 256)
    rng = np.random.default_rng(7)
    windows = rng.standard_normal((80, 16384)).astype(np.float32)     # (a chunk holds 34)
    probs, evidence = model.evidence(windows)
    first, second = model.evidence(windows[:41]), model.evidence(windows[41:])
    assert np.array_equal(probs, np.concatenate([first[0], second[0]]))
    assert np.array_equal(evidence, np.concatenate([first[1], second[1]]))
    assert np.array_equal(probs, model.predict(windows))
    assert evidence.max() > 0 and np.isfinite(evidence).all()


def test_a_persistent_model_has_no_evidence(hip, hip_models):
    model = hip_models[STARTS]
    assert model.kind == 0
    with pytest.raises(hip.HipBackendError):
        model.evidence(np.zeros((1, 1024), np.float32))
    import ctypes
    lib, n = hip.load_library(), ctypes.c_int64(-7)
    assert lib.dbh_evidence_floats(model.handle, ctypes.byref(n)) == 5 and n.value == -7
    with hip.device_arrays(1024 * 4, 13 * 4, 8 * 13 * 4) as (d_x, d_p, d_e):
        assert lib.dbh_evidence_dev(model.handle, d_x.ptr, 1, d_p.ptr, d_e.ptr, None) == 5
    samples, offsets = np.zeros(2000, np.int16), np.array([0, 2000], np.int64)
    out = np.zeros(1, ref.LOCATION)
    assert lib.dbh_locate_i16(model.handle, samples.ctypes.data, offsets.ctypes.data, 1, 0, 1024, 0.5,
                              np.zeros(13, np.float32).ctypes.data, np.zeros(1, np.int32).ctypes.data,
                              out.ctypes.data) == 5


# ---- 8: the kernel against its CPU model ---------------------------------------------------------------
@pytest.mark.parametrize('side', ['start', 'end'])
@pytest.mark.parametrize('cells,steps,n_classes,n_reads', ref.RANDOM_CASES)
def test_kernel_matches_the_host_model(hip, cells, steps, n_classes, n_reads, side):
    ev, calls, lengths, input_size = ref.random_case(cells, steps, n_classes, n_reads,
                                                     seed=cells + 1000 * steps)
    same_fields(hip.locate_rule_dev(ev, calls, lengths, input_size, side),
                hip.locate_rule(ev, calls, lengths, input_size, side))


def test_kernel_on_the_planted_cases(hip):
    for name, ev, c, n, input_size, side, want in ref.planted_cases():
        got = hip.locate_rule_dev(ev, [c], [n], input_size, side)
        same_fields(got, hip.locate_rule(ev, [c], [n], input_size, side))
        assert (got[0]['window'], got[0]['peak_cell'], got[0]['first_cell'], got[0]['last_cell'],
                got[0]['first_sample'], got[0]['end_sample']) == want, name


# ---- 9: the whole route ----------------------------------------------------------------------------------
def route_reads(input_size):
    scan = 6 * (input_size // 2)
    return golden_signals() + synthetic_reads(input_size, scan, input_size), scan


@functools.lru_cache(maxsize=None)
def route_oracle(input_size, n_classes, name, side):
    """The fp64 oracle of one case, computed once: calls, merged probabilities, evidence."""
    from oracle import classify_ref, network_ref
    weights = geometry(input_size, n_classes, name=name)
    signals, scan = route_reads(input_size)
    calls, probs = classify_ref.call_batch(
        lambda w: network_ref.forward(weights, np.asarray(w, dtype=np.float32), dtype=np.float64),
        signals, input_size, scan, 0.5, side)
    _, e64 = ref.read_evidence(weights, signals, scan, side)
    return calls, probs, e64


@pytest.mark.parametrize('side', ['start', 'end'])
@pytest.mark.parametrize('input_size,n_classes,name', ROUTE_GEOMETRIES)
def test_route_matches_the_restatement_on_the_oracle(models, monkeypatch, input_size, n_classes,
                                                     name, side):
    model = models(input_size, n_classes, name)
    signals, scan = route_reads(input_size)
    lengths = [len(s) for s in signals]
    monkeypatch.delenv('DEEPBINNER_LOCATE_GROUP', raising=False)
    probs, calls, locations = model.locate_signals(signals, side, scan, 0.5)
    # the calls are the general path's own, and no grouping of the reads shows in any result
    c_probs, c_calls = model.classify_signals(signals, side, scan, 0.5)
    assert np.array_equal(probs, c_probs) and np.array_equal(calls, c_calls)
    for group in (1, 7, 256):
        monkeypatch.setenv('DEEPBINNER_LOCATE_GROUP', str(group))
        g_probs, g_calls, g_locations = model.locate_signals(signals, side, scan, 0.5)
        assert np.array_equal(g_probs, probs) and np.array_equal(g_calls, calls)
        same_fields(g_locations, locations)
    monkeypatch.delenv('DEEPBINNER_LOCATE_GROUP')

    o_calls, o_probs, e64 = route_oracle(input_size, n_classes, name, side)
    assert float(np.abs(probs - o_probs).max()) <= 1e-4
    top = np.sort(np.asarray(o_probs), axis=1)[:, ::-1]
    near = (np.abs(top[:, 0] - top[:, 1] - 0.5) <= 1e-4) | (top[:, 0] - top[:, 1] <= 1e-4)
    scale = max(1.0, float(np.abs(e64).max()))
    cells = ref.cells_of(input_size)
    called = compared = skipped = 0
    for r in range(len(signals)):
        want_call = 0 if o_calls[r] == 'none' else int(o_calls[r])
        if not near[r]:
            assert calls[r] == want_call, (r, calls[r], want_call)
        got = locations[r]
        if calls[r] == 0:
            same_fields(got.reshape(1), ref.no_location().reshape(1))
            continue
        called += 1
        c = int(calls[r])
        if c != want_call or min(ref.margins(e64[r], c)) < 1e-4 * scale:
            skipped += 1
            continue
        compared += 1
        want = ref.locate_read(e64[r], c, lengths[r], input_size, side)
        for field in ref.INTEGERS:
            assert got[field] == want[field], (r, field, got[field], want[field])
        row = e64[r, want['window'], :, c]
        part, total = row[want['first_cell']:want['last_cell'] + 1].sum(), row.sum()
        assert abs(float(got['peak']) - row[want['peak_cell']]) <= BOUND * scale
        assert abs(float(got['share']) - part / total) <= (cells + 1) * BOUND * scale / total
        assert 0 <= got['first_sample'] <= got['end_sample'] <= lengths[r]
    print('locate route: L {} C {} {} side {}: {} reads, {} called, {} compared, {} skipped near a '
          'margin'.format(input_size, n_classes, name, side, len(signals), called, compared, skipped))
    assert skipped * 10 <= called
    if input_size == 1024 and (name, side) in ((STARTS, 'start'), (ENDS, 'end')):
        assert compared >= 5                     # the golden reads carry barcodes at this end


# ---- 10: the command ---------------------------------------------------------------------------------------
def command_rows(capsys, argv):
    from deepbinner_amd import deepbinner as cli
    capsys.readouterr()
    cli.main(argv)
    out, err = capsys.readouterr()
    lines = [line.split('\t') for line in out.strip().split('\n')]
    return lines[0], {row[0]: row[1:] for row in lines[1:]}, err


@pytest.mark.parametrize('multi', [False, True])
def test_command_beside_classify_and_the_restatement(hip, gold, models, capsys, multi):
    from oracle import classify_ref
    directory = os.path.join(GOLD, 'fast5', 'multi' if multi else 'single')
    ids = gold['multi_read_ids'] if multi else gold['read_ids']
    signals = dict(zip(ids, gold['multi_signals'] if multi else gold['signals']))
    more = ['--multi_read'] if multi else []
    _, classified, _ = command_rows(capsys, ['classify', '--native'] + more + [directory])
    header, rows, err = command_rows(capsys, ['locate', '--native', '--batch_size', '3'] + more +
                                     [directory])
    assert header == ['read_ID', 'barcode_call', 'samples'] + [
        side + '_' + column for side in ('start', 'end')
        for column in ('class', 'first', 'end', 'peak', 'share')]
    assert sorted(rows) == sorted(signals) == sorted(classified)
    located = {'start': 0, 'end': 0}
    for read_id, row in rows.items():
        signal = signals[read_id]
        assert row[0] == classified[read_id][0] and int(row[1]) == len(signal), read_id
        for k, (side, name) in enumerate((('start', STARTS), ('end', ENDS))):
            model = models(1024, 13, name)
            windows = classify_ref.make_windows([signal], 1024, 6144, side).reshape(-1, 1024)
            _, evidence = model.evidence(windows.astype(np.float32))
            _, calls = model.classify_signals([signal], side, 6144, 0.5)
            want = ref.locate(evidence[None], calls, [len(signal)], 1024, side)[0]
            fields = row[2 + 5 * k:7 + 5 * k]
            if want['cls'] == 0:
                assert fields == ['-'] * 5, (read_id, side)
                continue
            located[side] += 1
            # the integers as the restatement gives them; the floats as printed, to half a unit of
            # the last printed place and the evidence bound
            assert fields[:3] == [str(want['cls']), str(want['first_sample']),
                                  str(want['end_sample'])], (read_id, side)
            assert abs(float(fields[3]) - want['peak']) <= 0.05 + 1e-3
            assert abs(float(fields[4]) - want['share']) <= 0.005 + 1e-3
    assert '{} reads'.format(len(signals)) in err
    for side in ('start', 'end'):
        assert '{}: {} located'.format(side, located[side]) in err
    assert located['start'] + located['end'] > 0
