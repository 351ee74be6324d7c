"""The general forward path on the device: models of other input sizes and class counts than the
shipped ones (tests/general_fixtures.py) against the fp64 oracle, through every entry point."""
import ctypes
import os
import zlib

import numpy as np
import pytest

from general_fixtures import ENDS, STARTS, geometry, golden_signals, save, synthetic_reads

pytestmark = pytest.mark.gpu

GEOMETRIES = [(2048, 13), (1000, 13), (96, 13), (4096, 13), (1024, 2), (1024, 33), (1024, 97),
              (1024, 256)]


@pytest.fixture(scope='module')
def models(hip):
    out = {}

    def get(input_size, n_classes, general=False, name=STARTS):
        key = (input_size, n_classes, general, name)
        if key not in out:
            out[key] = hip.HipModel(geometry(input_size, n_classes, name=name), device=0,
                                    general=general)
        return out[key]
    yield get
    for m in out.values():
        m.close()


def oracle_probs(weights, windows):
    from oracle import network_ref
    return network_ref.forward(weights, np.asarray(windows, dtype=np.float32), dtype=np.float64)


@pytest.mark.parametrize('input_size,n_classes', GEOMETRIES)
def test_predict_matches_the_oracle(models, input_size, n_classes):
    from oracle import classify_ref
    # (a shipped-size model of at most 32 classes would go to the persistent kernel: forced here)
    model = models(input_size, n_classes, general=input_size == 1024 and n_classes <= 32)
    assert model.kind == 1
    windows = classify_ref.make_windows(golden_signals(), input_size, 3 * (input_size // 2),
                                        'start').reshape(-1, input_size)
    rng = np.random.default_rng(input_size + n_classes)
    windows = np.concatenate([windows, rng.standard_normal((6, input_size))]).astype(np.float32)
    got = model.predict(windows)
    want = oracle_probs(model.weights, windows)
    assert got.shape == (len(windows), n_classes)
    assert float(np.abs(got - want).max()) <= 1e-4


def test_forced_general_matches_the_persistent_kernel_and_the_oracle(models, hip):
    from oracle import classify_ref
    general = models(1024, 13, general=True)
    persistent = models(1024, 13)
    assert (general.kind, persistent.kind) == (1, 0)
    windows = classify_ref.make_windows(golden_signals(), 1024, 6144, 'end').reshape(-1, 1024)
    windows = windows.astype(np.float32)
    got = general.predict(windows)
    assert float(np.abs(got - oracle_probs(general.weights, windows)).max()) <= 1e-4
    assert float(np.abs(got - persistent.predict(windows)).max()) <= 1e-4


def near_threshold(probs, score_diff):
    """Reads whose oracle top-2 margin is within 1e-4 of score_diff (or of a tie)."""
    top = np.sort(probs, axis=1)[:, ::-1]
    margin = top[:, 0] - top[:, 1]
    return (np.abs(margin - score_diff) <= 1e-4) | (margin <= 1e-4)


def compare_calls(calls, probs, o_calls, o_probs, score_diff=0.5):
    assert float(np.abs(probs - o_probs).max()) <= 1e-4
    names = ['none' if c == 0 else str(int(c)) for c in calls]
    skip = near_threshold(np.asarray(o_probs), score_diff)
    for i, (a, b) in enumerate(zip(names, o_calls)):
        if not skip[i]:
            assert a == b, (i, a, b)
    print('calls compared: {}, excluded near the threshold: {}'.format(len(names) - skip.sum(),
                                                                        int(skip.sum())))


@pytest.mark.parametrize('input_size,n_classes', [(2048, 13), (1024, 97), (96, 13), (1024, 13)])
@pytest.mark.parametrize('side', ['start', 'end'])
def test_classify_matches_call_batch(models, hip, input_size, n_classes, side):
    from oracle import classify_ref
    model = models(input_size, n_classes, general=True)
    half = input_size // 2
    for k, scan in enumerate((half, 3 * half, 6 * half)):
        signals = golden_signals() + synthetic_reads(input_size, scan, k + input_size)
        probs, calls = model.classify_signals(signals, side, scan, 0.5)
        o_calls, o_probs = classify_ref.call_batch(
            lambda w: oracle_probs(model.weights, w), signals, input_size, scan, 0.5, side)
        compare_calls(calls, probs, o_calls, o_probs)

        # the device entry points give the same bits
        offsets = np.zeros(len(signals) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(s) for s in signals])
        samples = np.concatenate(signals + [np.zeros(1, np.int16)]).astype(np.int16)
        n = len(signals)
        d_s = hip.DeviceBuffer.from_array(samples)
        d_o = hip.DeviceBuffer.from_array(offsets)
        d_p = hip.DeviceBuffer(n * n_classes * 4)
        d_c = hip.DeviceBuffer(n * 4)
        work = model.workspace_bytes(n, scan)
        assert work > 0
        d_w = hip.DeviceBuffer(work)
        model.classify_dev(d_s.ptr, d_o.ptr, n, side, scan, 0.5, d_p.ptr, d_c.ptr, d_w.ptr)
        hip.synchronize()
        assert np.array_equal(d_p.download((n, n_classes), np.float32), probs)
        assert np.array_equal(d_c.download((n,), np.int32), calls)
        for batch in (1, 7, 256):
            d_p2 = hip.DeviceBuffer(n * n_classes * 4)
            d_c2 = hip.DeviceBuffer(n * 4)
            model.classify_batched_dev(d_s.ptr, d_o.ptr, n, batch, side, scan, 0.5, d_p2.ptr,
                                       d_c2.ptr)
            hip.synchronize()
            assert np.array_equal(d_p2.download((n, n_classes), np.float32), probs)
            assert np.array_equal(d_c2.download((n,), np.int32), calls)


def test_results_do_not_depend_on_batch_or_chunk(models):
    """At 16,384 samples a chunk of the layer chain holds a few dozen windows: 80 windows take
    several chunks, one window one; the bits are the same."""
    model = models(16384, 13)
    rng = np.random.default_rng(7)
    windows = rng.standard_normal((80, 16384)).astype(np.float32)
    whole = model.predict(windows)
    for batch in (1, 7, 33):
        parts = np.concatenate([model.predict(windows[i:i + batch])
                                for i in range(0, len(windows), batch)])
        assert np.array_equal(parts, whole)
    assert float(np.abs(whole[:4] - oracle_probs(model.weights, windows[:4])).max()) <= 1e-4


def deflate_reads(signals):
    """One zlib stream per read, as dbh_classify_pair_deflated takes them."""
    from deepbinner_amd import hip_backend as hb
    offsets = np.zeros(len(signals) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in signals])
    comp, records = b'', []
    for i, s in enumerate(signals):
        if len(s) == 0:
            continue
        z = zlib.compress(np.asarray(s, dtype='<i2').tobytes())
        records.append((len(comp), len(z), int(offsets[i]) * 2, len(s) * 2, hb.INFLATE_ZLIB, 0))
        comp += z
    comp = np.frombuffer(comp + bytes(64), dtype=np.uint8)
    return comp, np.array(records, dtype=hb.INFLATE_STREAM), offsets


@pytest.mark.parametrize('pair', ['persistent+general', 'general97'])
def test_pair_calls(models, hip, pair):
    from oracle import classify_ref
    if pair == 'persistent+general':
        start, end = models(1024, 13), models(2048, 13, name=ENDS)
        assert (start.kind, end.kind) == (0, 1)
    else:
        start, end = models(1024, 97), models(1024, 97, name=ENDS)
    scan = 6144
    signals = golden_signals() + synthetic_reads(2048, scan, 3)
    o = {}
    for side, model in (('start', start), ('end', end)):
        o[side] = classify_ref.call_batch(lambda w: oracle_probs(model.weights, w), signals,
                                          model.input_size, scan, 0.5, side)
    offsets = np.zeros(len(signals) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in signals])
    samples = np.concatenate(signals).astype(np.int16)
    calls, (s_calls, e_calls), (s_probs, e_probs) = hip.classify_pair(
        start, end, samples, offsets, scan, 0.5, want_sides=True, want_probs=True)
    compare_calls(s_calls, s_probs, *o['start'])
    compare_calls(e_calls, e_probs, *o['end'])
    skip = near_threshold(o['start'][1], 0.5) | near_threshold(o['end'][1], 0.5)
    want = [classify_ref.combine_calls(a, b, 'require_either') for a, b in zip(o['start'][0], o['end'][0])]
    got = ['none' if c == 0 else str(int(c)) for c in calls]
    assert [g for g, s in zip(got, skip) if not s] == [w for w, s in zip(want, skip) if not s]

    comp, records, offs = deflate_reads(signals)
    d_calls, status = hip.classify_pair_deflated(start, end, comp, records, offs, scan, 0.5)
    assert (status == 0).all()
    assert np.array_equal(d_calls, calls)
    v_calls, status, sides = hip.classify_pair_deflated(start, end, comp, records, offs, scan, 0.5,
                                                        want_sides=True)
    assert np.array_equal(v_calls, calls)
    assert np.array_equal(sides['start_calls'], s_calls) and np.array_equal(sides['end_calls'], e_calls)
    assert np.array_equal(sides['start_probs'], s_probs) and np.array_equal(sides['end_probs'], e_probs)


def test_introspection_is_refused_and_tuning_accepted(models, hip):
    model = models(2048, 13)
    lib = hip.load_library()
    h = model.handle
    x = np.zeros((1, 2048), dtype=np.float32)
    out = np.zeros(1 << 20, dtype=np.float32)
    stamps = np.zeros(1 << 16, dtype=np.int64)
    d = hip.DeviceBuffer(2048 * 4)
    i64, dbl = ctypes.c_int64(), ctypes.c_double()
    UNSUPPORTED = 5
    assert lib.dbh_debug_forward(h, x, 1, 0, out) == UNSUPPORTED
    assert lib.dbh_forward_truncated_dev(h, d.ptr, 1, 0, None) == UNSUPPORTED
    assert lib.dbh_forward_timeline(h, x, 1, stamps) == UNSUPPORTED
    assert lib.dbh_forward_timeline_i16(h, np.zeros(2048, np.int16), 1, stamps) == UNSUPPORTED
    assert lib.dbh_forward_timing_enable(h, 1) == UNSUPPORTED
    assert lib.dbh_forward_timing_enable_span(h, 2, 1) == UNSUPPORTED
    assert lib.dbh_forward_timing_read(h, ctypes.byref(dbl), ctypes.byref(i64),
                                       ctypes.byref(i64)) == UNSUPPORTED
    assert lib.dbh_forward_clock_enable(h, 1) == UNSUPPORTED
    assert lib.dbh_forward_clock_read(h, ctypes.byref(dbl)) == UNSUPPORTED
    assert lib.dbh_forward_phases_enable(h, 1) == UNSUPPORTED
    assert lib.dbh_forward_phases_read(h, (ctypes.c_double * 14)(), ctypes.byref(i64)) == UNSUPPORTED
    model.set_host_group(1000)
    model.reserve_cus(8)
    model.set_read_length_hint(4000, 1 << 20)
    size = ctypes.c_int()
    assert lib.dbh_model_input_size(h, ctypes.byref(size)) == 0 and size.value == 2048


def rows_of(text):
    return sorted(line.split('\t') for line in text.splitlines()[1:])


def same_table(got, want):
    """Equal tables; a 2-decimal probability may sit one step away where the fp32 device and
    the oracle straddle a rounding boundary."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w) and g[:2] == w[:2], (g, w)
        for a, b in zip(g[2:], w[2:]):
            if a != b:
                assert abs(float(a) - float(b)) <= 0.0100001, (g, w)


@pytest.mark.parametrize('geom', [(2048, 13), (1024, 97)])
def test_cli_classify_and_realtime(geom, tmp_path, capsys, monkeypatch):
    """`classify --verbose` and `realtime --stop` on the golden one-read files with both models
    of a geometry: same table and same bins as the oracle-backed runs."""
    import argparse
    import shutil
    from conftest import GOLD, OracleModel
    from deepbinner_amd import classify, deepbinner as cli, realtime
    start = save(geometry(geom[0], geom[1], name=STARTS), tmp_path / 's.dbw')
    end = save(geometry(geom[0], geom[1], name=ENDS), tmp_path / 'e.dbw')
    single = os.path.join(GOLD, 'fast5', 'single')
    argv = ['classify', '--start_model', start, '--end_model', end, '--verbose', single]
    tables, bins = [], []
    for backend in ('hip', 'oracle'):
        with monkeypatch.context() as mp:
            if backend == 'oracle':
                mp.setattr(classify, 'build_model', lambda w: OracleModel(w))
            capsys.readouterr()
            cli.main(argv)
            tables.append(rows_of(capsys.readouterr().out))
            mp.setattr(realtime, 'POLL_SECONDS', 0)
            in_dir, out_dir = tmp_path / (backend + '_in'), tmp_path / (backend + '_out')
            shutil.copytree(single, in_dir)
            realtime.realtime(argparse.Namespace(
                in_dir=str(in_dir), out_dir=str(out_dir), stop=True, start_model=start,
                end_model=end, scan_size=6144.0, score_diff=0.5, batch_size=4,
                require_either=True, require_start=False, require_both=False))
            capsys.readouterr()
            bins.append({d: sorted(os.listdir(out_dir / d)) for d in os.listdir(out_dir)})
    same_table(tables[0], tables[1])
    assert bins[0] == bins[1]
