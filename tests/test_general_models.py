"""Models of any supported geometry (input size 96 .. 16,384, even; 2 .. 256 classes): the C ABI's
refusals, the host checks and the loaders' kept samples - no device needed (the classify run here
goes through the oracle at seam b1)."""
import ctypes
import io
import os

import numpy as np
import pytest

from conftest import GOLD
from deepbinner_amd import classify, hip_backend
from deepbinner_amd.model_format import param_count
from general_fixtures import ENDS, geometry, save

UNSUPPORTED, BAD_WEIGHTS = 5, 4


def test_create_ex_is_exported_and_in_the_symbol_list():
    lib = hip_backend.load_library()
    for name in ('dbh_model_create_ex', 'dbh_model_kind'):
        assert hasattr(lib, name)
        assert name in hip_backend.EXPORTED_SYMBOLS


@pytest.mark.parametrize('input_size,n_classes', [
    (1023, 13), (2047, 97), (94, 13), (95, 13), (16386, 13), (32768, 13), (0, 13), (-1024, 13),
    (1024, 1), (1024, 0), (1024, 257), (2048, 1000)])
def test_create_ex_refuses_geometry_outside_the_limits(input_size, n_classes):
    lib = hip_backend.load_library()
    handle = ctypes.c_void_p()
    n = param_count(max(n_classes, 1))
    blob = np.zeros(n, dtype=np.float32)
    for flags in (0, 1):
        assert lib.dbh_model_create_ex(blob, n, n_classes, input_size, flags,
                                       ctypes.byref(handle)) == UNSUPPORTED
        assert not handle.value


@pytest.mark.parametrize('input_size,n_classes', [(96, 2), (1024, 13), (2048, 97), (16384, 256),
                                                  (1000, 33)])
def test_create_ex_refuses_a_wrong_blob_before_any_device_work(input_size, n_classes):
    lib = hip_backend.load_library()
    handle = ctypes.c_void_p()
    n = param_count(n_classes)
    blob = np.zeros(n + 1, dtype=np.float32)
    for flags in (0, 1):
        for wrong in (n - 1, n + 1, 10):
            assert lib.dbh_model_create_ex(blob, wrong, n_classes, input_size, flags,
                                           ctypes.byref(handle)) == BAD_WEIGHTS


def test_create_keeps_its_old_contract():
    lib = hip_backend.load_library()
    handle = ctypes.c_void_p()
    blob = np.zeros(param_count(97), dtype=np.float32)
    assert lib.dbh_model_create(blob, blob.size, 97, 1024, ctypes.byref(handle)) == UNSUPPORTED
    assert lib.dbh_model_create(blob, param_count(13), 13, 2048, ctypes.byref(handle)) == UNSUPPORTED
    assert lib.dbh_model_kind(None, ctypes.byref(ctypes.c_int())) == 1


@pytest.mark.parametrize('input_size,n_classes,message', [
    (1023, 13, 'the model input size must be even (currently 1023)'),
    (94, 13, 'model input size 94 is not supported'),
    (16386, 13, 'model input size 16386 is not supported'),
    (1024, 257, 'a model with 257 classes is not supported'),
])
def test_load_trained_model_refuses_outside_the_geometry(input_size, n_classes, message,
                                                         oracle_backend, tmp_path):
    path = save(geometry(input_size, n_classes), tmp_path / 'm.dbw')
    with pytest.raises(SystemExit) as e:
        classify.load_trained_model(path, out_dest=io.StringIO())
    assert message in str(e.value)


@pytest.mark.parametrize('input_size,n_classes', [(96, 13), (2048, 13), (4096, 25), (1024, 97),
                                                  (16384, 256), (1000, 2)])
def test_load_trained_model_takes_the_geometry(input_size, n_classes, oracle_backend, tmp_path):
    path = save(geometry(input_size, n_classes), tmp_path / 'm.dbw')
    model, size, classes = classify.load_trained_model(path, out_dest=io.StringIO())
    assert (size, classes) == (input_size, n_classes)


def test_reference_checks_keep_their_messages(oracle_backend, tmp_path):
    path = save(geometry(2048, 13), tmp_path / 'm.dbw')
    with pytest.raises(SystemExit) as e:      # not a whole number of 1024-sample half-windows
        classify.load_and_check_models(path, None, 5632, out_dest=io.StringIO())
    assert 'acceptable values for --scan_size are 2048, 3072, 4096' in str(e.value)
    other = save(geometry(2048, 25), tmp_path / 'n.dbw')
    with pytest.raises(SystemExit) as e:
        classify.load_and_check_models(path, other, 6144, out_dest=io.StringIO())
    assert 'two models have different number of barcode classes' in str(e.value)


def test_scanned_end_samples_for_mixed_sizes():
    assert classify.scanned_end_samples(6144) == 6144 + 512           # today's value
    assert classify.scanned_end_samples(6144, 1024) == 6144 + 512
    assert classify.scanned_end_samples(6144, 1024, 1024) == 6144 + 512
    assert classify.scanned_end_samples(6144, 1024, 2048) == 6144 + 1024
    assert classify.scanned_end_samples(6144, 4096, 2048) == 6144 + 2048
    assert classify.scanned_end_samples(6144, None, 2048) == 6144 + 1024
    assert classify.scanned_end_samples(6144, 96, None) == 6144 + 48
    assert classify.scanned_end_samples(6144.0, None, None) == 6144 + 512

    class M:
        def __init__(self, size):
            self.input_size = size
    assert classify.models_input_size(M(1024), M(2048)) == 2048
    assert classify.models_input_size(None, M(4096)) == 4096
    assert classify.models_input_size(None, None) == 1024


def expected_verbose_rows(weights, side, scan_size):
    """read_ID, call and the 2-decimal probabilities of every golden single-read fast5, from the
    oracle's own restatement of call_batch."""
    from conftest import OracleModel
    from oracle import classify_ref
    reads = np.load(os.path.join(GOLD, 'reads.npz'))
    offsets = reads['offsets']
    signals = [reads['samples'][offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
    model = OracleModel(weights)
    calls, probs = classify_ref.call_batch(model.predict, signals, weights.input_size, scan_size,
                                           0.5, side)
    return sorted('\t'.join([str(rid), call] + ['%.2f' % p for p in row])
                  for rid, call, row in zip(reads['read_ids'], calls, probs))


@pytest.mark.parametrize('reader', ['python', 'native'])
def test_classify_verbose_with_a_2048_sample_model(reader, oracle_backend, tmp_path, capsys,
                                                   monkeypatch):
    """`classify --verbose` of the golden one-read files with a 2048-sample end model: the
    loaders keep scan_size + 1024 samples per end, the table is the oracle's call_batch."""
    from deepbinner_amd import deepbinner as cli
    monkeypatch.setenv('DEEPBINNER_FAST5_READER', reader)
    weights = geometry(2048, 13, name=ENDS)
    path = save(weights, tmp_path / 'ends2048.dbw')
    capsys.readouterr()
    cli.main(['classify', '--end_model', path, '--verbose', '--scan_size', '6144',
              os.path.join(GOLD, 'fast5', 'single')])
    out = capsys.readouterr().out.splitlines()
    assert out[0] == '\t'.join(['read_ID', 'barcode_call', 'none'] + [str(i) for i in range(1, 13)])
    assert sorted(out[1:]) == expected_verbose_rows(weights, 'end', 6144)
