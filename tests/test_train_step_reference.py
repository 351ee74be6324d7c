"""The training step's second half without a device: tests/train_step_reference.py (what the GPU
tests hold dbh_train_noise, dbh_nadam_update and the trainer to) against implementations it shares
no line with, dbh_nadam_schedule (host code of the library) against the formulas, the defaults
against a shipped model file's training_config, ModelWeights.fresh, and the new entries' argument
checks (all made before any device work)."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest
import torch

import train_step_reference as ts
from conftest import GOLD
from deepbinner_amd import hdf5_lite, hip_backend
from deepbinner_amd.model_format import BN_CHANNELS, ModelWeights, conv_shapes, param_count

OK, INVALID, BAD_WEIGHTS, UNSUPPORTED = 0, 1, 4, 5
NOISE_SEED = 20181018          # chosen here, on the reference alone, so that the statistics pass


# ---- Nadam ---------------------------------------------------------------------------------------
def test_nadam_is_torchs_nadam_in_float64():
    """Six steps on 1,000 elements against torch.optim.NAdam (the same algorithm: Dozat's schedule
    with momentum_decay = Keras's schedule_decay) in float64: a sign or a misplaced t + 1 is off by
    far more than 1e-12."""
    rng = np.random.default_rng(7)
    start = rng.standard_normal(1000)
    grads = rng.standard_normal((6, 1000)) * np.exp(rng.standard_normal((6, 1000)))
    o = ts.DEFAULTS
    param = torch.tensor(start, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.NAdam([param], lr=o['lr'], betas=(o['beta_1'], o['beta_2']), eps=o['epsilon'],
                            momentum_decay=o['schedule_decay'])
    p, m, v, schedule = start.copy(), np.zeros(1000), np.zeros(1000), 1.0
    for t0 in range(6):
        param.grad = torch.tensor(grads[t0], dtype=torch.float64)
        # (torch keeps its product of the mu's in the default dtype: fp32 would cost 2e-8)
        before = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            opt.step()
        finally:
            torch.set_default_dtype(before)
        k = ts.nadam_coefficients(t0, schedule)
        p, m, v = ts.nadam_core(p, grads[t0], m, v, k)
        schedule = k['sched_new']
        want = param.detach().numpy()
        assert np.abs(p - want).max() <= 1e-12 * np.abs(want).max(), t0
    assert np.abs(p - start).max() > 5 * o['lr']         # it moved: six steps of about lr each


def test_update_rounds_once_and_leaves_the_moving_slots_to_the_average():
    rng = np.random.default_rng(3)
    n = param_count(5)
    p, g, v = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    m = rng.standard_normal(n).astype(np.float32)
    v = np.abs(v)
    stats = rng.standard_normal(960).astype(np.float32)
    k = ts.nadam_coefficients(3, 0.7, bn_momentum=0.9)
    p2, m2, v2 = ts.nadam_update(p, g, m, v, stats, 5, k)
    blob, stat = ts.moving_index(5)
    assert blob.size == 960 and np.array_equal(m2[blob], m[blob]) and np.array_equal(v2[blob], v[blob])
    want = p[blob].astype(np.float64) * 0.9 + stats[stat].astype(np.float64) * 0.1
    assert np.abs(p2[blob] - want).max() < 1e-6
    rest = np.setdiff1d(np.arange(n), blob)
    core = ts.nadam_core(*(a[rest].astype(np.float64) for a in (p, g, m, v)), k)
    for got, exact in zip((p2, m2, v2), core):
        assert np.array_equal(got[rest], exact.astype(np.float32))
    # BN5's 192 channels: its moving mean is the fifth layer's third quarter
    at = param_count(5) - 4 * sum(BN_CHANNELS) + 4 * sum(BN_CHANNELS[:4]) + 2 * 192
    assert blob[2 * sum(BN_CHANNELS[:4])] == at


# ---- dbh_nadam_schedule --------------------------------------------------------------------------
COEFFICIENTS = ('lr', 'beta_1', 'beta_2', 'epsilon', 'mu_t', 'mu_t1', 'sched_new', 'sched_next',
                'beta_2_t', 'bn_momentum')


@pytest.mark.parametrize('t0', [0, 1, 2, 999, 100000])
def test_schedule_entry_is_the_formulas(t0):
    for schedule, options in ((1.0, {}), (0.37, {'lr': 0.01, 'beta_1': 0.8, 'beta_2': 0.99,
                                                   'schedule_decay': 0.01, 'bn_momentum': 0.5})):
        got = hip_backend.nadam_schedule(t0, schedule, **options)
        want = ts.nadam_coefficients(t0, schedule, **options)
        assert sorted(got) == sorted(COEFFICIENTS)
        for name in COEFFICIENTS:
            assert abs(got[name] - want[name]) <= 1e-14 * abs(want[name]), (name, got[name], want[name])
    o = ts.DEFAULTS
    t = t0 + 1
    assert abs(got['beta_2_t'] - 0.99 ** t) <= 1e-14 * 0.99 ** t
    want_mu = o['beta_1'] * (1 - 0.5 * 0.96 ** (t * o['schedule_decay']))
    assert abs(hip_backend.nadam_schedule(t0)['mu_t'] - want_mu) <= 1e-14


def test_m_schedule_through_a_thousand_steps():
    """A product of a thousand factors near 0.5: it leaves the normal doubles at about step 970
    (Keras's own fp32 m_schedule is 0 long before).  Down there a product rounds to a multiple of
    2^-1074, so each step may add one of those to the 1e-12."""
    got = want = 1.0
    tiny = 0.0
    for t0 in range(1000):
        got = hip_backend.nadam_schedule(t0, got)['sched_new']
        want = ts.nadam_coefficients(t0, want)['sched_new']
        if want < 2.0 ** -1022:
            tiny += 2.0 ** -1074
        assert abs(got - want) <= 1e-12 * want + tiny, t0
    assert 0 < want < 1e-300 and tiny < 50 * 2.0 ** -1074


def test_step_seed():
    assert hip_backend.step_seed(5, 0) == 5 == ts.step_seed(5, 0)
    assert hip_backend.step_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert hip_backend.step_seed(2 ** 64 - 1, 3) == (3 * 0x9E3779B97F4A7C15 - 1) % 2 ** 64
    assert ts.step_seed(2 ** 64 - 1, 3) == hip_backend.step_seed(2 ** 64 - 1, 3)


# ---- defaults ------------------------------------------------------------------------------------
def test_defaults_are_the_shipped_models_training_config(tmp_path):
    path = str(tmp_path / 'model.h5')
    with gzip.open(os.path.join(GOLD, 'keras', 'EXP-NBD103_read_starts.gz'), 'rb') as f:
        with open(path, 'wb') as out:
            out.write(f.read())
    with hdf5_lite.File(path) as hf:
        assert hf.attrs['keras_version'] == b'2.1.4'
        config = json.loads(hf.attrs['training_config'].decode('utf-8'))
    assert config['optimizer_config']['class_name'] == 'Nadam'
    recorded = config['optimizer_config']['config']
    assert sorted(recorded) == ['beta_1', 'beta_2', 'epsilon', 'lr', 'schedule_decay']
    library = hip_backend.library_trainer_defaults()
    passed = hip_backend.trainer_options()
    for name, value in recorded.items():
        assert hip_backend.TRAINER_DEFAULTS[name] == value, name
        assert getattr(passed, name) == value and library[name] == value, name
        assert ts.DEFAULTS[name] == value, name
    assert recorded['lr'] == float(np.float32(0.002)) and recorded['beta_1'] == float(np.float32(0.9))
    # what the file does not record: Keras's BatchNormalization momentum, the network's own layers
    for name, value in (('bn_momentum', 0.99), ('seed', 0)):
        assert library[name] == value == hip_backend.TRAINER_DEFAULTS[name]
    for name, value in (('dropout_rate', 0.15), ('noise_std', 0.02)):
        assert library[name] == float(np.float32(value)) == getattr(passed, name)
    with pytest.raises(TypeError):
        hip_backend.trainer_options(learning_rate=1.0)


def test_header_cites_the_reference():
    from conftest import REPO
    text = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    for cite in ('train_network.py:53-55', 'network_architecture.py:25', 'Keras 2.1.4',
                 'n / (n - 1 - eps)', '0x9E3779B97F4A7C15'):
        assert cite in text, cite


# ---- noise ---------------------------------------------------------------------------------------
def test_noise_reference_is_standard_normal():
    windows, size = 256, 1024
    n = windows * size
    assert n == 2 ** 18
    z = ts.noise_z(windows, size, NOISE_SEED)
    x = np.zeros((windows, size), dtype=np.float32)
    noise = ts.add_noise(x, 0.02, NOISE_SEED).astype(np.float64)
    std = float(np.float32(0.02))
    assert np.abs(noise - std * z).max() <= 2.0 ** -24 * std * ts.Z_MAX      # one rounding to fp32
    assert abs(noise.mean()) <= 5 * 0.02 / np.sqrt(n)
    assert abs(noise.var() - 0.02 ** 2) <= 5 * 0.02 ** 2 * np.sqrt(2 / n)
    unit = (z - z.mean()) / z.std()
    assert abs((unit[:, 1:] * unit[:, :-1]).mean()) <= 5 / np.sqrt(n)       # along position
    assert abs((unit[1:, :] * unit[:-1, :]).mean()) <= 5 / np.sqrt(n)       # along window
    assert np.abs(z).max() <= ts.Z_MAX
    again = ts.add_noise(x, 0.02, NOISE_SEED)
    assert np.array_equal(again.view(np.uint32), noise.astype(np.float32).view(np.uint32))
    other = ts.add_noise(x, 0.02, ts.step_seed(NOISE_SEED, 1))
    assert (other != again).mean() > 0.99
    assert ts.step_seed(NOISE_SEED, 1) != ts.step_seed(NOISE_SEED, 0)
    # a seed's upper half takes part
    assert (ts.noise_z(4, 64, NOISE_SEED) != ts.noise_z(4, 64, NOISE_SEED + (1 << 32))).mean() > 0.99


def test_noise_of_nothing_is_the_input():
    x = np.array([[0.0, -0.0, 1.5, -2.0]], dtype=np.float32)
    assert np.array_equal(ts.add_noise(x, 0.0, 1).view(np.uint32), x.view(np.uint32))


# ---- fresh weights -------------------------------------------------------------------------------
def test_fresh_weights():
    w = ModelWeights.fresh(13, 1024, seed=4)
    assert (w.n_classes, w.input_size) == (13, 1024)
    for (kernel, bias), (name, k, cin, cout, _, _) in zip(w.convs, conv_shapes(13)):
        limit = np.sqrt(6.0 / (k * cin + k * cout))
        assert kernel.dtype == np.float32 and np.abs(kernel).max() <= limit, name
        assert np.abs(kernel).max() > 0.9 * limit or kernel.size < 200, name
        assert not bias.any() and bias.dtype == np.float32, name
        if (k, cin, cout) == (3, 48, 48):
            assert abs(kernel.astype(np.float64).var() / (limit ** 2 / 3) - 1) < 0.1, name
            assert abs(kernel.mean()) < 4 * limit / np.sqrt(3 * kernel.size), name
    for (gamma, beta, mean, var), c in zip(w.bns, BN_CHANNELS):
        assert all(a.shape == (c,) and a.dtype == np.float32 for a in (gamma, beta, mean, var))
        assert (gamma == 1).all() and (beta == 0).all() and (mean == 0).all() and (var == 1).all()
    flat = w.flat()
    assert flat.size == param_count(13) == 107197
    back = ModelWeights.from_flat(flat, 13, 1024)
    assert np.array_equal(back.flat().view(np.uint32), flat.view(np.uint32))
    assert np.array_equal(ModelWeights.fresh(13, 1024, seed=4).flat(), flat)
    assert (ModelWeights.fresh(13, 1024, seed=5).convs[1][0] != w.convs[1][0]).mean() > 0.99
    # no two layers share their draws
    assert not np.array_equal(w.convs[1][0], w.convs[2][0])
    small = ModelWeights.fresh(3, 96, seed=0)
    assert small.flat().size == param_count(3) and small.input_size == 96


# ---- arguments, checked before any device work ---------------------------------------------------
def _options(**kw):
    return ctypes.byref(hip_backend.trainer_options(**kw))


def test_trainer_create_arguments():
    lib = hip_backend.load_library()
    handle = ctypes.c_void_p()
    out = ctypes.byref(handle)
    n = param_count(13)
    blob = np.zeros(n, dtype=np.float32)
    ptr = blob.ctypes.data

    def create(n_floats=n, classes=13, size=1024, windows=20, options=None, weights=ptr, to=out):
        return lib.dbh_trainer_create(weights, n_floats, classes, size, windows, options, to)

    assert create(size=95) == UNSUPPORTED and create(size=1023) == UNSUPPORTED
    assert create(size=16386) == UNSUPPORTED
    assert create(classes=1) == UNSUPPORTED and create(classes=257) == UNSUPPORTED
    assert create(windows=1025) == UNSUPPORTED               # over dbh_gradients_max_windows
    assert create(size=16384, windows=65) == UNSUPPORTED
    assert create(n_floats=n - 1) == BAD_WEIGHTS
    assert create(classes=12) == BAD_WEIGHTS
    assert create(windows=0) == INVALID and create(windows=-3) == INVALID
    assert create(weights=None) == INVALID and create(to=None) == INVALID
    for bad in ({'dropout_rate': 1.0}, {'dropout_rate': -0.1}, {'dropout_rate': float('nan')},
                {'noise_std': -0.01}, {'noise_std': float('nan')}, {'bn_momentum': 1.5},
                {'bn_momentum': -0.5}, {'bn_momentum': float('nan')}):
        assert create(options=_options(**bad)) == INVALID, bad
    assert handle.value is None                              # nothing written
    assert lib.dbh_trainer_destroy(None) == OK


def test_trainer_entries_refuse_null():
    lib = hip_backend.load_library()
    x = np.zeros(96, dtype=np.float32)
    labels = np.zeros(1, dtype=np.int32)
    loss, count = ctypes.c_double(7.0), ctypes.c_int64(7)
    assert lib.dbh_trainer_step(None, x.ctypes.data, labels.ctypes.data, 1, ctypes.byref(loss),
                                ctypes.byref(count)) == INVALID
    assert lib.dbh_trainer_step_dev(None, None, None, 1, None, None, None) == INVALID
    assert lib.dbh_trainer_iterations(None, ctypes.byref(count)) == INVALID
    assert lib.dbh_trainer_set_state(None, None, None, 0, 0, 1.0) == INVALID
    assert (loss.value, count.value) == (7.0, 7)
    assert lib.dbh_trainer_default_options(None) == INVALID
    k = hip_backend.NadamCoefficients()
    assert lib.dbh_nadam_schedule(-1, 1.0, None, ctypes.byref(k)) == INVALID
    assert lib.dbh_nadam_schedule(0, 1.0, None, None) == INVALID
    assert lib.dbh_nadam_schedule(0, 1.0, None, ctypes.byref(k)) == OK      # null: the defaults
    assert k.mu_t == ts.nadam_coefficients(0)['mu_t'] and k.bn_momentum == 0.99


def test_noise_and_update_arguments():
    lib = hip_backend.load_library()
    x = np.ones((2, 96), dtype=np.float32)
    out = np.full_like(x, 5.0)
    assert lib.dbh_train_noise(x, 0, 96, 0.02, 1, out) == INVALID
    assert lib.dbh_train_noise(x, 2, 0, 0.02, 1, out) == INVALID
    assert lib.dbh_train_noise(x, 2, 96, -1.0, 1, out) == INVALID
    assert lib.dbh_train_noise(x, 2, 96, float('nan'), 1, out) == INVALID
    assert lib.dbh_train_noise(x, 2, 16385, 0.02, 1, out) == UNSUPPORTED
    assert lib.dbh_train_noise(x, 2 ** 20 // 96 + 1, 96, 0.02, 1, out) == UNSUPPORTED
    assert lib.dbh_train_noise_dev(None, 2, 96, 0.02, 1, None, None) == INVALID
    assert (out == 5.0).all()

    n = param_count(13)
    blobs = [np.ones(n, dtype=np.float32) for _ in range(4)]
    stats = np.ones(960, dtype=np.float32)
    ptrs = [a.ctypes.data for a in blobs] + [stats.ctypes.data]
    k = hip_backend.NadamCoefficients(**ts.nadam_coefficients(0))
    assert lib.dbh_nadam_update(*ptrs, n, 1, ctypes.byref(k)) == UNSUPPORTED
    assert lib.dbh_nadam_update(*ptrs, n, 257, ctypes.byref(k)) == UNSUPPORTED
    assert lib.dbh_nadam_update(*ptrs, n + 1, 13, ctypes.byref(k)) == BAD_WEIGHTS
    assert lib.dbh_nadam_update(*ptrs, n, 14, ctypes.byref(k)) == BAD_WEIGHTS
    assert lib.dbh_nadam_update(*ptrs, n, 13, None) == INVALID
    assert lib.dbh_nadam_update(None, *ptrs[1:], n, 13, ctypes.byref(k)) == INVALID
    assert lib.dbh_nadam_update_dev(*ptrs[:4], None, n, 13, ctypes.byref(k), None) == INVALID
    k.bn_momentum = 1.25
    assert lib.dbh_nadam_update(*ptrs, n, 13, ctypes.byref(k)) == INVALID
    assert all((a == 1).all() for a in blobs)
