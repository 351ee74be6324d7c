"""Pins tests/train_reference.py, the fp64 restatement that the device's gradients are held to
(tests/test_gpu_gradients.py), and the training section of the C ABI as far as it goes without a
device.  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_reference as tr
import weight_families as wf
from conftest import REPO
from deepbinner_amd import hip_backend
from deepbinner_amd.model_format import BN_CHANNELS, ModelWeights, conv_shapes, param_count
from oracle import network_ref


def windows(seed, n, size):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, size)).astype(np.float32)


# ---- a. the same graph as the inference oracle -----------------------------------------------
@pytest.mark.parametrize('size,n,classes', [(96, 3, 2), (130, 5, 13), (1024, 4, 13)])
def test_forward_is_the_inference_graph_on_batch_statistics(size, n, classes):
    """Dropout 0 and the batch's own statistics as moving statistics: oracle/network_ref.forward
    computes the same probabilities to fp64 rounding."""
    weights = wf.random_model(size, classes, input_size=size)
    x = windows(size, n, size)
    got = tr.loss_and_gradients(weights, x, np.zeros(n, dtype=int), rate=0.0, backward=False)
    bns, at = [], 0
    for (gamma, beta, _, _), c in zip(weights.bns, BN_CHANNELS):
        bns.append((gamma, beta, got.stats[at:at + c], got.stats[at + c:at + 2 * c]))
        at += 2 * c
    frozen = ModelWeights(classes, weights.convs, bns, input_size=size)
    want = network_ref.forward(frozen, x, dtype=np.float64)
    assert np.abs(got.probs - want).max() <= 1e-12 * np.abs(want).max()


# ---- b. central differences ----------------------------------------------------------------------
PER_TENSOR = 5
DIFF_CASES = [(96, 4, 5, 1), (130, 3, 5, 4)]      # input size, windows, classes, seed


def _coordinates(name, shape, weights_flat, sl, rng):
    """The coordinates a tensor must include (as offsets into it), then random ones."""
    must = []
    if name.endswith('/kernel') and len(shape) == 3 and shape[0] == 3:
        k, cin, cout = shape
        for tap in (0, k - 1):                    # both edge taps of a SAME kernel
            must.append((tap * cin + int(rng.integers(cin))) * cout + int(rng.integers(cout)))
    if name.endswith('/gamma') or name.endswith('/beta'):
        gamma_name_slice = sl if name.endswith('/gamma') else slice(sl.start - shape[0], sl.start)
        gamma = weights_flat[gamma_name_slice]
        must.append(int(np.flatnonzero(gamma < 0)[0]))
        must.append(int(np.flatnonzero(gamma == 0)[0]))
    return must


@pytest.mark.parametrize('size,n,classes,seed', DIFF_CASES)
def test_gradients_against_central_differences(size, n, classes, seed):
    """h = 1e-5 max(1, |w|); |analytic - numeric| <= 1e-6 max|gradient of the tensor| (truncation
    ~h^2 = 1e-10, rounding ~1e-16 / h = 1e-11, a wrong formula ~1).  A coordinate whose step flips
    a ReLU or a pool choice anywhere is replaced; at most one in ten may be."""
    weights = wf.random_model(seed, classes, input_size=size)
    x = windows(seed, n, size)
    rng = np.random.default_rng(seed)
    labels = rng.integers(classes, size=n)
    labels[0], labels[-1] = 0, classes - 1
    base = tr.loss_and_gradients(weights, x, labels, rate=0.15, seed=seed)
    flat = weights.flat().astype(np.float64)
    slices, moving = tr.tensor_slices(classes)
    for m in moving:
        assert not base.grads[m].any()

    def evaluate(vector):
        # (ModelWeights.from_flat rounds to fp32; the step must survive, so the arrays stay fp64)
        w = _as_float64(vector, classes, size)
        return tr.loss_and_gradients(w, x, labels, rate=0.15, seed=seed, backward=False)

    def same_pattern(r):
        return all(np.array_equal(a, b) for a, b in zip(r.patterns, base.patterns))

    assert abs(evaluate(flat).loss - base.loss) <= 1e-14 * max(1.0, abs(base.loss))
    shapes = {}
    for name, k, cin, cout, _, _ in conv_shapes(classes):
        shapes[name + '/kernel'] = (k, cin, cout)
        shapes[name + '/bias'] = (cout,)
    for i, c in enumerate(BN_CHANNELS, start=1):
        shapes['bn_%d/gamma' % i] = shapes['bn_%d/beta' % i] = (c,)

    checked = replaced = 0
    worst = 0.0
    for name, sl in slices.items():
        size_t = sl.stop - sl.start
        scale = np.abs(base.grads[sl]).max()
        assert scale > 0, name
        todo = _coordinates(name, shapes[name], flat, sl, rng)
        required = len(todo)
        done = 0
        tried = set()
        target = min(max(PER_TENSOR, required), size_t)
        while done < target:
            assert len(tried) < size_t or todo, 'no unflipped coordinate left in ' + name
            if todo:
                at, is_required = todo.pop(0), True
            else:
                at, is_required = int(rng.integers(size_t)), False
            if at in tried:
                continue
            tried.add(at)
            j = sl.start + at
            h = 1e-5 * max(1.0, abs(flat[j]))
            up, down = flat.copy(), flat.copy()
            up[j] += h
            down[j] -= h
            r_up, r_down = evaluate(up), evaluate(down)
            if not (same_pattern(r_up) and same_pattern(r_down)):
                replaced += 1
                if is_required:
                    # another coordinate of the same kind: the same tap / the same sign of gamma
                    todo.insert(0, _replacement(name, shapes[name], at, flat, sl, rng, tried))
                continue
            numeric = (r_up.loss - r_down.loss) / (2 * h)
            err = abs(base.grads[j] - numeric)
            worst = max(worst, err / scale)
            assert err <= 1e-6 * scale, (name, at, base.grads[j], numeric, scale)
            done += 1
            checked += 1
    print('checked {} coordinates, replaced {}, worst error {:.2e} of max|gradient| (bound 1e-6)'
          .format(checked, replaced, worst))
    assert checked >= 54 * min(PER_TENSOR, classes)
    assert replaced * 10 <= checked + replaced, (replaced, checked)


def _replacement(name, shape, at, flat, sl, rng, tried):
    if name.endswith('/kernel'):
        k, cin, cout = shape
        tap = at // (cin * cout)
        for _ in range(1000):
            new = (tap * cin + int(rng.integers(cin))) * cout + int(rng.integers(cout))
            if new not in tried:
                return new
    gamma_slice = sl if name.endswith('/gamma') else slice(sl.start - shape[0], sl.start)
    gamma = flat[gamma_slice]
    same = np.flatnonzero((gamma < 0) if gamma[at] < 0 else (gamma == 0))
    for new in same:
        if int(new) not in tried:
            return int(new)
    raise AssertionError('no coordinate of the required kind is left in ' + name)


def _as_float64(vector, classes, size):
    pos = 0
    convs, bns = [], []
    for _, k, cin, cout, _, _ in conv_shapes(classes):
        kernel = vector[pos:pos + k * cin * cout].reshape(k, cin, cout)
        pos += k * cin * cout
        convs.append((kernel, vector[pos:pos + cout]))
        pos += cout
    for c in BN_CHANNELS:
        bns.append(tuple(vector[pos + i * c:pos + (i + 1) * c] for i in range(4)))
        pos += 4 * c
    return ModelWeights(classes, convs, bns, input_size=size)


# ---- c. dropout --------------------------------------------------------------------------------
def test_dropout_share_layers_and_rate_zero():
    wider = tr.dropout_keep(7, 1, 41, 512, 48, 0.15)           # 1,007,616 elements
    assert wider.size >= 10 ** 6
    # four binomial standard deviations: 4 sqrt(0.15 * 0.85 / 1e6) = 1.4e-3
    assert abs(wider.mean() - 0.85) <= 1.4e-3, wider.mean()
    keep = tr.dropout_keep(7, 1, 40, 512, 48, 0.15)
    assert np.array_equal(keep, wider[:40])                    # a window's mask is its own
    assert np.array_equal(tr.dropout_keep(7, 1, 40, 100, 16, 0.15), keep[:, :100, :16])
    other = tr.dropout_keep(7, 2, 40, 512, 48, 0.15)
    assert 0.2 < (other != keep).mean() < 0.3                  # 2 * 0.15 * 0.85 = 0.255
    assert (tr.dropout_keep(8, 1, 40, 512, 48, 0.15) != keep).any()
    assert (tr.dropout_keep(7 + 2 ** 32, 1, 40, 512, 48, 0.15) != keep).any()
    assert tr.dropout_keep(7, 1, 40, 512, 48, 0.0).all()
    assert tr.dropout_scale(0.0) == 1.0
    for layer in range(1, 8):
        assert tr.dropout_keep(123, layer, 3, 17, 192, 0.0).all()


# ---- d. the ABI without a device -------------------------------------------------------------
NEW_SYMBOLS = ['dbh_gradients', 'dbh_gradients_dev', 'dbh_gradients_workspace_bytes',
               'dbh_gradients_max_windows', 'dbh_forward_phases_count']


def test_header_declares_and_library_exports_the_training_section():
    text = open(os.path.join(REPO, 'include', 'deepbinner_hip.h')).read()
    lib = hip_backend.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert hasattr(lib, name), name
        assert name in hip_backend.EXPORTED_SYMBOLS
    for cite in ('network_architecture.py:18-95', 'train_network.py:53-55', 'deepbinner.py:265'):
        assert cite in text
    assert hasattr(hip_backend, 'loss_and_gradients')


def test_phase_buffer_is_sized_by_the_library():
    lib = hip_backend.load_library()
    count = ctypes.c_int(0)
    assert lib.dbh_forward_phases_count(ctypes.byref(count)) == 0
    assert count.value == 14
    assert lib.dbh_forward_phases_count(None) == 1


def test_gradient_argument_errors_without_device():
    lib = hip_backend.load_library()
    OK, INVALID, BAD_WEIGHTS, UNSUPPORTED = 0, 1, 4, 5
    size = ctypes.c_size_t(0)
    assert lib.dbh_gradients_workspace_bytes(13, 1024, 256, ctypes.byref(size)) == OK
    at_256 = size.value
    assert lib.dbh_gradients_workspace_bytes(13, 16384, 20, ctypes.byref(size)) == OK
    assert 0 < at_256 < 2 ** 32 and 0 < size.value < 2 ** 32
    for classes, length, n, want in [(13, 1023, 4, UNSUPPORTED), (13, 94, 4, UNSUPPORTED),
                                     (1, 1024, 4, UNSUPPORTED), (257, 1024, 4, UNSUPPORTED),
                                     (13, 1024, 0, INVALID), (13, 1024, 1025, UNSUPPORTED),
                                     (13, 16384, 65, UNSUPPORTED)]:
        assert lib.dbh_gradients_workspace_bytes(classes, length, n, ctypes.byref(size)) == want
    limit = ctypes.c_int64(0)
    assert lib.dbh_gradients_max_windows(1024, ctypes.byref(limit)) == OK and limit.value == 1024
    assert lib.dbh_gradients_max_windows(16384, ctypes.byref(limit)) == OK and limit.value == 64

    n, length, classes = 4, 1024, 13
    count = param_count(classes)
    w = np.zeros(count, dtype=np.float32)
    x = np.zeros((n, length), dtype=np.float32)
    labels = np.zeros(n, dtype=np.int32)
    grads = np.full(count, 7.0, dtype=np.float32)
    stats = np.full(960, 7.0, dtype=np.float32)
    loss, correct = ctypes.c_double(7.0), ctypes.c_int64(7)

    def call(n_floats=count, classes=classes, length=length, labels=labels, n=n, rate=0.15):
        return lib.dbh_gradients(w, n_floats, classes, length, x, labels, n, rate, 0,
                                 ctypes.byref(loss), ctypes.byref(correct), grads, stats)

    assert call(length=1001) == UNSUPPORTED
    assert call(length=32768) == UNSUPPORTED
    assert call(classes=300) == UNSUPPORTED
    assert call(n_floats=count - 1) == BAD_WEIGHTS
    assert call(classes=14) == BAD_WEIGHTS
    assert call(n=0) == INVALID
    assert call(n=-3) == INVALID
    assert call(rate=1.0) == INVALID
    assert call(rate=-0.01) == INVALID
    assert call(rate=float('nan')) == INVALID
    assert call(n=2000) == UNSUPPORTED
    assert call(labels=np.array([0, 1, 13, 2], dtype=np.int32)) == INVALID
    assert call(labels=np.array([0, -1, 12, 2], dtype=np.int32)) == INVALID
    # nothing was written
    assert (grads == 7.0).all() and (stats == 7.0).all()
    assert loss.value == 7.0 and correct.value == 7
    # the device entry refuses the same before it touches a pointer
    assert lib.dbh_gradients_dev(None, count - 1, classes, length, None, None, n, 0.15, 0, None,
                                 None, None, None, None, None) == BAD_WEIGHTS
    assert lib.dbh_gradients_dev(None, count, classes, length, None, None, n, 0.15, 0, None,
                                 None, None, None, None, None) == INVALID


# ---- e. the model of the device's arithmetic and the inputs it is used on ------------------------
def model_bounds(r64, rm, slices):
    """name -> max(4 e_model, 1e-6): what tests/test_gpu_gradients.py allows the device."""
    return {name: max(4 * tr.model_error(r64, rm, sl), 1e-6) for name, sl in slices.items()}


@pytest.mark.parametrize('case', tr.GUARDED, ids=tr.case_id)
def test_model_rounds_and_turns_no_decision(case):
    """On every direct case of the device tests: no ReLU pre-activation and no pool pair of the fp64
    run lies within 8 x (what the model's rounding moved it by, floored at 1/16 of its layer's
    largest move), the model's patterns - in every order of its short sums - are the fp64 run's,
    its loss is the fp64 loss to 1e-6, and its gradients are not the fp64 bits - it does round."""
    r64, r32, rm = tr.guarded_references(case)
    print('{}: {} decisions, {} close; loss off by {:.2e}'.format(
        tr.case_id(case), rm.n_decisions, rm.close, abs(rm.loss - r64.loss) / abs(r64.loss)))
    assert rm.close == 0
    assert rm.same
    assert rm.n_correct == r64.n_correct
    assert abs(rm.loss - r64.loss) <= 1e-6 * abs(r64.loss)
    assert rm.grads.tobytes() != r64.grads.tobytes()
    assert rm.grads.astype(np.float32).astype(np.float64).tobytes() == rm.grads.tobytes()
    slices, moving = tr.tensor_slices(case[2])
    # every order of the short sums is another draw (but for one window at 96, where nothing in
    # front of the head has a gradient)
    piped = r64.grads[slices['conv1d_2/kernel']].any()
    assert piped or case[:2] == (96, 1)
    assert len({g.tobytes() for _, g, _ in rm.draws}) == (tr.ORDERS if piped else 1)
    for m in moving:
        assert not rm.grads[m].any()


def test_model_is_tighter_than_the_fp32_reference():
    """What the yardstick is for: on the default batch shape the fp32 run's error is a few turned
    decisions, not rounding, and the model's is far below it."""
    case = (1024, 4, 13, 0.0, tr.SEED, 1)
    assert case in tr.GUARDED
    r64, r32, rm = tr.guarded_references(case)
    slices, _ = tr.tensor_slices(13)
    e32, em = [], []
    for sl in slices.values():
        scale = np.abs(r64.grads[sl]).max()
        e32.append(np.abs(r32.grads[sl] - r64.grads[sl]).max() / scale)
        em.append(tr.model_error(r64, rm, sl))
    print('e_model {:.2e} .. {:.2e}, e32 {:.2e} .. {:.2e}'.format(min(em), max(em), min(e32), max(e32)))
    assert max(em) < 1e-4                       # (a turned decision moves a tensor by 1e-3 and more)
    assert np.median(em) < np.median(e32)


def test_a_repeated_batch_has_the_batch_s_gradients():
    """Dropout 0: a batch given R times with its labels has the same mean loss, statistics and
    gradients; only n_correct grows R-fold.  (What lets the device tests reach training-sized
    batches with a small case's reference.)  Bound 1e-9 of a tensor's size: fp64 sums in another
    order lose some 1e-16 x sqrt(rows) x cancellation, and 1e-9 is a thousandth of the floor the
    device is given."""
    case = (130, 5, 13, 0.0, tr.SEED, 0)
    r64, _, _ = tr.guarded_references(case)
    weights, x, labels = tr.case_inputs(130, 5, 13, 0)
    rep = tr.loss_and_gradients(weights, np.tile(x, (4, 1)), np.tile(labels, 4), rate=0.0, seed=tr.SEED)
    assert rep.n_correct == 4 * r64.n_correct
    assert abs(rep.loss - r64.loss) <= 1e-9 * abs(r64.loss)
    slices, _ = tr.tensor_slices(13)
    for name, sl in slices.items():
        scale = np.abs(r64.grads[sl]).max()
        assert np.abs(rep.grads[sl] - r64.grads[sl]).max() <= 1e-9 * scale, name
    assert np.abs(rep.stats - r64.stats).max() <= 1e-9 * np.abs(r64.stats).max()


@pytest.mark.parametrize('layers', tr.TIE_LAYERS, ids=lambda l: 'conv1d_' + '_'.join(map(str, l)))
def test_pool_tie_rule_is_observable(layers):
    """A zero kernel with bias 0.5 makes every pool pair behind the layer an exact positive tie.
    Upstream gradients are exactly 0, and the layer's own kernel gradient under "the second wins"
    is at least 100 bounds away from the contract's: the device test on these weights would
    notice a ``>`` for the ``>=``."""
    r64, _, rm = tr.tie_references(layers)
    assert rm.close == 0 and rm.same
    weights, x, labels = tr.tie_inputs(layers)
    assert np.abs(np.diff(x, axis=1)).min() > 0
    second = tr.loss_and_gradients(weights, x, labels, rate=0.0, seed=tr.SEED, tie_first=False)
    assert second.loss == r64.loss
    slices, _ = tr.tensor_slices(tr.TIE_SHAPE[2])
    bounds = model_bounds(r64, rm, slices)
    for i in layers:
        name = 'conv1d_%d/kernel' % i
        sl = slices[name]
        scale = np.abs(r64.grads[sl]).max()
        assert scale > 0
        moved = np.abs(second.grads[sl] - r64.grads[sl]).max() / scale
        print('{}: "second wins" moves it by {:.3f} of its size, bound {:.2e}'.format(
            name, moved, bounds[name]))
        assert moved >= 100 * bounds[name]
    convs, bns = tr.TIE_UPSTREAM[layers[0]]
    for name in (['conv1d_%d/%s' % (i, p) for i in convs for p in ('kernel', 'bias')]
                 + ['bn_%d/%s' % (i, p) for i in bns for p in ('gamma', 'beta')]):
        assert not r64.grads[slices[name]].any() and not rm.grads[slices[name]].any(), name
