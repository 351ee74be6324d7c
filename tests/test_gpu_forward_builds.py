"""
The two builds of the forward kernel that a model can launch (need an MI355X; `-m gpu`).

Production launches (debug_stage -1) run dbh_lean::dbh_forward_kernel, the build of dbh_forward.hip
with the debug stages compiled out (csrc/dbh_lean.hip); DEEPBINNER_FORWARD_BUILD=full, read when a
model is created, keeps them on dbh::dbh_forward_kernel, which serves the debug stages either way.
Both are the same source with the same flags (-ffp-contract=off) and issue the same MFMAs in the
same order, so every probability and call must be IDENTICAL TO THE BIT, on both seams and on every
path through the persistent loop: compared as uint32 with np.array_equal, no tolerance.
"""
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu

MODELS = ['EXP-NBD103_read_starts', 'SQK-RBK004_read_starts']      # 13 and 17 classes
# the environment a model is created under, besides DEEPBINNER_FORWARD_BUILD
SETTINGS = {'wide': {}, 'cap2': {'DEEPBINNER_GRID_CAP': '2'},
            'cap2_static': {'DEEPBINNER_GRID_CAP': '2', 'DEEPBINNER_STATIC_WINDOWS': '1'}}


@pytest.fixture(scope='module')
def builds(hip, weights):
    """{(model name, setting, 'full' | 'lean'): HipModel}"""
    models = {}
    with pytest.MonkeyPatch.context() as mp:
        for name in MODELS:
            for setting, env in SETTINGS.items():
                for key, value in env.items():
                    mp.setenv(key, value)
                mp.setenv('DEEPBINNER_FORWARD_BUILD', 'full')
                models[name, setting, 'full'] = hip.HipModel(weights[name], device=0)
                mp.delenv('DEEPBINNER_FORWARD_BUILD')
                models[name, setting, 'lean'] = hip.HipModel(weights[name], device=0)
                for key in env:
                    mp.delenv(key)
    yield models
    for model in models.values():
        model.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ragged(all_signals, n, seed):
    """n reads of ragged length, every third one shorter than a window"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        length = int(rng.integers(1, 1024)) if i % 3 == 1 else int(rng.integers(1024, 4000))
        out.append(all_signals[(seed + i) % len(all_signals)][:length])
    return out


@pytest.mark.parametrize('name', MODELS)
def test_seam_b2_a_few_reads(builds, all_signals, name):
    """Fewer reads than a group, one group, one more, two groups, one more (1 .. 9 reads), from the
    start and from the end of the read, one window per read (the kernel makes the call itself) and
    two scan steps (per-window probabilities through the merge kernel)."""
    full, lean = builds[name, 'wide', 'full'], builds[name, 'wide', 'lean']
    for n in (1, 2, 3, 4, 5, 8, 9):
        signals = ragged(all_signals, n, n)
        assert any(len(s) < 1024 for s in signals) or n == 1
        for side, scan in (('start', 512), ('end', 512), ('start', 1024), ('end', 1024)):
            want_p, want_c = full.classify_signals(signals, side, scan, 0.5)
            got_p, got_c = lean.classify_signals(signals, side, scan, 0.5)
            assert want_p.shape == (n, full.n_classes)
            assert same_bits(got_p, want_p) and same_bits(got_c, want_c), (n, side, scan)
    short = [all_signals[0][:700]]                  # (a single read below 1,024 samples)
    for side in ('start', 'end'):
        want_p, want_c = full.classify_signals(short, side, 512, 0.5)
        got_p, got_c = lean.classify_signals(short, side, 512, 0.5)
        assert same_bits(got_p, want_p) and same_bits(got_c, want_c), side


@pytest.mark.parametrize('name', MODELS)
def test_seam_b1_five_windows(builds, name):
    full, lean = builds[name, 'wide', 'full'], builds[name, 'wide', 'lean']
    x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)[:5]
    want = full.predict(x)
    assert want.shape == (5, full.n_classes) and np.isfinite(want).all()
    assert same_bits(lean.predict(x), want)


@pytest.mark.parametrize('setting', ['cap2', 'cap2_static'])
@pytest.mark.parametrize('name', MODELS)
def test_long_shares_on_two_workgroups(builds, all_signals, name, setting):
    """27 reads over two workgroups: several groups per workgroup - off the counter, where the
    groups shrink to two windows and to one at the launch's end, or in fixed shares - with full
    and partial tail batches and the next group staged under the current one.  The two builds
    agree with each other, and with a launch of one group per workgroup."""
    full, lean = builds[name, setting, 'full'], builds[name, setting, 'lean']
    wide = builds[name, 'wide', 'full']
    signals = ragged(all_signals, 27, 27)
    for side, scan in (('start', 512), ('end', 1024)):
        want_p, want_c = full.classify_signals(signals, side, scan, 0.5)
        got_p, got_c = lean.classify_signals(signals, side, scan, 0.5)
        assert same_bits(got_p, want_p) and same_bits(got_c, want_c), (side, scan)
        wide_p, wide_c = wide.classify_signals(signals, side, scan, 0.5)
        assert same_bits(got_p, wide_p) and same_bits(got_c, wide_c), (side, scan)


@pytest.mark.parametrize('name', MODELS)
def test_debug_launches_stay_on_the_full_kernel(builds, name):
    """The lean kernel has no debug stages: asked for stage A's activations, a model without the
    knob must launch the full kernel and return what the full model returns (the lean kernel would
    run the whole forward pass and write no activations at all)."""
    full, lean = builds[name, 'wide', 'full'], builds[name, 'wide', 'lean']
    x = np.load(os.path.join(GOLD, 'windows_start.npy')).reshape(-1, 1024)[:5]
    want = full.debug_stage(x, 'A')
    assert want.shape == (5, 512, 48) and np.abs(want).max() > 0
    assert same_bits(lean.debug_stage(x, 'A'), want)
