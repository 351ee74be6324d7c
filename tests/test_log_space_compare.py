"""The log-space comparison (tests/oracle_compare.py) without a device: a correct fp32 computation
of the network passes it, and faults that the 1e-4 probability bound misses fail it.  Also: the
general path's log-space sizes really cover both parities of every stage length."""
import os

import numpy as np
import pytest

from conftest import GOLD, PLAN
from general_fixtures import PARITY_GEOMETRIES, geometry
from oracle import classify_ref, network_ref
from oracle_compare import (PROB_TOL, assert_log_close, log_space_ratio, oracle_call_batch,
                            read_scale)


@pytest.fixture(scope='module')
def fp64(weights):
    """model -> (444 golden windows of its side, fp64 probabilities, fp64 stages)."""
    out = {}
    for model, side in PLAN:
        x = np.load(os.path.join(GOLD, 'windows_%s.npy' % side)).reshape(-1, 1024)
        probs, stages = network_ref.forward(weights[model], x, dtype=np.float64,
                                            return_stages=True)
        out[model] = (x, probs, stages)
    return out


def bf16(x):
    """Round to bfloat16 (nearest, ties to even), back in float64."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


@pytest.mark.parametrize('model,side', PLAN)
def test_fp32_oracle_passes(weights, fp64, model, side):
    x, _, stages = fp64[model]
    assert len(x) == 444
    p32 = network_ref.forward(weights[model], x, dtype=np.float32)
    ratio = assert_log_close(p32, logits=stages['logits'], what='fp32 oracle ' + model)
    assert ratio < 0.1      # (about 0.01-0.02: the log error of fp32 is near 1.6e-5)


@pytest.mark.parametrize('model,side', PLAN)
def test_a_barcode_logit_scaled_by_1_01_fails(fp64, model, side):
    _, probs, stages = fp64[model]
    for j in range(1, probs.shape[1]):
        logits = stages['logits'].copy()
        logits[:, j] *= 1.01
        p = network_ref.softmax(logits)
        assert log_space_ratio(p, logits=stages['logits']) > 10, j
        with pytest.raises(AssertionError):
            assert_log_close(p, logits=stages['logits'])
        if model == 'EXP-NBD103_read_starts' and j == 5:
            # the fault the 1e-4 probability check lets through
            assert np.abs(p - probs).max() < PROB_TOL


@pytest.mark.parametrize('model,side', PLAN)
def test_bf16_pooled_activations_fail(weights, fp64, monkeypatch, model, side):
    x, _, stages = fp64[model]
    pool = network_ref.max_pool2
    monkeypatch.setattr(network_ref, 'max_pool2', lambda t: bf16(pool(t)))
    p = network_ref.forward(weights[model], x, dtype=np.float64)
    assert log_space_ratio(p, logits=stages['logits']) > 10
    with pytest.raises(AssertionError):
        assert_log_close(p, logits=stages['logits'])


@pytest.mark.parametrize('model,side', PLAN)
def test_last_position_dropped_before_the_average_fails(weights, fp64, model, side):
    _, _, stages = fp64[model]
    kernel, bias = weights[model].convs[-1]
    conv20 = network_ref.relu(network_ref.conv1d(stages['G'], kernel.astype(np.float64),
                                                 bias.astype(np.float64), 1, 'same'))
    assert np.allclose(conv20.mean(axis=1), stages['logits'], rtol=0, atol=1e-12)
    p = network_ref.softmax(conv20[:, :-1].mean(axis=1))
    assert log_space_ratio(p, logits=stages['logits']) > 10
    with pytest.raises(AssertionError):
        assert_log_close(p, logits=stages['logits'])


@pytest.mark.parametrize('model,side', PLAN)
def test_merged_results_fp32_passes_and_a_scaled_logit_fails(weights, all_signals, model, side):
    """Per-read results: call_batch around the fp32 oracle passes against call_batch around the
    fp64 one (one scan step and twelve), and a barcode logit scaled by 1.01 in every window
    fails."""
    w = weights[model]
    for scan in (512, 6144):
        calls, probs, scale = oracle_call_batch(w, all_signals, scan, 0.5, side)
        _, p32 = classify_ref.call_batch(
            lambda x: network_ref.forward(w, x.astype(np.float32), dtype=np.float32),
            all_signals, 1024, scan, 0.5, side)
        assert_log_close(p32.astype(np.float32), probs=probs, scale=scale,
                         what='fp32 call_batch {} {}'.format(model, scan))

        def scaled(x):
            _, st = network_ref.forward(w, x.astype(np.float32), dtype=np.float64,
                                        return_stages=True)
            logits = st['logits']
            logits[:, 5] *= 1.01
            return network_ref.softmax(logits)
        _, bad = classify_ref.call_batch(scaled, all_signals, 1024, scan, 0.5, side)
        with pytest.raises(AssertionError):
            assert_log_close(bad.astype(np.float32), probs=probs, scale=scale)


def test_read_scale_takes_the_largest_window_of_each_read():
    logits = np.zeros((3, 2, 4))          # [steps, reads, classes]
    logits[1, 0, 2] = -7.0
    logits[2, 1, 0] = 0.5
    assert np.array_equal(read_scale(logits.reshape(-1, 4), 2), [7.0, 1.0])


def stage_lengths(input_size):
    """len[1..7] from the oracle's own stage shapes (stages A .. G) on one window."""
    w = geometry(input_size, 2)
    _, stages = network_ref.forward(w, np.zeros((1, input_size)), return_stages=True)
    return [stages[s].shape[1] for s in 'ABCDEFG']


def test_general_sizes_cover_both_parities_of_every_stage_length():
    lengths = {size: stage_lengths(size) for size, _ in PARITY_GEOMETRIES}
    sizes = sorted(lengths)
    for i in range(7):
        odd = [s for s in sizes if lengths[s][i] % 2]
        even = [s for s in sizes if lengths[s][i] % 2 == 0]
        assert odd and even, 'len[{}]: odd at {}, even at {}'.format(i + 1, odd, even)
    assert {96, 98, 16382} <= set(sizes)
    assert lengths[16382][:5] == [8191, 4095, 2047, 1023, 511]
    classes = [c for _, c in PARITY_GEOMETRIES]
    assert min(classes) == 2 and max(classes) == 256
