"""A helper, not a test: the training step's second half restated in NumPy - the contract of
``include/deepbinner_hip.h``, "a resident trainer" (DESIGN.md section 18): the step seed, the
Gaussian noise (reference ``network_architecture.py:25``), Keras 2.1.4's Nadam
(``train_network.py:53-55``) and BatchNormalization's moving statistics, and one whole step in fp64
(``full_step``: same hash, same noise, ``tests/train_reference.py``'s loss and gradients).

The update is written operation for operation as the header lists it, in NumPy float64 - IEEE
double like the device's - with one rounding to fp32 where m, v and p are stored: the device's
result is held to it bit for bit.  The noise goes through ``log``, ``cos`` and ``sqrt`` of another
library, a few fp64 units apart at most, so after its one rounding it is within one fp32 unit.
"""
import numpy as np

import train_reference as tr
from deepbinner_amd.model_format import ModelWeights

M32 = 0xFFFFFFFF
M64 = 2 ** 64 - 1
STEP_SEED_STRIDE = 0x9E3779B97F4A7C15
# Nadam's configuration under Keras 2.1.4, as a model file's training_config records it, with the
# BatchNormalization momentum and the network's Dropout and GaussianNoise
DEFAULTS = {
    'lr': float(np.float32(0.002)), 'beta_1': float(np.float32(0.9)),
    'beta_2': float(np.float32(0.999)), 'epsilon': 1e-7, 'schedule_decay': 0.004,
    'bn_momentum': 0.99, 'dropout_rate': 0.15, 'noise_std': 0.02, 'seed': 0,
}
Z_MAX = float(np.sqrt(2 * np.log(2.0 ** 24)))


def step_seed(seed, t0):
    return (int(seed) + int(t0) * STEP_SEED_STRIDE) & M64


def hash_bits(seed, layer, n_windows, length, channels):
    """uint64 [n_windows, length, channels] of 24-bit values: the hash of include/deepbinner_hip.h
    (dbh_gradients' dropout) before its comparison with the threshold."""
    seed = int(seed) & M64
    lo, hi = seed & M32, seed >> 32
    h = tr._mix(np.uint64((lo + layer * 0x9e3779b9) & M32))
    h = tr._mix(h ^ np.uint64(hi))
    window = np.arange(n_windows, dtype=np.uint64)[:, None, None]
    h = tr._mix((h + window) & np.uint64(M32))
    counter = (np.arange(length, dtype=np.uint64)[None, :, None] * np.uint64(256)
               + np.arange(channels, dtype=np.uint64)[None, None, :])
    return tr._mix(h ^ counter) >> np.uint64(8)


def noise_z(n_windows, input_size, seed):
    """The standard normal draws [n_windows, input_size] of a step seed, fp64 (Box-Muller)."""
    bits = hash_bits(seed, 0, n_windows, input_size, 2).astype(np.float64)
    u1 = (bits[:, :, 0] + 1.0) / 16777216.0
    u2 = bits[:, :, 1] / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos((2 * np.pi) * u2)


def add_noise(x, noise_std, seed):
    x = np.asarray(x, dtype=np.float32)
    if float(noise_std) == 0.0:
        return x.copy()
    z = noise_z(x.shape[0], x.shape[1], seed)
    return (x.astype(np.float64) + float(np.float32(noise_std)) * z).astype(np.float32)


def nadam_coefficients(t0, m_schedule=1.0, **options):
    """dbh_nadam_schedule in Python floats (doubles)."""
    o = dict(DEFAULTS, **options)
    t = float(t0) + 1.0
    mu_t = o['beta_1'] * (1.0 - 0.5 * 0.96 ** (t * o['schedule_decay']))
    mu_t1 = o['beta_1'] * (1.0 - 0.5 * 0.96 ** ((t + 1.0) * o['schedule_decay']))
    sched_new = m_schedule * mu_t
    return {'lr': o['lr'], 'beta_1': o['beta_1'], 'beta_2': o['beta_2'], 'epsilon': o['epsilon'],
            'mu_t': mu_t, 'mu_t1': mu_t1, 'sched_new': sched_new, 'sched_next': sched_new * mu_t1,
            'beta_2_t': o['beta_2'] ** t, 'bn_momentum': o['bn_momentum']}


def nadam_core(p, g, m, v, k):
    """Keras 2.1.4 Nadam.get_updates on float64 arrays, nothing rounded: (p, m, v)."""
    g_prime = g / (1.0 - k['sched_new'])
    m_keep = k['beta_1'] * m
    m_add = (1.0 - k['beta_1']) * g
    m_new = m_keep + m_add
    m_prime = m_new / (1.0 - k['sched_next'])
    v_keep = k['beta_2'] * v
    v_add = (1.0 - k['beta_2']) * (g * g)
    v_new = v_keep + v_add
    v_prime = v_new / (1.0 - k['beta_2_t'])
    bar = (1.0 - k['mu_t']) * g_prime + k['mu_t1'] * m_prime
    denom = np.sqrt(v_prime) + k['epsilon']
    return p - (k['lr'] * bar) / denom, m_new, v_new


def moving_index(n_classes):
    """(indices of the moving-mean and moving-variance slots in the blob, the index into the 960
    batch statistics each of them averages): BN by BN, mean then variance in both."""
    _, moving = tr.tensor_slices(n_classes)
    blob = np.concatenate([np.arange(sl.start, sl.stop) for sl in moving])
    return blob, np.arange(blob.size)


def nadam_update(params, grads, m, v, batch_stats, n_classes, k):
    """dbh_nadam_update: fp32 arrays in, new fp32 (params, m, v) out."""
    p32, g32, m32, v32 = (np.asarray(a, dtype=np.float32) for a in (params, grads, m, v))
    p, m_new, v_new = nadam_core(*(a.astype(np.float64) for a in (p32, g32, m32, v32)), k)
    p, m_new, v_new = (a.astype(np.float32) for a in (p, m_new, v_new))
    blob, stat = moving_index(n_classes)
    old = p32[blob].astype(np.float64)
    batch = np.asarray(batch_stats, dtype=np.float32)[stat].astype(np.float64)
    p[blob] = (old - (old - batch) * (1.0 - k['bn_momentum'])).astype(np.float32)
    m_new[blob] = m32[blob]
    v_new[blob] = v32[blob]
    return p, m_new, v_new


class State:
    """A trainer's state on the host: flat fp32 weights, m, v; iterations; m_schedule."""

    def __init__(self, weights):
        self.n_classes, self.input_size = weights.n_classes, weights.input_size
        self.flat = weights.flat()
        self.m = np.zeros_like(self.flat)
        self.v = np.zeros_like(self.flat)
        self.iterations = 0
        self.m_schedule = 1.0

    def weights(self):
        return ModelWeights.from_flat(self.flat, self.n_classes, self.input_size)


def full_step(state, x, labels, schedule=nadam_coefficients, gradients=None, noise=add_noise,
              **options):
    """One step on ``state`` in place; returns (loss, n_correct) of the batch before the update.
    ``gradients(weights, x, labels, rate, seed) -> (loss, n_correct, grads, stats)``: the fp64
    reference unless given (the GPU tests replay with the device's own dbh_gradients);
    ``noise(x, noise_std, seed)`` and ``schedule(t0, m_schedule, **options)`` likewise."""
    o = dict(DEFAULTS, **options)
    seed = step_seed(o['seed'], state.iterations)
    noisy = noise(np.asarray(x, dtype=np.float32), o['noise_std'], seed)
    if gradients is None:
        r = tr.loss_and_gradients(state.weights(), noisy, labels, rate=o['dropout_rate'], seed=seed)
        loss, n_correct, grads, stats = r.loss, r.n_correct, r.grads, r.stats
    else:
        loss, n_correct, grads, stats = gradients(state.weights(), noisy, labels, o['dropout_rate'], seed)
    k = schedule(state.iterations, state.m_schedule, **options)
    state.flat, state.m, state.v = nadam_update(state.flat, grads, state.m, state.v, stats,
                                                state.n_classes, k)
    state.iterations += 1
    state.m_schedule = k['sched_new']
    return loss, n_correct


# ---- the learning task of tests/test_gpu_trainer.py ---------------------------------------------
# Three classes, each a fixed motif of MOTIF_LENGTH samples (drawn once from N(0, 1), scaled by
# MOTIF_SCALE) added at a random offset to a window of N(0, 1) noise.
LEARN_INPUT, LEARN_CLASSES, LEARN_BATCH = 96, 3, 16
LEARN_STEPS = 300
LEARN_OPTIONS = {'bn_momentum': 0.9, 'seed': 20181018}
MOTIF_LENGTH, MOTIF_SCALE = 24, 3.0
LEARN_WEIGHT_SEED, LEARN_DATA_SEED, LEARN_HELD_OUT_SEED = 1, 2, 3


def motif_batch(rng, n):
    motifs = np.random.default_rng(LEARN_INPUT).standard_normal((LEARN_CLASSES, MOTIF_LENGTH))
    labels = rng.integers(LEARN_CLASSES, size=n).astype(np.int32)
    x = rng.standard_normal((n, LEARN_INPUT))
    for i, at in enumerate(rng.integers(LEARN_INPUT - MOTIF_LENGTH + 1, size=n)):
        x[i, at:at + MOTIF_LENGTH] += MOTIF_SCALE * motifs[labels[i]]
    return x.astype(np.float32), labels


def learning_batches():
    """The LEARN_STEPS training batches and the held-out batch of 64."""
    rng = np.random.default_rng(LEARN_DATA_SEED)
    train = [motif_batch(rng, LEARN_BATCH) for _ in range(LEARN_STEPS)]
    return train, motif_batch(np.random.default_rng(LEARN_HELD_OUT_SEED), 64)


def learning_weights():
    return ModelWeights.fresh(LEARN_CLASSES, LEARN_INPUT, seed=LEARN_WEIGHT_SEED)
