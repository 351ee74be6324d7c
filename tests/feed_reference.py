"""A helper, not a test: the training step's feed restated in NumPy - the contract of
``include/deepbinner_hip.h``, "device-fed batches, validation" (DESIGN.md section 19): a window's
normalisation from exact integer sums, the augmentation (the reference's ``modify_signal`` law on
``tests/train_step_reference.py``'s hash), the epoch order, the inference-phase loss, and NumPy
stand-ins for the device classes that ``deepbinner_amd.fit.fit`` takes as parameters.

Everything up to the one fp64 expression per value is integer arithmetic, and that expression is
IEEE double with correctly rounded division and square root on both sides: the device's batches
are held to this bit for bit.
"""
import re

import numpy as np

import train_reference as tr
import train_step_reference as ts
from deepbinner_amd.model_format import ModelWeights
from oracle import network_ref

M32 = 0xFFFFFFFF
M64 = 2 ** 64 - 1
LAYER_CHANCE, LAYER_KEY, LAYER_ORDER = 8, 9, 10


def bits(seed, layer, window, positions, channel=0):
    """uint64 array like ``positions`` of 24-bit values: the header's hash for one window number
    (or an array of them, broadcast against ``positions``)."""
    seed = int(seed) & M64
    lo, hi = seed & M32, seed >> 32
    h = tr._mix(np.uint64((lo + layer * 0x9e3779b9) & M32))
    h = tr._mix(h ^ np.uint64(hi))
    h = tr._mix((h + np.asarray(window, dtype=np.uint64)) & np.uint64(M32))
    counter = np.asarray(positions, dtype=np.uint64) * np.uint64(256) + np.uint64(channel)
    return tr._mix(h ^ counter) >> np.uint64(8)


# ---- normalise -----------------------------------------------------------------------------------
def special_windows(length):
    """constant; alternating -32768 / 32767; full-range draws; the alternating one with its first
    sample moved by one: its sum is odd, so D is, and at 16,384 samples (D > 2^53) (double)D rounds"""
    rng = np.random.default_rng(length)
    alternating = np.where(np.arange(length) % 2 == 0, -32768, 32767)
    odd = alternating.copy()
    odd[0] += 1
    return np.stack([np.full(length, 1234), alternating,
                     rng.integers(-32768, 32768, size=length), odd]).astype(np.int16)


def window_stats(samples):
    """(mean, std) fp64 per window of int16 ``samples`` [n, L], from S, Q and D in int64."""
    x = np.asarray(samples).astype(np.int64)
    length = x.shape[1]
    s = x.sum(axis=1)
    q = (x * x).sum(axis=1)
    d = length * q - s * s
    assert (d >= 0).all() and length * int(q.max(initial=0)) < 2 ** 63
    return s.astype(np.float64) / length, np.sqrt(d.astype(np.float64)) / length, d


def normalise(samples):
    """fp32 [n, L]: ((double)x - mean) / std, or (double)x - mean where D == 0, rounded once."""
    mean, std, d = window_stats(samples)
    centred = np.asarray(samples).astype(np.float64) - mean[:, None]
    safe = np.where(d == 0, 1.0, std)[:, None]
    return np.where((d == 0)[:, None], centred, centred / safe).astype(np.float32)


def keras_side_normalise(window):
    """What the reference feeds its network for one window of integers: trim_signal.normalise's
    formula (mean and population standard deviation of the float64 array), cast to fp32."""
    signal = np.asarray(window).astype(np.int64)
    mean, stdev = np.mean(signal), np.std(signal)
    out = (signal - mean) / stdev if stdev > 0.0 else signal - mean
    return out.astype(np.float32)


# ---- augment -------------------------------------------------------------------------------------
def augment_threshold(augmentation):
    augmentation = float(augmentation)
    if not augmentation >= 1.0:
        raise ValueError('augmentation must be at least 1')
    return int(np.floor((1.0 - 1.0 / augmentation) * 16777216.0))


def half_of(length):
    return int(round(length / 4))            # Python's round: half to even


def slot_is_augmented(seed, slot, threshold):
    return int(bits(seed, LAYER_CHANCE, slot, 0)) < threshold


def keys_of(seed, slot, length):
    return bits(seed, LAYER_KEY, slot, np.arange(length)).astype(np.int64)


def ranks_of(keys, ties='ascending'):
    """rank(i) = the place of (key(i), i) in ascending order; ``ties='descending'`` ranks equal
    keys by descending index instead - the rule the contract does NOT have."""
    index = np.arange(keys.size)
    order = np.lexsort((index if ties == 'ascending' else -index, keys))
    ranks = np.empty(keys.size, dtype=np.int64)
    ranks[order] = index
    return ranks


def copies_of(ranks, half):
    return np.where(ranks < half, 2, np.where(ranks < 2 * half, 0, 1))


def augment_sources(seed, slot, length, ties='ascending'):
    """The source position of each of the ``length`` outputs of an augmented slot."""
    copies = copies_of(ranks_of(keys_of(seed, slot, length), ties), half_of(length))
    return np.repeat(np.arange(length), copies)


def batch(samples, labels, indices, augmentation=1.0, seed=0):
    """dbh_dataset_batch: (x fp32 [N, L], labels int32 [N])."""
    samples = np.asarray(samples)
    indices = np.asarray(indices, dtype=np.int64)
    threshold = augment_threshold(augmentation)
    x = normalise(samples[indices])
    for slot in range(indices.size):
        if slot_is_augmented(seed, slot, threshold):
            x[slot] = x[slot][augment_sources(seed, slot, samples.shape[1])]
    return x, np.asarray(labels, dtype=np.int32)[indices]


# ---- epoch order ---------------------------------------------------------------------------------
def epoch_order(seed, epoch_pass, n):
    keys = bits(seed, LAYER_ORDER, np.arange(n), int(epoch_pass) % 2 ** 14)
    return np.argsort(keys, kind='stable').astype(np.int64)


def stream_indices(seed, n, first, count):
    """Positions [first, first + count) of the sample stream: pass 0's order, then pass 1's ..."""
    out = []
    for p in range(first // n, (first + count - 1) // n + 1):
        order = epoch_order(seed, p, n)
        lo, hi = max(first, p * n), min(first + count, (p + 1) * n)
        out.append(order[lo - p * n:hi - p * n])
    return np.concatenate(out)


# ---- inference-phase loss ------------------------------------------------------------------------
def evaluate(weights, x, labels, dtype=np.float64):
    """(loss per window fp64, argmax per window, logits) of network_ref.forward in ``dtype``: the
    loss is -log softmax(logits)[label] by a log-sum-exp in fp64 from that run's logits."""
    _, stages = network_ref.forward(weights, np.asarray(x, dtype=np.float32), dtype=dtype,
                                    return_stages=True)
    logits = stages['logits'].astype(np.float64)
    top = logits.max(axis=1)
    lse = top + np.log(np.exp(logits - top[:, None]).sum(axis=1))
    labels = np.asarray(labels, dtype=np.int64)
    return lse - logits[np.arange(len(labels)), labels], logits.argmax(axis=1), logits


# ---- stand-ins for fit()'s device classes ---------------------------------------------------------
class HostDataset:
    """``hip_backend.Dataset``'s interface on host arrays."""

    def __init__(self, samples, labels, n_classes, device=None):
        self.samples = np.ascontiguousarray(samples, dtype=np.int16)
        self.labels = np.asarray(labels, dtype=np.int32)
        self.input_size, self.n_classes = self.samples.shape[1], int(n_classes)

    from_arrays = classmethod(lambda cls, *a, **k: cls(*a, **k))

    def __len__(self):
        return self.samples.shape[0]

    def batch(self, indices, augmentation=1.0, seed=0):
        return batch(self.samples, self.labels, indices, augmentation, seed)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HostTrainer:
    """``hip_backend.Trainer``'s interface in fp64 NumPy: tests/train_step_reference.py's step."""

    def __init__(self, weights, max_windows, device=None, **options):
        self.state = ts.State(weights)
        self.options = dict(ts.DEFAULTS, **options)
        self._given = options
        self.max_windows = int(max_windows)

    @property
    def iterations(self):
        return self.state.iterations

    def step_dataset(self, dataset, indices, augmentation=1.0):
        seed = ts.step_seed(self.options['seed'], self.state.iterations)
        x, labels = dataset.batch(indices, augmentation, seed)
        return ts.full_step(self.state, x, labels, **self._given)

    def run_epoch(self, dataset, indices, batch_size, augmentation):
        steps = len(indices) // batch_size
        results = [self.step_dataset(dataset, indices[t * batch_size:(t + 1) * batch_size],
                                     augmentation) for t in range(steps)]
        return (np.array([r[0] for r in results], dtype=np.float64),
                np.array([r[1] for r in results], dtype=np.int64))

    def evaluate(self, dataset, first=0, count=None, window_losses=False):
        count = len(dataset) - first if count is None else count
        x, labels = dataset.batch(np.arange(first, first + count))
        losses, best, _ = evaluate(self.state.weights(), x, labels)
        total = 0.0
        for value in losses:
            total += float(value)
        result = (total, int((best == labels).sum()))
        return result + (losses,) if window_losses else result

    def weights(self):
        return self.state.weights()

    def save_checkpoint(self, path):
        self.weights().save(path)
        from deepbinner_amd.hip_backend import write_npz
        write_npz(str(path) + '.state.npz', dict(
            m=self.state.m, v=self.state.v,
            iterations=np.asarray(self.state.iterations, dtype=np.int64),
            m_schedule=np.asarray(self.state.m_schedule, dtype=np.float64)))

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the learning task of tests/test_gpu_feed.py: section 18's three motifs as int16 text files ---
# Section 18 ran its 300 steps with bn_momentum 0.9.  The command has Keras's 0.99, as the reference
# does: after 300 steps 0.99^300 = 5 % of the initial moving variance of 1 is still in the average,
# against channel variances far below 1, and the fp64 restatement calls 40 of 64 validation windows
# right while its training loss is long under the line.  So the task is adjusted, not the bars: the
# motif twice as strong and 600 steps (0.99^600 = 0.2 %), six epochs of one pass over 1,600 samples.
FIT_INPUT, FIT_CLASSES, FIT_BATCH = ts.LEARN_INPUT, 4, ts.LEARN_BATCH
FIT_MOTIF_SCALE = 6.0
FIT_SCALE = 100.0              # a window's values times this, rounded to integers
FIT_TRAIN, FIT_VAL = 1600, 64  # 100 steps per epoch
FIT_EPOCHS = 6
FIT_SEED = 20181018


def fit_task(rng, n):
    """(int16 samples [n, 96], labels 1..3): ts.motif_batch's windows with FIT_MOTIF_SCALE, scaled
    and rounded."""
    motifs = np.random.default_rng(FIT_INPUT).standard_normal((3, ts.MOTIF_LENGTH))
    labels = rng.integers(3, size=n).astype(np.int32)
    x = rng.standard_normal((n, FIT_INPUT))
    for i, at in enumerate(rng.integers(FIT_INPUT - ts.MOTIF_LENGTH + 1, size=n)):
        x[i, at:at + ts.MOTIF_LENGTH] += FIT_MOTIF_SCALE * motifs[labels[i]]
    return np.rint(x * FIT_SCALE).astype(np.int16), labels + 1


def fit_sets():
    train = fit_task(np.random.default_rng(ts.LEARN_DATA_SEED), FIT_TRAIN)
    val = fit_task(np.random.default_rng(ts.LEARN_HELD_OUT_SEED), FIT_VAL)
    return train, val


# one line per epoch, as deepbinner_amd/fit.py prints it
EPOCH_LINE = re.compile(r'^Epoch (\d+)/(\d+) - loss: ([\d.]+) - acc: ([\d.]+) - val_loss: ([\d.]+) - '
                        r'val_acc: ([\d.]+) - val_acc (improved from \S+ to [\d.]+, saved (.+)|'
                        r'did not improve from [\d.]+)$')


def write_training_file(path, samples, labels):
    with open(path, 'wt') as f:
        for label, row in zip(labels, samples):
            f.write('{}\t{}\n'.format(int(label), ','.join(str(int(v)) for v in row)))


def fresh_weights(n_classes, input_size, seed=0):
    return ModelWeights.fresh(n_classes, input_size, seed=seed)


# ---- the evaluate cases of tests/test_gpu_feed.py --------------------------------------------------
# (input size, windows, classes): weights of tests/weight_families.py's random_model (moving means
# N(0.5, 0.5), moving variances exp(N(0, 1)), gammas of both signs) on normal windows.
EVAL_CASES = [(96, 5, 2), (130, 5, 13), (200, 3, 256), (1024, 4, 13)]
EVAL_GAP = 1e-3
_eval_cache = {}


def eval_case(case):
    """-> dict: weights, x, labels, and the reference's results in fp64 and fp32 (loss per window,
    argmax, the top-two logit gap of the fp64 run).  Computed once per session."""
    if case not in _eval_cache:
        size, n, classes = case
        weights, x, labels = tr.case_inputs(size, n, classes, draw=0)
        loss64, best64, logits = evaluate(weights, x, labels, np.float64)
        loss32, best32, _ = evaluate(weights, x, labels, np.float32)
        top = np.sort(logits, axis=1)
        _eval_cache[case] = dict(weights=weights, x=x, labels=labels, loss64=loss64, best64=best64,
                                 loss32=loss32, best32=best32, gap=top[:, -1] - top[:, -2])
    return _eval_cache[case]
