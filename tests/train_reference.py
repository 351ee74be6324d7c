"""A helper, not a test: the training step's first half restated in NumPy - the Deepbinner graph
(reference ``network_architecture.py:18-95``) in Keras's training phase, the categorical
cross-entropy of ``train_network.py:53-55`` and the analytic gradient of the mean loss with respect
to every trainable parameter.  It is the contract of ``include/deepbinner_hip.h``, "training"
(DESIGN.md section 17), and what ``dbh_gradients`` is held to; ``tests/test_train_reference.py``
pins it against ``oracle/network_ref.forward`` and against central differences.

Everything runs in ``dtype`` (float64 for the reference proper, float32 to measure what plain fp32
arithmetic loses on a case).  The layer primitives are ``oracle.network_ref``'s, so the edge rules
(SAME padding, the average pool's valid-tap count, the 'valid' max-pool) are the inference
oracle's.  Not restated here: GaussianNoise (the caller's to add) and Keras's clipping of the
probability to [1e-7, 1 - 1e-7].
"""
import numpy as np

from deepbinner_amd.model_format import BN_CHANNELS, BN_EPSILON, conv_shapes, param_count
from oracle import network_ref

M32 = 0xFFFFFFFF


def _mix(h):
    """32-bit integer hash step on uint64 arrays holding 32-bit values."""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7feb352d)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846ca68b)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(16))
    return h


def dropout_keep(seed, layer, n_windows, length, channels, rate):
    """Boolean [n_windows, length, channels]: which elements dropout layer ``layer`` (1..7) keeps.
    The function written out in include/deepbinner_hip.h."""
    seed = int(seed) & (2 ** 64 - 1)
    lo, hi = seed & M32, seed >> 32
    h = _mix(np.uint64((lo + layer * 0x9e3779b9) & M32))
    h = _mix(h ^ np.uint64(hi))
    window = np.arange(n_windows, dtype=np.uint64)[:, None, None]
    h = _mix((h + window) & np.uint64(M32))
    counter = (np.arange(length, dtype=np.uint64)[None, :, None] * np.uint64(256)
               + np.arange(channels, dtype=np.uint64)[None, None, :])
    h = _mix(h ^ counter)
    threshold = int(float(np.float32(rate)) * 16777216.0)
    return (h >> np.uint64(8)) >= np.uint64(threshold)


def dropout_scale(rate):
    """(float)(1 / (1 - rate)) as the device forms it; exactly 1 at rate 0."""
    return float(np.float32(1.0 / (1.0 - float(np.float32(rate)))))


def _pads(length, k, stride, padding):
    if padding == 'same':
        out = -(-length // stride)
        total = max((out - 1) * stride + k - length, 0)
        return out, total // 2, total - total // 2
    return (length - k) // stride + 1, 0, 0


def conv1d_backward(x, kernel, stride, padding, dz):
    """Gradients of ``network_ref.conv1d`` given dz at its output: (dx, dkernel, dbias)."""
    n, length, cin = x.shape
    k = kernel.shape[0]
    out, left, right = _pads(length, k, stride, padding)
    assert dz.shape[1] == out
    xp = np.pad(x, ((0, 0), (left, right), (0, 0)))
    dxp = np.zeros_like(xp)
    dkernel = np.empty_like(kernel)
    span = (out - 1) * stride + 1
    flat = dz.reshape(-1, dz.shape[2])
    for j in range(k):
        dkernel[j] = xp[:, j:j + span:stride, :].reshape(-1, cin).T @ flat
        dxp[:, j:j + span:stride, :] += dz @ kernel[j].T
    return dxp[:, left:left + length, :], dkernel, flat.sum(axis=0)


def max_pool2_first(x):
    """Which of each pair the 'valid' pool takes: True = the first (it wins exact ties)."""
    n, length, c = x.shape
    half = length // 2
    pairs = x[:, :2 * half, :].reshape(n, half, 2, c)
    return pairs[:, :, 0, :] >= pairs[:, :, 1, :]


def max_pool2_backward(x, g):
    first = max_pool2_first(x)
    half = first.shape[1]
    dx = np.zeros_like(x)                   # a dropped last position keeps 0
    dx[:, 0:2 * half:2, :] = g * first
    dx[:, 1:2 * half:2, :] = g * ~first
    return dx


def avg_pool3_backward(g):
    n, length, c = g.shape
    count = np.full((length, 1), 3.0, dtype=g.dtype)
    count[0] = 2.0
    count[-1] = 2.0
    if length == 1:
        count[0] = 1.0
    gp = np.pad(g / count, ((0, 0), (1, 1), (0, 0)))
    return gp[:, 0:length] + gp[:, 1:length + 1] + gp[:, 2:length + 2]


class Result:
    """loss, n_correct, grads (flat, the blob's layout, dtype), stats (960: mean then variance per
    BN layer), probs, logits, patterns (every ReLU mask and pool choice, for flip detection)."""


def loss_and_gradients(weights, x, labels, rate=0.15, seed=0, dtype=np.float64, backward=True):
    dtype = np.dtype(dtype).type
    x = np.asarray(x, dtype=dtype)
    if x.ndim == 2:
        x = x[:, :, None]
    n = x.shape[0]
    labels = np.asarray(labels).astype(np.int64)
    shapes = conv_shapes(weights.n_classes)
    scale = dtype(dropout_scale(rate))
    eps = dtype(BN_EPSILON)
    patterns = []
    tape = []                                # the backward pass, last step first when reversed
    grads_conv = [None] * 20
    grads_bn = [None] * 7
    stats = []

    def conv(i, t):
        kernel, bias = (a.astype(dtype) for a in weights.convs[i - 1])
        _, _, _, _, stride, padding = shapes[i - 1]
        y = network_ref.relu(network_ref.conv1d(t, kernel, bias, stride, padding))
        live = y > 0                         # ReLU'(0) = 0
        patterns.append(live)

        def back(g):
            dx, dk, db = conv1d_backward(t, kernel, stride, padding, g * live)
            grads_conv[i - 1] = (dk, db)
            return dx
        tape.append(back)
        return y

    def pool(t):
        patterns.append(max_pool2_first(t))
        tape.append(lambda g: max_pool2_backward(t, g))
        return network_ref.max_pool2(t)

    def bn(i, t):
        gamma, beta = (a.astype(dtype) for a in weights.bns[i - 1][:2])
        rows = dtype(t.shape[0] * t.shape[1])
        mean = t.mean(axis=(0, 1))
        var = ((t - mean) ** 2).mean(axis=(0, 1))            # biased, two passes
        stats.extend([mean, var])
        istd = dtype(1) / np.sqrt(var + eps)
        xhat = (t - mean) * istd
        keep = dropout_keep(seed, i, t.shape[0], t.shape[1], t.shape[2], rate) * scale

        def back(g):
            g = g * keep
            dbeta = g.sum(axis=(0, 1))
            dgamma = (g * xhat).sum(axis=(0, 1))
            grads_bn[i - 1] = (dgamma, dbeta)
            return (gamma * istd) * (g - dbeta / rows - xhat * (dgamma / rows))
        tape.append(back)
        return (xhat * gamma + beta) * keep

    def run_back(g, upto):
        while len(tape) > upto:
            g = tape.pop()(g)
        return g

    t = bn(1, conv(1, x))
    t = bn(2, pool(conv(4, conv(3, conv(2, t)))))
    t = bn(3, pool(conv(7, conv(6, conv(5, t)))))
    t = bn(4, pool(conv(9, conv(8, t))))
    trunk = len(tape)
    d = t
    marks = [len(tape)]
    x1 = conv(10, network_ref.avg_pool3_same(d))
    marks.append(len(tape))
    x2 = conv(11, d)
    marks.append(len(tape))
    x3 = conv(13, conv(12, d))
    marks.append(len(tape))
    x4 = conv(16, conv(15, conv(14, d)))
    marks.append(len(tape))
    branch_tapes = [tape[marks[k]:marks[k + 1]] for k in range(4)]
    del tape[trunk:]
    cat = np.concatenate([x1, x2, x3, x4], axis=2)

    def inception_back(g):
        total = None
        for k, steps in enumerate(branch_tapes):
            gb = g[:, :, 48 * k:48 * (k + 1)]
            for step in reversed(steps):
                gb = step(gb)
            if k == 0:
                gb = avg_pool3_backward(gb)
            total = gb if total is None else total + gb
        return total
    tape.append(inception_back)
    t = bn(5, pool(cat))
    t = bn(6, conv(17, t))
    t = bn(7, pool(conv(19, conv(18, t))))
    z = conv(20, t)
    l7 = z.shape[1]
    logits = z.mean(axis=1)
    mx = logits.max(axis=1, keepdims=True)
    e = np.exp(logits - mx)
    se = e.sum(axis=1, keepdims=True)
    probs = e / se
    losses = (mx[:, 0] + np.log(se[:, 0])) - logits[np.arange(n), labels]

    out = Result()
    out.loss = float(losses.astype(np.float64).sum() / n) if dtype is np.float64 else float(losses.mean())
    out.n_correct = int((np.argmax(logits, axis=1) == labels).sum())   # lowest index on ties
    out.probs, out.logits, out.patterns = probs, logits, patterns
    out.stats = np.concatenate(stats)
    out.grads = None
    if backward:
        dlogits = probs.copy()
        dlogits[np.arange(n), labels] -= 1
        dlogits /= dtype(n)
        g = np.repeat((dlogits / dtype(l7))[:, None, :], l7, axis=1)
        run_back(g, 0)
        parts = []
        for dk, db in grads_conv:
            parts += [dk.ravel(), db.ravel()]
        for (dgamma, dbeta), c in zip(grads_bn, BN_CHANNELS):
            parts += [dgamma, dbeta, np.zeros(2 * c, dtype=dtype)]
        out.grads = np.concatenate(parts)
        assert out.grads.size == param_count(weights.n_classes)
    return out


def tensor_slices(n_classes):
    """name -> slice of the flat blob, the 54 trainable tensors in blob order."""
    out = {}
    pos = 0
    for name, k, cin, cout, _, _ in conv_shapes(n_classes):
        out[name + '/kernel'] = slice(pos, pos + k * cin * cout)
        pos += k * cin * cout
        out[name + '/bias'] = slice(pos, pos + cout)
        pos += cout
    moving = []
    for i, c in enumerate(BN_CHANNELS, start=1):
        out['bn_%d/gamma' % i] = slice(pos, pos + c)
        out['bn_%d/beta' % i] = slice(pos + c, pos + 2 * c)
        moving.append(slice(pos + 2 * c, pos + 4 * c))
        pos += 4 * c
    assert pos == param_count(n_classes) and len(out) == 54
    return out, moving
