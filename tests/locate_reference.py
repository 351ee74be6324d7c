"""A helper, not a test: the contract of ``locate`` (include/deepbinner_hip.h, "locate") restated in
NumPy, as simply as it can be said - the evidence from the oracle's stage G, the rule as a plain
loop over reads, the margins below which a rounding may change an integer - the synthetic evidence
arrays and planted cases the rule is tested on, and a host stand-in for the command's backend
(``HostBackend``), which drives a model that only has ``predict`` and ``weights`` - the oracle of the
conftest - through ``classify``'s windows."""
import numpy as np

from deepbinner_amd.model_format import conv_shapes

LOCATION = np.dtype([('cls', np.int32), ('window', np.int32), ('peak_cell', np.int32),
                     ('first_cell', np.int32), ('last_cell', np.int32), ('peak', np.float32),
                     ('share', np.float32), ('reserved', np.int32), ('first_sample', np.int64),
                     ('end_sample', np.int64)])
INTEGERS = ('cls', 'window', 'peak_cell', 'first_cell', 'last_cell', 'first_sample', 'end_sample')
CELL = 128


def cells_of(input_size):
    """len7: the positions of the last stage (dbh_network.h: stage_lengths)."""
    n = (input_size + 1) // 2
    for _ in range(4):
        n //= 2
    return ((n + 1) // 2) // 2


def evidence(weights, windows, dtype=np.float64):
    """windows [N, L] -> (probs [N, C], evidence [N, cells, C], the oracle's own logits [N, C]):
    conv1d_20 + ReLU on the oracle's stage G (which holds BN7's output), before the global average."""
    from oracle import network_ref
    dtype = np.dtype(dtype).type
    probs, stages = network_ref.forward(weights, np.asarray(windows, dtype=np.float32), dtype=dtype,
                                        return_stages=True)
    kernel, bias = weights.convs[19]
    _, _, _, _, stride, padding = conv_shapes(weights.n_classes)[19]
    e = network_ref.relu(network_ref.conv1d(stages['G'], kernel.astype(dtype), bias.astype(dtype),
                                            stride, padding))
    return probs, e, stages['logits']


def read_evidence(weights, signals, scan_size, side, dtype=np.float64):
    """Reads -> (window probs [N, steps, C], evidence [N, steps, cells, C]) over ``classify``'s own
    windows, laid out [read][step]."""
    from oracle import classify_ref
    size = weights.input_size
    windows = classify_ref.make_windows(signals, size, scan_size, side)      # [steps, N, L]
    steps, n, _ = windows.shape
    probs, e, _ = evidence(weights, windows.reshape(-1, size), dtype)
    return (probs.reshape(steps, n, -1).transpose(1, 0, 2),
            e.reshape(steps, n, e.shape[1], e.shape[2]).transpose(1, 0, 2, 3))


def no_location():
    out = np.zeros((), dtype=LOCATION)
    for name in INTEGERS[1:]:
        out[name] = -1
    return out


def pick(e):
    """e [steps, cells] of the called class -> (flat index, peak): the highest value that is not
    below zero and no NaN, the lowest flat index among equals; nothing to take: (0, 0)."""
    flat = np.asarray(e).ravel()
    with np.errstate(invalid='ignore'):
        ok = flat >= 0
    if not ok.any():
        return 0, flat.dtype.type(0)
    top = flat[ok].max()
    i = int(np.flatnonzero(ok & (flat == top))[0])
    return i, flat[i]


def span(row, p, peak):
    """The longest run of cells around p with row >= half the peak, compared in the row's type."""
    half = row.dtype.type(0.5) * row.dtype.type(peak)
    first = last = p
    with np.errstate(invalid='ignore'):
        while first > 0 and row[first - 1] >= half:
            first -= 1
        while last + 1 < len(row) and row[last + 1] >= half:
            last += 1
    return first, last


def samples_of(side, window, first, last, n, input_size):
    """[first sample, end sample) of cells first .. last of window ``window`` of a read of n samples."""
    half = input_size // 2
    o = window * half if side == 'start' else n - window * half - input_size
    lo = min(max(o + CELL * first, 0), n)
    hi = min(max(o + min(CELL * (last + 1), input_size), 0), n)
    return lo, max(hi, lo)


def locate_read(ev, c, n, input_size, side):
    """ev [steps, cells, C], the side's call c, n samples -> a LOCATION record."""
    out = no_location()
    if not 0 < c < ev.shape[2]:
        return out
    e = ev[:, :, c]
    cells = e.shape[1]
    i, peak = pick(e)
    s, p = divmod(i, cells)
    first, last = span(e[s], p, peak)
    sums = np.cumsum(e[s].astype(np.float64))                 # (sequential: cell order)
    part = np.cumsum(e[s, first:last + 1].astype(np.float64))[-1]
    out['cls'], out['window'], out['peak_cell'] = c, s, p
    out['first_cell'], out['last_cell'] = first, last
    out['peak'] = peak
    with np.errstate(invalid='ignore'):
        out['share'] = 0 if sums[-1] == 0 else np.float32(part / sums[-1])
    out['first_sample'], out['end_sample'] = samples_of(side, s, first, last, int(n), input_size)
    return out


def locate(ev, calls, lengths, input_size, side):
    """ev [N, steps, cells, C] -> LOCATION [N]."""
    return np.array([locate_read(ev[r], int(calls[r]), int(lengths[r]), input_size, side)
                     for r in range(len(calls))], dtype=LOCATION)


def margins(ev, c):
    """The three margins of a read's fp64 evidence below which a rounding may change an integer of
    its location: best against second window peak, the peak against the next cell of its window, and
    any other cell of that window against half the peak."""
    e = np.asarray(ev, dtype=np.float64)[:, :, c]
    i, peak = pick(e)
    s, p = divmod(i, e.shape[1])
    peaks = np.sort(e.max(axis=1))
    others = np.delete(e[s], p)
    return (peaks[-1] - peaks[-2] if len(peaks) > 1 else np.inf,
            peak - others.max() if len(others) else np.inf,
            np.abs(others - 0.5 * peak).min() if len(others) else np.inf)


# ---- synthetic evidence for the rule ------------------------------------------------------------------
def lengths_for(input_size, scan_size, n_reads, rng):
    """The read lengths of general_fixtures.synthetic_reads, then random ones."""
    L = input_size
    fixed = [0, 1, L // 3, L - 1, L, L + 17, scan_size + L // 2, 2 * scan_size + L + 5]
    more = rng.integers(0, 3 * scan_size + 2 * L, max(n_reads - len(fixed), 0))
    return np.concatenate([fixed, more])[:n_reads].astype(np.int64)


def random_case(cells, steps, n_classes, n_reads, seed):
    """-> (evidence float32 [n_reads, steps, cells, C], calls, lengths, input_size): mostly zeros
    with bumps a few cells wide - a peak, shoulders at exact binary fractions of it so that the
    half-height edge and ties are hit often - and calls 0, 1 and C - 1."""
    rng = np.random.default_rng(seed)
    input_size = CELL * cells if cells > 1 else 96
    ev = np.zeros((n_reads, steps, cells, n_classes), dtype=np.float32)
    ev += (rng.random(ev.shape) < 0.3) * rng.choice([0.125, 0.25, 0.5], ev.shape).astype(np.float32)
    calls = rng.choice([0, 1, n_classes - 1], n_reads).astype(np.int32)
    calls[:3] = (0, 1, n_classes - 1)[:n_reads]
    for r in range(n_reads):
        for c in {1, n_classes - 1}:
            for _ in range(int(rng.integers(0, 4))):
                s, p = int(rng.integers(steps)), int(rng.integers(cells))
                top = float(rng.choice([1.0, 2.0, 2.0, 3.0]))
                ev[r, s, p, c] = top
                for q in range(max(p - 2, 0), min(p + 3, cells)):
                    if q != p:
                        ev[r, s, q, c] = top * float(rng.choice([0.25, 0.5, 0.75, 1.0]))
    return ev, calls, lengths_for(input_size, steps * (input_size // 2), n_reads, rng), input_size


# (cells, steps, classes, reads): every value of the contract's lists in at least one case, the
# large ones not multiplied with each other - 128 cells x 24 steps x 256 classes x 1,000 reads
# would be 3 GB
RANDOM_CASES = [(1, 1, 2, 1), (2, 2, 13, 64), (8, 12, 13, 65), (63, 24, 13, 65), (64, 2, 256, 64),
                (65, 12, 2, 65), (128, 24, 13, 64), (8, 12, 13, 1000), (128, 1, 256, 8),
                (1, 24, 256, 65)]


def planted_cases():
    """[(name, evidence [1, steps, cells, C], call, length, input_size, side, want)], want = (window,
    peak cell, first cell, last cell, first sample, end sample)."""
    cases = []

    def add(name, steps, cells, n_classes, input_size, side, c, n, values, want):
        ev = np.zeros((1, steps, cells, n_classes), dtype=np.float32)
        for (s, p), v in values.items():
            ev[0, s, p, c] = v
        cases.append((name, ev, c, n, input_size, side, want))

    below = np.nextafter(np.float32(1.5), np.float32(0))
    add('equal peaks in two windows and two cells', 3, 8, 13, 1024, 'start', 5, 5000,
        {(2, 6): 4, (1, 3): 4, (1, 5): 4}, (1, 3, 3, 3, 896, 1024))
    add('half height inside, one ulp below outside', 2, 8, 2, 1024, 'start', 1, 5000,
        {(0, 4): 3, (0, 3): 1.5, (0, 5): below}, (0, 4, 3, 4, 384, 640))
    add('peak in the first cell', 1, 8, 256, 1024, 'start', 255, 4000, {(0, 0): 1},
        (0, 0, 0, 0, 0, 128))
    add('peak in the last cell', 1, 8, 256, 1024, 'start', 255, 4000, {(0, 7): 1},
        (0, 7, 7, 7, 896, 1024))
    add('span of the whole window, L = 1000', 2, 8, 13, 1000, 'start', 12, 3000,
        {(1, p): 1 + 0.125 * p for p in range(8)}, (1, 7, 0, 7, 500, 1500))
    add('all zero', 12, 63, 13, 8064, 'start', 3, 100000, {}, (0, 0, 0, 62, 0, 8064))
    add('end side, span partly in the padding', 1, 8, 13, 1024, 'end', 2, 300, {(0, 5): 1},
        (0, 5, 5, 5, 0, 44))
    add('end side, span wholly in the padding', 1, 8, 13, 1024, 'end', 2, 300, {(0, 2): 1},
        (0, 2, 2, 2, 0, 0))
    add('end side, second window', 2, 8, 13, 1024, 'end', 2, 4971, {(1, 4): 1, (1, 5): 0.75},
        (1, 4, 4, 5, 3947, 4203))
    add('start side, behind the read', 2, 8, 13, 1024, 'start', 2, 300, {(1, 6): 1},
        (1, 6, 6, 6, 300, 300))
    add('one cell that stops at 128 of 160', 1, 1, 4, 160, 'start', 3, 1000, {(0, 0): 2},
        (0, 0, 0, 0, 0, 128))
    return cases


# ---- the command's backend on the host ---------------------------------------------------------------
class HostBackend:
    """What ``locate.locate`` asks of ``hip_backend`` - ``general_model`` and ``locate_packed`` - on
    the host, for models with ``weights`` (the conftest's OracleModel), in fp32 as the device."""

    def __init__(self):
        self.batches = 0

    @staticmethod
    def general_model(model):
        return model

    def locate_packed(self, model, samples, offsets, side, scan_size, score_diff):
        from oracle import classify_ref
        self.batches += 1
        signals = [samples[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
        weights = model.weights
        wprobs, ev = read_evidence(weights, signals, scan_size, side, dtype=np.float32)
        merged = classify_ref.merge_steps(wprobs.transpose(1, 0, 2).astype(np.float32))
        probs = np.array([classify_ref.make_sum_to_one(p) for p in merged])
        names = [classify_ref.barcode_call(p, score_diff) for p in probs]
        calls = np.array([0 if c == 'none' else int(c) for c in names], dtype=np.int32)
        return (probs.astype(np.float32), calls,
                locate(ev.astype(np.float32), calls, np.diff(offsets), weights.input_size, side))
