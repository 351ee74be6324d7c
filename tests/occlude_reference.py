"""A helper, not a test: the contract of ``locate --occlude`` (include/deepbinner_hip.h, "occlude")
restated in NumPy, as simply as it can be said - the scanned region, the plan as a plain function of
one location, the blanking as a mask over read samples - on top of ``locate_reference`` and the
oracle's network; the geometries, read lengths and planted locations it is tested on; the fp64 route
of one case; and a host stand-in for the command's backend."""
import functools

import numpy as np

import locate_reference as loc_ref

OUT, ONLY, CTRL = 0, 1, 2
VARIANTS = ('out', 'only', 'ctrl')
PLAN = np.dtype([('first', np.int64, 3), ('end', np.int64, 3), ('invert', np.int32),
                 ('valid', np.int32), ('reserved', np.int64)])
OCCLUSION = np.dtype([('cls', np.int32), ('p', np.float32)] +
                     [(v + field, kind) for v in VARIANTS
                      for field, kind in (('_call', np.int32), ('_p', np.float32))] +
                     [('ctrl_first', np.int64), ('ctrl_end', np.int64), ('reserved', np.int64, 2)])


def scanned(n, steps, input_size, side):
    """R: the read samples the side's windows cover."""
    reach = (steps - 1) * (input_size // 2) + input_size
    return (0, min(n, reach)) if side == 'start' else (max(0, n - reach), n)


def origin(n, s, input_size, side):
    return s * (input_size // 2) if side == 'start' else n - s * (input_size // 2) - input_size


def no_result(cls=0):
    occ = np.zeros((), dtype=OCCLUSION)
    occ['cls'], occ['p'] = cls, np.nan
    for v in VARIANTS:
        occ[v + '_call'], occ[v + '_p'] = -1, np.nan
    occ['ctrl_first'] = occ['ctrl_end'] = -1
    return occ


def plan_read(location, n, steps, input_size, side):
    """One location and the read's length -> (PLAN record, OCCLUSION record with nothing but cls
    and the control samples filled in)."""
    plan = np.zeros((), dtype=PLAN)
    cls = max(int(location['cls']), 0)
    occ = no_result(cls)
    lo, hi = scanned(n, steps, input_size, side)
    first, end = max(int(location['first_sample']), lo), min(int(location['end_sample']), hi)
    m = end - first
    if cls > 0 and m > 0:
        plan['first'][[OUT, ONLY]], plan['end'][[OUT, ONLY]] = first, end
        plan['invert'], plan['valid'] = 1 << ONLY, (1 << OUT) | (1 << ONLY)
        c_first = hi - m if first + end < lo + hi else lo
        if c_first + m <= first or c_first >= end:
            plan['first'][CTRL], plan['end'][CTRL] = c_first, c_first + m
            occ['ctrl_first'], occ['ctrl_end'] = c_first, c_first + m
            plan['valid'] |= 1 << CTRL
    return plan, occ


def plan(locations, lengths, steps, input_size, side):
    plans = np.zeros(len(locations), dtype=PLAN)
    occlusions = np.zeros(len(locations), dtype=OCCLUSION)
    for r in range(len(locations)):
        p, o = plan_read(locations[r], int(lengths[r]), steps, input_size, side)
        plans[r], occlusions[r] = p[()], o[()]
    return plans, occlusions


def blank_mask(one_plan, v, n, steps, input_size, side):
    """bool [steps, L]: the window positions variant v stores as 0."""
    mask = np.zeros((steps, input_size), dtype=bool)
    for s in range(steps):
        t = origin(n, s, input_size, side) + np.arange(input_size)
        inside = (t >= one_plan['first'][v]) & (t < one_plan['end'][v])
        if (int(one_plan['invert']) >> v) & 1:
            inside = ~inside
        mask[s] = inside & (t >= 0) & (t < n)
    return mask


def blank(x, lengths, plans, side):
    """x [N, steps, L] -> [3, N, steps, L] in x's type: copies, and zeros where blanked."""
    x = np.asarray(x)
    out = np.stack([x, x, x]).copy()
    n_reads, steps, input_size = x.shape
    for r in range(n_reads):
        for v in range(3):
            out[v, r][blank_mask(plans[r], v, int(lengths[r]), steps, input_size, side)] = 0
    return out


# ---- the shapes the kernels are tested on --------------------------------------------------------------
# (input size, steps, reads): 98 has a scalar head or tail in every window of the 16-byte path, and
# with an odd count of windows variants whose rows are aligned unlike the input's; 160 is one cell
# with 32 positions in none
GEOMETRIES = [(96, 1, 1), (96, 2, 65), (98, 1, 65), (98, 2, 64), (98, 12, 1), (160, 12, 64),
              (160, 1, 65), (1024, 2, 65), (1024, 12, 64), (1024, 1, 1)]


def lengths_for(input_size, steps, n_reads, rng):
    """Shorter than a window, exactly L, L + h - 1, L + h, long - then random ones."""
    L, h = input_size, input_size // 2
    fixed = [L // 3, L, L + h - 1, L + h, steps * h + 3 * L + 7, 1, L - 1, 0]
    more = rng.integers(0, (steps + 3) * h + 2 * L, max(n_reads - len(fixed), 0))
    return np.concatenate([fixed, more])[:n_reads].astype(np.int64)


def location_of(cls, first, end):
    out = loc_ref.no_location()
    if cls > 0:
        out['cls'], out['window'], out['peak_cell'] = cls, 0, 0
        out['first_cell'] = out['last_cell'] = 0
        out['peak'], out['share'] = 1, 1
        out['first_sample'], out['end_sample'] = first, end
    return out


def random_case(input_size, steps, n_reads, side, seed):
    """-> (x float32 [N, steps, L] with zeros where a window has no sample, lengths, locations): the
    planted spans in turn, read by read."""
    rng = np.random.default_rng(seed)
    lengths = lengths_for(input_size, steps, n_reads, rng)
    x = rng.standard_normal((n_reads, steps, input_size)).astype(np.float32)
    x[np.abs(x) < 0.05] = -0.0                          # (a value that is zero already, signed)
    locations = []
    for r in range(n_reads):
        n = int(lengths[r])
        lo, hi = scanned(n, steps, input_size, side)
        for s in range(steps):
            t = origin(n, s, input_size, side) + np.arange(input_size)
            x[r, s][(t < 0) | (t >= n)] = 0
        size = hi - lo
        kind = r % 10
        m = int(rng.integers(1, max(size // 3, 2)))
        if kind == 0 or size == 0:
            locations.append(location_of(0 if kind == 0 else 3, lo, lo))      # no call; m == 0
        elif kind == 1:
            locations.append(location_of(1, lo, min(lo + m, hi)))            # at R's first sample
        elif kind == 2:
            locations.append(location_of(2, max(hi - m, lo), hi))            # at R's last sample
        elif kind == 3:
            locations.append(location_of(3, lo, hi))                         # all of R
        elif kind == 4:                                                      # midpoint on R's
            d = int(rng.integers(0, max(size // 2, 1)))
            locations.append(location_of(4, lo + d, hi - d))
        elif kind == 5:                                                      # control touches
            m = max(size // 2, 1)
            locations.append(location_of(5, lo, lo + m))
        elif kind == 6:                                                      # ... overlaps by one
            m = size // 2 + 1
            locations.append(location_of(6, lo, min(lo + m, hi)))
        elif kind == 7:                                                      # empty after clipping
            locations.append(location_of(7, lo, lo))
        elif kind == 8:                                                      # reaches out of R
            locations.append(location_of(8, lo - 5, hi + 5 if m % 2 else min(lo + m, hi)))
        else:
            first = int(rng.integers(lo, hi))
            locations.append(location_of(int(rng.integers(1, 13)), first,
                                         int(rng.integers(first, hi + 1))))
    return x, lengths, np.array(locations, dtype=loc_ref.LOCATION)


# ---- the whole route in fp64 -------------------------------------------------------------------------
def route_reads(input_size, steps, n_reads=32, seed=0):
    """The seven golden reads cut to differing lengths, then noise reads: shorter than a window,
    exactly L, L + h - 1, L + h, and long."""
    from general_fixtures import golden_signals
    rng = np.random.default_rng([seed, input_size])
    L, h = input_size, input_size // 2
    reads = [np.asarray(s[:(steps + 2) * h + 13 * i], dtype=np.int16)
             for i, s in enumerate(golden_signals())]
    reads += [np.asarray(s[-((steps + 1) * h + 7 * i):], dtype=np.int16)
              for i, s in enumerate(golden_signals())]
    lengths = [L // 3, L, L + h - 1, L + h] + list(rng.integers(L, (steps + 3) * h + L, n_reads))
    for n in lengths[:n_reads - len(reads)]:
        base = rng.normal(500, 80, int(n))
        bump = 150 * np.sin(np.arange(int(n)) / rng.uniform(3, 40))
        reads.append(np.clip(base + bump, -32768, 32767).astype(np.int16))
    return reads


# (input size, classes, model, steps, score_diff): every pair of L in {96, 160, 1024} and C in
# {2, 13}, each with the shipped start model bent to the geometry and channel-flipped
# (weight_families.flipped: few calls, of several classes) and with one random model
# (weight_families.random_model: many calls, mostly of one class).  The small sizes take twelve
# steps - with two their one-cell span is all of R and there is no control - the shipped size two.
# Seeds and score_diff chosen so that some reads are called and the fp64 oracle alone has fewer than
# 1 read in 20 within 1e-4 of a threshold (test_occlude.py asserts both).
ROUTE_CASES = [(96, 2, 'flipped', 12, 0.5), (96, 2, 'random-2', 12, 0.5),
               (96, 13, 'flipped', 12, 0.1), (96, 13, 'random-0', 12, 0.1),
               (160, 2, 'flipped', 12, 0.5), (160, 2, 'random-0', 12, 0.5),
               (160, 13, 'flipped', 12, 0.1), (160, 13, 'random-1', 12, 0.5),
               (1024, 2, 'flipped', 2, 0.5), (1024, 2, 'random-1', 2, 0.5),
               (1024, 13, 'flipped', 2, 0.5), (1024, 13, 'random-1', 2, 0.5)]


def route_model(input_size, n_classes, model):
    from general_fixtures import geometry
    from weight_families import flipped, random_model
    if model == 'flipped':
        return flipped(geometry(input_size, n_classes), input_size + n_classes)
    return random_model(int(model.split('-')[1]), n_classes, input_size=input_size)


def merged_call(window_probs, score_diff):
    """window probs [N, steps, C] -> (probs float64 [N, C], calls int [N], lead over score_diff of
    the best class [N])."""
    from oracle import classify_ref
    merged = classify_ref.merge_steps(np.asarray(window_probs).transpose(1, 0, 2))
    probs = np.array([classify_ref.make_sum_to_one(p) for p in merged])
    names = [classify_ref.barcode_call(p, score_diff) for p in probs]
    calls = np.array([0 if c == 'none' else int(c) for c in names], dtype=np.int32)
    top = np.sort(probs, axis=1)[:, ::-1]
    return probs, calls, top[:, 0] - top[:, 1] - score_diff


def variant_results(weights, signals, locations, side, scan_size, score_diff, dtype=np.float64):
    """The rule from given locations on: -> (occlusions OCCLUSION [N] with everything but p filled
    in, variant probs [3, N, C], lead [3, N]) with the oracle's forward in ``dtype``."""
    from oracle import classify_ref, network_ref
    L = weights.input_size
    steps = scan_size // (L // 2)
    lengths = np.array([len(s) for s in signals], dtype=np.int64)
    x = classify_ref.make_windows(signals, L, scan_size, side).transpose(1, 0, 2).astype(np.float32)
    plans, occlusions = plan(locations, lengths, steps, L, side)
    variants = blank(x, lengths, plans, side)
    probs = network_ref.forward(weights, variants.reshape(-1, L), dtype=np.dtype(dtype).type)
    probs = np.asarray(probs).reshape(3, len(signals), steps, -1)
    all_probs, leads = [], []
    for v, name in enumerate(VARIANTS):
        v_probs, v_calls, lead = merged_call(probs[v], score_diff)
        all_probs.append(v_probs)
        leads.append(lead)
        for r in range(len(signals)):
            if (int(plans[r]['valid']) >> v) & 1:
                occlusions[r][name + '_call'] = v_calls[r]
                occlusions[r][name + '_p'] = v_probs[r, occlusions[r]['cls']]
    return occlusions, np.array(all_probs), np.array(leads)


@functools.lru_cache(maxsize=None)
def oracle_route(input_size, n_classes, model, steps, score_diff, side):
    """One case of the fp64 route from the oracle's own evidence on, computed once: (signals, calls,
    locations, occlusions, variant probs [3, N, C], leads [3, N])."""
    weights = route_model(input_size, n_classes, model)
    signals = route_reads(input_size, steps)
    scan = steps * (input_size // 2)
    wprobs, ev = loc_ref.read_evidence(weights, signals, scan, side)
    probs, calls, _ = merged_call(wprobs, score_diff)
    lengths = [len(s) for s in signals]
    locations = loc_ref.locate(ev, calls, lengths, input_size, side)
    occlusions, v_probs, leads = variant_results(weights, signals, locations, side, scan, score_diff)
    for r in range(len(signals)):
        if calls[r] > 0:
            occlusions[r]['p'] = probs[r, calls[r]]
    return signals, calls, locations, occlusions, v_probs, leads


# ---- the command's backend on the host ---------------------------------------------------------------
class HostBackend(loc_ref.HostBackend):
    """``locate_reference.HostBackend`` with ``locate_occluded_packed``: the variants through the
    oracle's network in fp32."""

    def __init__(self):
        super().__init__()
        self.occluded = 0

    def locate_occluded_packed(self, model, samples, offsets, side, scan_size, score_diff):
        probs, calls, locations = self.locate_packed(model, samples, offsets, side, scan_size,
                                                     score_diff)
        self.occluded += 1
        signals = [samples[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
        occlusions, _, _ = variant_results(model.weights, signals, locations, side, scan_size,
                                           score_diff, dtype=np.float32)
        for r in range(len(signals)):
            if calls[r] > 0:
                occlusions[r]['p'] = probs[r, calls[r]]
        return probs, calls, locations, occlusions
