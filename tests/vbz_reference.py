"""
A reference for the streamvbyte + zigzag + delta stage of VBZ ("VBZ") and the streams
the GPU decoder (deepbinner_amd/csrc/dbh_vbz.hip) is held to it on.  No GPU, no ctypes.

``decode`` / ``expected`` restate fast5_codecs.h's ``vbz_unpack`` with the header rules the
kernel states and the cut / zero-extension contract of include/deepbinner_hip.h;
``decode_plain`` is the same thing one value at a time, in plain Python integers, and the CPU
tests hold the two (and both host decoders) to each other.

The case families (all seeded, nothing read from a file): ``codes_cases``, ``unwrapped_cases``,
``padding_cases``, ``shape_cases``, ``mutant_cases``; ``loop_cases`` is the batch of the launch
that loops.  ``census`` counts, on the reference alone, what the streams exercise.
"""

import struct
from types import SimpleNamespace

import numpy as np

import vbz_fixtures as vf

LANE = 16                     # values per lane and step of the kernel
STEP = 64 * LANE              # values per step of a wavefront


# ---- the reference ------------------------------------------------------------------------------
def header(payload):
    """(n values, control bytes) of a stream whose header checks pass, else None: fewer than 4
    bytes, an odd original_size, control bytes beyond the stream."""
    if len(payload) < 4:
        return None
    size = struct.unpack_from('<I', payload)[0]
    if size & 1:
        return None
    n = size // 2
    ctrl = (n + 3) // 4
    if ctrl > len(payload) - 4:
        return None
    return n, ctrl


def code_lengths(payload):
    """bytes each value takes (1..4), from the control bytes; None if the header checks fail"""
    head = header(payload)
    if head is None:
        return None
    n, ctrl = head
    c = np.frombuffer(payload, dtype=np.uint8, count=ctrl, offset=4)
    codes = (c[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3
    return codes.reshape(-1)[:n].astype(np.int64) + 1


def decode(payload):
    """u32 LE original_size + streamvbyte bytes -> int16 samples, or None for a stream the
    decoders refuse: the header rules, and data bytes that do not end exactly at the stream's end.
    Sum modulo 2^32, truncated to int16."""
    payload = bytes(payload)
    lengths = code_lengths(payload)
    if lengths is None:
        return None
    n = len(lengths)
    data = np.frombuffer(payload, dtype=np.uint8, offset=4 + (n + 3) // 4)
    if int(lengths.sum()) != len(data):
        return None
    at = np.cumsum(lengths) - lengths
    padded = np.concatenate([data, np.zeros(3, dtype=np.uint8)]).astype(np.uint64)
    u = np.zeros(n, dtype=np.uint64)
    for k in range(4):
        u |= np.where(lengths > k, padded[at + k], np.uint64(0)) << np.uint64(8 * k)
    delta = (u >> np.uint64(1)) ^ (np.uint64(0xFFFFFFFF) * (u & np.uint64(1)))
    total = np.cumsum(delta, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    return (total & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16)


def decode_plain(payload):
    """``decode`` as vbz_unpack has it: one value after the other, Python integers"""
    payload = bytes(payload)
    head = header(payload)
    if head is None:
        return None
    n, ctrl = head
    d, end, prev = 4 + ctrl, len(payload), 0
    out = np.zeros(n, dtype=np.uint16)
    for i in range(n):
        length = ((payload[4 + (i >> 2)] >> ((i & 3) * 2)) & 3) + 1
        if end - d < length:
            return None
        u = int.from_bytes(payload[d:d + length], 'little')
        d += length
        prev = (prev + ((u >> 1) ^ (0xFFFFFFFF if u & 1 else 0))) & 0xFFFFFFFF
        out[i] = prev & 0xFFFF
    return out.view(np.int16) if d == end else None


def expected(payload, out_bytes):
    """(status is zero, int16[out_bytes // 2]): the samples cut to ``out_bytes`` or zero-extended
    to it; all zeros for a refused stream"""
    out = np.zeros(out_bytes // 2, dtype=np.int16)
    samples = decode(payload)
    if samples is None:
        return False, out
    m = min(len(samples), len(out))
    out[:m] = samples[:m]
    return True, out


# ---- streams ------------------------------------------------------------------------------------
def case(family, name, payload, out_bytes, **more):
    """One stream for the decoder: ``align`` (None, or the residue of out_offset modulo 16 it is to
    get), ``origin`` (a mutant's valid stream), ``unwrapped`` (encoded from samples with 32-bit
    deltas, nothing forced), ``twin`` (payload of the other encoding of the same samples)."""
    fields = dict(align=None, origin=None, unwrapped=False, twin=None, samples=None)
    fields.update(more)
    return SimpleNamespace(family=family, name=name, payload=bytes(payload), out_bytes=int(out_bytes),
                           **fields)


def any_values(rng, n):
    """uint32 values uniform in bit length 0..32 (bit 31 is set in about 3 %)"""
    bits = rng.integers(0, 33, n)
    top = np.where(bits > 0, np.uint64(1) << np.maximum(bits - 1, 0).astype(np.uint64), np.uint64(0))
    low = rng.integers(0, 1 << 32, n, dtype=np.uint64) & (np.maximum(top, np.uint64(1)) - np.uint64(1))
    return (top | low).astype(np.uint32)


def stream_of(u, lengths=None):
    return struct.pack('<I', 2 * len(u)) + vf.pack_values(u, lengths)


def mixed_stream(rng, n):
    """n values over the whole range, their codes forced at random to 1..4 bytes"""
    return stream_of(any_values(rng, n), rng.integers(1, 5, n))


CODE_COUNTS = ([0] + list(range(1, 18)) + [63, 64, 65, 1007, 1008, 1009, 1023, 1024, 1025, 1039, 1040,
                                           1041, 2047, 2048, 2049] +
               [16 * k + d for k in (5, 37, 100, 333) for d in (-1, 0, 1)] +
               [1024 * k + d for k in (3, 5, 9) for d in (-1, 1)])
LONG_READ = 1500000


def long_read_stream():
    """1,500,000 values (1,465 steps), every code, the sum wrapping many times"""
    return mixed_stream(np.random.default_rng(1500000), LONG_READ)


def codes_cases(long_read=True):
    rng = np.random.default_rng(32020)
    cases = []
    for n in CODE_COUNTS:
        cases.append(case('codes', 'mixed_n%d' % n, mixed_stream(rng, n), 2 * n))
    # one code only: 16 / 32 / 48 / 64 data bytes in every lane, 4,096 in a step of 4-byte codes;
    # 15 and 1,039 values end in a partial lane of 15 values, each of them this code
    for length in (1, 2, 3, 4):
        for n in (15, 16, 1039, 2049, 3000):
            u = rng.integers(0, 256, n).astype(np.uint32) << np.uint32(8 * (length - 1))
            u |= rng.integers(0, 256, n).astype(np.uint32)
            cases.append(case('codes', 'only%d_n%d' % (length, n),
                              stream_of(u, np.full(n, length)), 2 * n))
    if long_read:
        cases.append(case('codes', 'long_read', long_read_stream(), 2 * LONG_READ))
    return cases


def unwrapped_cases():
    """full-range int16 signals through the encoder that takes deltas in 32 bits (3-byte codes
    arise by themselves) and, as twins, through the one that wraps them to int16"""
    rng = np.random.default_rng(65536)
    signals = {'random_n%d' % n: rng.integers(-32768, 32768, n).astype(np.int16)
               for n in (7, 1025, 5000, 40000)}
    signals['jumps'] = np.array([-32768, 32767] * 1500 + [0, -32768, 32767, -1], dtype=np.int16)
    cases = []
    for name, samples in sorted(signals.items()):
        size = struct.pack('<I', 2 * len(samples))
        wide, narrow = size + vf.streamvbyte(samples, wrap=False), size + vf.streamvbyte(samples)
        cases.append(case('unwrapped', name + '_32bit', wide, 2 * len(samples), unwrapped=True,
                          twin=narrow, samples=samples))
        cases.append(case('unwrapped', name + '_wrapped', narrow, 2 * len(samples), twin=wide,
                          samples=samples))
    return cases


def padding_cases():
    """n % 4 != 0 (over every such residue modulo 16): the 2-bit fields of the last control byte
    behind the last value set to every non-zero pattern - accepted, same samples"""
    rng = np.random.default_rng(3)
    cases = []
    for base in (0, 64, 1024, 2160):
        for r in (1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15):
            n = base + r
            clean = bytearray(mixed_stream(rng, n))
            last = 4 + (n + 3) // 4 - 1
            used = 2 * (n % 4)
            patterns = range(1, 1 << (8 - used)) if base < 2160 else [(1 << (8 - used)) - 1]
            for p in patterns:
                dirty = bytearray(clean)
                dirty[last] |= p << used
                cases.append(case('padding', 'n%d_bits%d' % (n, p), dirty, 2 * n, twin=bytes(clean)))
    return cases


SHAPE_COUNTS = (3072, 3109)


def shape_cases():
    """streams of three steps and more, cut and zero-extended at every seam of the store paths,
    at every even residue of out_offset modulo 16"""
    rng = np.random.default_rng(16)
    cases = []
    for n in SHAPE_COUNTS:
        payload = mixed_stream(rng, n)
        wanted = [0, 2, 30, 32, 34, 2 * 517, 2 * 1023, 2 * 1024, 2 * 1025, 2 * 2047, 2 * 2048,
                  2 * 2049, 2 * (n - 3), 2 * n, 2 * n + 2, 2 * n + 4096]
        for out_bytes in wanted:
            for align in range(0, 16, 2):
                cases.append(case('shapes', 'n%d_out%d_at%d' % (n, out_bytes, align), payload,
                                  out_bytes, align=align))
    return cases


MUTANT_COUNTS = (5, 300, 1025, 2500, 5000)


def set_code(stream, i, code):
    at = 4 + (i >> 2)
    stream[at] = (stream[at] & ~(3 << ((i & 3) * 2))) | (code << ((i & 3) * 2))


def mutant_cases(seeds=4):
    """damaged copies of valid streams: the kinds of damage DESIGN.md's self-checks are for, and
    the kinds that leave a valid stream with other samples"""
    rng = np.random.default_rng(404)
    cases = []
    for n in MUTANT_COUNTS:
        for seed in range(seeds):
            good = mixed_stream(rng, n)
            codes = code_lengths(good) - 1
            ctrl = (n + 3) // 4
            mutants = []
            for k in range(1, 9):
                mutants.append(('cut%d' % k, good[:-k]))
                mutants.append(('long%d' % k, good + rng.integers(0, 256, k, dtype=np.uint8).tobytes()))
            for d in (-8, -2, -1, 1, 2, 8, 4096):
                mutants.append(('size%+d' % d, struct.pack('<I', 2 * n + d) + good[4:]))
            for k in range(10):
                m = bytearray(good)
                i = int(rng.integers(0, n))
                set_code(m, i, int((codes[i] + rng.integers(1, 4)) % 4))
                mutants.append(('code%d' % k, m))
                m = bytearray(good)                    # one code longer, another as much shorter
                i = int(rng.choice(np.nonzero(codes < 3)[0]))
                room = np.nonzero((codes > 0) & (np.arange(n) != i))[0]
                j = int(rng.choice(room))
                d = int(rng.integers(1, min(3 - codes[i], codes[j]) + 1))
                set_code(m, i, int(codes[i]) + d)
                set_code(m, j, int(codes[j]) - d)
                mutants.append(('codes%d' % k, m))
                m = bytearray(good)
                m[int(rng.integers(4 + ctrl, len(good)))] ^= 1 << int(rng.integers(0, 8))
                mutants.append(('bit%d' % k, m))
            for kind, m in mutants:
                cases.append(case('mutants', 'n%d_%d_%s' % (n, seed, kind), m, 2 * n, origin=good))
    return cases


def all_cases(long_read=True):
    return (codes_cases(long_read) + unwrapped_cases() + padding_cases() + shape_cases() +
            mutant_cases())


LOOP_STREAMS = 40000


def loop_cases():
    """40,000 streams of 1..64 values, mixed codes, every hundredth one a refused mutant (its last
    data byte cut off): more than the 32,768 streams one trip of the kernel's stream loop takes"""
    rng = np.random.default_rng(8192)
    cases = []
    for k in range(LOOP_STREAMS):
        n = int(rng.integers(1, 65))
        payload = mixed_stream(rng, n)
        if k % 100 == 99:
            cases.append(case('loop', 'k%d_cut' % k, payload[:-1], 2 * n, origin=payload))
        else:
            cases.append(case('loop', 'k%d' % k, payload, 2 * n))
    return cases


# ---- what a list of cases exercises -------------------------------------------------------------
def census(cases):
    """Counted on the reference alone.  Codes, lanes and steps are those of streams the reference
    accepts (a decoder goes through all of them); distinct payloads are counted once."""
    out = SimpleNamespace(
        streams=len(cases), accepted=0, refused=0,
        codes=[0, 0, 0, 0],                # values by code length 1..4
        unwrapped_three_byte=0,            # 3-byte codes the 32-bit encoder made by itself
        full_lane=set(), partial_lane=set(), last_code=set(),      # (code, position) / code
        lane_bytes=[0] * 65, max_step_bytes=0,                     # lanes by their data bytes
        bit31=0, wrapping_streams=0,
        mutants_refused=0, mutants_accepted=0, mutants_accepted_other_samples=0,
        refused_behind_whole_steps=0)      # > 2,048 values, header checks pass, refused
    seen = set()
    for c in cases:
        samples = decode(c.payload)
        if c.origin is not None:
            if samples is None:
                out.mutants_refused += 1
                if header(c.payload) is not None and header(c.payload)[0] > 2 * STEP:
                    out.refused_behind_whole_steps += 1
            else:
                out.mutants_accepted += 1
                if not np.array_equal(samples, decode(c.origin)):
                    out.mutants_accepted_other_samples += 1
        if samples is None:
            out.refused += 1
            continue
        out.accepted += 1
        if c.payload in seen:
            continue
        seen.add(c.payload)
        lengths = code_lengths(c.payload)
        n = len(lengths)
        if n == 0:
            continue
        counts = np.bincount(lengths, minlength=5)
        for k in range(4):
            out.codes[k] += int(counts[k + 1])
        if c.unwrapped:
            out.unwrapped_three_byte += int(counts[3])
        out.last_code.add(int(lengths[-1]))
        position = np.arange(n) % LANE
        in_full = np.arange(n) < n - n % LANE
        for where, mask in ((out.full_lane, in_full), (out.partial_lane, ~in_full)):
            where.update(zip(lengths[mask].tolist(), position[mask].tolist()))
        padded = np.zeros(-(-n // STEP) * STEP, dtype=np.int64)
        padded[:n] = lengths
        for b, k in zip(*np.unique(padded.reshape(-1, LANE).sum(1), return_counts=True)):
            out.lane_bytes[int(b)] += int(k)
        out.max_step_bytes = max(out.max_step_bytes, int(padded.reshape(-1, STEP).sum(1).max()))
        # the values again, for bit 31 and a running sum that leaves 32 bits
        data = np.frombuffer(c.payload, dtype=np.uint8, offset=4 + (n + 3) // 4)
        at = np.cumsum(lengths) - lengths
        top = np.where(lengths == 4, data[np.minimum(at + 3, len(data) - 1)], 0)
        out.bit31 += int((top >= 128).sum())
        u = np.zeros(n, dtype=np.int64)
        wide = np.concatenate([data, np.zeros(3, dtype=np.uint8)]).astype(np.int64)
        for k in range(4):
            u |= np.where(lengths > k, wide[at + k], 0) << (8 * k)
        running = np.cumsum((u >> 1) ^ -(u & 1))
        if running.max() >= 1 << 31 or running.min() < -(1 << 31):
            out.wrapping_streams += 1
    return out


def census_text(c):
    lanes = ', '.join('%d:%d' % (b, k) for b, k in enumerate(c.lane_bytes) if k and b in
                      (0, 16, 17, 32, 33, 48, 63, 64))
    return '\n'.join([
        'census: %d streams, %d accepted, %d refused by the reference' % (c.streams, c.accepted, c.refused),
        '  codes by length 1/2/3/4 bytes: %d / %d / %d / %d (3-byte codes of the 32-bit encoder: %d; '
        'values with bit 31: %d)' % (tuple(c.codes) + (c.unwrapped_three_byte, c.bit31)),
        '  lanes by data bytes (bytes:lanes, a choice): %s; most in one lane %d, in one step %d'
        % (lanes, max(b for b, k in enumerate(c.lane_bytes) if k), c.max_step_bytes),
        '  (code, position) pairs: %d in full lanes, %d in partial lanes; codes as last value: %s; '
        'streams whose sum leaves 32 bits: %d' % (len(c.full_lane), len(c.partial_lane),
                                                   sorted(c.last_code), c.wrapping_streams),
        '  mutants: %d refused (%d of them behind whole steps), %d accepted, %d of those with other '
        'samples' % (c.mutants_refused, c.refused_behind_whole_steps, c.mutants_accepted,
                     c.mutants_accepted_other_samples)])
