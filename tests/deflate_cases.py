"""
Deflate streams written bit by bit (RFC 1950 / 1951), for the GPU inflate (deepbinner_amd/csrc/
dbh_inflate_core.h, dbh_inflate_wave.h, dbh_inflate.hip): everything the format allows and zlib's
own encoder never writes - single, empty and 15-bit codes, padded HLIT / HDIST, repeat codes that
run from the literal lengths into the distance lengths, 258 as symbol 284 + 31 - the refusals of a
dynamic block's header, and tokens placed at the seams of the resolve kernel's ring.

A case is (name, stream, wanted bytes, expected): expected is the bytes the decoder is to hand
out (the stream's content cut at `wanted`), or None - then STATUS[name] is the dbi::Status the
decoder is to answer.  Family G (single-bit flips of dynamic block headers) has zlib as its only
judge: None there means "any status but 0".  families() builds the tables once per process;
check_against_zlib() holds every case of them to Python's zlib, the only judge of all of this.
"""
import struct
import zlib

import numpy as np

M64 = (1 << 64) - 1
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
            131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
             2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
# dbi::Status (dbh_inflate_core.h)
OK, BAD_HEADER, BAD_BLOCK, BAD_CODES, BAD_SYMBOL, TRUNCATED = 0, 1, 2, 3, 4, 5
BAD_DISTANCE, BAD_CHECKSUM = 8, 9
RING = 8192                                   # dbi::kSmallRing
HOME_BITS = 544                               # dbi::kSubBits: a lane's home; 64 of them are a chunk

LENGTH_SYMBOL = {}                            # length -> (symbol, extra bits' value)
for _c in range(28):
    for _x in range(1 << LEN_EXTRA[_c]):
        LENGTH_SYMBOL.setdefault(LEN_BASE[_c] + _x, (257 + _c, _x))
LENGTH_SYMBOL[258] = (285, 0)


def distance_symbol(distance):
    s = max(k for k in range(30) if DIST_BASE[k] <= distance)
    return s, distance - DIST_BASE[s]


def reverse(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def codes_of(lens):
    """Code lengths -> per symbol (the canonical code with its first bit lowest, its length), None
    for a symbol without a code.  Lengths that make no valid code still give numbers: such blocks
    are written for their headers alone."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l:
            out.append((reverse(nxt[l] & ((1 << l) - 1), l), l))
            nxt[l] += 1
        else:
            out.append(None)
    return out


FIXED_LIT = codes_of([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = codes_of([5] * 32)


def lens_of(table, n):
    """{symbol: code length} -> the n code lengths"""
    lens = [0] * n
    for s, l in table.items():
        lens[s] = l
    return lens


class Deflate:
    """A zlib stream in the making.  field(): a number, lowest bit first; code(): a Huffman code,
    first bit first - whole fields and whole codes at once, 64 bits of them flushed at a time."""

    def __init__(self, head=b'\x78\x01'):
        self.out = bytearray(head)
        self.acc = 0
        self.n = 0

    def clone(self):
        other = Deflate(b'')
        other.out, other.acc, other.n = bytearray(self.out), self.acc, self.n
        return other

    def field(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 64:
            self.out += (self.acc & M64).to_bytes(8, 'little')
            self.acc >>= 64
            self.n -= 64

    def code(self, code, nbits):
        self.field(reverse(code, nbits), nbits)

    def bit_position(self):
        return (8 * len(self.out) + self.n) & 7

    def align(self):
        self.n = (self.n + 7) & ~7
        self.out += self.acc.to_bytes(self.n // 8, 'little')
        self.acc = self.n = 0

    def raw_bytes(self, data):
        self.align()
        self.out += data

    def literals(self, data, lit):
        """a run of literal bytes (the bulk of every large case: one tight loop)"""
        acc, n, out = self.acc, self.n, self.out
        for b in data:
            c, l = lit[b]
            acc |= c << n
            n += l
            if n >= 64:
                out += (acc & M64).to_bytes(8, 'little')
                acc >>= 64
                n -= 64
        self.acc, self.n = acc, n

    def tokens(self, tokens, lit, dist):
        for t in tokens:
            if isinstance(t, (bytes, bytearray)):
                self.literals(t, lit)
            elif isinstance(t, (int, np.integer)):
                self.field(*lit[t])
            elif t[0] == 'bits':
                self.code(t[1], t[2])
            else:
                if len(t) == 2:
                    (ls, lx), (ds, dx) = LENGTH_SYMBOL[t[0]], distance_symbol(t[1])
                else:
                    ls, lx, ds, dx = t
                self.field(*lit[ls])
                if 257 <= ls <= 285:
                    self.field(lx, LEN_EXTRA[ls - 257])
                if ds is not None:
                    self.field(*dist[ds])
                    if ds < 30:
                        self.field(dx, DIST_EXTRA[ds])

    def stored_block(self, data, final, nlen=None):
        self.field(final, 1)
        self.field(0, 2)
        self.align()
        self.out += struct.pack('<HH', len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen)
        self.out += data
        return self

    def fixed_block(self, tokens, final, eob=True):
        self.field(final, 1)
        self.field(1, 2)
        self.tokens(tokens, FIXED_LIT, FIXED_DIST)
        if eob:
            self.field(*FIXED_LIT[256])
        return self

    def dynamic_block(self, tokens, final, lit_lens, dist_lens, cl_ops=None, cl_lens=None, hclen=None,
                      eob=True):
        """HLIT and HDIST are the numbers of lengths given (trailing zeros included).  cl_ops: the
        code-length symbols as they are written, a length 0-15 or (16 | 17 | 18, extra bits' value);
        default: every length as itself.  cl_lens: the 19 lengths of the code-length code; default:
        a complete code of 4 and 5 bits that has every symbol."""
        self.field(final, 1)
        self.field(2, 2)
        self.field(len(lit_lens) - 257, 5)
        self.field(len(dist_lens) - 1, 5)
        cl_ops = list(lit_lens) + list(dist_lens) if cl_ops is None else cl_ops
        cl_lens = [4] * 13 + [5] * 6 if cl_lens is None else cl_lens
        hclen = 19 if hclen is None else hclen
        self.field(hclen - 4, 4)
        for i in range(hclen):
            self.field(cl_lens[CL_ORDER[i]], 3)
        cl = codes_of(cl_lens)
        for op in cl_ops:
            if isinstance(op, tuple):
                self.field(*cl[op[0]])
                self.field(op[1], CL_EXTRA[op[0]])
            else:
                self.field(*cl[op])
        lit = codes_of(lit_lens)
        self.tokens(tokens, lit, codes_of(dist_lens))
        if eob:
            self.field(*lit[256])
        return self

    def zlib(self, data, adler=None):
        """-> the finished stream: the Adler-32 of `data` behind the last block"""
        self.align()
        return bytes(self.out) + struct.pack('>I', zlib.adler32(data) if adler is None else adler)


def expand(tokens, start=b''):
    """The bytes the tokens stand for, behind `start`."""
    out = bytearray(start)
    for t in tokens:
        if isinstance(t, (bytes, bytearray)):
            out += t
        elif isinstance(t, (int, np.integer)):
            out.append(int(t))
        else:
            if len(t) == 2:
                length, distance = t
            else:
                length = LEN_BASE[t[0] - 257] + t[1]
                distance = DIST_BASE[t[2]] + t[3]
            assert 1 <= distance <= len(out), t
            if distance >= length:
                out += out[len(out) - distance:len(out) - distance + length]
            else:
                for _ in range(length):
                    out.append(out[-distance])
    return bytes(out)


STATUS = {}                                   # name of a refused case of A-F -> dbi::Status


def refused(name, stream, wanted, status):
    STATUS[name] = status
    return (name, stream, wanted, None)


def accepted(name, stream, data, wanted=None):
    wanted = len(data) if wanted is None else wanted
    return (name, stream, wanted, data[:wanted])


def random_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def fixed_prefix(data):
    """a fixed block, not final and still open, that begins with `data` as literals"""
    d = Deflate()
    d.field(0, 1)
    d.field(1, 2)
    d.literals(data, FIXED_LIT)
    return d


def close_fixed(d):
    """the end-of-block code of an open fixed block, and an empty final one behind it"""
    d.field(*FIXED_LIT[256])
    d.field(1, 1)
    d.field(1, 2)
    d.field(*FIXED_LIT[256])
    return d


def behind_prefix(prefix, data, tail):
    """-> (stream, bytes): the open fixed block `prefix` (holding `data`) with the tokens `tail`,
    its end-of-block code and the checksum"""
    d = prefix.clone()
    d.tokens(tail, FIXED_LIT, FIXED_DIST)
    whole = expand(tail, data)
    return close_fixed(d).zlib(whole), whole


# ---- A: the code space of the fixed block -------------------------------------------------------
def family_a():
    rng = np.random.default_rng(101)
    cases = []
    data = random_bytes(rng, 300)
    prefix = fixed_prefix(data)
    for distance in (1, 2, 3, 4, 7, 8, 9, 255, 256, 257, 300):
        ds, dx = distance_symbol(distance)
        for length in list(range(3, 259)) + ['258 as 284 + 31']:
            match = (284, 31, ds, dx) if isinstance(length, str) else (length, distance)
            name = 'A.len%s.d%d' % ('258alt' if isinstance(length, str) else length, distance)
            stream, whole = behind_prefix(prefix, data, [match, 7, 8, 9])
            cases.append(accepted(name, stream, whole))
    data = random_bytes(rng, 32768)
    prefix = fixed_prefix(data)
    for ds in range(30):
        for dx in sorted({0, (1 << DIST_EXTRA[ds]) - 1}):
            for ls, lx, length in ((257, 0, 3), (265, 0, 11)):
                stream, whole = behind_prefix(prefix, data, [(ls, lx, ds, dx), 1, 2, 3])
                cases.append(accepted('A.dist%d.x%d.len%d' % (ds, dx, length), stream, whole))
    return cases


# ---- B: refusals inside the data ----------------------------------------------------------------
def family_b():
    rng = np.random.default_rng(102)
    cases = []
    data = random_bytes(rng, 6000)            # (a chunk is 64 homes = 4,352 bytes of the stream)
    prefix = fixed_prefix(data)
    for name, bad in (('B.symbol286', (286, 0, None, 0)), ('B.symbol287', (287, 0, None, 0)),
                      ('B.distance30', (257, 0, 30, 0)), ('B.distance31', (257, 0, 31, 0))):
        d = prefix.clone()
        d.tokens([bad, 1, 2, 3], FIXED_LIT, FIXED_DIST)
        cases.append(refused(name, close_fixed(d).zlib(data), len(data) + 100, BAD_SYMBOL))
    stream = Deflate().fixed_block([(3, 1), 1, 2, 3], 1).zlib(b'')
    cases.append(refused('B.match_first', stream, 100, BAD_DISTANCE))
    for position in (10, 8192, 8195, 32767):
        data = random_bytes(rng, position)
        prefix = fixed_prefix(data)
        d = prefix.clone()
        d.tokens([(3, position + 1), 1, 2, 3], FIXED_LIT, FIXED_DIST)
        cases.append(refused('B.before_start.p%d' % position, close_fixed(d).zlib(data), position + 100,
                             BAD_DISTANCE))
        stream, whole = behind_prefix(prefix, data, [(3, position), 1, 2, 3])
        cases.append(accepted('B.from_start.p%d' % position, stream, whole))
    return cases


# ---- C: dynamic headers and codes ---------------------------------------------------------------
LIT0 = {97: 2, 98: 2, 256: 2, 257: 3, 258: 3}              # a small complete code: a, b, end, 3, 4
DIST0 = [1, 1]


def greedy_ops(lens):
    """the code lengths run-length coded, every run as long as it can be"""
    ops, k = [], 0
    while k < len(lens):
        v, run = lens[k], 1
        while k + run < len(lens) and lens[k + run] == v:
            run += 1
        if v == 0 and run >= 3:
            n = min(run, 138)
            ops.append((18, n - 11) if n >= 11 else (17, n - 3))
            k += n
            continue
        ops.append(v)
        k += 1
        run -= 1
        while run >= 3:
            n = min(run, 6)
            ops.append((16, n - 3))
            k += n
            run -= n
    return ops


def ladder_case(rng):
    """Both codes with the lengths 1, 2, .. 14, 15, 15: the wave's first-level tables answer the
    short codes, the canonical decode the literal codes of 12-15 and the distance codes of 9-15
    bits - in lanes beside each other."""
    lit_syms = [65, 66, 257, 67, 260, 256, 68, 270, 69, 285, 70, 71, 72, 73, 74, 284]
    dist_syms = [0, 1, 2, 3, 4, 5, 8, 10, 12, 14, 16, 18, 20, 22, 24, 29]
    depth = list(range(1, 16)) + [15]
    lit_lens = lens_of(dict(zip(lit_syms, depth)), 286)
    dist_lens = lens_of(dict(zip(dist_syms, depth)), 30)
    literals = [s for s in lit_syms if s < 256]
    weights = np.array([8.0 if lit_lens[s] < 12 else 1.0 for s in literals])
    head = bytes(rng.choice(literals, 33000, p=weights / weights.sum()).astype(np.uint8))
    tokens = [head]                              # (33,000 bytes: every distance lies inside them)
    for _ in range(3000):
        if rng.random() < 0.5:
            tokens.append(int(rng.choice(literals)))
        else:
            ls = int(rng.choice([s for s in lit_syms if s > 256]))
            ds = int(rng.choice(dist_syms))
            lx = int(rng.integers(0, 1 << LEN_EXTRA[ls - 257]))
            dx = int(rng.integers(0, 1 << DIST_EXTRA[ds]))
            tokens.append((ls, lx, ds, dx))
    data = expand(tokens)
    stream = Deflate().dynamic_block(tokens, 1, lit_lens, dist_lens).zlib(data)
    return stream, data


def family_c():
    rng = np.random.default_rng(103)
    cases = []
    stream, data = ladder_case(rng)
    cases.append(accepted('C.lengths_1_to_15', stream, data))
    cases.append(accepted('C.lengths_1_to_15.short', stream, data, len(data) - 777))

    lit0, lit0_long = lens_of(LIT0, 259), lens_of(LIT0, 286)
    ab = bytes(rng.choice([97, 98], 40000).astype(np.uint8))
    # one distance code of length 1
    for sym, matches in ((0, [(257, 0, 0, 0), (258, 0, 0, 0)]), (29, [(257, 0, 29, 0), (258, 0, 29, 8191)])):
        dist_lens = lens_of({sym: 1}, sym + 1)
        tokens = [ab, matches[0], 97, matches[1], 98, 98]
        data = expand(tokens)
        stream = Deflate().dynamic_block(tokens, 1, lit0, dist_lens).zlib(data)
        cases.append(accepted('C.one_distance_code.symbol%d' % sym, stream, data))
        tokens = [ab, matches[0], 97, (257, 0, None, 0), ('bits', 1, 1), 98, 98]
        stream = Deflate().dynamic_block(tokens, 1, lit0, dist_lens).zlib(ab)
        cases.append(refused('C.one_distance_code.symbol%d.unused_code' % sym, stream, len(ab) + 100, BAD_SYMBOL))
    # no distance code at all
    tokens = [ab[:9000], 97, 98]
    data = expand(tokens)
    stream = Deflate().dynamic_block(tokens, 1, lit0, [0]).zlib(data)
    cases.append(accepted('C.no_distance_code.literals', stream, data))
    tokens = [ab[:9000], (257, 0, None, 0), ('bits', 0, 1), 97, 98]
    stream = Deflate().dynamic_block(tokens, 1, lit0, [0]).zlib(ab[:9000])
    cases.append(refused('C.no_distance_code.length', stream, 9100, BAD_SYMBOL))
    # a literal/length code that is the end-of-block code alone
    d = Deflate()
    for _ in range(3):
        d.dynamic_block([], 0, lens_of({256: 1}, 257), [0])
    data = random_bytes(rng, 500)
    cases.append(accepted('C.end_of_block_only', d.fixed_block([data], 1).zlib(data), data))
    # two 1-bit codes: as many tokens as bits, 544 to a home
    two = lens_of({120: 1, 256: 1}, 257)
    for n in (1, 543, 544, 545, 64 * HOME_BITS - 1, 64 * HOME_BITS, 64 * HOME_BITS + 1, 100000):
        data = b'x' * n
        stream = Deflate().dynamic_block([data], 1, two, [0]).zlib(data)
        cases.append(accepted('C.two_1bit_codes.n%d' % n, stream, data))
        cases.append(accepted('C.two_1bit_codes.n%d.short' % n, stream, data, n - 1))
    # code sets that are refused
    header_only = dict(eob=False)
    for name, lit, dist in (('C.no_end_of_block', lens_of({97: 1, 98: 1}, 257), DIST0),
                            ('C.oversubscribed.literal', lens_of({97: 1, 98: 1, 256: 1}, 257), DIST0),
                            ('C.oversubscribed.distance', lit0, [1, 1, 1]),
                            ('C.incomplete.literal', lens_of({97: 2, 256: 2}, 257), DIST0),
                            ('C.incomplete.distance', lit0, [2, 2])):
        stream = Deflate().dynamic_block([], 1, lit, dist, **header_only).zlib(b'')
        cases.append(refused(name, stream, 100, BAD_CODES))
    for name, lit, dist in (('C.hlit287', lens_of(LIT0, 287), DIST0), ('C.hlit288', lens_of(LIT0, 288), DIST0),
                            ('C.hdist31', lit0, lens_of({0: 1, 1: 1}, 31)),
                            ('C.hdist32', lit0, lens_of({0: 1, 1: 1}, 32))):
        # (whole streams, checksum and all: a decoder that took the header would answer 0)
        stream = Deflate().dynamic_block([b'abba'], 1, lit, dist).zlib(b'abba')
        cases.append(refused(name, stream, 100, BAD_CODES))
    # HCLEN 4 has lengths for 16, 17, 18 and 0 only: nothing but zeros can be said, so no end of block
    cl = lens_of({18: 1, 0: 1}, 19)
    stream = Deflate().dynamic_block([], 1, lit0, DIST0, cl_ops=[(18, 127), (18, 112 - 11), (18, 0)], cl_lens=cl,
                                     hclen=4, **header_only).zlib(b'')
    cases.append(refused('C.hclen4', stream, 100, BAD_CODES))
    tokens = [ab[:700], (3, 1), (4, 2), 97]
    data = expand(tokens)
    lit15 = lens_of({97: 1, 98: 2, 256: 3, 257: 4, 258: 5, 259: 6, 260: 7, 261: 8, 262: 9, 263: 10, 264: 11,
                     265: 12, 266: 13, 267: 14, 268: 15, 269: 15}, 270)
    stream = Deflate().dynamic_block(tokens, 1, lit15, DIST0, hclen=19).zlib(data)
    cases.append(accepted('C.hclen19', stream, data))
    # repeat codes
    total = len(lit0) + len(DIST0)
    plain = lit0 + DIST0
    # (three zeros are what a decoder without the check would take the `16` for: the rest is whole)
    assert plain[:3] == [0, 0, 0]
    stream = Deflate().dynamic_block([b'abba'], 1, lit0, DIST0, cl_ops=[(16, 0)] + plain[3:]).zlib(b'abba')
    cases.append(refused('C.repeat16_first', stream, 100, BAD_CODES))
    lit_run = lens_of({s: 3 for s in (97, 98, 99, 100, 101, 102, 103, 256)}, 257)
    ops = greedy_ops(lit_run + DIST0)
    assert any(isinstance(b, tuple) and b[0] == 16 and not isinstance(a, tuple) for a, b in zip(ops, ops[1:]))
    tokens = [bytes(rng.integers(97, 104, 5000).astype(np.uint8))]
    data = expand(tokens)
    stream = Deflate().dynamic_block(tokens, 1, lit_run, DIST0, cl_ops=ops).zlib(data)
    cases.append(accepted('C.repeat16_after_length', stream, data))
    lit_pad = lens_of(LIT0, 270)                       # 11 zeros at the end, three more begin the distances
    tokens = [ab[:5000], (3, 4), (4, 5), 98]          # (distance symbols 3 and 4)
    data = expand(tokens)
    stream = Deflate().dynamic_block(tokens, 1, lit_pad, [0, 0, 0, 1, 1],
                                     cl_ops=lit_pad[:259] + [(18, 3), 1, 1]).zlib(data)
    cases.append(accepted('C.repeat18_across_both', stream, data))
    for sym, extra, rep in ((16, 0, 3), (17, 0, 3), (18, 0, 11)):
        ops = plain[:total - rep + 1] + [(sym, extra)]
        stream = Deflate().dynamic_block([], 1, lit0, DIST0, cl_ops=ops, **header_only).zlib(b'')
        cases.append(refused('C.repeat%d_one_beyond' % sym, stream, 100, BAD_CODES))
    # the code-length code itself
    stream = Deflate().dynamic_block([], 1, lit0, DIST0, cl_ops=[], cl_lens=lens_of({0: 1}, 19),
                                     **header_only).zlib(b'')
    cases.append(refused('C.code_length_code.single', stream, 100, BAD_CODES))
    stream = Deflate().dynamic_block([], 1, lit0, DIST0, cl_ops=[], cl_lens=[0] * 19, **header_only).zlib(b'')
    cases.append(refused('C.code_length_code.zeros', stream, 100, BAD_SYMBOL))
    cl7 = lens_of({0: 1, 2: 2, 3: 3, 1: 4, 18: 5, 17: 6, 16: 7, 4: 7}, 19)
    lit7 = lens_of({97: 3, 98: 3, 99: 3, 100: 3, 101: 3, 256: 3, 257: 3, 258: 3}, 265)
    tokens = [bytes(rng.integers(97, 102, 600).astype(np.uint8)), (3, 1), (4, 2), 97]
    data = expand(tokens)
    ops = greedy_ops(lit7 + DIST0)
    assert {16, 17, 18} <= {op[0] for op in ops if isinstance(op, tuple)}
    stream = Deflate().dynamic_block(tokens, 1, lit7, DIST0, cl_ops=ops, cl_lens=cl7).zlib(data)
    cases.append(accepted('C.code_length_code.7bit', stream, data))
    return cases


# ---- D: stored blocks ---------------------------------------------------------------------------
def family_d():
    rng = np.random.default_rng(104)
    cases = []
    data = random_bytes(rng, 65535)
    cases.append(accepted('D.stored_65535', Deflate().stored_block(data, 0).stored_block(b'', 1).zlib(data), data))
    ends = set()
    for j in range(8):
        head = bytes([200] * j + [65] * 5)            # nine-bit literals move the block's end bit by bit
        d = Deflate().fixed_block([head], 0)
        ends.add(d.bit_position())
        tail = random_bytes(rng, 300)
        cases.append(accepted('D.stored_behind_fixed.bit%d' % d.bit_position(),
                              d.stored_block(tail, 1).zlib(head + tail), head + tail))
    assert len(ends) == 8
    a, b = random_bytes(rng, 700), bytes(rng.choice([97, 98], 700).astype(np.uint8))
    d = Deflate().fixed_block([a], 0).stored_block(b'', 0).dynamic_block([b, (3, 1)], 1, lens_of(LIT0, 259), DIST0)
    cases.append(accepted('D.empty_stored_between', d.zlib(expand([a, b, (3, 1)])), expand([a, b, (3, 1)])))
    big = random_bytes(rng, 6000)
    d = Deflate().fixed_block([big], 0).stored_block(b'hello', 1, nlen=0xFFFA ^ 0x0100)
    cases.append(refused('D.len_nlen', d.zlib(big + b'hello'), 6100, BAD_BLOCK))
    d = Deflate().fixed_block([big], 0)
    d.field(1, 1)
    d.field(3, 2)
    cases.append(refused('D.block_type_3', d.zlib(big), 6100, BAD_BLOCK))
    d = Deflate().fixed_block([big], 0).stored_block(bytes(100), 1)
    cases.append(refused('D.stored_cut', bytes(d.out[:-50]), 6200, TRUNCATED))
    d = Deflate().fixed_block([big], 1, eob=False)
    d.align()
    cases.append(refused('D.fixed_cut', bytes(d.out), 6100, TRUNCATED))
    d = Deflate().fixed_block([big], 0).stored_block(b'hello', 1)
    cases.append(refused('D.checksum', d.zlib(b'', adler=zlib.adler32(big + b'hellp')), 6100, BAD_CHECKSUM))
    return cases


# ---- E: placement at the seams of the resolve kernel --------------------------------------------
E_LENGTHS = (3, 4, 7, 8, 9, 16, 258)
E_PREFIXES = (RING - 9, RING - 1, RING, RING + 1, 2 * RING - 4, 32767, 32768, 32773, 40000)


def family_e():
    rng = np.random.default_rng(105)
    cases = []
    for p in E_PREFIXES:
        data = random_bytes(rng, p)
        prefix = fixed_prefix(data)
        distances = sorted({d for d in (1, 2, 3, 5, 7, 8, 9, 4095, 4096, 4097, RING - 8, RING - 1, RING,
                                        RING + 1, RING + 8, p - 1, p, 32768) if d <= min(p, 32768)})
        for length in E_LENGTHS:
            for dist in distances:
                m = (length, dist)
                tail = [m, 1, 2, 3, 4, 5, m, m, m, 6, 7, 8]
                stream, whole = behind_prefix(prefix, data, tail)
                cases.append(accepted('E.p%d.len%d.d%d' % (p, length, dist), stream, whole))
    for k in range(-12, 13):
        p = 3 * RING + k
        data = random_bytes(rng, p)
        prefix = fixed_prefix(data)
        pairs = ((3, RING), (8, RING - 4), (8, RING + k), (5, 2), (258, 1), (258, 7), (20, RING - 6))
        for j, m in enumerate(pairs):
            stream, whole = behind_prefix(prefix, data, [m, m, 9, m])
            cases.append(accepted('E.sweep%+d.pair%d.len%d.d%d' % (k, j, m[0], m[1]), stream, whole))
    return cases


# ---- F: seeded random streams -------------------------------------------------------------------
def leaf_split(rng, n, max_bits):
    """the lengths of a random complete code of n >= 2 codes, none longer than max_bits"""
    if n == 1:
        return [1]
    leaves = [1, 1]
    while len(leaves) < n:
        open_ = [i for i, l in enumerate(leaves) if l < max_bits]
        if rng.random() < 0.3:
            deepest = max(leaves[i] for i in open_)
            open_ = [i for i in open_ if leaves[i] == deepest]
        i = open_[int(rng.integers(0, len(open_)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    return leaves


def random_code(rng, symbols, n, max_bits):
    depths = leaf_split(rng, len(symbols), max_bits)
    rng.shuffle(depths)
    return lens_of(dict(zip(symbols, depths)), n)


def random_ops(rng, lens):
    """the code lengths run-length coded with 16 / 17 / 18 used at random, runs of random length"""
    ops, k = [], 0
    while k < len(lens):
        run = 1
        while k + run < len(lens) and lens[k + run] == lens[k]:
            run += 1
        if lens[k] == 0 and run >= 11 and rng.random() < 0.6:
            n = int(rng.integers(11, min(run, 138) + 1))
            ops.append((18, n - 11))
        elif lens[k] == 0 and run >= 3 and rng.random() < 0.6:
            n = int(rng.integers(3, min(run, 10) + 1))
            ops.append((17, n - 3))
        elif k > 0 and lens[k] == lens[k - 1] and run >= 3 and rng.random() < 0.7:
            n = int(rng.integers(3, min(run, 6) + 1))
            ops.append((16, n - 3))
        else:
            n = 1
            ops.append(lens[k])
        k += n
    return ops


def random_tokens(rng, pos, count, literals, length_syms, dist_syms):
    """-> (tokens, the position behind them): matches of random symbols, their extra bits 0, all
    ones or random, no distance beyond the output so far"""
    tokens = []
    literals = np.asarray(literals)

    def extra(bits, cap):
        top = min((1 << bits) - 1, cap)
        return (0, top, int(rng.integers(0, top + 1)))[int(rng.integers(0, 3))]

    for _ in range(count):
        near = [s for s in dist_syms if DIST_BASE[s] <= pos]
        if near and length_syms and rng.random() < 0.4:
            ls, ds = int(rng.choice(length_syms)), int(rng.choice(near))
            lx = extra(LEN_EXTRA[ls - 257], 1 << 30)
            dx = extra(DIST_EXTRA[ds], pos - DIST_BASE[ds])
            tokens.append((ls, lx, ds, dx))
            pos += LEN_BASE[ls - 257] + lx
        else:
            run = int(rng.integers(1, 6))
            tokens.append(bytes(rng.choice(literals, run).astype(np.uint8)))
            pos += run
    return tokens, pos


def random_count(rng, small):
    kind = rng.random()
    if small:
        return int(rng.integers(1, 40))
    return 0 if kind < 0.05 else int(rng.integers(1, 50)) if kind < 0.5 else int(rng.integers(50, 800)) \
        if kind < 0.9 else int(rng.integers(800, 6000))


def random_dynamic_block(rng, d, pos, final, small=False):
    """one dynamic block with random complete codes -> (its tokens, the position behind it)"""
    if rng.integers(0, 7) == 0:                        # a two-symbol literal code
        literals, length_syms = [int(rng.integers(0, 256))], []
    else:
        literals = sorted(rng.choice(256, int(rng.integers(1, 12 if small else 257)), replace=False).tolist())
        length_syms = sorted(rng.choice(np.arange(257, 286), int(rng.integers(0, 6 if small else 30)),
                                        replace=False).tolist())
    lit_syms = literals + [256] + length_syms
    lit_lens = random_code(rng, lit_syms, int(rng.integers(max(lit_syms) + 1, 287)), 15)
    if rng.integers(0, 7) == 0:                        # a single distance code, or none
        dist_syms = [int(rng.integers(0, 30))] if rng.random() < 0.5 else []
    else:
        dist_syms = sorted(rng.choice(30, int(rng.integers(2, 6 if small else 31)), replace=False).tolist())
    dist_lens = random_code(rng, dist_syms, int(rng.integers(max(dist_syms + [0]) + 1, 31)), 15) \
        if dist_syms else [0] * int(rng.integers(1, 31))
    tokens, pos = random_tokens(rng, pos, random_count(rng, small), literals, length_syms, dist_syms)
    ops = random_ops(rng, lit_lens + dist_lens)
    used = sorted({op[0] if isinstance(op, tuple) else op for op in ops})
    if len(used) == 1:
        used = sorted(set(used) | {(used[0] + 1) % 19})
    cl_lens = random_code(rng, used, 19, 7)
    hclen = max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1
    d.dynamic_block(tokens, final, lit_lens, dist_lens, cl_ops=ops, cl_lens=cl_lens,
                    hclen=int(rng.integers(max(hclen, 4), 20)))
    return tokens, pos


def random_stream(seed, kinds=('stored', 'fixed', 'dynamic'), blocks=None, small=False):
    rng = np.random.default_rng(seed)
    d, every, pos = Deflate(), [], 0
    n_blocks = int(rng.integers(1, 7)) if blocks is None else blocks
    for k in range(n_blocks):
        kind, final = kinds[int(rng.integers(0, len(kinds)))], int(k == n_blocks - 1)
        if kind == 'stored':
            data = random_bytes(rng, int(rng.integers(0, 3) * rng.integers(0, 1500)))
            d.stored_block(data, final)
            tokens, pos = [data], pos + len(data)
        elif kind == 'fixed':
            tokens, pos = random_tokens(rng, pos, random_count(rng, small), np.arange(256), list(range(257, 286)),
                                        list(range(30)))
            d.fixed_block(tokens, final)
        else:
            tokens, pos = random_dynamic_block(rng, d, pos, final, small)
        every += tokens
    data = expand(every)
    return d.zlib(data), data


def family_f():
    cases = []
    for seed in range(150):
        stream, data = random_stream(5000 + seed)
        wanted = None
        if seed % 5 == 4 and len(data) > 1:
            wanted = int(np.random.default_rng(seed).integers(1, len(data)))
        cases.append(accepted('F.seed%d' % seed, stream, data, wanted))
    return cases


# ---- G: every single-bit flip of a dynamic block's header ---------------------------------------
G_BITS = 400
G_WANTED = 8192


def fails_within(stream, n_bytes):
    """does zlib meet the stream's error - a bad code, or the end of the input - before it has
    produced n_bytes?"""
    d = zlib.decompressobj()
    try:
        got = d.decompress(stream, n_bytes)
    except zlib.error:
        return True
    return len(got) < n_bytes and not d.eof


def family_g(c_cases):
    by_name = {c[0]: c for c in c_cases}
    bases = [(name, by_name[name][1]) for name in ('C.code_length_code.7bit', 'C.repeat18_across_both',
                                                    'C.hclen19', 'C.two_1bit_codes.n543')]
    bases += [('F.small%d' % seed, random_stream(7000 + seed, kinds=('dynamic',), blocks=1, small=True)[0])
              for seed in (1, 2)]
    cases = []
    for name, stream in bases:
        for bit in range(min(G_BITS, 8 * (len(stream) - 2))):
            mutant = bytearray(stream)
            mutant[2 + bit // 8] ^= 1 << (bit % 8)
            mutant = bytes(mutant)
            wanted = G_WANTED
            try:
                want = zlib.decompress(mutant)[:wanted]
            except zlib.error:
                want = None
                # the error must come well before `wanted` bytes: the decoder stops reading behind them
                if not fails_within(mutant, wanted - 300):
                    wanted = 1 << 20
                    assert fails_within(mutant, wanted - 300), (name, bit)
            cases.append(('G.%s.bit%d' % (name, bit), mutant, wanted, want))
    return cases


_FAMILIES = {}


def families():
    """{'A': cases, .. 'G': cases}, built once"""
    if not _FAMILIES:
        _FAMILIES.update(A=family_a(), B=family_b(), C=family_c(), D=family_d(), E=family_e(), F=family_f())
        _FAMILIES['G'] = family_g(_FAMILIES['C'])
        names = [c[0] for cases in _FAMILIES.values() for c in cases]
        assert len(names) == len(set(names))
    return _FAMILIES


def check_against_zlib(cases):
    """zlib's verdict on every case is the table's own -> (accepted, refused)"""
    n_ok = n_bad = 0
    for name, stream, wanted, expected in cases:
        try:
            whole = zlib.decompress(stream)
        except zlib.error:
            whole = None
        if expected is None:
            assert whole is None, '%s: zlib accepts what the table has as refused' % name
            assert name.startswith('G.') or STATUS[name] != OK, name
            n_bad += 1
        else:
            assert whole is not None, '%s: zlib refuses what the table has as accepted' % name
            assert whole[:wanted] == expected, '%s: zlib gives other bytes' % name
            n_ok += 1
    return n_ok, n_bad
