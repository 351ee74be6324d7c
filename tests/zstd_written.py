"""
zstd frames written bit by bit (RFC 8878), for the GPU's zstd decoder (deepbinner_amd/csrc/
dbh_zstd_core.h, dbh_zstd.hip): everything the format allows and libzstd's own encoder never or
hardly ever writes - non-canonical headers, the 3-byte sequence count, repeat mode behind every
other mode, treeless literals across blocks, every row of the repeat-offset table, trees of depth
11, fourth streams without a symbol, alphabets that never re-synchronise, blocks and matches beyond
128 KiB - and frames shaped for the device's own copy, fill and match (dbh_zstd.hip, WaveExec).

The parts: a backward bitstream writer (Back), FSE (the decoding table of a distribution, an encoder
that walks a symbol list backwards through that table, the table-description writer, the two-state
encoder of Huffman weights), Huffman (weights to codes, direct and FSE-compressed descriptions, 1 and
4 streams, all four header sizes), sequences (codes with chosen extra bits, each table in any mode,
the count in any form), blocks and frame headers with every field settable, and a replay in plain
Python that gives each valid frame its content independently of any decoder.

A case is (name, frame, content | None, status | None): content is what the frame decodes to, or
None - then status is the dbz::Status the decoder is to answer.  families() builds them once per
process.  ROOM[name] is the capacity a refused case is decoded into.  libzstd is the judge of all of
it (tests/test_zstd_written.py).

    python tests/zstd_written.py --dump FILE

writes [u32 frame bytes][u32 capacity][frame] records for csrc/zstd_model_check.cpp.
"""
import struct
import sys

import numpy as np

MAGIC = 0xFD2FB528
# dbz::Status (dbh_zstd_core.h)
OK, BAD_MAGIC, UNSUPPORTED, TRUNCATED, BAD_BLOCK, BAD_LITERALS, BAD_TREE = 0, 16, 17, 18, 19, 20, 21
BAD_FSE, BAD_SEQUENCES, BAD_BITSTREAM, BAD_OFFSET, BAD_SIZE, NO_SPACE, TRAILING = 22, 23, 24, 25, 26, 27, 28

# ---- the code tables of RFC 8878, 3.1.1.3.2.1.1 -------------------------------------------------
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192,
                             16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099,
                                8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
assert len(LL_BASE) == len(LL_BITS) == 36 and len(ML_BASE) == len(ML_BITS) == 53
# the predefined distributions (3.1.1.3.2.2)
LL_PRE = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1,
          -1, -1, -1, -1]
ML_PRE = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_PRE = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
TABLES = ('ll', 'of', 'ml')                     # in the order of their descriptions
PRE_NORM = {'ll': (LL_PRE, 6), 'of': (OF_PRE, 5), 'ml': (ML_PRE, 6)}
MAX_LOG = {'ll': 9, 'of': 8, 'ml': 9}
MAX_SYM = {'ll': 35, 'of': 31, 'ml': 52}
MODE_NAMES = ('predefined', 'rle', 'compressed', 'repeat')
PRE, REP = ('pre',), ('rep',)


def ll_code(n, code=None):
    c = max(k for k in range(36) if LL_BASE[k] <= n) if code is None else code
    assert 0 <= n - LL_BASE[c] < 1 << LL_BITS[c]
    return c, n - LL_BASE[c]


def ml_code(n, code=None):
    c = max(k for k in range(53) if ML_BASE[k] <= n) if code is None else code
    assert 0 <= n - ML_BASE[c] < 1 << ML_BITS[c]
    return c, n - ML_BASE[c]


def S(ll, ml, offset):
    """A sequence with a new offset -> (ll code, extra, ml code, extra, offset code, extra)."""
    v = offset + 3
    oc = v.bit_length() - 1
    return ll_code(ll) + ml_code(ml) + (oc, v - (1 << oc))


def R(ll, ml, value):
    """A sequence with offset value 1, 2 or 3 (a repeat offset; which one depends on ll == 0)."""
    return ll_code(ll) + ml_code(ml) + ((0, 0), (1, 0), (1, 1))[value - 1]


# ---- bitstreams ---------------------------------------------------------------------------------
class Back:
    """A backward bitstream: fields in the order the decoder reads them; the first is written just
    below the marker bit, the last ends at bit 0 of the first byte."""

    def __init__(self):
        self.parts = []
        self.bits = 0

    def add(self, value, n):
        assert 0 <= value < (1 << n) or (n == 0 and value == 0), (value, n)
        if n:
            self.parts.append(format(value, '0%db' % n))
            self.bits += n

    def add_str(self, s):
        self.parts.append(s)
        self.bits += len(s)

    def marker_bit(self):
        """the marker's position in the last byte, 0..7"""
        return self.bits % 8

    def bytes(self):
        s = '1' + ''.join(self.parts)           # (the marker; a stream without one: append a zero byte)
        return int(s, 2).to_bytes((len(s) + 7) // 8, 'little')


class Fwd:
    """A forward bitstream (first bit lowest): the FSE table descriptions."""

    def __init__(self):
        self.acc = 0
        self.bits = 0

    def add(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc |= value << self.bits
        self.bits += n

    def bytes(self):
        return self.acc.to_bytes((self.bits + 7) // 8, 'little')


# ---- FSE ----------------------------------------------------------------------------------------
def fse_table(norm, log):
    """The decoding table of a distribution: [(symbol, bits, base)] per state (RFC 8878, 4.1.1)."""
    size = 1 << log
    assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
    sym = [None] * size
    high = size - 1
    nxt = {}
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
            nxt[s] = 1
        else:
            nxt[s] = c
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    tab = []
    for u in range(size):
        ns = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb = log - (ns.bit_length() - 1)
        tab.append((sym[u], nb, (ns << nb) - size))
    return tab


def fse_chain(tab, syms, need_bits_last=False, pick=0):
    """The states a decoder goes through while it yields ``syms``: the last is free (``pick`` among
    the symbol's states; ``need_bits_last``: one that reads at least a bit to move on), every one
    before it is the state of its symbol whose range holds the state behind it."""
    by_sym = {}
    for st, (s, nb, base) in enumerate(tab):
        by_sym.setdefault(s, []).append(st)
    states = [0] * len(syms)
    cands = [st for st in by_sym[syms[-1]] if tab[st][1] > 0 or not need_bits_last]
    states[-1] = cands[pick % len(cands)]
    for i in range(len(syms) - 2, -1, -1):
        for st in by_sym[syms[i]]:
            if tab[st][2] <= states[i + 1] < tab[st][2] + (1 << tab[st][1]):
                states[i] = st
                break
        else:
            raise AssertionError('no state of symbol %d leads to %d' % (syms[i], states[i + 1]))
    return states


def ncount(norm, log, long_runs=True):
    """The description of a distribution (RFC 8878, 4.1.1): accuracy, then a value per symbol in as
    many bits as the points left allow, runs of zeros behind a zero as 2-bit counts (3 = more to
    come) or, ``long_runs``, 24 at a time as sixteen 1 bits."""
    norm = list(norm)
    while norm and norm[-1] == 0:
        norm.pop()
    w = Fwd()
    w.add(log - 5, 4)
    remaining, threshold, nb, s, prev0 = (1 << log) + 1, 1 << log, log + 1, 0, False
    while remaining > 1:
        if prev0:
            run = 0
            while norm[s + run] == 0:
                run += 1
            s += run
            while long_runs and run >= 24:
                w.add(0xFFFF, 16)
                run -= 24
            while run >= 3:
                w.add(3, 2)
                run -= 3
            w.add(run, 2)
        count = norm[s]
        s += 1
        small = 2 * threshold - 1 - remaining
        v = count + 1
        remaining -= abs(count)
        if v < small:
            w.add(v, nb - 1)
        else:
            w.add(v + small if v >= threshold else v, nb)
        prev0 = count == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    assert remaining == 1 and s == len(norm)
    return w.bytes()


def spread(symbols, log, less_than_one=(), heavy=None):
    """A distribution of accuracy ``log`` that holds ``symbols``: 1 each (-1 for those in
    ``less_than_one``), the rest of the points on ``heavy`` (the first by default)."""
    symbols = sorted(set(symbols))
    norm = [0] * (max(symbols) + 1)
    for s in symbols:
        norm[s] = -1 if s in less_than_one else 1
    heavy = symbols[0] if heavy is None else heavy
    norm[heavy] = 0
    norm[heavy] = (1 << log) - sum(abs(c) for c in norm)
    assert norm[heavy] >= 1
    return norm


def normalize(counts, log):
    """Counts per symbol -> a distribution of accuracy ``log`` with every counted symbol in it."""
    total, size = sum(counts), 1 << log
    norm = [max(1, c * size // total) if c else 0 for c in counts]
    while sum(norm) != size:
        k = max(range(len(norm)), key=lambda i: norm[i])
        norm[k] += 1 if sum(norm) < size else -1
        assert norm[k] >= 1
    return norm


# ---- Huffman ------------------------------------------------------------------------------------
def full_weights(given):
    """The weights a description gives -> (all weights, the implied last one included; table log)."""
    total = sum((1 << w) >> 1 for w in given)
    log = total.bit_length()
    rest = (1 << log) - total
    assert rest and rest & (rest - 1) == 0, 'the weights do not complete a power of two'
    return list(given) + [rest.bit_length()], log


def huf_codes(weights, log):
    """{symbol: its code as a string of bits, first bit read first}: per weight from 1 upwards and
    per symbol in ascending order the codes take the table from its low end (4.2.1)."""
    at, first = 0, {}
    for w in range(1, log + 1):
        first[w] = at
        at += sum(1 for x in weights if x == w) << (w - 1)
    assert at == 1 << log
    codes = {}
    for s, w in enumerate(weights):
        if w:
            codes[s] = format(first[w] >> (w - 1), '0%db' % (log + 1 - w))
            first[w] += 1 << (w - 1)
    return codes


def tree_direct(given):
    assert 1 <= len(given) <= 128
    padded = list(given) + [0]
    return bytes([127 + len(given)]) + bytes((padded[k] << 4) | padded[k + 1] for k in range(0, len(given), 2))


def tree_fse(given, log=6, norm=None, less_than_one=()):
    """The weights as two interleaved FSE states (4.2.1.2): the description of their distribution,
    then the stream - both states, then the bits that move state 1 and state 2 on in turn; it ends
    where a state that needs bits finds none."""
    assert len(given) >= 2
    if norm is None:
        counts = [0] * (max(given) + 1)
        for w in given:
            counts[w] += 1
        norm = normalize(counts, log)
        for w in less_than_one:
            big = max(range(len(norm)), key=lambda i: norm[i])
            norm[big] += norm[w] - 1
            norm[w] = -1
    tab = fse_table(norm, log)
    n = len(given)
    chains = [None, None]
    for j in (0, 1):
        syms = given[j::2]
        chains[j] = fse_chain(tab, syms, need_bits_last=((n - 2) % 2 == j))
    states = [chains[i % 2][i // 2] for i in range(n)]
    b = Back()
    b.add(states[0], log)
    b.add(states[1], log)
    for i in range(n - 2):
        _, nb, base = tab[states[i]]
        b.add(states[i + 2] - base, nb)
    body = ncount(norm, log) + b.bytes()
    assert len(body) < 128, len(body)
    return bytes([len(body)]) + body


def huf_stream(data, codes):
    b = Back()
    b.add_str(''.join(codes[x] for x in data))
    return b


def lit_header(ltype, sf, regen, comp=None):
    """The literals section header in the size format the caller names, not the smallest fit."""
    if ltype < 2:
        if sf in (0, 2):                        # (one bit says "1 byte": 10 is that form with an odd size)
            assert regen < 32 and sf == 2 * (regen & 1)
            return bytes([ltype | regen << 3])
        n = 2 if sf == 1 else 3
        assert regen < 1 << (8 * n - 4)
        return (ltype | sf << 2 | regen << 4).to_bytes(n, 'little')
    bits, n = {0: (10, 3), 1: (10, 3), 2: (14, 4), 3: (18, 5)}[sf]
    assert regen < 1 << bits and comp < 1 << bits, (regen, comp, sf)
    return (ltype | sf << 2 | regen << 4 | comp << (4 + bits)).to_bytes(n, 'little')


class Raw:
    def __init__(self, data, sf=None):
        self.data = bytes(data)
        self.sf = sf if sf is not None else 2 * (len(data) & 1) if len(data) < 32 else 1 if len(data) < 4096 else 3

    def encode(self, frame):
        return lit_header(0, self.sf, len(self.data)) + self.data


class Rle:
    def __init__(self, byte, n, sf=None):
        self.data = bytes([byte]) * n
        self.byte = byte
        self.sf = sf if sf is not None else 2 * (n & 1) if n < 32 else 1 if n < 4096 else 3

    def encode(self, frame):
        return lit_header(1, self.sf, len(self.data)) + bytes([self.byte])


class Huf:
    """Huffman-coded literals.  ``given``: the weights the description lists (the last one is
    implied), or None for treeless literals (the tree of the block before); ``tree``: 'direct' or
    'fse'; ``streams`` 1 or 4; ``sf`` the size format (0: 1 stream; 1, 2, 3: 4 streams of 10, 14
    and 18-bit sizes), by default the smallest that fits."""

    def __init__(self, data, given=None, streams=1, sf=None, tree='direct', **fse_args):
        self.data = bytes(data)
        self.given, self.streams, self.sf, self.tree, self.fse_args = given, streams, sf, tree, fse_args

    def encode(self, frame):
        if self.given is not None:
            weights, log = full_weights(self.given)
            desc = tree_direct(self.given) if self.tree == 'direct' else tree_fse(self.given, **self.fse_args)
            frame.tree = (weights, log)
        else:
            weights, log = frame.tree
            desc = b''
        codes = huf_codes(weights, log)
        if self.streams == 1:
            payload = huf_stream(self.data, codes).bytes()
        else:
            seg = (len(self.data) + 3) // 4
            parts = [huf_stream(self.data[k * seg:(k + 1) * seg], codes).bytes() for k in range(4)]
            payload = b''.join(struct.pack('<H', len(p)) for p in parts[:3]) + b''.join(parts)
        comp = len(desc) + len(payload)
        sf = self.sf
        if sf is None:
            sf = 0 if self.streams == 1 else 1 if max(len(self.data), comp) < 1024 else \
                2 if max(len(self.data), comp) < 16384 else 3
        assert (sf == 0) == (self.streams == 1)
        return lit_header(2 if self.given is not None else 3, sf, len(self.data), comp) + desc + payload


def equal_weights(n):
    """The description of n = 2^k symbols 0..n-1 with codes of k bits: n - 1 weights of 1."""
    return [1] * (n - 1)


# ---- sequences ----------------------------------------------------------------------------------
def seq_count(n, form=None):
    form = form or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert 0 < n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
    return b'\xff' + struct.pack('<H', n - 0x7F00)


def fit(which, codes, log=None, less_than_one=(), heavy=None):
    """A compressed-mode table spec that holds ``codes`` (5 bits of accuracy unless said)."""
    log = log or max(5, (len(set(codes)) - 1).bit_length())
    return ('fse', spread(codes, log, less_than_one, heavy), log)


def resolve(which, spec, prev):
    """A table spec -> (mode, description bytes, decoding table, log)."""
    if spec[0] == 'pre':
        norm, log = PRE_NORM[which]
        return 0, b'', fse_table(norm, log), log
    if spec[0] == 'rle':
        return 1, bytes([spec[1]]), [(spec[1], 0, 0)], 0
    if spec[0] == 'fse':
        norm, log = spec[1], spec[2]
        return 2, ncount(norm, log, *spec[3:]), fse_table(norm, log), log
    assert prev is not None, 'repeat mode with no table before it'
    return 3, b'', prev[0], prev[1]


def seq_section(seqs, specs, prev, count_form=None, reserved=0, extra_bits=0):
    """The sequences section: count, modes, table descriptions, bitstream.  ``prev``: the tables
    of the block before {which: (table, log)}, replaced by this block's.  ``extra_bits``: zeros
    written behind the last field (a stream not consumed exactly), or, negative, bits cut off it."""
    if not seqs:
        return b'\0'
    out = seq_count(len(seqs), count_form)
    modes, descs, tabs = reserved, b'', {}
    for which, shift in zip(TABLES, (6, 4, 2)):
        mode, desc, tab, log = resolve(which, specs[which], prev.get(which))
        modes |= mode << shift
        descs += desc
        tabs[which] = prev[which] = (tab, log)
    col = {'ll': 0, 'ml': 2, 'of': 4}
    chains = {w: fse_chain(tabs[w][0], [q[col[w]] for q in seqs]) for w in TABLES}
    b = Back()
    for w in TABLES:
        b.add(chains[w][0], tabs[w][1])
    for i, (lc, lx, mc, mx, oc, ox) in enumerate(seqs):
        b.add(ox, oc)
        b.add(mx, ML_BITS[mc])
        b.add(lx, LL_BITS[lc])
        if i + 1 < len(seqs):
            for w in ('ll', 'ml', 'of'):
                _, nb, base = tabs[w][0][chains[w][i]]
                b.add(chains[w][i + 1] - base, nb)
    if extra_bits < 0:                          # (the last field cut short)
        s = ''.join(b.parts)
        b.parts, b.bits = [s[:extra_bits]], b.bits + extra_bits
    else:
        b.add(0, extra_bits)
    return out + bytes([modes]) + descs + b.bytes()


# ---- the replay ---------------------------------------------------------------------------------
def take_offset(rep, value, ll):
    """The offset of a sequence with offset value ``value`` and ``ll`` literals in front (RFC 8878,
    3.1.1.5); ``rep``, the three repeat offsets, updated in place."""
    if value > 3:
        offset = value - 3
        rep[:] = [offset, rep[0], rep[1]]
        return offset
    k = value - 1 + (1 if ll == 0 else 0)
    if k == 0:
        return rep[0]
    offset = rep[k] if k < 3 else (rep[0] - 1 or 1)          # (0 is not an offset: libzstd makes it 1)
    rep[:] = [offset, rep[0], rep[2] if k == 1 else rep[1]]
    return offset


def replay(out, rep, literals, seqs):
    """Literals and sequences executed on ``out`` (a bytearray) by the rules of RFC 8878, 3.1.1.4
    and 3.1.1.5; ``rep``: the three repeat offsets, updated in place."""
    at = 0
    for lc, lx, mc, mx, oc, ox in seqs:
        ll, ml, value = LL_BASE[lc] + lx, ML_BASE[mc] + mx, (1 << oc) + ox
        assert at + ll <= len(literals), 'a literal length beyond the literals left'
        out += literals[at:at + ll]
        at += ll
        offset = take_offset(rep, value, ll)
        assert 0 < offset <= len(out), 'an offset beyond the bytes produced'
        if offset >= ml:
            out += out[len(out) - offset:len(out) - offset + ml]
        else:
            period = bytes(out[-offset:])
            out += (period * (ml // offset + 1))[:ml]
    out += literals[at:]


# ---- blocks and frames --------------------------------------------------------------------------
def frame_header(content, single=True, window=None, fcs=None, reserved=0, checksum=0, dict_id=None,
                 dict_bytes=0):
    """``fcs``: the width of the content size in bytes (0: none), by default the smallest;
    ``window``: the window descriptor's byte, for frames that are not single-segment."""
    if fcs is None:
        fcs = 1 if content < 256 and single else 2 if 256 <= content < 65792 else 4 if content < 1 << 32 else 8
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs]
    assert not (fcs == 1 and not single) and not (fcs == 0 and single)
    fhd = flag << 6 | (1 if single else 0) << 5 | reserved << 3 | checksum << 2 | {0: 0, 1: 1, 2: 2, 4: 3}[dict_bytes]
    out = struct.pack('<IB', MAGIC, fhd)
    if not single:
        out += bytes([window])
    out += (dict_id or 0).to_bytes(dict_bytes, 'little')
    if fcs:
        out += (content - 256 if fcs == 2 else content).to_bytes(fcs, 'little')
    return out


def block(last, btype, body, size=None):
    """A block header and what follows it; ``size`` is what the header states (an RLE block's
    length; by default the body's length: it may lie)."""
    size = len(body) if size is None else size
    assert size < 1 << 21
    return (last | btype << 1 | size << 3).to_bytes(3, 'little') + body


class Frame:
    """Blocks appended one by one, replayed as they are, the tables, the tree and the repeat
    offsets carried from one to the next as a decoder carries them."""

    def __init__(self, **header):
        self.header = header
        self.blocks = []                       # (type, body, stated size)
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.prev = {}
        self.tree = None
        self.lits = []

    def raw(self, data):
        self.blocks.append((0, bytes(data), None))
        self.out += data
        return self

    def rle(self, byte, n):
        self.blocks.append((1, bytes([byte]), n))
        self.out += bytes([byte]) * n
        return self

    def comp(self, lit, seqs=(), ll=PRE, of=PRE, ml=PRE, **section):
        seqs = list(seqs)
        body = lit.encode(self) + seq_section(seqs, {'ll': ll, 'of': of, 'ml': ml}, self.prev, **section)
        assert len(body) < 131072, len(body)
        self.blocks.append((2, body, None))
        self.lits.append(lit)
        replay(self.out, self.rep, lit.data, seqs)
        return self

    def put(self, btype, body, size=None):
        """a block of any bytes: not replayed"""
        self.blocks.append((btype, bytes(body), size))
        return self

    def body(self):
        n = len(self.blocks)
        return b''.join(block(1 if k + 1 == n else 0, t, b, size) for k, (t, b, size) in enumerate(self.blocks))

    def done(self):
        """(frame, content)"""
        content = bytes(self.out)
        return frame_header(len(content), **self.header) + self.body(), content


def rnd(n, seed, symbols=256):
    return np.random.RandomState(seed).randint(0, symbols, size=n).astype(np.uint8).tobytes()


def xxh64(data, seed=0):
    """XXH64 (the frame's content checksum is its low 32 bits)."""
    p1, p2, p3, p4, p5 = (11400714785074694791, 14029467366897019727, 1609587929392839161,
                          9650029242287828579, 2870177450012600261)
    m = (1 << 64) - 1

    def rotl(x, r):
        return ((x << r) | (x >> (64 - r))) & m

    def lane(acc, v):
        return rotl((acc + v * p2) & m, 31) * p1 & m

    n, i = len(data), 0
    if n >= 32:
        v = [(seed + p1 + p2) & m, (seed + p2) & m, seed, (seed - p1) & m]
        while i + 32 <= n:
            for k in range(4):
                v[k] = lane(v[k], int.from_bytes(data[i + 8 * k:i + 8 * k + 8], 'little'))
            i += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & m
        for k in range(4):
            h = ((h ^ lane(0, v[k])) * p1 + p4) & m
    else:
        h = (seed + p5) & m
    h = (h + n) & m
    while i + 8 <= n:
        h = (rotl(h ^ lane(0, int.from_bytes(data[i:i + 8], 'little')), 27) * p1 + p4) & m
        i += 8
    if i + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[i:i + 4], 'little') * p1 & m), 23) * p2 + p3) & m
        i += 4
    while i < n:
        h = rotl(h ^ (data[i] * p5 & m), 11) * p1 & m
        i += 1
    h ^= h >> 33
    h = h * p2 & m
    h ^= h >> 29
    h = h * p3 & m
    return h ^ (h >> 32)


# ---- the families -------------------------------------------------------------------------------
ROOM = {}                   # refused case -> the capacity it is decoded into
# what differs between libzstd versions (judged one-sidedly: where the model accepts, libzstd must)
VERSION_DEPENDENT = ('b_bad_compressed_2_bytes', 'd_rep0_minus_1_is_0', 'c_streams4_of_3', 'c_streams4_of_4',
                     'c_bad_streams4_of_1', 'c_bad_streams4_of_2', 'c_bad_streams4_of_5')


def _ok(cases, name, fr):
    frame, content = fr.done()
    cases.append((name, frame, content, None))
    return fr


def _bad(cases, name, frame, status, room=64):
    ROOM[name] = room
    cases.append((name, bytes(frame), None, status))


def one_block(content, body, **header):
    return frame_header(content, **header) + block(1, 2, body)


def family_a():
    c = []
    _ok(c, 'a_fcs1_5', Frame().raw(b'hello'))
    _ok(c, 'a_fcs1_0', Frame().raw(b''))
    _ok(c, 'a_fcs2_256', Frame().raw(rnd(256, 1)))
    _ok(c, 'a_fcs2_65791', Frame(fcs=2).raw(rnd(65791, 2)))
    _ok(c, 'a_fcs4_5', Frame(fcs=4).raw(b'hello'))
    _ok(c, 'a_fcs4_300', Frame(fcs=4).raw(rnd(300, 3)))
    _ok(c, 'a_fcs4_65792', Frame().raw(rnd(65792, 4)))
    _ok(c, 'a_fcs8_5', Frame(fcs=8).raw(b'hello'))
    _ok(c, 'a_fcs8_300', Frame(fcs=8).raw(rnd(300, 5)))
    for mantissa in range(8):                   # windows of 1024 + 128 * mantissa; the match within it
        _ok(c, 'a_window_m%d' % mantissa, Frame(single=False, window=mantissa, fcs=(2, 4, 8)[mantissa % 3])
            .raw(rnd(1100, 10 + mantissa)).comp(Raw(b'ab'), [S(1, 20, 1024)]))
    _ok(c, 'a_window_log31', Frame(single=False, window=21 << 3, fcs=4).raw(rnd(40, 6)).comp(Raw(b'a'), [S(1, 9, 30)]))
    body = block(1, 0, b'hello')
    _bad(c, 'a_bad_window_log32', frame_header(5, single=False, window=22 << 3, fcs=4) + body, UNSUPPORTED)
    _bad(c, 'a_bad_reserved_bit', frame_header(5, reserved=1) + body, UNSUPPORTED)
    _bad(c, 'a_checksum', frame_header(5, checksum=1) + body + struct.pack('<I', xxh64(b'hello') & 0xFFFFFFFF),
         UNSUPPORTED)
    for n in (1, 2, 4):
        _bad(c, 'a_dictionary_id_%d_zero' % n, frame_header(5, dict_bytes=n, dict_id=0) + body, UNSUPPORTED)
        _bad(c, 'a_bad_dictionary_id_%d' % n, frame_header(5, dict_bytes=n, dict_id=7) + body, UNSUPPORTED)
    _bad(c, 'a_no_content_size', frame_header(0, single=False, window=0, fcs=0) + body, UNSUPPORTED)
    whole = frame_header(5) + body
    _bad(c, 'a_skippable_in_front', struct.pack('<II', 0x184D2A50, 4) + b'abcd' + whole, BAD_MAGIC)
    _bad(c, 'a_second_frame_behind', whole + whole, TRAILING)
    return c


def family_b():
    c = []
    for n in (0, 1, 131072, 131073, 1 << 20):
        _ok(c, 'b_raw_%d' % n, Frame().raw(rnd(n, 20 + n % 7)))
        _ok(c, 'b_rle_%d' % n, Frame().rle(0x5A, n))
    fr = Frame()
    for b in rnd(300, 21):
        fr.raw(bytes([b]))
    _ok(c, 'b_300_raw_blocks', fr)
    _ok(c, 'b_empty_last_raw', Frame().raw(b'abc').rle(7, 9).raw(b''))
    _bad(c, 'b_bad_type_3', frame_header(0) + block(1, 3, b''), BAD_BLOCK)
    _bad(c, 'b_bad_compressed_2_bytes', one_block(0, lit_header(0, 0, 0) + b'\0'), BAD_BLOCK)
    big = Raw(rnd(131068, 22)).encode(None) + b'\0'
    assert len(big) == 131072
    _bad(c, 'b_bad_compressed_131072', one_block(131068, big), BAD_BLOCK, room=131072)
    _bad(c, 'b_bad_block_overruns_content', frame_header(5) + block(1, 0, b'abcdef'), BAD_SIZE)
    _bad(c, 'b_bad_rle_overruns_content', frame_header(5) + block(1, 1, b'a', 6), BAD_SIZE)
    _bad(c, 'b_bad_one_byte_short', frame_header(6) + block(1, 0, b'abcde'), BAD_SIZE)
    return c


def symbols_of(given, n, seed):
    """n literals that use every symbol of the tree the weights describe"""
    weights, _ = full_weights(given)
    have = [s for s, w in enumerate(weights) if w]
    r = np.random.RandomState(seed)
    data = have + [have[k] for k in r.randint(0, len(have), size=max(0, n - len(have)))]
    return bytes(data[:n]) if n < len(have) else bytes(data)


def family_c():
    c = []
    four = equal_weights(4)
    # every size format of every literals type, small sizes in wide fields included
    for sf in range(4):
        n = 4 if sf == 0 else 5
        _ok(c, 'c_raw_sf%d_%d' % (sf, n), Frame().comp(Raw(b'abcde'[:n], sf=sf)))
        _ok(c, 'c_rle_sf%d_%d' % (sf, n + 2), Frame().comp(Rle(0x41, n + 2, sf=sf)))
        streams = 1 if sf == 0 else 4
        _ok(c, 'c_huffman_sf%d_6' % sf, Frame().comp(Huf(b'\0\1\2\3\3\1', four, streams, sf)))
        _ok(c, 'c_treeless_sf%d_6' % sf, Frame().comp(Huf(b'\0\1\2\3\3\1', four, 4 if sf == 0 else 1))
            .comp(Huf(b'\3\1\0\0\2\1', None, streams, sf)))
    _ok(c, 'c_raw_sf1_4095', Frame().comp(Raw(rnd(4095, 30), sf=1)))
    _ok(c, 'c_raw_sf3_70000', Frame().comp(Raw(rnd(70000, 31), sf=3)))
    _ok(c, 'c_raw_0', Frame().comp(Raw(b'', sf=1)))
    _ok(c, 'c_rle_0', Frame().comp(Rle(9, 0)))
    _ok(c, 'c_rle_sf1_4095', Frame().comp(Rle(9, 4095, sf=1)))
    _ok(c, 'c_rle_131072', Frame().comp(Rle(9, 131072, sf=3)))
    _ok(c, 'c_huffman_sf2_16383', Frame().comp(Huf(rnd(16383, 32, 4), four, 4, 2)))
    _ok(c, 'c_huffman_sf3_131072', Frame().comp(Huf(rnd(131072, 33, 4), four, 4, 3)))
    # direct weights
    for name, given in (('1', [1]), ('2_implied_largest', [1, 1]), ('3_implied_largest', [2, 1, 1]),
                        ('2_implied_smallest', [2, 1]), ('3_implied_smallest', [3, 2, 1]),
                        ('127', [1] * 126 + [2]), ('128', [1] * 128), ('5_zeros_between', [2, 0, 0, 1, 0]),
                        ('depth_11', [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10])):
        for streams in (1, 4):
            _ok(c, 'c_direct_%s_x%d' % (name, streams),
                Frame().comp(Huf(symbols_of(given, 300, len(given)), given, streams)))
    # alphabets of equal-length codes: a piece that starts inside a code never finds the boundary
    for n in (2, 4, 8, 64, 128):
        _ok(c, 'c_equal_%d_x1' % n, Frame().comp(Huf(rnd(1023, 40 + n, n), equal_weights(n), 1)))
        _ok(c, 'c_equal_%d_x4' % n, Frame().comp(Huf(rnd(4001, 41 + n, n), equal_weights(n), 4)))
    # FSE-compressed weights
    fse = (('log6_even', [1, 1, 2, 3, 3, 4, 4, 0], {}), ('log5_even', [1, 1, 2, 3, 3, 4, 4, 0], {'log': 5}),
           ('log6_odd', [1, 1, 2, 3, 4, 4, 0], {}), ('log5_odd', [1, 1, 2, 3, 4, 4, 0], {'log': 5}),
           ('3_symbols', [2, 1], {}), ('3_symbols_log5', [2, 1], {'log': 5}),
           ('less_than_one', [1, 1, 1, 1, 2, 2, 3, 5], {'less_than_one': (3, 5)}),
           ('129', [1] * 128 + [8], {}), ('254', [1] * 252 + [2, 2], {}), ('255', [1] * 254 + [2], {}),
           ('169_mixed', [1, 2] * 84 + [2], {'log': 5}))
    for name, given, args in fse:
        for streams in (1, 4):
            _ok(c, 'c_fse_%s_x%d' % (name, streams),
                Frame().comp(Huf(symbols_of(given, 400, len(given)), given, streams, tree='fse', **args)))
    # streams
    for n in range(1, 10):                     # 1-bit codes: the marker at every position of its byte
        _ok(c, 'c_stream1_of_%d' % n, Frame().comp(Huf(rnd(n, 50 + n, 2), [1], 1)))
    for n in (3, 4, 6, 7, 8, 9, 64, 65):
        _ok(c, 'c_streams4_of_%d' % n, Frame().comp(Huf(rnd(n, 60 + n, 2), [1], 4)))
        if n >= 6:
            _ok(c, 'c_streams4_of_%d_wide' % n, Frame().comp(Huf(rnd(n, 61 + n, 8), equal_weights(8), 4)))
    _ok(c, 'c_streams4_under_16_bits', Frame().comp(Huf(rnd(20, 70, 4), four, 4)))
    # treeless literals
    _ok(c, 'c_treeless_across_raw_block', Frame().comp(Huf(rnd(50, 71, 4), four, 1)).raw(b'between')
        .comp(Huf(rnd(70, 72, 4), None, 4)))
    _ok(c, 'c_treeless_across_raw_literals', Frame().comp(Huf(rnd(50, 73, 4), four, 4))
        .comp(Raw(b'raw literals'), [S(3, 4, 2)]).comp(Rle(3, 10)).comp(Huf(rnd(70, 74, 4), None, 1), [S(5, 9, 60)]))
    _ok(c, 'c_treeless_twice', Frame().comp(Huf(rnd(50, 75, 8), equal_weights(8), 4))
        .comp(Huf(rnd(9, 76, 8), None, 4)).comp(Huf(rnd(1000, 77, 8), None, 1)))

    # refused
    def huf_frame(regen, desc, payload, sf=0, ltype=2):
        return one_block(regen, lit_header(ltype, sf, regen, len(desc) + len(payload)) + desc + payload + b'\0')

    deep = [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    frame, content = Frame().comp(Huf(symbols_of(deep, 300, 1), deep, 1)).done()
    _bad(c, 'c_depth_12', frame, BAD_TREE, room=len(content))
    one = huf_stream(b'\0\1\0\1', {0: '0', 1: '1'}).bytes()
    _bad(c, 'c_bad_weights_no_power_of_two', huf_frame(4, tree_direct([2, 2, 1]), one), BAD_TREE)
    _bad(c, 'c_bad_no_weight_1', huf_frame(4, tree_direct([2]), one), BAD_TREE)
    _bad(c, 'c_bad_all_weights_zero', huf_frame(4, tree_direct([0, 0]), one), BAD_TREE)
    _bad(c, 'c_bad_weight_12', huf_frame(4, tree_direct([12, 1]), one), BAD_TREE)
    _bad(c, 'c_bad_tree_fills_compressed_size', huf_frame(4, tree_direct([1]), b''), BAD_LITERALS)
    for n in (1, 2, 5):
        frame, _ = Frame().comp(Huf(rnd(n, 80 + n, 2), [1], 4)).done()
        _bad(c, 'c_bad_streams4_of_%d' % n, frame, BAD_LITERALS)
    parts = [huf_stream(bytes(2), {0: '0', 1: '1'}).bytes()] * 4
    jump = struct.pack('<HHH', 1000, 1, 1)
    _bad(c, 'c_bad_jump_table_beyond_payload', huf_frame(8, tree_direct([1]), jump + b''.join(parts), sf=1),
         BAD_LITERALS)
    _bad(c, 'c_bad_stream_ends_in_0', huf_frame(4, tree_direct([1]), one + b'\0'), BAD_BITSTREAM)
    _bad(c, 'c_bad_stream_one_symbol_more', huf_frame(3, tree_direct([1]), one), BAD_BITSTREAM)
    _bad(c, 'c_bad_stream_one_symbol_fewer', huf_frame(5, tree_direct([1]), one), BAD_BITSTREAM)
    uneven = [huf_stream(bytes(k), {0: '0', 1: '1'}).bytes() for k in (3, 2, 2, 1)]
    _bad(c, 'c_bad_streams4_uneven', huf_frame(8, tree_direct([1]), struct.pack('<HHH', 1, 1, 1) + b''.join(uneven),
                                               sf=1), BAD_BITSTREAM)
    _bad(c, 'c_bad_treeless_first', huf_frame(4, b'', one, ltype=3), BAD_TREE)
    return c


BASE_SEQS = [S(2, 4, 5)] * 3                    # codes 2, 1 and 3: what every table of the mode cases holds
BASE_CODE = {'ll': 2, 'of': 3, 'ml': 1}


def mode_spec(which, mode, log=None):
    code = BASE_CODE[which]
    return (PRE, ('rle', code), fit(which, [code, code + 1], log, heavy=code + 1), REP)[mode]


def counted(n, form):
    """n sequences of one literal and a match of 3 at the repeat offset: all-RLE tables, no bits"""
    return Frame().comp(Raw(rnd(n, n)), [R(1, 3, 1)] * n, ll=('rle', 1), of=('rle', 0), ml=('rle', 0),
                        count_form=form)


COPY_LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 70000)
MATCH_OFFSETS = tuple(range(1, 71)) + (127, 128, 129, 1000)
MATCH_LENGTHS = (3, 4, 7, 63, 64, 65, 130, 1000)
FIT_GAPS = (0, 3, 15, 16, 17, 1030)


def family_d():
    c = []
    # the count's forms
    for n, form in ((1, 1), (1, 2), (5, 2), (127, 1), (127, 2), (128, 2), (0x7EFF, 2), (0x7F00, 3), (0x7F07, 3)):
        _ok(c, 'd_count_%d_form%d' % (n, form), counted(n, form))
    # modes: all 64 combinations, those with a repeat in them behind a block of compressed tables
    for a in range(4):
        for b in range(4):
            for m in range(4):
                fr = Frame().raw(rnd(8, 90))
                if 3 in (a, b, m):
                    fr.comp(Raw(rnd(6, 91)), BASE_SEQS, ll=mode_spec('ll', 2, 6), of=mode_spec('of', 2, 6),
                            ml=mode_spec('ml', 2, 6))
                fr.comp(Raw(rnd(7, 92)), BASE_SEQS, ll=mode_spec('ll', a), of=mode_spec('of', b), ml=mode_spec('ml', m))
                _ok(c, 'd_modes_%d%d%d' % (a, b, m), fr)
    varied = [S(2, 4, 5), S(3, 5, 6), S(2, 5, 5), S(3, 4, 6), S(2, 4, 6)]
    for first in (0, 1, 2):
        seqs = BASE_SEQS if first == 1 else varied
        args = dict(ll=mode_spec('ll', first), of=mode_spec('of', first), ml=mode_spec('ml', first))
        rep = dict(ll=REP, of=REP, ml=REP)
        lits = rnd(40, 93)
        name = 'd_repeat_after_' + MODE_NAMES[first]
        _ok(c, name, Frame().raw(rnd(8, 94)).comp(Raw(lits), seqs, **args).comp(Raw(lits), seqs[::-1], **rep)
            .comp(Raw(lits), seqs, **rep))
        _ok(c, name + '_across_raw_block', Frame().raw(rnd(8, 95)).comp(Raw(lits), seqs, **args).raw(b'between')
            .rle(4, 11).comp(Raw(lits), seqs[::-1], **rep))
        _ok(c, name + '_across_no_sequences', Frame().raw(rnd(8, 96)).comp(Raw(lits), seqs, **args)
            .comp(Raw(b'no sequences')).comp(Rle(8, 3)).comp(Raw(lits), seqs[::-1], **rep))
    # table descriptions
    seqs = [S(2, 4, 5), S(3, 5, 6), S(2, 5, 6)]
    for log in ((5, 5, 5), (9, 8, 9), (6, 7, 8)):
        _ok(c, 'd_accuracy_%d_%d_%d' % log, Frame().raw(rnd(8, 97)).comp(
            Raw(rnd(9, 98)), seqs, ll=fit('ll', [2, 3], log[0]), of=fit('of', [3], log[1]), ml=fit('ml', [1, 2], log[2])))
    _ok(c, 'd_less_than_one', Frame().raw(rnd(8, 99)).comp(
        Raw(rnd(9, 100)), seqs, ll=fit('ll', [0, 2, 3, 9], 5, less_than_one=(2, 9)),
        of=fit('of', [1, 3, 7], 5, less_than_one=(3, 7)), ml=fit('ml', [1, 2, 30], 6, less_than_one=(1, 2, 30))))
    gaps = [0, 2, 6, 13, 40, 52]                 # zeros: 1, 3, 6, 26 and 11 of them in a run
    seqs = [(k % 4, 0, mc, 0, 3, k % 8) for k, mc in enumerate(gaps[:-1] * 2)]
    for long_runs in (True, False):
        _ok(c, 'd_zero_runs_' + ('ffff' if long_runs else '2bit'), Frame().raw(rnd(8, 101)).comp(
            Raw(rnd(40, 102)), seqs, ll=fit('ll', [0, 1, 2, 3, 35], 6), of=fit('of', [3, 31], 5),
            ml=('fse', spread(gaps, 6), 6, long_runs)))
    _ok(c, 'd_zero_runs_48', Frame().raw(rnd(8, 103)).comp(
        Raw(rnd(40, 104)), [(1, 0, mc, 0, 3, 1) for mc in (1, 51, 1)], ml=('fse', spread([1, 51, 52], 5, heavy=51), 5)))
    # every literal-length and match-length code, the extra bits all 0 and all 1; the literals a
    # 1-bit alphabet, the matches at offset 1
    fr, seqs, lits, seed = Frame().raw(b'Q'), [], 0, 110
    for ones in (0, 1):
        for k in range(53):
            lc = k % 36
            q = (lc, ((1 << LL_BITS[lc]) - 1) * ones, k, ((1 << ML_BITS[k]) - 1) * ones, 2, 0)
            if lits + LL_BASE[lc] + q[1] > 131072:
                fr.comp(Huf(rnd(lits, seed, 2), [1], 4, 3), seqs)
                seqs, lits, seed = [], 0, seed + 1
            seqs.append(q)
            lits += LL_BASE[lc] + q[1]
    _ok(c, 'd_every_ll_and_ml_code', fr.comp(Huf(rnd(lits + 3, seed, 2), [1], 4, 3), seqs))
    # offset codes 0 to 21, the far ones into 2 MiB of RLE blocks
    fr = Frame()
    for k in range(64):
        fr.rle(k + 1, 32768 + k)
    fr.raw(rnd(64, 120))
    seqs = [R(1, 40, 1), R(1, 40, 2), R(1, 40, 3)]
    for oc in range(2, 22):
        for ox in (0, 2000 if oc == 21 else (1 << oc) - 1, 2000 % (1 << oc)):
            seqs.append(ll_code(1) + ml_code(40 + oc) + (oc, ox))
    _ok(c, 'd_offset_codes_0_to_21', fr.comp(Raw(rnd(len(seqs), 121)), seqs))
    # the repeat offsets: every row of the table, carried across blocks
    rows = [S(1, 3, 7), S(1, 3, 5), S(1, 3, 3), R(0, 4, 1), R(0, 4, 2), R(0, 4, 3), R(1, 4, 1), R(1, 4, 2),
            R(1, 4, 3), R(2, 5, 3), R(0, 5, 2), R(0, 6, 1)]
    more = [R(1, 5, 3), R(0, 5, 3), R(1, 5, 2), R(0, 7, 1), R(2, 3, 1), R(0, 4, 2)]
    _ok(c, 'd_repeat_offsets', Frame().raw(rnd(16, 122)).comp(Raw(rnd(12, 123)), rows)
        .comp(Raw(b'no sequences: the offsets stay')).raw(b'raw').rle(1, 5).comp(Raw(rnd(9, 124)), more)
        .comp(Rle(2, 8), more[::-1]))
    for value, ll in ((1, 1), (2, 4), (3, 8), (1, 9), (2, 9), (3, 9)):
        _ok(c, 'd_first_sequence_repeat_%d_of_%d' % (value, ll), Frame().comp(Raw(rnd(ll + 2, 125)), [R(ll, 6, value)]))
    _ok(c, 'd_rep0_minus_1_is_0', Frame().raw(rnd(9, 126)).comp(Raw(b'abc'), [S(1, 3, 1), R(0, 5, 3), R(1, 3, 1)]))
    # the device's match: offsets below, at and above the length, around 64 and 128
    seqs = [S(1 + k % 3, ml, off) for k, (off, ml) in
            enumerate((off, ml) for off in MATCH_OFFSETS for ml in MATCH_LENGTHS)]
    _ok(c, 'd_match_grid', Frame().raw(rnd(1024, 127)).comp(Raw(rnd(sum(LL_BASE[q[0]] for q in seqs), 128)), seqs))
    _ok(c, 'd_match_131074_offset_1', Frame().raw(rnd(65, 129)).comp(Raw(b'ab'), [S(1, 131074, 1)]))
    _ok(c, 'd_match_131074_offset_65', Frame().raw(rnd(65, 130)).comp(Raw(b'ab'), [S(1, 131074, 65)]))
    # the device's copy: literal runs around 16, 1,024 and 2,048, the raw ones at every alignment
    total = sum(COPY_LENGTHS) + 5
    for shift in range(16):
        seqs = [S(ll, 4 + k, 1 + k % (shift + 1)) for k, ll in enumerate(COPY_LENGTHS)]
        _ok(c, 'd_copy_raw_shift_%d' % shift, Frame().raw(rnd(shift + 1, 140 + shift))
            .comp(Raw(rnd(total, 160 + shift)), seqs))
    for shift in (0, 5):
        seqs = [S(ll, 4 + k, 1 + k % (shift + 1)) for k, ll in enumerate(COPY_LENGTHS[::-1])]
        _ok(c, 'd_copy_huffman_shift_%d' % shift, Frame().raw(rnd(shift + 1, 180 + shift))
            .comp(Huf(rnd(total, 181 + shift, 128), equal_weights(128), 4), seqs))
    # exact fit: the region as large as the content, the parked literals where the output lands
    for run, gaps in ((3000, FIT_GAPS), (70000, (0, 3, 17)), (1000, (0, 3))):
        for gap in gaps:
            run8 = run + (-(16 + 5 + 8 + run + gap)) % 8
            seqs = [S(5, 8, 2)] + ([S(run8, gap, 7)] if gap else [])
            fr = _ok(c, 'd_fit_%d_gap_%d' % (run, gap), Frame().raw(rnd(16, 190)).comp(
                Huf(rnd(5 + run8, 191 + gap, 128), equal_weights(128), 4 if run8 > 1023 else 1), seqs))
            assert len(fr.out) % 8 == 0
    # (a match is 3 bytes at least, so no exact fit leaves 1 or 2: the region's slack does - in a
    # region of 2 * ceil(content / 8) * 4 bytes the last literals move down by 8 - content % 8)
    for slack in (1, 2, 5, 7):
        run = 3000 + (8 - slack - (16 + 5 + 8 + 3000)) % 8
        fr = _ok(c, 'd_slack_%d' % slack, Frame().raw(rnd(16, 195)).comp(
            Huf(rnd(5 + run, 196 + slack, 128), equal_weights(128), 4), [S(5, 8, 2)]))
        assert (-len(fr.out)) % 8 == slack

    # refused
    def seq_frame(content, lit, section, head=b'', **header):
        return frame_header(content, **header) + head + block(1, 2, lit.encode(None) + section)

    abc = Raw(b'abc')
    _bad(c, 'd_bad_repeat_first', seq_frame(6, abc, b'\x01\xfc\x01'), BAD_SEQUENCES)
    ok = dict(ll=PRE, of=PRE, ml=PRE)
    _bad(c, 'd_reserved_mode_bits', seq_frame(6, abc, seq_section([S(3, 3, 1)], ok, {}, reserved=1)), BAD_SEQUENCES)
    _bad(c, 'd_bad_accuracy_10', seq_frame(6, abc, b'\x01\x80\x05\x00\x00\x00\x01'), BAD_FSE)
    whole = seq_section([S(3, 3, 1)] * 2, dict(ok, ll=fit('ll', [3, 20, 30], 9)), {})
    _bad(c, 'd_bad_description_cut', seq_frame(9, abc, whole[:3]), BAD_FSE)
    _bad(c, 'd_bad_symbol_36', seq_frame(6, abc, seq_section([S(3, 3, 1)], dict(ok, ll=fit('ll', [3, 36])), {})),
         BAD_FSE)
    _bad(c, 'd_bad_symbol_32_of_offsets', seq_frame(6, abc, seq_section(
        [S(3, 3, 1)], dict(ok, of=fit('of', [2, 32])), {})), BAD_FSE)
    section = bytearray(seq_section([S(3, 3, 1)], dict(ok, ll=('rle', 3)), {}))
    assert section[2] == 3
    section[2] = 36
    _bad(c, 'd_bad_rle_symbol_36', seq_frame(6, abc, bytes(section)), BAD_SEQUENCES)
    _bad(c, 'd_bad_literal_length', seq_frame(7, abc, seq_section([S(4, 3, 1)], ok, {})), BAD_SEQUENCES)
    _bad(c, 'd_bad_offset', seq_frame(6, abc, seq_section([S(2, 3, 3)], ok, {})), BAD_OFFSET)
    _bad(c, 'd_bad_first_repeat_4', seq_frame(6, abc, seq_section([R(3, 3, 2)], ok, {})), BAD_OFFSET)
    _bad(c, 'd_bad_first_repeat_8', seq_frame(10, Raw(b'abcdefg'), seq_section([R(7, 3, 3)], ok, {})), BAD_OFFSET)
    _bad(c, 'd_offset_beyond_window', seq_frame(2006, Raw(b'a'), seq_section([S(1, 5, 1500)], ok, {}),
                                                 head=block(0, 0, rnd(2000, 200)), single=False, window=0, fcs=2),
         BAD_OFFSET, room=2006)
    _bad(c, 'd_bits_left_over', seq_frame(6, abc, seq_section([S(3, 3, 1)], ok, {}, extra_bits=1)), BAD_BITSTREAM)
    _bad(c, 'd_byte_left_over', seq_frame(6, abc, seq_section([S(3, 3, 1)], ok, {}, extra_bits=8)), BAD_BITSTREAM)
    _bad(c, 'd_one_bit_short', seq_frame(6, abc, seq_section([S(3, 3, 1)], ok, {}, extra_bits=-1)), BAD_BITSTREAM)
    _bad(c, 'd_bad_no_marker', seq_frame(6, abc, seq_section([S(3, 3, 1)], ok, {}) + b'\0'), BAD_BITSTREAM)
    return c


# ---- random by construction ---------------------------------------------------------------------
def random_weights(r, direct):
    """The weights a description gives, of a random complete tree over random symbols"""
    k = int(r.randint(2, 40))
    lens = [1, 1]
    while len(lens) < k:
        i = int(r.randint(0, len(lens)))
        if lens[i] < 11:
            lens[i] += 1
            lens.append(lens[i])
    log = max(lens)
    symbols = sorted(int(s) for s in r.choice(128 if direct else 256, size=len(lens), replace=False))
    given = [0] * symbols[-1]
    r.shuffle(lens)
    for s, l in zip(symbols[:-1], lens[:-1]):
        given[s] = log + 1 - l
    assert full_weights(given)[0][-1] == log + 1 - lens[-1]
    return given


def short(r, n):
    """a size format for n raw or RLE literals: any that holds n (an empty section in two bytes, so
    that the block has its three)"""
    return int(r.choice([sf for sf in (2 * (n & 1), 1, 3) if n < (32, 4096, 32, 1 << 20)[sf] and (n or sf == 1)]))


def random_literals(r, fr, n):
    kind = r.choice(['raw', 'rle', 'huffman', 'treeless'], p=[0.2, 0.1, 0.4, 0.3])
    if n == 0 or (kind == 'treeless' and fr.tree is None):
        kind = 'raw'
    if kind == 'raw':
        return Raw(rnd(n, int(r.randint(1 << 30))), sf=short(r, n))
    if kind == 'rle':
        return Rle(int(r.randint(256)), n, sf=short(r, n))
    given, tree, args = None, 'direct', {}
    if kind == 'huffman':
        tree = 'direct' if r.rand() < 0.5 else 'fse'
        given = random_weights(r, tree == 'direct')
        args = {'log': int(r.choice([5, 6]))} if tree == 'fse' else {}
        if tree == 'fse':
            try:
                tree_fse(given, **args)
            except AssertionError:              # (a description of 128 bytes or more: direct weights then)
                given, tree, args = random_weights(r, True), 'direct', {}
        weights = full_weights(given)[0]
    else:
        weights = fr.tree[0]
    have = np.array([s for s, w in enumerate(weights) if w], dtype=np.uint8)
    p = np.array([2.0 ** weights[s] for s in have])
    data = r.choice(have, size=n, p=p / p.sum()).astype(np.uint8).tobytes()
    streams = 4 if n >= 1024 or (n >= 6 and r.rand() < 0.5) else 1
    sizes = [1, 2, 3] if streams == 4 else [0]
    sf = int(r.choice(sizes)) if n < 1024 else int(r.choice([2, 3])) if n < 16384 else 3
    return Huf(data, given, streams, sf if r.rand() < 0.5 else None, tree, **args)


def random_table(r, which, codes, prev):
    codes = set(codes)
    can = [2]
    if max(codes) < len(PRE_NORM[which][0]):
        can.append(0)
    if len(codes) == 1:
        can.append(1)
    if prev is not None and codes <= set(s for s, _, _ in prev[0]):
        can += [3, 3]
    mode = int(r.choice(can))
    if mode == 2:
        low = max(5, (len(codes) - 1).bit_length())
        extra = [int(s) for s in r.randint(0, MAX_SYM[which] + 1, size=int(r.randint(0, 4)))]
        every = sorted(codes | set(extra))
        low = max(5, (len(every) - 1).bit_length())
        less = [s for s in every if r.rand() < 0.3]
        return fit(which, every, int(r.randint(low, MAX_LOG[which] + 1)), less_than_one=less,
                   heavy=int(r.choice(every)))
    return (PRE, ('rle', min(codes)), None, REP)[mode]


def random_frame(seed):
    r = np.random.RandomState(seed)
    header = {}
    if r.rand() < 0.3:
        header = {'single': False, 'window': int(r.randint(7, 12)) << 3 | int(r.randint(8)), 'fcs': int(r.choice([4, 8]))}
    elif r.rand() < 0.3:
        header = {'fcs': int(r.choice([4, 8]))}
    fr = Frame(**header)
    for _ in range(int(r.randint(1, 7))):
        kind = r.choice(['raw', 'rle', 'compressed'], p=[0.15, 0.15, 0.7])
        size = int(2 ** r.uniform(0, 13)) - 1
        if kind == 'raw':
            fr.raw(rnd(size, int(r.randint(1 << 30))))
            continue
        if kind == 'rle':
            fr.rle(int(r.randint(256)), size)
            continue
        n_lit = int(2 ** r.uniform(0, 12)) - 1
        lit = random_literals(r, fr, n_lit)
        seqs, left, rep, produced = [], n_lit, list(fr.rep), len(fr.out)
        for _ in range(int(r.choice([0, 1, 2, 5, 20, 130]))):
            ll = min(left, int(2 ** r.uniform(0, 8)) - 1 if r.rand() < 0.9 else left)
            ml = 3 + int(2 ** r.uniform(0, 10 if r.rand() < 0.9 else 12.5)) - 1
            if produced + ll == 0:
                ll, left = 1, max(left, 1)
                if n_lit == 0:
                    break
            q, value = None, int(r.randint(1, 4))
            if r.rand() < 0.4:
                trial = list(rep)
                if 0 < take_offset(trial, value, ll) <= produced + ll and not (value + (ll == 0) == 4 and rep[0] == 1):
                    q, rep = R(ll, ml, value), trial
            if q is None:
                offset = 1 + int(r.randint(0, min(produced + ll, 1 << int(r.randint(1, 17)))))
                q = S(ll, ml, offset)
                take_offset(rep, offset + 3, ll)
            seqs.append(q)
            left -= ll
            produced += ll + ml
            if produced > 60000:
                break
        tables = {w: random_table(r, w, [q[i] for q in seqs], fr.prev.get(w)) if seqs else PRE
                  for w, i in (('ll', 0), ('ml', 2), ('of', 4))}
        form = int(r.choice([f for f in (1, 2) if f == 2 or len(seqs) < 128])) if seqs else None
        fr.comp(lit, seqs, count_form=form, **tables)
        if len(fr.out) > 60000:
            break
    return fr


# ---- a walker: which parts of the format a valid frame uses -------------------------------------
def read_ncount(p):
    """(accuracy, bytes taken) of the distribution described at p"""
    word = int.from_bytes(p[:600], 'little')

    def bits(pos, n):
        return (word >> pos) & ((1 << n) - 1)

    log = bits(0, 4) + 5
    pos, remaining, threshold, nb, prev0 = 4, (1 << log) + 1, 1 << log, log + 1, False
    while remaining > 1:
        if prev0:
            while bits(pos, 16) == 0xFFFF:
                pos += 16
            while bits(pos, 2) == 3:
                pos += 2
            pos += 2
        small = 2 * threshold - 1 - remaining
        v = bits(pos, nb)
        if v & (threshold - 1) < small:
            count, pos = v & (threshold - 1), pos + nb - 1
        else:
            count, pos = (v - small if v >= threshold else v), pos + nb
        count -= 1
        remaining -= abs(count)
        prev0 = count == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    return log, (pos + 7) // 8


def walk(frame, info=None):
    """What a valid frame holds, added to ``info``: 'fcs' widths, 'windowed', 'blocks' types,
    'literals' {(raw|rle|huffman|treeless, size format)}, 'streams' {(1|4, literals)}, 'markers'
    {the marker's bit in the last byte of a single stream}, 'trees' {direct|fse}, 'depths' (of
    directly described trees), 'given' {how many weights given directly}, 'counts' {(form, sequences)},
    'modes' {(ll, of, ml)}, 'accuracy' {(table, log)}."""
    keys = ('fcs', 'windowed', 'blocks', 'literals', 'streams', 'markers', 'trees', 'depths', 'given', 'counts',
            'modes', 'accuracy')
    info = info if info is not None else {}
    for k in keys:
        info.setdefault(k, set())
    f = bytes(frame)
    assert struct.unpack('<I', f[:4])[0] == MAGIC
    single = (f[4] >> 5) & 1
    fcs = (single, 2, 4, 8)[f[4] >> 6]
    info['fcs'].add(fcs)
    info['windowed'].add(not single)
    at = 5 + (0 if single else 1) + fcs
    while True:
        bh = int.from_bytes(f[at:at + 3], 'little')
        at += 3
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        info['blocks'].add(('raw', 'rle', 'compressed')[btype])
        if btype == 2:
            _walk_block(f[at:at + size], info)
        at += 1 if btype == 1 else size
        if last:
            assert at == len(f)
            return info


def _walk_block(p, info):
    ltype, sf = p[0] & 3, (p[0] >> 2) & 3
    if ltype < 2:
        lh = 1 if not sf & 1 else 2 if sf == 1 else 3
        lit = int.from_bytes(p[:lh], 'little') >> (3 if lh == 1 else 4)
        at = lh + (lit if ltype == 0 else 1)
    else:
        lh, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        word = int.from_bytes(p[:5], 'little')
        lit, comp = (word >> 4) & ((1 << bits) - 1), (word >> (4 + bits)) & ((1 << bits) - 1)
        tree = 0
        if ltype == 2:
            hb = p[lh]
            kind = 'direct' if hb >= 128 else 'fse'
            info['trees'].add(kind)
            tree = 1 + ((hb - 127 + 1) // 2 if hb >= 128 else hb)
            if hb >= 128:
                given = [(p[lh + 1 + k // 2] >> (0 if k & 1 else 4)) & 15 for k in range(hb - 127)]
                weights, log = full_weights(given)
                info['depths'].add(log + 1 - min(w for w in weights if w))
                info['given'].add(len(given))
        info['streams'].add((1 if sf == 0 else 4, lit))
        if sf == 0:
            info['markers'].add(p[lh + comp - 1].bit_length() - 1)
        at = lh + comp
    info['literals'].add((('raw', 'rle', 'huffman', 'treeless')[ltype], sf))
    n = p[at]
    at += 1
    if not n:
        return
    form = 1
    if n == 255:
        n, at, form = p[at] + (p[at + 1] << 8) + 0x7F00, at + 2, 3
    elif n > 127:
        n, at, form = ((n - 128) << 8) + p[at], at + 1, 2
    info['counts'].add((form, n))
    modes = p[at]
    at += 1
    info['modes'].add((modes >> 6, (modes >> 4) & 3, (modes >> 2) & 3))
    for which, shift in zip(TABLES, (6, 4, 2)):
        mode = (modes >> shift) & 3
        if mode == 1:
            at += 1
        elif mode == 2:
            log, taken = read_ncount(p[at:])
            info['accuracy'].add((which, log))
            at += taken


_FAMILIES = None


def families():
    """{'A'..'D', 'R': [(name, frame, content | None, status | None)]}, built once per process"""
    global _FAMILIES
    if _FAMILIES is None:
        r = [('r_%03d' % seed,) + random_frame(seed).done() + (None,) for seed in range(300)]
        _FAMILIES = {'A': family_a(), 'B': family_b(), 'C': family_c(), 'D': family_d(), 'R': r}
        names = [x[0] for fam in _FAMILIES.values() for x in fam]
        assert len(names) == len(set(names))
    return _FAMILIES


def all_cases():
    return [x for fam in families().values() for x in fam]


def dump(path):
    """[u32 frame bytes][u32 capacity][frame] per case, valid ones also with room to spare"""
    with open(path, 'wb') as f:
        for name, frame, content, status in all_cases():
            rooms = [ROOM[name]] if content is None else [len(content), len(content) + 5]
            for room in rooms:
                f.write(struct.pack('<II', len(frame), room) + frame)


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--dump', 'usage: zstd_written.py --dump FILE'
    dump(sys.argv[2])
