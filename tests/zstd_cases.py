"""
zstd frames for the tests of the GPU's zstd decoder (deepbinner_amd/csrc/dbh_zstd_core.h): the
valid frames (streamvbyte bytes of signals, and inputs chosen for the parts of the format signal
data does not reach), a small frame walker that says which parts of the format a frame uses,
seeded mutants of the frames, and damaged streamvbyte bytes inside intact frames.  The frames are
made by the system's libzstd (vbz_fixtures.zstd_compress, and the advanced parameters through
ctypes); nothing here is committed as a file.
"""

import ctypes
import struct

import numpy as np

import vbz_fixtures

MAGIC = 0xFD2FB528
PAD = 64            # the decoder may read this far beyond a frame


def lib():
    z = vbz_fixtures.zstd_lib()
    if z is None:
        return None
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    z.ZSTD_compress2.restype = ctypes.c_size_t
    z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                 ctypes.c_size_t]
    z.ZSTD_compressStream2.restype = ctypes.c_size_t
    z.ZSTD_compressStream2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return z


def zstd_decompress(frame, capacity):
    """(bytes, None) if libzstd accepts the frame into ``capacity`` bytes, else (None, code)."""
    z = lib()
    out = ctypes.create_string_buffer(max(1, capacity))
    k = z.ZSTD_decompress(out, capacity, bytes(frame), len(frame))
    if z.ZSTD_isError(k):
        return None, k
    return out.raw[:k], None


# ZSTD_cParameter
C_LEVEL, C_WINDOWLOG, C_CONTENTSIZE, C_CHECKSUM, C_DICTID = 100, 101, 200, 201, 202


class _Buf(ctypes.Structure):
    _fields_ = [('p', ctypes.c_void_p), ('size', ctypes.c_size_t), ('pos', ctypes.c_size_t)]


def zstd_compress_adv(data, params=(), flush_at=()):
    """``data`` through ZSTD_compressStream2 with the parameters [(id, value)]; ``flush_at``: input
    offsets behind which the block at hand is ended (ZSTD_e_flush), so that a frame has several
    blocks, later ones free to reuse the tree and tables of the one before."""
    z = lib()
    data = bytes(data)
    cctx = z.ZSTD_createCCtx()
    try:
        for k, v in params:
            assert not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(cctx, k, v))
        cap = z.ZSTD_compressBound(len(data)) + 64 * (len(flush_at) + 1)
        dst = ctypes.create_string_buffer(cap)
        src = ctypes.create_string_buffer(data, max(1, len(data)))
        ob = _Buf(ctypes.cast(dst, ctypes.c_void_p), cap, 0)
        cuts = sorted(set(int(c) for c in flush_at if 0 < c < len(data))) + [len(data)]
        begin = 0
        for cut in cuts:
            ib = _Buf(ctypes.cast(src, ctypes.c_void_p), cut, begin)
            end = 2 if cut == len(data) else 1              # ZSTD_e_end / ZSTD_e_flush
            while True:
                left = z.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(ib), end)
                assert not z.ZSTD_isError(left)
                if left == 0 and ib.pos == ib.size:
                    break
            begin = cut
        return dst.raw[:ob.pos]
    finally:
        z.ZSTD_freeCCtx(cctx)


def random_walk(n, seed=0):
    r = np.random.RandomState(seed)
    steps = r.randint(-12, 13, size=n) + (r.rand(n) < 0.01) * r.randint(-300, 300, size=n)
    return (500 + np.cumsum(steps)).astype(np.int16)


SIGNAL_SIZES = (0, 1, 2, 3, 4, 5, 200, 4000, 27000, 100000, 400000, 1500000)
LEVELS = (1, 3, 9, 19)


def text_like(n, symbols, seed):
    r = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, symbols + 1) ** 1.3
    return r.choice(symbols, size=n, p=p / p.sum()).astype(np.uint8).tobytes()


def wordy(n, seed):
    """Bytes with repeats at recurring distances and literals between them (repeat offsets, all
    the sequence modes over several blocks)."""
    r = np.random.RandomState(seed)
    words = [bytes(r.randint(97, 123, size=r.randint(3, 12)).astype(np.uint8)) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += words[int(abs(r.standard_cauchy()) * 8) % len(words)] + b' '
    return bytes(out[:n])


def valid_frames(sizes=SIGNAL_SIZES, levels=LEVELS):
    """[(name, frame, content)]: every frame here is one libzstd itself decodes to ``content``."""
    out = []
    for n in sizes:
        packed = vbz_fixtures.streamvbyte(random_walk(n, seed=n))
        for level in levels:
            out.append(('walk_%d_l%d' % (n, level), vbz_fixtures.zstd_compress(packed, level), packed))
    const = vbz_fixtures.streamvbyte(np.full(60000, 431, dtype=np.int16))
    square = vbz_fixtures.streamvbyte(np.tile(np.r_[np.full(50, 400), np.full(50, 620)], 900).astype(np.int16))
    r = np.random.RandomState(7)
    others = [('constant', const), ('square', square), ('zeros', bytes(200000)), ('one_byte_run', b'\x07' * 9)]
    for n in (1, 1000, 300000):
        others.append(('random_%d' % n, r.randint(0, 256, size=n).astype(np.uint8).tobytes()))
    others += [('text_few', text_like(5000, 9, 1)), ('text_many', text_like(60000, 200, 2)),
               ('seam_131072', text_like(131072, 40, 3)), ('seam_131073', text_like(131073, 40, 4)),
               ('wordy', wordy(500000, 5))]
    for name, data in others:
        for level in (1, 19):
            out.append(('%s_l%d' % (name, level), vbz_fixtures.zstd_compress(data, level), data))
    # what the simple call does not emit: a window descriptor (no single segment: the content size
    # is known but the frame is streamed), content sizes of 2 and 8 bytes' worth, and blocks that
    # reuse the tree and the tables of the block before (treeless literals, repeat mode)
    adv = [('windowed', wordy(70000, 6), [(C_LEVEL, 3), (C_WINDOWLOG, 12)], ()),
           ('flushed_text', text_like(90000, 30, 8), [(C_LEVEL, 3)], range(3000, 90000, 3000)),
           ('flushed_wordy', wordy(120000, 9), [(C_LEVEL, 19)], range(2500, 120000, 2500)),
           ('flushed_walk', vbz_fixtures.streamvbyte(random_walk(40000, 11)), [(C_LEVEL, 1)],
            range(1500, 50000, 1500))]
    # runs of one byte between matches into the block before
    first = wordy(4000, 12)
    second = b''.join(b'x' * (5 + i % 7) + first[i * 50:i * 50 + 40] for i in range(70))
    adv.append(('x_runs', first + second, [(C_LEVEL, 3)], (len(first),)))
    for name, data, params, cuts in adv:
        # (the content size is not written by the streaming call unless it is pledged: patched in)
        out.append((name, with_content_size(zstd_compress_adv(data, params, cuts), len(data)), data))
    # a period of 64 bytes set up in one block and kept, between altered bytes, in the next: every
    # match of the second block is at the repeat offset (offset code 0: an RLE offset table)
    r = np.random.RandomState(31)
    base = r.randint(0, 256, size=64).astype(np.uint8)
    tail = np.tile(base, 60).copy()
    tail[np.arange(17, len(tail), 23)] ^= 0x55
    data = np.tile(base, 40).tobytes() + tail.tobytes()
    out.append(('repeat_offset', with_content_size(zstd_compress_adv(data, [(C_LEVEL, 3)], (40 * 64,)),
                                                   len(data)), data))
    # RLE literals, which this libzstd's compressor does not emit on its own: assembled by hand
    # (a compressed block of a literals section of type 1 and no sequences; a 1-byte and a 2-byte
    # literals header), and accepted by libzstd like every other frame here
    out.append(('rle_literals_20', bytes.fromhex('28b52ffd20141d0000a17800'), b'x' * 20))
    out.append(('rle_literals_300', bytes.fromhex('28b52ffd602c00250000c5127800'), b'x' * 300))
    return out


def with_content_size(frame, size):
    """The frame with its header rewritten to carry ``size`` as an 8-byte (or, below 65,792, a
    2-byte) content size in front of the same blocks; the window descriptor is kept."""
    frame = bytes(frame)
    fhd = frame[4]
    single = (fhd >> 5) & 1
    fcs = fhd >> 6
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3]
    at += (1 if single else 0, 2, 4, 8)[fcs]
    window = b'' if single else frame[5:6]
    if 256 <= size < 65536 + 256:
        return frame[:4] + bytes([(1 << 6) | (single << 5)]) + window + struct.pack('<H', size - 256) + frame[at:]
    return frame[:4] + bytes([(3 << 6) | (single << 5)]) + window + struct.pack('<Q', size) + frame[at:]


# ---- a frame walker: which parts of the format a frame uses -----------------------------------
def walk(frame):
    """{'blocks': set of raw|rle|compressed, 'literals': set of raw|rle|huffman|treeless,
    'streams': set of 1|4, 'modes': set of (table, predefined|rle|compressed|repeat),
    'tree': set of direct|fse, 'sections': [(kind, begin, end)] byte ranges for the mutants,
    'content': the content size, 'single': whether the frame is single-segment}"""
    f = bytes(frame)
    assert struct.unpack('<I', f[:4])[0] == MAGIC
    fhd = f[4]
    single = (fhd >> 5) & 1
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3]
    fcs = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    content = int.from_bytes(f[at:at + fcs], 'little') + (256 if fcs == 2 else 0)
    at += fcs
    info = {'blocks': set(), 'literals': set(), 'streams': set(), 'modes': set(), 'tree': set(),
            'sections': [('frame_header', 0, at)], 'content': content, 'single': bool(single),
            'n_blocks': 0, 'n_seq': 0, 'repeat_offset': False}
    while True:
        bh = int.from_bytes(f[at:at + 3], 'little')
        info['sections'].append(('block_header', at, at + 3))
        at += 3
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        info['n_blocks'] += 1
        info['blocks'].add(('raw', 'rle', 'compressed')[btype])
        if btype == 2:
            _walk_block(f, at, size, info)
        at += 1 if btype == 1 else size
        if last:
            break
    info['end'] = at
    return info


def _walk_block(f, b0, size, info):
    p = f[b0:b0 + size]
    ltype, sf = p[0] & 3, (p[0] >> 2) & 3
    if ltype < 2:
        lh = 1 if not sf & 1 else 2 if sf == 1 else 3
        lit = int.from_bytes(p[:lh], 'little') >> (3 if lh == 1 else 4)
        at = lh + (lit if ltype == 0 else 1)
        info['literals'].add(('raw', 'rle')[ltype])
    else:
        lh = 3 if sf < 2 else 4 if sf == 2 else 5
        word = int.from_bytes(p[:5], 'little')
        bits = 10 if sf < 2 else 14 if sf == 2 else 18
        comp = (word >> (4 + bits)) & ((1 << bits) - 1)
        info['literals'].add('huffman' if ltype == 2 else 'treeless')
        info['streams'].add(1 if sf == 0 else 4)
        if ltype == 2:
            hb = p[lh]
            tree = 1 + ((hb - 127 + 1) // 2 if hb >= 128 else hb)
            info['tree'].add('direct' if hb >= 128 else 'fse')
            info['sections'].append(('tree', b0 + lh, b0 + lh + tree))
            if sf:
                info['sections'].append(('jump_table', b0 + lh + tree, b0 + lh + tree + 6))
        at = lh + comp
    info['sections'].append(('literals_header', b0, b0 + lh))
    s0 = at
    n = p[at]
    at += 1
    if n:
        if n == 255:
            n = p[at] + (p[at + 1] << 8) + 0x7F00
            at += 2
        elif n > 127:
            n = ((n - 128) << 8) + p[at]
            at += 1
        modes = p[at]
        at += 1
        names = ('predefined', 'rle', 'compressed', 'repeat')
        for table, shift in (('ll', 6), ('of', 4), ('ml', 2)):
            info['modes'].add((table, names[(modes >> shift) & 3]))
        # an RLE offset table of code 0: every match of the block is at a repeat offset
        if (modes >> 6) != 2 and ((modes >> 4) & 3) == 1 and p[at + (1 if (modes >> 6) == 1 else 0)] == 0:
            info['repeat_offset'] = True
    info['n_seq'] += n
    # (the table descriptions and the first bytes of the bitstream follow: all of the section,
    # up to 160 bytes of it, is mutated byte by byte)
    info['sections'].append(('sequences', b0 + s0, b0 + min(size, s0 + 160)))


# ---- mutants ---------------------------------------------------------------------------------
def mutants(frames, seed=1234, random_per_frame=40):
    """[(label, bytes)] damaged copies of the frames [(name, frame, content)]: every byte of the
    headers, tree descriptions, jump tables and sequence sections changed once, bytes changed at
    random offsets elsewhere, truncations and extensions, the content size edited up and down, the
    checksum, dictionary and single-segment flags flipped."""
    r = np.random.RandomState(seed)
    out = []
    for name, frame, _ in frames:
        frame = bytes(frame)
        info = walk(frame)
        seen = set()
        for kind, a, b in info['sections']:
            for at in range(a, min(b, len(frame))):
                if at in seen:
                    continue
                seen.add(at)
                m = bytearray(frame)
                m[at] ^= int(r.randint(1, 256))
                out.append(('%s:%s@%d' % (name, kind, at), bytes(m)))
        for _ in range(random_per_frame):
            at = int(r.randint(0, len(frame)))
            m = bytearray(frame)
            m[at] ^= 1 << int(r.randint(0, 8))
            out.append(('%s:bit@%d' % (name, at), bytes(m)))
        for cut in sorted(set([1, 2, 3, 4, 5, 8] + [int(c) for c in r.randint(1, len(frame), size=6)])):
            if cut < len(frame):
                out.append(('%s:cut-%d' % (name, cut), frame[:len(frame) - cut]))
        out.append(('%s:extended1' % name, frame + b'\0'))
        out.append(('%s:extended_frame' % name, frame + frame))
        out.append(('%s:extended_skippable' % name, frame + struct.pack('<II', 0x184D2A50, 4) + b'abcd'))
        for delta in (-1, 1, 255, -256):
            m = _edit_content_size(frame, delta)
            if m is not None:
                out.append(('%s:content%+d' % (name, delta), m))
        for bit in (0x04, 0x01, 0x20, 0x08):
            m = bytearray(frame)
            m[4] ^= bit
            out.append(('%s:flag^%02x' % (name, bit), bytes(m)))
    return out


def _edit_content_size(frame, delta):
    fhd = frame[4]
    single = (fhd >> 5) & 1
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3]
    fcs = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    if not fcs:
        return None
    v = int.from_bytes(frame[at:at + fcs], 'little') + delta
    if v < 0 or v >= 1 << (8 * fcs):
        return None
    return frame[:at] + v.to_bytes(fcs, 'little') + frame[at + fcs:]


def mutant_parents(frames):
    """A dozen of the valid frames, small enough to mutate byte by byte, that together hold every
    part of the format."""
    want = ['walk_200_l1', 'walk_4000_l1', 'walk_4000_l19', 'walk_27000_l19', 'walk_5_l3', 'walk_0_l1',
            'constant_l1', 'square_l19', 'random_1000_l1', 'text_few_l1', 'text_many_l19', 'one_byte_run_l1',
            'windowed', 'flushed_text', 'flushed_wordy', 'x_runs', 'rle_literals_20', 'rle_literals_300']
    by_name = {name: (name, frame, content) for name, frame, content in frames}
    return [by_name[n] for n in want if n in by_name]


# ---- the model through ctypes ----------------------------------------------------------------
def model_lib(path):
    m = ctypes.CDLL(path)
    m.dbh_zstd_decode_host.restype = ctypes.c_int
    m.dbh_zstd_decode_host.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]
    return m


GUARD = 4096


def model_decode(m, frame, capacity):
    """(status, bytes) of dbh_zstd_decode_host on the frame, which lies PAD readable bytes in
    front of the end of its buffer; the output buffer has guard bytes on both sides, which must
    come back untouched."""
    frame = bytes(frame)
    src = ctypes.create_string_buffer(frame + b'\0' * PAD, len(frame) + PAD)
    dst = (ctypes.c_uint8 * (capacity + 2 * GUARD))()
    ctypes.memset(dst, 0xA5, capacity + 2 * GUARD)
    produced = ctypes.c_size_t(0)
    status = ctypes.c_int32(-1)
    rc = m.dbh_zstd_decode_host(src, len(frame), ctypes.byref(dst, GUARD), capacity, ctypes.byref(produced),
                                ctypes.byref(status))
    assert rc == 0
    raw = bytes(dst)
    assert raw[:GUARD] == b'\xA5' * GUARD and raw[GUARD + capacity:] == b'\xA5' * GUARD, 'wrote outside out_capacity'
    return status.value, raw[GUARD:GUARD + produced.value]


# ---- damaged streamvbyte bytes inside intact frames (the generators of test_gpu_vbz.py, rebuilt) --
def damaged_vbz_chunks(seed=99):
    """[(label, chunk)] mode-3 chunks whose zstd stage is intact and whose streamvbyte stage must be
    refused: control bytes beyond the stream, data that run past its end, data that end before it,
    an odd original_size."""
    samples = random_walk(3000, seed)
    packed = vbz_fixtures.streamvbyte(samples)
    n = len(samples)
    ctrl = (n + 3) // 4
    out = []

    def chunk(body, size=2 * n, level=1):
        return struct.pack('<I', size) + vbz_fixtures.zstd_compress(body, level)

    out.append(('data_short', chunk(packed[:-1])))
    out.append(('data_long', chunk(packed + b'\x01')))
    out.append(('ctrl_beyond', chunk(packed[:ctrl - 1])))
    out.append(('odd_size', chunk(packed, size=2 * n + 1)))
    longer = bytearray(packed)
    longer[0] |= 3                                   # the first value claims 4 bytes
    out.append(('code_longer', chunk(bytes(longer))))
    return out
