// dbh_zstd_core.h - RFC 8878 decoding (zstd frames: the outer stage of ONT's VBZ filter), written
// once for the GPU kernel (dbh_zstd.hip, one wavefront per frame) and for its CPU model
// (dbh_zstd_decode_host, the same code with a loop standing in for the lanes), as
// dbh_inflate_core.h is for deflate.  libzstd is the judge of both (tests/test_zstd_model.py).
//
// What is decoded: one frame - single-segment or with a window descriptor, content size of 1, 2, 4
// or 8 bytes - of raw, RLE and compressed blocks; literals raw, RLE, Huffman-coded in 1 or 4
// streams, or with the tree of the block before; the tree from direct or FSE-compressed weights;
// sequences in all four modes per table, tables and repeat offsets carried from block to block.
// What is refused (status != 0, never guessed at): a dictionary id, the checksum flag, no content
// size, anything behind the frame (a second or skippable frame included), a content size beyond
// the room the caller gives, and every inconsistency libzstd looks for - weights that do not
// complete a power of two or give codes longer than 11 bits (libzstd takes 12: the one place this
// decoder is narrower by design), FSE distributions that overrun or whose accuracy is out of
// range, a bitstream without its marker bit or not consumed exactly, stream sizes that disagree
// with the jump table, literal lengths beyond the literals left, offsets beyond the bytes produced
// or the window, a frame that produces other than its content size.  A bitstream read that
// reaches beyond the stream's first bit is refused where it happens (libzstd 1.4.8 reads on and
// refuses, or in a few cases accepts, at the end).
// Refused here and taken by libzstd 1.4.8's one-shot call, all by design (tests/test_zstd_written.py
// holds a written frame for each): the checksum flag; a dictionary id field, also one that holds 0;
// no content size; a skippable frame in front of the frame; a second frame behind it; a tree of
// depth 12; reserved bits set in the sequences' modes byte; an offset beyond the window but inside
// the output; sequence bits left over behind the last sequence; a last sequence whose fields reach
// beyond the stream's first bit.
//
// THE SCHEDULE.  Serial work (headers, tree and table descriptions) is one lane's; the tables it
// builds live in a Ctx (LDS on the device).  The Huffman table is filled by all lanes.  The
// literals - on signal data nearly all of a frame - are decoded by all 64 lanes at once: the 1 or
// 4 backward bitstreams are cut into 64 or 16 pieces of equal bit length, every lane decodes its
// piece from a guessed first bit down to the next piece's, and is re-decoded until it starts
// where the lane before it ended (Huffman codes re-synchronise; lane 0 of a stream starts at the
// marker, so round r has lanes 0..r right and the rounds end); a prefix sum of the symbol counts
// says where each lane's bytes go, and a last pass writes them.  Sequences are decoded by every
// lane alike (uniform), each executed with wave-wide copies.
//
// WHERE THE BYTES GO.  The caller gives one region of `cap` bytes: the frame's content grows from
// its front; a compressed block's Huffman-decoded literals are parked at its END and consumed from
// there as the sequences are executed.  Content size <= cap is all a valid frame needs: a block
// still has to emit every literal not yet consumed, so the write position never passes the first
// unread literal (checked per sequence all the same: a damaged frame must not).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DBZ_HD __host__ __device__ __forceinline__
#else
#define DBZ_HD inline
#endif

namespace dbz {

enum Status : int32_t {
    kOk = 0,
    kBadMagic = 16,        // not a zstd frame (a skippable frame included)
    kUnsupported = 17,     // dictionary id, checksum, no content size, reserved bit
    kTruncated = 18,       // the frame ends inside a header or a block
    kBadBlock = 19,        // reserved block type, block sizes out of range
    kBadLiterals = 20,     // literals section header, jump table, stream sizes
    kBadTree = 21,         // Huffman tree description
    kBadFse = 22,          // FSE table description
    kBadSequences = 23,    // sequences section header, modes, symbols
    kBadBitstream = 24,    // no marker bit, read beyond the first bit, not consumed exactly
    kBadOffset = 25,       // a match reaching before the frame's first byte or beyond the window
    kBadSize = 26,         // a block or the frame producing other than it states
    kNoSpace = 27,         // content size beyond the caller's room
    kTrailing = 28,        // bytes behind the frame
};

constexpr int kLanes = 64;
constexpr int kHufLogMax = 11;
constexpr int kLLLogMax = 9, kMLLogMax = 9, kOFLogMax = 8;
constexpr int kMaxLL = 35, kMaxML = 52, kMaxOF = 31;
constexpr uint32_t kBlockMax = 128u * 1024u;

// Everything the lanes of a frame share (LDS on the device: 11.8 KB, thirteen frames per CU)
struct Ctx {
    uint16_t huf[1 << kHufLogMax];         // index: the next huf_log bits; symbol | bits << 8
    uint32_t ll[1 << kLLLogMax];           // FSE: new state | bits << 16 | symbol << 24
    uint32_t ml[1 << kMLLogMax];
    uint32_t of[1 << kOFLogMax];
    uint32_t wfse[64];                     // the table of FSE-compressed Huffman weights
    int16_t norm[256];                     // a distribution being read
    uint16_t next[256];                    // FSE build: next state per symbol
    uint16_t first[256];                   // tree: first table entry per symbol
    uint8_t weights[256];
    uint32_t rank[16];
    // carried from block to block
    uint32_t rep[3];
    int32_t ll_log, ml_log, of_log, huf_log, huf_syms;
    int32_t have_huf, have_fse;
    // the block at hand
    int32_t status;
    int32_t lit_type;                      // 0 raw, 1 RLE, 2 Huffman
    int32_t lit_new_tree;
    uint32_t lit_size, lit_streams, lit_byte;
    uint32_t lit_off;                      // frame offset of the raw literals / the first stream
    uint32_t stream_bytes[4];
    uint32_t n_seq, seq_off, seq_end;      // the sequences' bitstream: frame offsets
};

struct Frame {
    uint64_t content;
    uint64_t window;
    uint32_t header_bytes;
};

DBZ_HD int highbit(uint32_t v) { return 31 - __builtin_clz(v); }
DBZ_HD uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
DBZ_HD uint32_t le24(const uint8_t* p) { return le16(p) | (uint32_t)p[2] << 16; }
DBZ_HD uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }
DBZ_HD uint64_t load64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// ---- frame header ------------------------------------------------------------------------
DBZ_HD int frame_header(const uint8_t* f, size_t n, Frame* out) {
    if (n < 5) return kTruncated;
    if (le32(f) != 0xFD2FB528u) return kBadMagic;
    const uint32_t fhd = f[4];
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u;
    if (fhd & 0x08u) return kUnsupported;              // reserved bit
    if (fhd & 0x04u) return kUnsupported;              // content checksum
    if (fhd & 0x03u) return kUnsupported;              // dictionary id
    if (fcs_flag == 0 && !single) return kUnsupported; // no content size
    const uint32_t fcs_bytes = fcs_flag == 0 ? 1u : fcs_flag == 1 ? 2u : fcs_flag == 2 ? 4u : 8u;
    uint32_t at = 5;
    if (n < at + (single ? 0u : 1u) + fcs_bytes) return kTruncated;
    uint64_t window = 0;
    if (!single) {
        const uint32_t wd = f[at++];
        const uint32_t log = 10u + (wd >> 3);
        if (log > 31u) return kUnsupported;            // (libzstd: window too large)
        window = (1ull << log) + ((1ull << log) >> 3) * (wd & 7u);
    }
    uint64_t content = 0;
    if (fcs_bytes == 1) content = f[at];
    else if (fcs_bytes == 2) content = le16(f + at) + 256u;
    else if (fcs_bytes == 4) content = le32(f + at);
    else content = (uint64_t)le32(f + at) | (uint64_t)le32(f + at + 4) << 32;
    at += fcs_bytes;
    out->content = content;
    out->window = single ? content : window;
    out->header_bytes = at;
    return kOk;
}

// ---- sequence codes ----------------------------------------------------------------------
DBZ_HD uint32_t ll_bits(uint32_t c) {
    return c < 16 ? 0u : c >= 25 ? c - 19u : (uint32_t)(0x433221111ull >> (4 * (c - 16))) & 15u;
}
DBZ_HD uint32_t ll_base(uint32_t c) {
    return c < 16 ? c : c >= 25 ? 1u << (c - 19) : c == 24 ? 48u
                  : (uint32_t)(0x28201C1816141210ull >> (8 * (c - 16))) & 255u;
}
DBZ_HD uint32_t ml_bits(uint32_t c) {
    return c < 32 ? 0u : c >= 43 ? c - 36u : (uint32_t)(0x54433221111ull >> (4 * (c - 32))) & 15u;
}
DBZ_HD uint32_t ml_base(uint32_t c) {
    return c < 32 ? c + 3u : c >= 43 ? (1u << (c - 36)) + 3u : c == 40 ? 67u : c == 41 ? 83u : c == 42 ? 99u
                  : (uint32_t)(0x3B332F2B29272523ull >> (8 * (c - 32))) & 255u;
}
// the predefined distributions (RFC 8878, 3.1.1.3.2.2)
DBZ_HD int ll_default(int s) {
    return s == 0 ? 4 : (s == 1 || s == 25) ? 3 : (s <= 12 || (s >= 16 && s <= 24) || s == 26) ? 2 : s <= 31 ? 1 : -1;
}
DBZ_HD int ml_default(int s) { return s == 0 ? 1 : s == 1 ? 4 : s == 2 ? 3 : s < 9 ? 2 : s < 46 ? 1 : -1; }
DBZ_HD int of_default(int s) { return (s < 6 || (s >= 9 && s < 24)) ? 1 : s < 9 ? 2 : -1; }

// ---- FSE ---------------------------------------------------------------------------------
// bits [pos, pos + n) of a forward bitstream (first bit lowest), zeros beyond its end; n <= 16
DBZ_HD uint32_t fwd_bits(const uint8_t* p, uint32_t avail, uint32_t pos, uint32_t n) {
    uint32_t v = 0;
    const uint32_t b = pos >> 3;
    for (uint32_t k = 0; k < 4; ++k)
        if (b + k < avail) v |= (uint32_t)p[b + k] << (8 * k);
    return (v >> (pos & 7u)) & ((1u << n) - 1u);
}

// a distribution (FSE_readNCount's format and verdicts): bytes taken, or -1
DBZ_HD int read_ncount(const uint8_t* p, uint32_t avail, int max_sym, int max_log, int16_t* norm,
                       int* n_sym, int* log_out) {
    if (avail < 1) return -1;
    const int log = (int)fwd_bits(p, avail, 0, 4) + 5;
    if (log > max_log) return -1;
    uint32_t pos = 4;
    int remaining = (1 << log) + 1, threshold = 1 << log, nb = log + 1, s = 0;
    bool prev0 = false;
    const uint32_t end_bits = 8u * avail;
    while (remaining > 1 && s <= max_sym) {
        if (prev0) {
            int n0 = s;
            while (fwd_bits(p, avail, pos, 16) == 0xFFFFu) {
                n0 += 24;
                pos += 16;
            }
            while (fwd_bits(p, avail, pos, 2) == 3u) {
                n0 += 3;
                pos += 2;
            }
            n0 += (int)fwd_bits(p, avail, pos, 2);
            pos += 2;
            if (n0 > max_sym) return -1;
            while (s < n0) norm[s++] = 0;
        }
        if (pos > end_bits) return -1;
        const int max = 2 * threshold - 1 - remaining;
        const int v = (int)fwd_bits(p, avail, pos, (uint32_t)nb);
        int count;
        if ((v & (threshold - 1)) < max) {
            count = v & (threshold - 1);
            pos += (uint32_t)nb - 1u;
        } else {
            count = v & (2 * threshold - 1);
            if (count >= threshold) count -= max;
            pos += (uint32_t)nb;
        }
        --count;
        remaining -= count < 0 ? -count : count;
        norm[s++] = (int16_t)count;
        prev0 = count == 0;
        while (remaining < threshold) {
            --nb;
            threshold >>= 1;
        }
    }
    if (remaining != 1 || pos > end_bits) return -1;
    *n_sym = s;
    *log_out = log;
    return (int)((pos + 7u) >> 3);
}

// the decoding table of a distribution (FSE_buildDTable / ZSTD_buildFSETable's layout)
DBZ_HD bool fse_build(uint32_t* tab, int log, const int16_t* norm, int n_sym, uint16_t* next) {
    const int size = 1 << log, mask = size - 1;
    int high = size - 1;
    for (int s = 0; s < n_sym; ++s) {
        if (norm[s] == -1) {
            if (high < 0) return false;
            tab[high--] = (uint32_t)s << 24;
            next[s] = 1;
        } else {
            next[s] = (uint16_t)norm[s];
        }
    }
    const int step = (size >> 1) + (size >> 3) + 3;
    int pos = 0, placed = size - 1 - high;
    for (int s = 0; s < n_sym; ++s) {
        for (int i = 0; i < norm[s]; ++i) {
            if (++placed > size) return false;
            tab[pos] = (uint32_t)s << 24;
            pos = (pos + step) & mask;
            while (pos > high) pos = (pos + step) & mask;
        }
    }
    if (pos != 0 || placed != size) return false;
    for (int u = 0; u < size; ++u) {
        const uint32_t sym = tab[u] >> 24;
        const uint32_t ns = next[sym]++;
        const uint32_t nb = (uint32_t)(log - highbit(ns));
        tab[u] = (((ns << nb) - (uint32_t)size) & 0xFFFFu) | nb << 16 | sym << 24;
    }
    return true;
}

// ---- backward bitstreams -----------------------------------------------------------------
// the 32 bits below bit position pos (bit 31 of the result is bit pos - 1), zeros below bit 0.
// Reads 8 bytes from inside the stream or up to 7 behind its end (the caller's padding).
DBZ_HD uint32_t window32(const uint8_t* src, int32_t pos) {
    if (pos >= 32) {
        const uint32_t p = (uint32_t)pos - 32u;
        return (uint32_t)(load64(src + (p >> 3)) >> (p & 7u));
    }
    return (uint32_t)(load64(src) << (32 - pos));       // (pos >= 0)
}
// n <= 32 bits below pos
DBZ_HD uint32_t back_bits(const uint8_t* src, int32_t pos, uint32_t n) {
    return n == 0 ? 0u : window32(src, pos) >> (32u - n);
}
// the number of bits below the marker of a stream of `bytes` bytes, or -1 (empty, no marker)
DBZ_HD int32_t back_start(const uint8_t* src, uint32_t bytes) {
    if (bytes < 1 || src[bytes - 1] == 0) return -1;
    return (int32_t)(bytes - 1) * 8 + highbit(src[bytes - 1]);
}

// ---- the Huffman tree --------------------------------------------------------------------
// Its description at p (avail bytes) -> weights, huf_log, huf_syms, and per symbol the first table
// entry (first[]): bytes taken, or -1.  HUF_readStats + the layout of HUF_readDTableX1.
DBZ_HD int read_tree(Ctx& c, const uint8_t* p, uint32_t avail) {
    if (avail < 1) return -1;
    const uint32_t hb = p[0];
    uint32_t taken, n = 0;
    if (hb >= 128) {
        n = hb - 127u;
        taken = (n + 1) / 2;
        if (taken + 1 > avail) return -1;
        for (uint32_t k = 0; k < n; k += 2) {
            c.weights[k] = p[1 + k / 2] >> 4;
            c.weights[k + 1] = p[1 + k / 2] & 15;       // (n <= 128: inside weights[])
        }
    } else {
        taken = hb;
        if (taken + 1 > avail) return -1;
        int n_sym = 0, log = 0;
        const int hdr = read_ncount(p + 1, taken, 255, 6, c.norm, &n_sym, &log);
        if (hdr < 0) return -1;
        if (!fse_build(c.wfse, log, c.norm, n_sym, c.next)) return -1;
        const uint8_t* s = p + 1 + hdr;
        const uint32_t len = taken - (uint32_t)hdr;
        int32_t pos = back_start(s, len);
        if (pos < 2 * log) return -1;                   // (no marker, or states beyond the first bit)
        uint32_t s1 = back_bits(s, pos, (uint32_t)log);
        pos -= log;
        uint32_t s2 = back_bits(s, pos, (uint32_t)log);
        pos -= log;
        for (;;) {                                       // FSE_decompress_usingDTable's tail loop
            if (n > 253) return -1;
            uint32_t e = c.wfse[s1];
            c.weights[n++] = (uint8_t)(e >> 24);
            uint32_t nb = (e >> 16) & 255u;
            s1 = (e & 0xFFFFu) + (pos >= (int32_t)nb ? back_bits(s, pos, nb) : 0u);
            pos -= (int32_t)nb;
            if (pos < 0) {
                c.weights[n++] = (uint8_t)(c.wfse[s2] >> 24);
                break;
            }
            if (n > 253) return -1;
            e = c.wfse[s2];
            c.weights[n++] = (uint8_t)(e >> 24);
            nb = (e >> 16) & 255u;
            s2 = (e & 0xFFFFu) + (pos >= (int32_t)nb ? back_bits(s, pos, nb) : 0u);
            pos -= (int32_t)nb;
            if (pos < 0) {
                c.weights[n++] = (uint8_t)(c.wfse[s1] >> 24);
                break;
            }
        }
    }
    for (int k = 0; k < 16; ++k) c.rank[k] = 0;
    uint32_t total = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t w = c.weights[k];
        if (w >= 12) return -1;
        c.rank[w]++;
        total += (1u << w) >> 1;
    }
    if (total == 0) return -1;
    const int log = highbit(total) + 1;
    if (log > kHufLogMax) return -1;
    const uint32_t rest = (1u << log) - total;
    if (rest & (rest - 1)) return -1;                    // the weights do not complete a power of two
    const uint32_t last = (uint32_t)highbit(rest) + 1u;
    c.weights[n] = (uint8_t)last;
    c.rank[last]++;
    if (c.rank[1] < 2 || (c.rank[1] & 1)) return -1;
    ++n;
    // first entry per weight, then per symbol (symbols of a weight in ascending order)
    uint32_t at = 0;
    for (int w = 1; w <= log; ++w) {
        const uint32_t cur = at;
        at += c.rank[w] << (w - 1);
        c.rank[w] = cur;
    }
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t w = c.weights[k];
        c.first[k] = (uint16_t)c.rank[w];
        if (w) c.rank[w] += 1u << (w - 1);
    }
    c.huf_log = log;
    c.huf_syms = (int32_t)n;
    return (int)(taken + 1);
}

// the table's entries, lane's share (every symbol's range by all lanes together)
DBZ_HD void fill_tree(Ctx& c, int lane, int lanes) {
    const int log = c.huf_log;
    for (int s = 0; s < c.huf_syms; ++s) {
        const uint32_t w = c.weights[s];
        if (!w) continue;
        const int len = 1 << (w - 1);
        const uint16_t e = (uint16_t)((uint32_t)s | (uint32_t)(log + 1 - (int)w) << 8);
        uint16_t* to = c.huf + c.first[s];
        for (int k = lane; k < len; k += lanes) to[k] = e;
    }
}

// One lane's piece of a Huffman bitstream: from bit position `start` down until `stop` is reached
// or passed; symbols to out (if not null).  end = where it stopped (0 and bad if a code reached
// beyond the stream's first bit).
struct Piece {
    int32_t end, count, bad;
};
DBZ_HD Piece huf_piece(const uint16_t* tab, int log, const uint8_t* src, int32_t start, int32_t stop,
                       uint8_t* out) {
    Piece r;
    int32_t pos = start, count = 0;
    r.bad = 0;
    while (pos > stop) {
        // two symbols per load: 32 bits hold two codes and the index of the second
        uint32_t w = window32(src, pos);
        uint32_t e = tab[w >> (32 - log)];
        int32_t nb = (int32_t)(e >> 8);
        if (nb > pos) {
            r.bad = 1;
            pos = 0;
            break;
        }
        if (out) out[count] = (uint8_t)e;
        ++count;
        pos -= nb;
        if (pos <= stop) break;
        w <<= nb;
        e = tab[w >> (32 - log)];
        nb = (int32_t)(e >> 8);
        if (nb > pos) {
            r.bad = 1;
            pos = 0;
            break;
        }
        if (out) out[count] = (uint8_t)e;
        ++count;
        pos -= nb;
    }
    r.end = pos;
    r.count = count;
    return r;
}
// where piece k of n begins in a stream of `bits` bits (piece 0 at the marker, piece n at bit 0)
DBZ_HD int32_t piece_start(int32_t bits, int k, int n) {
    return bits - (int32_t)(((int64_t)bits * k) / n);
}

// ---- a compressed block's headers (one lane) ---------------------------------------------
DBZ_HD int seq_table(Ctx& c, uint32_t mode, uint32_t* tab, int32_t* log, int max_log, int max_sym,
                     int which, const uint8_t* f, uint32_t* at, uint32_t end) {
    if (mode == 0) {                                      // predefined
        const int n = which == 0 ? 36 : which == 1 ? 29 : 53;
        for (int s = 0; s < n; ++s)
            c.norm[s] = (int16_t)(which == 0 ? ll_default(s) : which == 1 ? of_default(s) : ml_default(s));
        *log = which == 1 ? 5 : 6;
        return fse_build(tab, *log, c.norm, n, c.next) ? kOk : kBadFse;
    }
    if (mode == 1) {                                      // RLE: one symbol, no bits
        if (*at >= end) return kBadSequences;
        const uint32_t s = f[(*at)++];
        if ((int)s > max_sym) return kBadSequences;
        tab[0] = s << 24;
        *log = 0;
        return kOk;
    }
    if (mode == 2) {
        int n_sym = 0, lg = 0;
        const int taken = read_ncount(f + *at, end - *at, max_sym, max_log, c.norm, &n_sym, &lg);
        if (taken < 0) return kBadFse;
        if (!fse_build(tab, lg, c.norm, n_sym, c.next)) return kBadFse;
        *log = lg;
        *at += (uint32_t)taken;
        return kOk;
    }
    return c.have_fse ? kOk : kBadSequences;              // repeat: the table of the block before
}

// The block [b0, b0 + size) of frame f: literals header, tree, jump table, sequences header and
// tables -> c (ZSTD_decodeLiteralsBlock + ZSTD_decodeSeqHeaders).
DBZ_HD int block_headers(Ctx& c, const uint8_t* f, uint32_t b0, uint32_t size) {
    if (size < 3 || size >= kBlockMax) return kBadBlock;
    const uint8_t* p = f + b0;
    const uint32_t type = p[0] & 3u, sf = (p[0] >> 2) & 3u;
    uint32_t lh, lit, comp = 0, at;
    c.lit_new_tree = 0;
    if (type < 2) {
        if (!(sf & 1u)) {
            lh = 1;
            lit = p[0] >> 3;
        } else if (sf == 1) {
            lh = 2;
            lit = le16(p) >> 4;
        } else {
            lh = 3;
            lit = le24(p) >> 4;
        }
        c.lit_type = (int32_t)type;
        c.lit_off = b0 + lh;
        if (type == 0) {
            if (lh + lit > size) return kBadLiterals;
            at = lh + lit;
        } else {
            if (lit > kBlockMax || lh + 1 > size) return kBadLiterals;
            c.lit_byte = p[lh];
            at = lh + 1;
        }
        c.lit_streams = 0;
    } else {
        if (size < 5) return kBadLiterals;
        const uint32_t lhc = le32(p);
        if (sf < 2) {
            lh = 3;
            lit = (lhc >> 4) & 0x3FFu;
            comp = (lhc >> 14) & 0x3FFu;
        } else if (sf == 2) {
            lh = 4;
            lit = (lhc >> 4) & 0x3FFFu;
            comp = lhc >> 18;
        } else {
            lh = 5;
            lit = (lhc >> 4) & 0x3FFFFu;
            comp = (lhc >> 22) + ((uint32_t)p[4] << 10);
        }
        if (lit > kBlockMax || lit == 0 || comp == 0 || lh + comp > size) return kBadLiterals;
        c.lit_type = 2;
        c.lit_streams = sf == 0 ? 1u : 4u;
        uint32_t tree = 0;
        if (type == 2) {
            const int taken = read_tree(c, p + lh, comp);
            if (taken < 0) return kBadTree;
            tree = (uint32_t)taken;
            if (tree >= comp) return kBadLiterals;
            c.lit_new_tree = 1;
            c.have_huf = 1;
        } else if (!c.have_huf) {
            return kBadTree;                              // treeless, and no tree before it
        }
        uint32_t s0 = b0 + lh + tree, left = comp - tree;
        if (c.lit_streams == 4) {
            if (left < 10) return kBadLiterals;
            const uint32_t l1 = le16(f + s0), l2 = le16(f + s0 + 2), l3 = le16(f + s0 + 4);
            if (l1 + l2 + l3 + 6 > left) return kBadLiterals;
            // the first three streams hold (lit + 3) / 4 symbols each, the fourth the rest
            if (3 * ((lit + 3) / 4) > lit) return kBadLiterals;
            c.stream_bytes[0] = l1;
            c.stream_bytes[1] = l2;
            c.stream_bytes[2] = l3;
            c.stream_bytes[3] = left - 6 - l1 - l2 - l3;
            s0 += 6;
        } else {
            c.stream_bytes[0] = left;
        }
        c.lit_off = s0;
        at = lh + comp;
    }
    c.lit_size = lit;
    // the sequences section
    if (at >= size) return kBadSequences;
    uint32_t n = p[at++];
    if (n == 0) {
        if (at != size) return kBadSequences;
        c.n_seq = 0;
        return kOk;
    }
    if (n > 0x7F) {
        if (n == 0xFF) {
            if (at + 2 > size) return kBadSequences;
            n = le16(p + at) + 0x7F00u;
            at += 2;
        } else {
            if (at >= size) return kBadSequences;
            n = ((n - 0x80u) << 8) + p[at++];
        }
    }
    if (at + 1 > size) return kBadSequences;
    const uint32_t modes = p[at++];
    if (modes & 3u) return kBadSequences;                 // reserved bits
    uint32_t fat = b0 + at;
    const uint32_t fend = b0 + size;
    int st = seq_table(c, modes >> 6, c.ll, &c.ll_log, kLLLogMax, kMaxLL, 0, f, &fat, fend);
    if (st == kOk) st = seq_table(c, (modes >> 4) & 3u, c.of, &c.of_log, kOFLogMax, kMaxOF, 1, f, &fat, fend);
    if (st == kOk) st = seq_table(c, (modes >> 2) & 3u, c.ml, &c.ml_log, kMLLogMax, kMaxML, 2, f, &fat, fend);
    if (st != kOk) return st;
    c.n_seq = n;
    c.seq_off = fat;
    c.seq_end = fend;
    if (n) c.have_fse = 1;
    return kOk;
}

// ---- sequences ---------------------------------------------------------------------------
struct SeqState {
    const uint8_t* src;
    int32_t pos;
    uint32_t ll, of, ml;
    uint32_t rep[3];
};
struct Seq {
    uint32_t lit, match;
    uint64_t offset;
    int32_t bad;
};
DBZ_HD bool seq_start(const Ctx& c, const uint8_t* f, SeqState& s) {
    s.src = f + c.seq_off;
    s.pos = back_start(s.src, c.seq_end - c.seq_off);
    if (s.pos < c.ll_log + c.of_log + c.ml_log) return false;
    s.ll = back_bits(s.src, s.pos, (uint32_t)c.ll_log);
    s.pos -= c.ll_log;
    s.of = back_bits(s.src, s.pos, (uint32_t)c.of_log);
    s.pos -= c.of_log;
    s.ml = back_bits(s.src, s.pos, (uint32_t)c.ml_log);
    s.pos -= c.ml_log;
    for (int k = 0; k < 3; ++k) s.rep[k] = c.rep[k];
    return true;
}
DBZ_HD uint32_t seq_take(SeqState& s, uint32_t n, int32_t& bad) {
    if ((int32_t)n > s.pos) {
        bad = 1;
        s.pos = 0;
        return 0u;
    }
    const uint32_t v = back_bits(s.src, s.pos, n);
    s.pos -= (int32_t)n;
    return v;
}
// (ZSTD_decodeSequence; `last`: the states are not moved on behind the last sequence)
DBZ_HD Seq seq_next(const Ctx& c, SeqState& s, bool last) {
    Seq q;
    q.bad = 0;
    const uint32_t le = c.ll[s.ll], oe = c.of[s.of], me = c.ml[s.ml];
    const uint32_t lc = le >> 24, oc = oe >> 24, mc = me >> 24;
    const uint32_t ll0 = ll_base(lc) == 0 ? 1u : 0u;
    uint64_t offset;
    if (oc > 1) {
        offset = ((1ull << oc) - 3ull) + seq_take(s, oc, q.bad);
        s.rep[2] = s.rep[1];
        s.rep[1] = s.rep[0];
        s.rep[0] = (uint32_t)offset;
    } else if (oc == 0) {
        if (!ll0) {
            offset = s.rep[0];
        } else {
            offset = s.rep[1];
            s.rep[1] = s.rep[0];
            s.rep[0] = (uint32_t)offset;
        }
    } else {
        const uint32_t idx = 1u + ll0 + seq_take(s, 1, q.bad);
        uint32_t t = idx == 3 ? s.rep[0] - 1u : s.rep[idx];
        t += !t;                                          // (0 is not valid: libzstd makes it 1)
        if (idx != 1) s.rep[2] = s.rep[1];
        s.rep[1] = s.rep[0];
        s.rep[0] = t;
        offset = t;
    }
    q.offset = offset;
    q.match = ml_base(mc) + seq_take(s, ml_bits(mc), q.bad);
    q.lit = ll_base(lc) + seq_take(s, ll_bits(lc), q.bad);
    if (!last) {
        s.ll = (le & 0xFFFFu) + seq_take(s, (le >> 16) & 255u, q.bad);
        s.ml = (me & 0xFFFFu) + seq_take(s, (me >> 16) & 255u, q.bad);
        s.of = (oe & 0xFFFFu) + seq_take(s, (oe >> 16) & 255u, q.bad);
    }
    return q;
}

// ---- the frame, by the lanes of an Exec ----------------------------------------------------
// Exec stands for the wave: first() is true in the one lane that does the serial work, settle()
// makes what lanes wrote (shared tables, output bytes) visible to all of them, and
//   fill_tree(c)                       all lanes' shares of the Huffman table
//   literals(c, f, dst) -> status      the block's Huffman streams to dst[0, lit_size)
//   copy(dst, src, n)                  n bytes forward; dst may lie below src and overlap it
//   fill(dst, byte, n)
//   match(dst, offset, n)              dst[k] = dst[k - offset], k ascending
// The control flow below is uniform: every lane takes the same branches.
template <class Exec>
DBZ_HD int decode_frame(Exec& x, Ctx& c, const uint8_t* f, size_t n, uint8_t* out, size_t cap,
                        size_t* produced) {
    *produced = 0;
    Frame fr;
    int st = frame_header(f, n, &fr);
    if (st != kOk) return st;
    if (fr.content > cap) return kNoSpace;
    if (n > 0xFFFFFFF0ull) return kUnsupported;
    if (x.first()) {
        c.rep[0] = 1;
        c.rep[1] = 4;
        c.rep[2] = 8;
        c.have_huf = c.have_fse = 0;
    }
    x.settle();
    const uint64_t content = fr.content;
    uint64_t w = 0;                                        // bytes produced
    uint32_t at = fr.header_bytes;
    for (;;) {
        if (n - at < 3) return kTruncated;
        const uint32_t bh = le24(f + at);
        at += 3;
        const uint32_t last = bh & 1u, type = (bh >> 1) & 3u, size = bh >> 3;
        if (type == 3) return kBadBlock;
        if (type == 0) {
            if (size > n - at) return kTruncated;
            if (size > content - w) return kBadSize;
            x.copy(out + w, f + at, size);
            w += size;
            at += size;
        } else if (type == 1) {
            if (n - at < 1) return kTruncated;
            if (size > content - w) return kBadSize;
            x.fill(out + w, f[at], size);
            w += size;
            at += 1;
        } else {
            if (size > n - at) return kTruncated;
            if (x.first()) c.status = block_headers(c, f, at, size);
            x.settle();
            if (c.status != kOk) return c.status;
            if (c.lit_new_tree) {
                x.fill_tree(c);
                x.settle();
            }
            const uint32_t lit_size = c.lit_size, n_seq = c.n_seq;
            if (lit_size > content - w) return kBadSize;
            // Huffman-coded literals: straight to their place if the block has no sequences,
            // else parked at the end of the region
            const uint8_t* lit = f + c.lit_off;
            if (c.lit_type == 2) {
                uint8_t* to = n_seq ? out + (cap - lit_size) : out + w;
                st = x.literals(c, f, to);
                if (st != kOk) return st;
                x.settle();
                lit = to;
            }
            const bool rle = c.lit_type == 1;
            const uint32_t lit_byte = c.lit_byte;
            uint32_t used = 0;                             // literals consumed
            if (n_seq) {
                SeqState s;
                if (!seq_start(c, f, s)) return kBadBitstream;
                for (uint32_t k = 0; k < n_seq; ++k) {
                    const Seq q = seq_next(c, s, k + 1 == n_seq);
                    if (q.bad) return kBadBitstream;
                    if (q.lit > lit_size - used) return kBadSequences;
                    if ((uint64_t)q.lit + q.match > content - w) return kBadSize;
                    // (holds for every valid frame: the literals still unread have to fit behind)
                    if (c.lit_type == 2 && w + q.lit + q.match > cap - (lit_size - used - q.lit)) return kNoSpace;
                    if (q.offset > w + q.lit || q.offset > fr.window) return kBadOffset;
                    if (q.lit) {
                        if (rle) x.fill(out + w, lit_byte, q.lit);
                        else x.copy(out + w, lit + used, q.lit);
                        w += q.lit;
                        used += q.lit;
                    }
                    x.settle();
                    x.match(out + w, (size_t)q.offset, q.match);
                    w += q.match;
                    x.settle();
                }
                if (s.pos != 0) return kBadBitstream;
                if (x.first())
                    for (int k = 0; k < 3; ++k) c.rep[k] = s.rep[k];
            }
            const uint32_t rest = lit_size - used;
            if (rest > content - w) return kBadSize;
            if (rest && !(c.lit_type == 2 && !n_seq)) {
                if (rle) x.fill(out + w, lit_byte, rest);
                else x.copy(out + w, lit + used, rest);
            }
            w += rest;
            x.settle();
            at += size;
        }
        if (last) break;
    }
    if (w != content) return kBadSize;
    if (at != n) return kTrailing;
    *produced = (size_t)w;
    return kOk;
}

// the sizes of a block's Huffman streams in symbols
DBZ_HD uint32_t stream_symbols(const Ctx& c, int j) {
    if (c.lit_streams == 1) return c.lit_size;
    const uint32_t seg = (c.lit_size + 3) / 4;
    return j < 3 ? seg : c.lit_size - 3 * seg;
}

// ---- the CPU model's Exec: the lanes as loops ----------------------------------------------
struct HostExec {
    bool first() const { return true; }
    void settle() const {}
    void fill_tree(Ctx& c) const {
        for (int lane = 0; lane < kLanes; ++lane) dbz::fill_tree(c, lane, kLanes);
    }
    void copy(uint8_t* dst, const uint8_t* src, size_t n) const {
        for (size_t k = 0; k < n; ++k) dst[k] = src[k];
    }
    void fill(uint8_t* dst, uint32_t b, size_t n) const {
        for (size_t k = 0; k < n; ++k) dst[k] = (uint8_t)b;
    }
    void match(uint8_t* dst, size_t offset, size_t n) const {
        for (size_t k = 0; k < n; ++k) dst[k] = dst[(ptrdiff_t)k - (ptrdiff_t)offset];
    }
    // the device's rounds (dbh_zstd.hip, WaveExec::literals), lane by lane
    int literals(Ctx& c, const uint8_t* f, uint8_t* dst) const {
        const int streams = (int)c.lit_streams, per = kLanes / streams;
        const uint8_t* src[4];
        int32_t bits[4];
        uint32_t off = c.lit_off;
        for (int j = 0; j < streams; ++j) {
            src[j] = f + off;
            bits[j] = back_start(src[j], c.stream_bytes[j]);
            if (bits[j] < 0) return kBadBitstream;
            off += c.stream_bytes[j];
        }
        int32_t start[kLanes], stop[kLanes];
        Piece r[kLanes];
        for (int lane = 0; lane < kLanes; ++lane) {
            const int j = lane / per, k = lane % per;
            start[lane] = piece_start(bits[j], k, per);
            stop[lane] = piece_start(bits[j], k + 1, per);
            r[lane] = huf_piece(c.huf, c.huf_log, src[j], start[lane], stop[lane], nullptr);
        }
        for (;;) {
            bool moved = false;
            int32_t want[kLanes];
            for (int lane = 0; lane < kLanes; ++lane)
                want[lane] = lane % per == 0 ? start[lane] : r[lane - 1].end;
            for (int lane = 0; lane < kLanes; ++lane) {
                if (want[lane] == start[lane]) continue;
                moved = true;
                start[lane] = want[lane];
                r[lane] = huf_piece(c.huf, c.huf_log, src[lane / per], start[lane], stop[lane], nullptr);
            }
            if (!moved) break;
        }
        uint32_t before[kLanes];
        for (int j = 0; j < streams; ++j) {
            uint32_t sum = 0;
            int bad = 0;
            for (int lane = j * per; lane < (j + 1) * per; ++lane) {
                before[lane] = sum;
                sum += (uint32_t)r[lane].count;
                bad |= r[lane].bad;
            }
            if (bad || sum != stream_symbols(c, j)) return kBadBitstream;
        }
        const uint32_t seg = (c.lit_size + 3) / 4;
        for (int lane = 0; lane < kLanes; ++lane)
            huf_piece(c.huf, c.huf_log, src[lane / per], start[lane], stop[lane],
                      dst + (size_t)(lane / per) * seg + before[lane]);
        return kOk;
    }
};

inline int decode_host(const uint8_t* frame, size_t frame_bytes, uint8_t* out, size_t out_capacity,
                       size_t* produced) {
    Ctx* c = new Ctx();
    HostExec x;
    const int st = decode_frame(x, *c, frame, frame_bytes, out, out_capacity, produced);
    delete c;
    return st;
}

}  // namespace dbz
