// dbh_inflate.hip - inflating the Signal chunks of fast5 files ON THE GPU (C ABI: the
// "compressed input" section of include/deepbinner_hip.h).
//
// The reference inflates on the host: h5py -> libhdf5 -> zlib, one chunk after the other
// (deepbinner/load_fast5s.py:33-43).  For this package's native loader that is ~100 of the ~118 us
// a 55 KB read costs a CPU core, and the box hands a process 16 cores: one host stops at ~130 k
// reads/s while ONE GPU classifies 214 k (profiles/r03_*).  A container of 4,000 reads is 4,000
// independent zlib streams - latency-bound, branchy, byte-granular work that a CPU runs 16 at a
// time and a GPU runs thousands at a time.
//
// Two kernels (RFC 1950 / 1951; bit-exact with zlib, same accept / reject decisions; the decoder
// core is dbh_inflate_core.h + dbh_inflate_wave.h, which the CPU test harness compiles too):
//   1. Huffman codes -> tokens (literal | match {length, distance}): no output bytes, no window -
//      nothing here depends on memory the kernel wrote itself.  inflate_tokens_wave_kernel - ONE
//      WAVEFRONT PER STREAM: the 64 lanes decode 64 consecutive pieces of the same Huffman block
//      at once, each from a guessed first bit, and re-decode until every piece begins where the
//      one before it ended (prefix codes re-synchronise: ~2.7 rounds; dbh_inflate_wave.h); 4,000
//      streams are 4,000 waves, a dozen per CU.  (The one-lane-per-stream kernel of rounds 3 and 4
//      is retired; what it measured is in HISTORY.md.)
//   2. tokens -> bytes, ONE WAVE PER STREAM, up to 64 tokens per step: a wave-wide prefix sum of
//      the token lengths gives every token its output position.  inflate_resolve_pre_kernel
//      (described in front of it) - an 8 KiB ring in LDS and the stream's own flushed output
//      behind it, twenty streams per CU; the short matches whose source is complete before their
//      step (four fifths of all) read it at the step boundary and are stored with the literals,
//      the others go in rounds by the exact rule: 0.84 ms per 4,000 x 54 KB streams.  (The
//      32 KiB-ring kernel of rounds 3-5 is retired: HISTORY.md.)
//      The ring is written out in coalesced 256-byte pieces, with the Adler-32 sums on the way.
// A stream of mode DBH_INFLATE_ZLIB_SHUFFLE (shuffle + deflate) is a zlib stream behind a 4-byte
// prefix to every kernel here (zlib_view); its bytes are de-interleaved behind them (dbh_vbz.hip).
// Streams of mode DBH_INFLATE_VBZ (ONT's VBZ filter, zstd stage undone by the loader) and
// DBH_INFLATE_VBZ_ZSTD (the chunk as stored) are no kernel's here: both kernels pass them by, and
// dbh_zstd.hip's and dbh_vbz.hip's kernels, launched behind them by dbh_inflate_dev, decode them;
// so are DBH_INFLATE_SVB16 and DBH_INFLATE_SVB16_ZSTD, the rows of a POD5 signal table.
// What dbh_inflate_dev launches is both of them AT ONCE, a pair of waves per stream
// (inflate_pair_kernel: wave 0 is kernel 1, wave 1 is kernel 2 resolving the tokens as they come;
// described in front of it) - a stream then lasts as long as the slower of its halves, not their
// sum; DEEPBINNER_INFLATE_PAIR=0: the two launches.
// HBM traffic per read (55 KB of samples, ~22 k tokens): 35 KB compressed in, 88 KB of tokens out
// and in again, 55 KB of samples out - latency and instruction issue, not bandwidth, are what
// both kernels are bound by.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/deepbinner_hip.h"
#include "dbh_host_layout.h"
#include "dbh_inflate_core.h"
#include "dbh_inflate_wave.h"
#include "dbh_owned.h"
#include "dbh_wave.h"

namespace dbh_inflate_detail {

using dbi::Lane;
using dbh_wave::from_lane_before;
using dbh_wave::wave_scan_inclusive;
using dbh_wave::wave_sum;

// what kernel 1 leaves for kernel 2 (and for the caller) per stream
struct StreamInfo {
    int32_t status;
    int32_t ended;
    uint32_t adler;
    int32_t n_tokens;
    int64_t produced;
};

// What the inflate kernels make of a record - both forms of them, through this one helper.
// A stream of mode DBH_INFLATE_ZLIB_SHUFFLE (u32 LE N, then a zlib stream whose content is N
// shuffled bytes) is to them the DBH_INFLATE_ZLIB stream behind its prefix, wanted N: its bytes go
// to the stream's output region, where dbh_vbz.hip's kernel finds and de-interleaves them.  With a
// prefix that cannot be (odd, beyond out_bytes, outside the buffer) there is nothing to decode: a
// stored stream of no bytes, i.e. zeros - dbh_vbz.hip's kernel applies the same test and refuses
// it.  DBH_INFLATE_STORED_SHUFFLE is that kernel's alone (passed_by).  Every other record: itself.
__device__ __forceinline__ dbh_inflate_stream zlib_view(const dbh_inflate_stream& s,
                                                        const uint8_t* __restrict__ comp,
                                                        int64_t comp_total) {
    if (s.mode != DBH_INFLATE_ZLIB_SHUFFLE) return s;
    dbh_inflate_stream v = s;
    v.mode = DBH_INFLATE_STORED;
    v.comp_bytes = 0;
    if (s.comp_offset < 0 || s.comp_bytes < 4 || s.comp_offset > comp_total - s.comp_bytes) return v;
    uint32_t n;
    __builtin_memcpy(&n, comp + s.comp_offset, 4);
    if ((n & 1u) || (int64_t)n > s.out_bytes) return v;
    v.mode = DBH_INFLATE_ZLIB;
    v.comp_offset = s.comp_offset + 4;
    v.comp_bytes = s.comp_bytes - 4;
    v.out_bytes = (int64_t)n;
    return v;
}
// the modes that are other kernels' (dbh_vbz.hip, dbh_zstd.hip): kernel 2 leaves their output alone
__device__ __forceinline__ bool passed_by(int mode) {
    return mode == DBH_INFLATE_VBZ || mode == DBH_INFLATE_VBZ_ZSTD || mode == DBH_INFLATE_STORED_SHUFFLE ||
           mode == DBH_INFLATE_SVB16 || mode == DBH_INFLATE_SVB16_ZSTD;
}

// ---------------------------------------------------------------------------------------------
// Kernel 1: ONE WAVE PER STREAM (dbh_inflate_wave.h - the rounds, why they end, what
// they cost).  One wavefront per workgroup, one stream per workgroup, in the caller's order (the
// longest first, if the caller has sorted them).  LDS: the staged chunk (4.4 KB) and ONE set of
// canonical code tables (1.3 KB) - a dozen and more waves per CU, which is what hides the LDS
// round trips of a token's dependent chain here.
// ---------------------------------------------------------------------------------------------
struct WaveLds {
    uint32_t stage[dbi::kStageDwords];
    uint32_t ring[dbi::kRingStore], lit_pair[16], dist_pair[16];
    uint16_t lit_sym[dbi::kLitSyms], cnt[16];
    uint16_t wave_lit_tab[dbi::kWaveLitEntries], wave_dist_tab[dbi::kWaveDistEntries];
    uint8_t dist_sym[dbi::kDistSyms], lens[dbi::kMaxLens];
};
// (the code-length code's table - 128 bytes, lane 0's, needed only while a block header is read -
// lies in the chunk's stage: no chunk is staged then.  128 bytes more would make a CU's LDS hold
// 15 of these instead of 16.)
static_assert(sizeof(((WaveLds*)nullptr)->stage) >= (1 << dbi::kClTableBits), "");
struct WaveMem {
    WaveLds* m;
    __device__ __forceinline__ uint32_t cl_tab(int i) const {
        return reinterpret_cast<const uint8_t*>(m->stage)[i];
    }
    __device__ __forceinline__ void set_cl_tab(int i, uint32_t v) {
        reinterpret_cast<uint8_t*>(m->stage)[i] = (uint8_t)v;
    }
    __device__ __forceinline__ uint32_t stage(int i) const { return m->stage[i]; }
    __device__ __forceinline__ uint32_t wave_lit_tab(int i) const { return m->wave_lit_tab[i]; }
    __device__ __forceinline__ uint32_t wave_dist_tab(int i) const { return m->wave_dist_tab[i]; }
    __device__ __forceinline__ uint32_t ring(int r) const { return m->ring[r]; }
    __device__ __forceinline__ void set_ring(int r, uint32_t v) { m->ring[r] = v; }
    __device__ __forceinline__ int len(int i) const { return m->lens[i]; }
    __device__ __forceinline__ void set_len(int i, int v) { m->lens[i] = (uint8_t)v; }
    __device__ __forceinline__ int cnt(int l) const { return m->cnt[l]; }
    __device__ __forceinline__ void set_cnt(int l, int v) { m->cnt[l] = (uint16_t)v; }
    __device__ __forceinline__ uint32_t lit_pair(int l) const { return m->lit_pair[l]; }
    __device__ __forceinline__ void set_lit_pair(int l, uint32_t v) { m->lit_pair[l] = v; }
    __device__ __forceinline__ uint32_t dist_pair(int l) const { return m->dist_pair[l]; }
    __device__ __forceinline__ void set_dist_pair(int l, uint32_t v) { m->dist_pair[l] = v; }
    __device__ __forceinline__ uint32_t lit_sym(int i) const { return m->lit_sym[i]; }
    __device__ __forceinline__ void set_lit_sym(int i, uint32_t v) { m->lit_sym[i] = (uint16_t)v; }
    __device__ __forceinline__ uint32_t dist_sym(int i) const { return m->dist_sym[i]; }
    __device__ __forceinline__ void set_dist_sym(int i, uint32_t v) { m->dist_sym[i] = (uint8_t)v; }
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t uni(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// a compiler barrier that also drains the wave's LDS queue: what other lanes wrote is there (a
// wave's LDS operations execute in order; this is all the synchronisation ONE wave needs)
__device__ __forceinline__ void lds_settle() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

struct NoProgress {
    __device__ __forceinline__ void tokens(int) const {}
};

// One stream through kernel 1: the tokens to `tokens` + the stream's out_offset, its record
// returned (lane 0's copy is the stream's state).  `lds` is this wave's own, the wave synchronises with nobody (inflate_tokens_wave_kernel: one wave per
// workgroup; inflate_pair_kernel: beside the wave that resolves the same stream's tokens, which
// `progress.tokens(n)` tells how many are there - behind every chunk and every stored run).
template <class Progress>
__device__ __forceinline__ StreamInfo tokens_wave_stream(
    WaveLds& lds, const uint8_t* __restrict__ comp, int64_t comp_total, const dbh_inflate_stream& st,
    uint32_t* tokens, int lane, const Progress& progress) {
    using namespace dbi;
    if (st.mode != DBH_INFLATE_ZLIB)                     // nothing to decode: kernel 2 copies it
        return StreamInfo{kOk, 0, 0u, 0, 0};
    WaveMem mem{&lds};
    // Lane 0's copy of L is the stream's state; the serial code (header, block headers with their
    // code builds, stored bytes) runs on lane 0 alone, and what the whole wave needs of it is
    // handed round afterwards.
    Lane L;
    uint32_t* const tok = tokens + st.out_offset;        // one token slot per byte of output
    int n_tok = 0;
    // (the caller's buffer is readable for 64 bytes beyond comp_total)
    lane_start(L, mem, comp + st.comp_offset, st.comp_bytes, st.out_bytes,
               comp_total + 64 - st.comp_offset);        // (every lane the same: uniform so far)
    WaveBlock B;
    while (uni(L.state) != kDone) {
        const int state = uni(L.state);
        if (state == kNeedBlock) {
            if (lane == 0) lane_block(L, mem);
#pragma unroll
            for (int l = 0; l < 15; ++l) {
                B.lim_lit[l] = uni(L.lim_lit[l]);
                B.lim_dist[l] = uni(L.lim_dist[l]);
            }
            lds_settle();                                 // (the tables lane 0 wrote: for all lanes)
            if (kWaveTables && uni(L.state) == kDecode) {
                // the first-level tables of this block's two codes: every lane its share of the
                // indices, decoded the canonical way (dbh_inflate_wave.h)
                for (int k = lane; k < kWaveLitEntries; k += kWaveLanes)
                    lds.wave_lit_tab[k] = (uint16_t)wave_lit_entry((uint32_t)k, B.lim_lit, mem);
                for (int k = lane; k < kWaveDistEntries; k += kWaveLanes)
                    lds.wave_dist_tab[k] = (uint16_t)wave_dist_entry((uint32_t)k, B.lim_dist, mem);
                lds_settle();    
            }
            continue;
        }
        if (state == kStored) {
            // the bytes of a stored block: literal tokens, 64 at a time
            L.stored_left = uni(L.stored_left);
            L.out_pos = uni(L.out_pos);
            L.br.bp = uni(L.br.bp);
            L.final_block = uni(L.final_block);
            const int n = stored_run(L);
            const uint8_t* src = comp + st.comp_offset + (L.br.bp >> 3);
            for (int k = lane; k < n; k += kWaveLanes) tok[n_tok + k] = src[k];
            n_tok += n;
            progress.tokens(n_tok);
            if (stored_advance(L, n) && lane == 0) L.br.seek(mem, L.br.bp);
            continue;
        }
        // ---- inside a Huffman block: one chunk of 64 homes ----
        const uint32_t bp = uni(L.br.bp);
        int out_pos = uni(L.out_pos);
        const int out_cap = uni(L.out_cap);
        const uint32_t first_dword = bp >> 5, rel0 = bp & 31u;
        const uint32_t fetch_cap = uni(L.br.fetch_cap);
        const uint8_t* in = comp + st.comp_offset;
        lds_settle();                                     // (nobody still reads the chunk before)
        for (int piece = lane; piece < kStageDwords / 4; piece += kWaveLanes) {
            U4 v;
            __builtin_memcpy(&v, in + stage_piece_at(first_dword, piece, fetch_cap), 16);
            *reinterpret_cast<U4*>(&lds.stage[4 * piece]) = v;
        }
        lds_settle();    
        B.limit_rel = uni(L.br.limit_bits) - first_dword * 32u;
        uint32_t x = sub_start(rel0, lane);
        const uint32_t stop = sub_start(rel0, lane + 1);
        // (the walks keep their tokens at the end of the stream's token region, if there is room)
        const KeepTokens kept{keep_room(n_tok, st.out_bytes) ? tok + (st.out_bytes - kKeepSlots) : nullptr, lane};
        SubResult r = sub_decode(B, mem, x, stop, kept);
        int last;
        for (;;) {
            const uint32_t prev_end = from_lane_before(r.end);
            const int prev_flag = (int)from_lane_before((uint32_t)r.flag);
            const uint32_t want = lane == 0 ? rel0 : prev_flag != kSubNone ? sub_start(rel0, lane) : prev_end;
            const bool moved = want != x;
            const unsigned long long m_moved = __ballot(moved), m_flag = __ballot(r.flag != kSubNone);
            const int first_moved = m_moved ? __ffsll((long long)m_moved) - 1 : kWaveLanes;
            const int first_flag = m_flag ? __ffsll((long long)m_flag) - 1 : kWaveLanes;
            if (first_moved > first_flag || first_moved == kWaveLanes) {
                last = uni(first_flag < kWaveLanes ? first_flag : kWaveLanes - 1);
                break;
            }
            if (moved) {
                x = want;
                r = sub_decode(B, mem, x, stop, kept);
            }
        }
        // where every lane's tokens and bytes go; the lane in which the wanted number of bytes is
        // exceeded ends the chunk, if that comes first
        const int cnt_m = lane <= last ? r.count : 0, bytes_m = lane <= last ? r.bytes : 0;
        const int incl_c = wave_scan_inclusive(cnt_m), incl_b = wave_scan_inclusive(bytes_m);
        const unsigned long long m_over = __ballot(lane <= last && out_pos + incl_b > out_cap);
        if (m_over) {
            const int over = __ffsll((long long)m_over) - 1;
            last = uni(over < last ? over : last);
        }
        SubResult e;
        e.end = 0;
        e.count = e.bytes = 0;
        e.flag = kSubNone;
        if (kept.keep != nullptr && m_over == 0ull && !__any(lane <= last && r.count > kSubKeep)) {
            // the output pass as a copy: what the lanes' last walks kept, to where it belongs
            uint32_t* to = tok + n_tok + incl_c - cnt_m;
            for (int k = 0; __any(k < cnt_m); ++k)
                if (k < cnt_m) to[k] = kept.keep[k * kWaveLanes + lane];
            if (lane <= last) e = r;
        } else if (lane <= last) {
            e = sub_emit(B, mem, x, stop, out_pos + incl_b - bytes_m, out_cap, tok + n_tok + incl_c - cnt_m);
        }
        const int flag = __builtin_amdgcn_readlane(e.flag, last);
        n_tok += __builtin_amdgcn_readlane(incl_c - cnt_m, last) + __builtin_amdgcn_readlane(e.count, last);
        progress.tokens(n_tok);
        out_pos += __builtin_amdgcn_readlane(incl_b - bytes_m, last) + __builtin_amdgcn_readlane(e.bytes, last);
        L.out_pos = out_pos;
        L.br.bp = first_dword * 32u + (uint32_t)__builtin_amdgcn_readlane((int)e.end, last);
        if (flag == kSubBad) lane_fail(L, kBadSymbol);
        else if (flag == kSubTrunc) lane_fail(L, kTruncated);
        else if (flag == kSubBeyond) L.state = kDone;
        else if (flag == kSubEnd) {
            L.state = kNeedBlock;
            if (uni(L.final_block)) {
                lane_ended(L);                   // (every lane the same)
            } else if (lane == 0) {
                L.br.seek(mem, L.br.bp);
            }
        }
    }
    StreamInfo rec;
    rec.status = L.status;
    rec.ended = L.ended;
    rec.adler = L.adler;
    rec.n_tokens = n_tok;
    rec.produced = L.out_pos;
    return rec;
}

__global__ __launch_bounds__(dbi::kWaveLanes) __attribute__((amdgpu_waves_per_eu(4, 8))) void inflate_tokens_wave_kernel(
    const uint8_t* __restrict__ comp, int64_t comp_total,
    const dbh_inflate_stream* __restrict__ streams, int n_streams, uint32_t* __restrict__ tokens,
    StreamInfo* __restrict__ info) {
    __shared__ __attribute__((aligned(16))) WaveLds lds;
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    if (i >= n_streams) return;
    const dbh_inflate_stream st = zlib_view(streams[i], comp, comp_total);
    const StreamInfo rec = tokens_wave_stream(lds, comp, comp_total, st, tokens, lane, NoProgress());
    if (lane == 0) info[i] = rec;
}

static_assert(dbi::kStepTokens == 64, "one token per lane and step");

// ---------------------------------------------------------------------------------------------
// Kernel 2: one wave per stream and up to 64 tokens per step (dbh_inflate_core.h: "Phase 2's
// second form").  Its first form (rounds 3-5, retired: HISTORY.md) sent every match through the
// rounds: a step's ~38 matches of ~3.6 bytes took 3.65 rounds of 4.6 four-byte turns, each a
// dependent LDS load and store behind a drained queue - ~5 k cycles per step, 60 % of them
// waiting, with five waves per CU (32 KiB rings) and nothing to fill the waits.  Here
//   * a short match whose source is complete before its step ("pre", 82 %) reads its eight source
//     bytes at the boundary in front of the step - one unaligned ds_read_b64 from the ring, or one
//     unaligned global load from the stream's own output where the source lies further back than
//     the ring reaches - and is two overlapping four-byte stores (or two two-byte ones) at the top
//     of its step, together with the literals;
//   * the others ("late": ~3.9 per step) go in rounds by the exact rule (a scalar loop over the
//     waiting lanes): 1.36 rounds per step, eight bytes in the first turn; a match that overlaps
//     itself repeats its first dist bytes (k2_pattern8);
//   * the ring is 8 KiB: twenty streams per CU, one wave per workgroup (a CU's LDS comes back
//     stream by stream, not when the longest of five has ended).
// The CPU harness models this schedule byte for byte - which copy of a position (ring slot or
// flushed output) every read sees - and holds it against the tokens resolved in order.
constexpr int kRing = dbi::kSmallRing;
__device__ __forceinline__ uint64_t ring_read8(const uint8_t* ring, int p) {
    const int slot = p & (kRing - 1);
    uint64_t v;
    if (slot <= kRing - 8) {
        __builtin_memcpy(&v, ring + slot, 8);          // (byte-aligned: hipcc emits ds_read_b64)
    } else {                                           // over the end of the ring: byte by byte
        v = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) v |= (uint64_t)ring[(slot + j) & (kRing - 1)] << (8 * j);
    }
    return v;
}
__device__ __forceinline__ uint64_t output_read8(const uint8_t* dst, int p) {
    uint64_t v;
    __builtin_memcpy(&v, dst + p, 8);                  // (one unaligned global_load_dwordx2)
    return v;
}
// the first `len` (1..8) bytes of v to positions p, p + 1, ...
__device__ __forceinline__ void ring_store_short(uint8_t* ring, int p, int len, uint64_t v) {
    const int slot = p & (kRing - 1);
    if (len >= 3 && slot + len <= kRing) {
        if (len >= 4) {                                // two four-byte stores that may overlap
            const uint32_t a = (uint32_t)v, b = (uint32_t)(v >> (8 * (len - 4)));
            __builtin_memcpy(ring + slot, &a, 4);
            __builtin_memcpy(ring + slot + (len - 4), &b, 4);
        } else {                                       // three bytes: two two-byte stores
            const uint16_t a = (uint16_t)v, b = (uint16_t)(v >> 8);
            __builtin_memcpy(ring + slot, &a, 2);
            __builtin_memcpy(ring + slot + 1, &b, 2);
        }
    } else {                                           // a cut match of one or two bytes, or over
#pragma unroll                                         // the end of the ring
        for (int j = 0; j < 8; ++j)
            if (j < len) ring[(slot + j) & (kRing - 1)] = (uint8_t)(v >> (8 * j));
    }
}

// A step's tokens, decoded and placed: lane l holds token first + l if the step takes it.
struct StepTokens {
    uint32_t t;
    bool valid, is_match;
    int len, dist, my;
    int total, count;          // (uniform) bytes and tokens of the step
};
// `raw` = tok[first + lane] (0 behind the last token).  The step takes the tokens that together
// span at most kStepSpan bytes - all 64 unless there are long matches among them.
__device__ __forceinline__ StepTokens place_step(uint32_t raw, int first, int n_tok, int base, int lane) {
    StepTokens s;
    s.t = raw;
    s.valid = first + lane < n_tok;
    s.is_match = s.valid && (raw & dbi::kMatchFlag);
    s.len = !s.valid ? 0 : s.is_match ? (int)(raw & 0x1FFu) : 1;
    s.dist = (int)((raw >> 9) & 0x7FFFu) + 1;
    const int incl = wave_scan_inclusive(s.len);
    s.total = __builtin_amdgcn_readlane(incl, 63);
    s.count = n_tok - first < 64 ? n_tok - first : 64;
    if (s.total > dbi::kStepSpan) {                    // (rare: long matches)
        const bool keep = s.valid && incl <= dbi::kStepSpan;      // a prefix of the lanes, never empty
        s.count = __popcll(__ballot(keep));
        s.total = __builtin_amdgcn_readlane(incl, s.count - 1);
        s.valid = keep;
        s.is_match = s.is_match && keep;
        s.len = keep ? s.len : 0;
    }
    s.my = base + incl - s.len;
    return s;
}

// Adler-32 from sums that do not need the stream's length while they are taken (the pair kernel
// resolves a stream whose end kernel 1 has not reached yet): S = sum of the bytes, P = sum of
// position x byte; s1 = 1 + S, s2 = n + n S - P (mod 65521) once n is known.  Every lane keeps its
// own two sums, the wave adds them up once per stream.
struct AdlerSums {
    unsigned bytes;
    unsigned long long weighted;
    __device__ __forceinline__ void add4(unsigned w, unsigned position) {
        const unsigned b0 = w & 255u, b1 = (w >> 8) & 255u, b2 = (w >> 16) & 255u, b3 = w >> 24;
        const unsigned s = b0 + b1 + b2 + b3;
        bytes += s;
        weighted += (unsigned long long)position * s + (b1 + 2u * b2 + 3u * b3);
    }
    __device__ __forceinline__ void add1(unsigned b, unsigned position) {
        bytes += b;
        weighted += (unsigned long long)position * b;
    }
    // (wave-uniform) the stream's Adler-32, n = its length
    __device__ __forceinline__ unsigned finish(unsigned n) const {
        const unsigned long long S = wave_sum(bytes) % 65521u, P = wave_sum(weighted) % 65521ull;
        const unsigned long long nm = n % 65521u;
        const unsigned s1 = (unsigned)((1ull + S) % 65521ull);
        const unsigned s2 = (unsigned)((nm + nm * S + 65521ull - P) % 65521ull);
        return (s2 << 16) | s1;
    }
};

// how many of a stream's tokens are there: all of them (kernel 1 has ended: the two launches) ...
struct AllTokensThere {
    StreamInfo r;
    __device__ __forceinline__ void wait(int, int& limit, bool& done) const {
        limit = r.n_tokens;
        done = true;
    }
    __device__ __forceinline__ StreamInfo record() const { return r; }
};

// One stream through kernel 2: its bytes to out + the stream's out_offset, the
// verdict to *status_slot.  `ring` (kSmallRing bytes) is this wave's own.  `there.wait(need, limit,
// done)` returns once tokens [0, need) are there or kernel 1 is done with the stream; `limit` = the
// number of tokens if it is done, INT_MAX otherwise.
template <class Tokens>
__device__ __forceinline__ void resolve_pre_stream(
    uint8_t* ring, const uint8_t* __restrict__ comp, const dbh_inflate_stream& s,
    const uint32_t* tokens, const Tokens& there, uint8_t* out, int32_t* status_slot, int lane) {
    {
        uint8_t* dst = out + s.out_offset;
        const int64_t cap = s.out_bytes;
        if (passed_by(s.mode)) return;               // (dbh_vbz.hip, dbh_zstd.hip)
        if (s.mode != DBH_INFLATE_ZLIB) {
            const int64_t have = s.comp_bytes < cap ? s.comp_bytes : cap;
            const uint8_t* src = comp + s.comp_offset;
            const int64_t whole = have & ~(int64_t)7;
            for (int64_t k = 8 * (int64_t)lane; k < whole; k += 512) {
                uint64_t v;
                __builtin_memcpy(&v, src + k, 8);
                __builtin_memcpy(dst + k, &v, 8);
            }
            for (int64_t k = whole + lane; k < cap; k += 64) dst[k] = k < have ? src[k] : (uint8_t)0;
            if (lane == 0) *status_slot = dbi::kOk;
            return;
        }
        int status = dbi::kOk;                       // (kernel 1's verdict joins at the end)
        const uint32_t* tok = tokens + s.out_offset;
        int n_tok;                                    // INT_MAX while kernel 1 is still at the stream
        bool all_there;
        // (a step needs its own tokens and the next step's, which are decoded while it runs)
        there.wait(128, n_tok, all_there);
        int pos = 0, flushed = 0;
        AdlerSums adler = {0u, 0ull};
        if (n_tok > 0) {
            int first = 0;                            // this step's first token
            StepTokens c = place_step(lane < n_tok ? tok[lane] : 0u, 0, n_tok, 0, lane);
            uint32_t raw_next = 64 + lane < n_tok ? tok[64 + lane] : 0u;      // (if this step takes 64)
            bool pre = false;                         // (nothing lies before the first step)
            uint64_t pv = 0ull;
            for (;;) {
                const int end = pos + c.total;
                if (__any(c.is_match && c.dist > c.my)) {   // reaches before the start of the output
                    status = dbi::kBadDistance;
                    break;
                }
                // the step behind this one is decoded and placed while this one's stores land
                const int first_n = first + c.count;
                // the next step's tokens are in registers; the ones behind them are requested now
                if (!all_there) there.wait(first_n + 128, n_tok, all_there);
                if (c.count != 64) raw_next = first_n + lane < n_tok ? tok[first_n + lane] : 0u;
                const uint32_t raw_after = first_n + 64 + lane < n_tok ? tok[first_n + 64 + lane] : 0u;
                const StepTokens n = place_step(raw_next, first_n, n_tok, end, lane);

                const int src = c.my - c.dist;
                const int reach = src + (c.len < c.dist ? c.len : c.dist);
                const int my_end = c.my + c.len;
                if (c.valid && !c.is_match) ring[c.my & (kRing - 1)] = (uint8_t)c.t;
                if (pre) ring_store_short(ring, c.my, c.len, c.dist < c.len ? dbi::k2_pattern8(pv, c.dist) : pv);
                bool waiting = c.is_match && !pre;
                unsigned long long mask = __ballot(waiting);
                while (mask != 0ull) {
                    lds_settle();
                    bool blocked = false;
                    for (unsigned long long it = mask; it != 0ull; it &= it - 1ull) {
                        const int w = __ffsll((long long)it) - 1;
                        blocked = blocked || dbi::k2_blocks(__builtin_amdgcn_readlane(c.my, w),
                                                            __builtin_amdgcn_readlane(my_end, w), src, reach);
                    }
                    const bool go = waiting && !blocked;
                    if (go) {
                        uint64_t v = dbi::k2_in_ring(src, end) ? ring_read8(ring, src) : output_read8(dst, src);
                        if (c.dist < 8 && c.dist < c.len) v = dbi::k2_pattern8(v, c.dist);
                        ring_store_short(ring, c.my, c.len < 8 ? c.len : 8, v);
                    }
                    if (__any(go && c.len > 8)) {
                        // what is left of a long match: four bytes per turn, byte k = byte k mod
                        // dist of the dist bytes before the match
                        int k = 8, o = 8 % c.dist;
                        while (__any(go && k < c.len)) {
                            if (go && k < c.len) {
                                int o1 = o + 1;
                                o1 = o1 == c.dist ? 0 : o1;
                                int o2 = o1 + 1;
                                o2 = o2 == c.dist ? 0 : o2;
                                int o3 = o2 + 1;
                                o3 = o3 == c.dist ? 0 : o3;
                                const bool near = dbi::k2_in_ring(src, end);      // (then all of [src, my) is)
                                const uint8_t b0 = near ? ring[(src + o) & (kRing - 1)] : dst[src + o];
                                const uint8_t b1 = near ? ring[(src + o1) & (kRing - 1)] : dst[src + o1];
                                const uint8_t b2 = near ? ring[(src + o2) & (kRing - 1)] : dst[src + o2];
                                const uint8_t b3 = near ? ring[(src + o3) & (kRing - 1)] : dst[src + o3];
                                ring[(c.my + k) & (kRing - 1)] = b0;
                                if (k + 1 < c.len) ring[(c.my + k + 1) & (kRing - 1)] = b1;
                                if (k + 2 < c.len) ring[(c.my + k + 2) & (kRing - 1)] = b2;
                                if (k + 3 < c.len) ring[(c.my + k + 3) & (kRing - 1)] = b3;
                                o = o3 + 1;
                                o = o == c.dist ? 0 : o;
                                k += 4;
                            }
                        }
                    }
                    waiting = waiting && !go;
                    mask = __ballot(waiting);
                }
                lds_settle();                          // everything of this step is in the ring
                pos = end;
                // the boundary: the next step's short matches whose source is complete read it now -
                // from the ring, or from the flushed output where the ring no longer holds it
                const int src_n = n.my - n.dist;
                const bool pre_n = dbi::k2_pre(n.is_match, n.len,
                                               src_n + (n.len < n.dist ? n.len : n.dist), pos);
                uint64_t pv_n = 0ull;
                if (pre_n && src_n >= 0)
                    pv_n = dbi::k2_in_ring(src_n, pos) ? ring_read8(ring, src_n) : output_read8(dst, src_n);
                // whole 256-byte pieces out of the ring, the Adler-32 sums on the way
                if (pos - flushed >= 256) {
                    do {
                        const uint32_t w = *reinterpret_cast<const uint32_t*>(
                            ring + ((flushed + 4 * lane) & (kRing - 1)));
                        uint16_t* d16 = reinterpret_cast<uint16_t*>(dst + flushed + 4 * lane);
                        d16[0] = (uint16_t)w;             // (a read starts at an even byte, not
                        d16[1] = (uint16_t)(w >> 16);     //  necessarily at a multiple of four)
                        adler.add4(w, (unsigned)(flushed + 4 * lane));
                        flushed += 256;
                    } while (pos - flushed >= 256);
                }
                if (first_n >= n_tok) break;
                first = first_n;
                c = n;
                raw_next = raw_after;
                pre = pre_n;
                pv = pv_n;
            }
        }
        // (the loop ends when kernel 1 has - its record is there - or on this wave's own error, with
        // the partner possibly still decoding: record() waits for its verdict, so that the code
        // handed back is the one the two-launch path gives)
        const StreamInfo r = there.record();
        if (r.status != dbi::kOk) status = r.status;
        if (status == dbi::kOk) {
            lds_settle();
            const int rest = pos - flushed;           // < 256
            for (int k = lane; k < rest; k += 64) {
                const unsigned b = ring[(flushed + k) & (kRing - 1)];
                dst[flushed + k] = (uint8_t)b;
                adler.add1(b, (unsigned)(flushed + k));
            }
            if (r.ended && adler.finish((unsigned)r.produced) != r.adler) status = dbi::kBadChecksum;
            // a stream that ends early (MinKNOW's short final chunk): libhdf5 zero-extends it
            for (int64_t k = pos + lane; k < cap; k += 64) dst[k] = 0;
        }
        if (status != dbi::kOk)                       // nothing of a damaged stream is handed on
            for (int64_t k = lane; k < cap; k += 64) dst[k] = 0;
        if (lane == 0) *status_slot = status;
    }
}

__global__ __launch_bounds__(64) void inflate_resolve_pre_kernel(
    const uint8_t* __restrict__ comp, int64_t comp_total,
    const dbh_inflate_stream* __restrict__ streams, int n_streams,
    const uint32_t* __restrict__ tokens, StreamInfo* __restrict__ info, uint8_t* out,
    int32_t* __restrict__ status_out) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < n_streams; i += gridDim.x) {
        const dbh_inflate_stream s = zlib_view(streams[i], comp, comp_total);
        resolve_pre_stream(ring, comp, s, tokens, AllTokensThere{info[i]}, out, status_out + i, lane);
    }
}

// ---------------------------------------------------------------------------------------------
// BOTH KERNELS AS A PAIR OF WAVES PER STREAM (what runs; DEEPBINNER_INFLATE_PAIR=0: two launches).
// A stream is one wave's sequential work in either kernel, and as two launches a container's
// inflating lasts as long as its longest stream takes in kernel 1 PLUS as long as it takes in
// kernel 2 - 4.8 + 3.9 ms for a read of 400 k samples, whatever else the launches hold; for
// containers of long reads (1,000 of ~100 k samples) that, not the kernels' CU time, set the
// streaming path's rate (profiles/r05_k2/long_reads_100k_samples.txt).  Here a workgroup is two
// waves on one stream: wave 0 is kernel 1 and says behind every chunk how many tokens are there
// (a word in LDS, behind a workgroup-scope release: the two waves share the CU's L1, the tokens
// need no more than to have left the wave), wave 1 is kernel 2 and resolves them as they come -
// a step at a time once its tokens, the next step's and the ones prefetched behind them are
// there, sleeping otherwise.  The same tokens, the same schedule, the same bytes; a stream lasts
// as long as the slower of its two halves.
struct PairWords {
    int committed;             // tokens kernel 1 has stored so far
    int done;                  // kernel 1 has ended; the record below is its verdict
    int status, ended, n_tokens, produced;
    unsigned adler;
};
struct PairProgress {
    PairWords* w;
    int lane;
    __device__ __forceinline__ void tokens(int n) const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // (the tokens have left the wave)
        if (lane == 0) __hip_atomic_store(&w->committed, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};
struct TokensFromPartner {
    PairWords* w;
    __device__ __forceinline__ void wait(int need, int& limit, bool& done) const {
        for (;;) {
            const int d = __hip_atomic_load(&w->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int c = __hip_atomic_load(&w->committed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (d != 0 || c >= need) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                done = d != 0;
                limit = done ? __hip_atomic_load(&w->n_tokens, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                             : 0x7FFFFFFF;
                return;
            }
            __builtin_amdgcn_s_sleep(16);
        }
    }
    __device__ __forceinline__ StreamInfo record() const {
        // (the resolver may get here on an error of its own while the decoder still runs: the words
        // below are written just before `done`)
        while (__hip_atomic_load(&w->done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0)
            __builtin_amdgcn_s_sleep(16);
        StreamInfo r;
        r.status = w->status;
        r.ended = w->ended;
        r.adler = w->adler;
        r.n_tokens = w->n_tokens;
        r.produced = w->produced;
        return r;
    }
};

__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(4, 8))) void inflate_pair_kernel(
    const uint8_t* __restrict__ comp, int64_t comp_total,
    const dbh_inflate_stream* __restrict__ streams, int n_streams, uint32_t* tokens,
    StreamInfo* __restrict__ info, uint8_t* out, int32_t* __restrict__ status_out) {
    __shared__ __attribute__((aligned(16))) WaveLds decode;
    __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
    __shared__ PairWords words;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x;
    if (i >= n_streams) return;
    if (threadIdx.x == 0) {
        words.committed = 0;
        words.done = 0;
    }
    __syncthreads();
    const dbh_inflate_stream st = zlib_view(streams[i], comp, comp_total);
    if (wave == 0) {
        const StreamInfo rec = tokens_wave_stream(decode, comp, comp_total, st, tokens, lane,
                                                  PairProgress{&words, lane});
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) {                                   // (lane 0's copy is the stream's state)
            info[i] = rec;
            words.status = rec.status;
            words.ended = rec.ended;
            words.adler = rec.adler;
            words.n_tokens = rec.n_tokens;
            words.produced = (int)rec.produced;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __hip_atomic_store(&words.done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    } else {
        resolve_pre_stream(ring, comp, st, tokens, TokensFromPartner{&words}, out, status_out + i, lane);
    }
}


thread_local char g_error[256];

// both kernels as one launch, a pair of waves per stream (DEEPBINNER_INFLATE_PAIR=0: two launches)
bool pair_of_waves() {
    const char* v = std::getenv("DEEPBINNER_INFLATE_PAIR");
    return !(v && std::strcmp(v, "0") == 0);
}

int hip_failed(hipError_t e, const char* what) {
    std::snprintf(g_error, sizeof(g_error), "%s: %s", what, hipGetErrorString(e));
    return DBH_ERR_HIP;
}
#define DBI_HIP(call)                                          \
    do {                                                       \
        hipError_t e_ = (call);                                \
        if (e_ != hipSuccess) return hip_failed(e_, #call);    \
    } while (0)

}  // namespace dbh_inflate_detail

using namespace dbh_inflate_detail;

// dbh_vbz.hip: the streams of mode DBH_INFLATE_VBZ (the kernels above leave them alone), and the
// de-interleave of the shuffled ones (DBH_INFLATE_ZLIB_SHUFFLE, whose records of kernel 1 it reads:
// `ended` and `produced`; DBH_INFLATE_STORED_SHUFFLE)
hipError_t dbh_vbz_launch(const uint8_t* comp_dev, int64_t comp_bytes,
                          const dbh_inflate_stream* streams_dev, int n_streams,
                          int64_t total_out_bytes, uint8_t* out_dev, int32_t* status_dev,
                          uint8_t* work_dev, const char* produced0, const char* ended0,
                          int64_t record_stride, hipStream_t stream);
// dbh_zstd.hip: the zstd stage of the streams of mode DBH_INFLATE_VBZ_ZSTD, into their workspace
// slots; the content size of each into the `produced` word of its record
hipError_t dbh_zstd_launch(const uint8_t* comp_dev, int64_t comp_bytes,
                           const dbh_inflate_stream* streams_dev, int n_streams,
                           int64_t total_out_bytes, uint8_t* work_dev, int32_t* status_dev,
                           char* produced0, int64_t produced_stride, hipStream_t stream);

namespace dbh_inflate_detail {
// the two VBZ stages behind the inflate kernels, on the same queue
int vbz_stages(const uint8_t* comp_dev, int64_t comp_bytes, const dbh_inflate_stream* streams_dev, int n,
               int64_t total_out_bytes, uint8_t* out_dev, void* workspace_dev, StreamInfo* info,
               int32_t* status_dev, hipStream_t stream) {
    char* produced0 = reinterpret_cast<char*>(&info[0].produced);
    DBI_HIP(dbh_zstd_launch(comp_dev, comp_bytes, streams_dev, n, total_out_bytes,
                            (uint8_t*)workspace_dev, status_dev, produced0, (int64_t)sizeof(StreamInfo), stream));
    DBI_HIP(dbh_vbz_launch(comp_dev, comp_bytes, streams_dev, n, total_out_bytes, out_dev, status_dev,
                           (uint8_t*)workspace_dev, produced0, reinterpret_cast<const char*>(&info[0].ended),
                           (int64_t)sizeof(StreamInfo), stream));
    return DBH_OK;
}
}  // namespace dbh_inflate_detail

extern "C" {

const char* dbh_inflate_last_error(void) { return g_error; }

int dbh_inflate_workspace_bytes(int64_t total_out_bytes, int64_t n_streams, size_t* bytes) {
    if (!bytes || total_out_bytes < 0 || n_streams < 0) return DBH_ERR_INVALID_ARGUMENT;
    // one token slot per byte of output (a token yields at least one byte), then the per-stream
    // records of kernel 1
    *bytes = (size_t)total_out_bytes * sizeof(uint32_t) + 512 +
             (size_t)n_streams * sizeof(StreamInfo);
    return DBH_OK;
}

int dbh_inflate_dev(const uint8_t* comp_dev, int64_t comp_bytes,
                    const dbh_inflate_stream* streams_dev, int64_t n_streams,
                    int64_t total_out_bytes, uint8_t* out_dev, void* workspace_dev,
                    int32_t* status_dev, int streams_per_lane, dbh_stream stream) {
    if (n_streams < 0 || n_streams > 0x7FFFFFFF || total_out_bytes < 0 || comp_bytes < 0 ||
        streams_per_lane < 0)
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return DBH_OK;
    if (!comp_dev || !streams_dev || !out_dev || !workspace_dev || !status_dev)
        return DBH_ERR_INVALID_ARGUMENT;
    uint32_t* tokens = (uint32_t*)workspace_dev;
    char* behind = (char*)workspace_dev + dbh_host::align256((size_t)total_out_bytes * sizeof(uint32_t));
    StreamInfo* info = (StreamInfo*)(behind + 256);      // (the 256 bytes in front: unused, kept
    const int n = (int)n_streams;                        //  so that the records do not move)
    if (pair_of_waves()) {
        hipLaunchKernelGGL(inflate_pair_kernel, dim3((unsigned)n), dim3(128), 0, (hipStream_t)stream,
                           comp_dev, comp_bytes, streams_dev, n, tokens, info, out_dev, status_dev);
    } else {
        hipLaunchKernelGGL(inflate_tokens_wave_kernel, dim3((unsigned)n), dim3(dbi::kWaveLanes), 0,
                           (hipStream_t)stream, comp_dev, comp_bytes, streams_dev, n, tokens, info);
        DBI_HIP(hipGetLastError());
        hipLaunchKernelGGL(inflate_resolve_pre_kernel, dim3((unsigned)(n < 65536 ? n : 65536)), dim3(64), 0,
                           (hipStream_t)stream, comp_dev, comp_bytes, streams_dev, n, (const uint32_t*)tokens,
                           info, out_dev, status_dev);
    }
    DBI_HIP(hipGetLastError());
    return vbz_stages(comp_dev, comp_bytes, streams_dev, n, total_out_bytes, out_dev, workspace_dev, info,
                      status_dev, (hipStream_t)stream);
}

int dbh_inflate(const uint8_t* comp_host, size_t comp_bytes, const dbh_inflate_stream* streams_host,
                int64_t n_streams, uint8_t* out_host, size_t out_bytes, int32_t* status_host,
                int streams_per_lane, double* kernel_ms) {
    if (n_streams < 0 || streams_per_lane < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_streams == 0) return DBH_OK;
    if (!comp_host || !streams_host || !out_host || !status_host) return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_streams; ++i) {
        const dbh_inflate_stream& s = streams_host[i];
        if (s.comp_offset < 0 || s.comp_bytes < 0 || s.out_offset < 0 || s.out_bytes < 0 ||
            (size_t)(s.comp_offset + s.comp_bytes) > comp_bytes ||
            (size_t)(s.out_offset + s.out_bytes) > out_bytes)
            return DBH_ERR_INVALID_ARGUMENT;
    }
    dbh_owned::DeviceBlock d_comp, d_out, d_streams, d_work, d_status;      // (freed on return)
    dbh_owned::Event e0, e1;
    size_t work = 0;
    int st = dbh_inflate_workspace_bytes((int64_t)out_bytes, n_streams, &work);
    hipError_t e = d_comp.reserve(comp_bytes + 64);        // (padded: see the header)
    if (e == hipSuccess) e = hipMemset(d_comp.as<uint8_t>(comp_bytes), 0, 64);
    if (e == hipSuccess) e = d_out.reserve(out_bytes ? out_bytes : 1);
    if (e == hipSuccess) e = d_streams.reserve((size_t)n_streams * sizeof(dbh_inflate_stream));
    if (e == hipSuccess) e = d_work.reserve(work);
    if (e == hipSuccess) e = d_status.reserve((size_t)n_streams * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(d_comp.get(), comp_host, comp_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(d_streams.get(), streams_host, (size_t)n_streams * sizeof(dbh_inflate_stream),
                      hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&e0.h);
    if (e == hipSuccess) e = hipEventCreate(&e1.h);
    if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
    if (e == hipSuccess && st == DBH_OK)
        st = dbh_inflate_dev(d_comp.as<uint8_t>(), (int64_t)comp_bytes,
                             d_streams.as<dbh_inflate_stream>(), n_streams, (int64_t)out_bytes,
                             d_out.as<uint8_t>(), d_work.get(), d_status.as<int32_t>(),
                             streams_per_lane, nullptr);
    if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out_host, d_out.get(), out_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpy(status_host, d_status.get(), (size_t)n_streams * sizeof(int32_t),
                      hipMemcpyDeviceToHost);
    if (e == hipSuccess && kernel_ms) {
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, e0, e1);
        *kernel_ms = ms;
    }
    if (e != hipSuccess) return hip_failed(e, "dbh_inflate");
    return st;
}

}  // extern "C"
