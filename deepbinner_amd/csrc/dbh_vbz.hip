// dbh_vbz.hip - the streamvbyte + zigzag + delta stage of ONT's VBZ filter (HDF5 filter 32020,
// version 0) ON THE GPU: streams of mode DBH_INFLATE_VBZ of dbh_inflate_dev (C ABI: the
// "compressed input" section of include/deepbinner_hip.h), launched in the same call as the
// inflate kernels, behind them on the same queue.  The loader's threads have undone the zstd stage
// (f5_stream_open_raw, f5_load_batch_raw: vbz_host_stage in fast5_batch.h); a stream holds
//   u32 LE original_size | ceil(n/4) control bytes | data bytes        (n = original_size / 2)
// control byte j holds the 2-bit codes of values 4j..4j+3, low bits first; value k takes
// code + 1 little-endian bytes; u -> (u >> 1) ^ -(u & 1) -> running sum, truncated to int16.
//
// ONE WAVEFRONT PER STREAM, 64 lanes x 4 control bytes (16 values) per step:
//   - a lane's data bytes are 16 + the sum of its 2-bit codes (two popcounts, no table);
//   - a wave prefix sum of those (DPP, no LDS) gives every lane where its data start;
//   - the lane decodes its 16 values (their addresses are known before the first load, so the
//     loads go out together) and sums their deltas;
//   - a second wave prefix sum of the lane sums, on top of the carry of the steps before, gives
//     every sample.
// Self-checks as the host's (fast5_codecs.h, vbz_unpack): an odd original_size, control bytes
// beyond the stream, data that would run past its end or that end before it: status != 0 and
// the stream's output all zeros; its neighbours are not touched.  Reads stay inside the stream's
// bytes plus the 3 bytes a 4-byte load of its last value may take beyond them (the compressed
// buffer is readable for 64 bytes beyond its end).  No LDS, vector loads and stores only.
//
// Streams of mode DBH_INFLATE_SVB16 and DBH_INFLATE_SVB16_ZSTD - the rows of a POD5 signal table,
// whose code has 1-bit keys and 1- or 2-byte values (dbh_svb16_core.h) - are decoded by the same
// grid in the same shape (svb16_stream below); dbh_svb16_decode_host at the end of this file runs
// the same rules with loops for lanes.
//
// The same grid undoes HDF5's shuffle filter for the streams of mode DBH_INFLATE_ZLIB_SHUFFLE and
// DBH_INFLATE_STORED_SHUFFLE (shuffle_stream below): it visits every stream behind the inflate
// kernels anyway, and a launch of its own would be empty on every default route.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/deepbinner_hip.h"
#include "dbh_svb16_core.h"
#include "dbh_wave.h"

namespace dbh_vbz_detail {

constexpr int kWaves = 4;                  // streams per workgroup: one wave each
constexpr int kPerLane = 16;               // values per lane and step (4 control bytes)
constexpr int kStep = 64 * kPerLane;
constexpr int kRefused = 1;                // status of a stream that fails a self-check

using dbh_wave::wave_scan_inclusive;       // (of unsigned here: modulo 2^32)

__device__ __forceinline__ uint32_t load_u32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// `unpacked` (mode DBH_INFLATE_VBZ_ZSTD): the streamvbyte bytes lie there, unpacked_bytes of them,
// put there by dbh_zstd.hip's kernel, whose verdict is in *status_slot; the stream's bytes in comp
// then hold the original_size alone.  Null: they follow the original_size in comp.
__device__ __forceinline__ void vbz_stream(const uint8_t* __restrict__ comp, int64_t comp_total,
                                           const dbh_inflate_stream& s, int64_t total_out,
                                           uint8_t* __restrict__ out, int32_t* status_slot,
                                           int lane, const uint8_t* unpacked = nullptr,
                                           int64_t unpacked_bytes = 0) {
    // an output region outside the buffer is not written at all
    if (s.out_offset < 0 || s.out_bytes < 0 || (s.out_offset & 1) ||
        s.out_offset > total_out - s.out_bytes) {
        if (lane == 0) *status_slot = kRefused;
        return;
    }
    int16_t* const dst = reinterpret_cast<int16_t*>(out + s.out_offset);
    const int64_t out_n = s.out_bytes / 2;
    bool bad = s.comp_offset < 0 || s.comp_bytes < 4 || s.comp_offset > comp_total - s.comp_bytes;
    int64_t n = 0, written = 0;
    int refused = kRefused;
    if (unpacked && !bad) {
        const int before = *status_slot;                   // (every lane reads it before lane 0 writes)
        if (before != 0) {
            bad = true;
            refused = before;
        }
    }
    const int64_t payload = unpacked ? unpacked_bytes : s.comp_bytes - 4;
    if (!bad) {
        const uint8_t* const src = comp + s.comp_offset;
        const uint32_t size = load_u32(src);
        n = size / 2;
        const int64_t ctrl = (n + 3) / 4;
        bad = (size & 1) || ctrl > payload;
        const uint8_t* const cbase = unpacked ? unpacked : src + 4;
        const uint8_t* const dbase = cbase + ctrl;
        const int64_t data_len = payload - ctrl;
        const int64_t keep = n < out_n ? n : out_n;
        const bool aligned16 = (s.out_offset & 15) == 0;
        int64_t doff = 0;                          // data bytes of the steps before (uniform)
        uint32_t carry = 0;                        // the running sample behind them (uniform)
        for (int64_t v0 = 0; !bad && v0 < n; v0 += kStep) {
            const int64_t base = v0 + (int64_t)lane * kPerLane;
            const int64_t left = n - base;
            const int valid = left <= 0 ? 0 : left >= kPerLane ? kPerLane : (int)left;
            uint32_t w = 0;
            if (valid == kPerLane) {
                w = load_u32(cbase + base / 4);
            } else if (valid > 0) {
                for (int b = 0; b < (valid + 3) / 4; ++b) w |= (uint32_t)cbase[base / 4 + b] << (8 * b);
                w &= (1u << (2 * valid)) - 1u;     // (codes of values beyond n are not counted)
            }
            const uint32_t span = (uint32_t)valid + (uint32_t)__builtin_popcount(w & 0x55555555u) +
                                  2u * (uint32_t)__builtin_popcount(w & 0xAAAAAAAAu);
            const uint32_t incl = wave_scan_inclusive(span);
            const uint32_t step_bytes = __builtin_amdgcn_readlane(incl, 63);
            const int64_t my = doff + (int64_t)(incl - span);
            const bool overrun = my + (int64_t)span > data_len;
            // the 16 values: addresses first, then the loads, then the deltas
            uint32_t at[kPerLane];
            uint32_t pos = 0;
#pragma unroll
            for (int k = 0; k < kPerLane; ++k) {
                at[k] = pos;
                pos += ((w >> (2 * k)) & 3u) + 1u;
            }
            uint32_t run[kPerLane];
            uint32_t sum = 0;
            const uint8_t* const mine = dbase + my;
#pragma unroll
            for (int k = 0; k < kPerLane; ++k) {
                uint32_t u = 0;
                if (k < valid && !overrun) {
                    const uint32_t code = (w >> (2 * k)) & 3u;
                    u = load_u32(mine + at[k]);
                    u &= code == 3u ? 0xFFFFFFFFu : (1u << (8 * code + 8)) - 1u;
                }
                sum += k < valid ? (u >> 1) ^ (0u - (u & 1u)) : 0u;
                run[k] = sum;
            }
            const uint32_t incl2 = wave_scan_inclusive(sum);
            const uint32_t prefix = carry + incl2 - sum;
            carry += __builtin_amdgcn_readlane(incl2, 63);
            doff += step_bytes;
            if (__builtin_amdgcn_ballot_w64(overrun) != 0) {
                bad = true;
                break;
            }
            // int16 stores: a lane's 16 samples are 32 consecutive bytes
            if (aligned16 && base + kPerLane <= keep) {
                uint32_t packed[8];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    packed[k] = ((prefix + run[2 * k]) & 0xFFFFu) | ((prefix + run[2 * k + 1]) << 16);
                uint4* q = reinterpret_cast<uint4*>(dst + base);
                q[0] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
                q[1] = make_uint4(packed[4], packed[5], packed[6], packed[7]);
            } else {
#pragma unroll
                for (int k = 0; k < kPerLane; ++k)
                    if (base + k < keep) dst[base + k] = (int16_t)(uint16_t)(prefix + run[k]);
            }
        }
        if (!bad && doff != data_len) bad = true;  // data that end before the stream does
        written = bad ? 0 : keep;
    }
    // zero-extension (a chunk shorter than asked for), or all of it for a refused stream
    for (int64_t k = written + lane; k < out_n; k += 64) dst[k] = 0;
    if (lane == 0) *status_slot = bad ? refused : 0;
}

// ---- POD5's 16-bit streamvbyte code (DBH_INFLATE_SVB16, DBH_INFLATE_SVB16_ZSTD) ----
// The same shape as vbz_stream with the rules of dbh_svb16_core.h: 1-bit keys, two key bytes per
// lane and step, a lane's data 16 + popcount(keys) bytes, fetched as four 8-byte groups whose
// addresses the key bits give before the first load; sums modulo 2^32, cut to 16 bits at the store.
// Reads stay inside the stream's bytes plus the dbh_svb16::kReadBeyond (7) a group's fetch may
// take beyond its last value.  `unpacked`: as for vbz_stream (mode DBH_INFLATE_SVB16_ZSTD).
__device__ __forceinline__ uint64_t load_u64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

__device__ __forceinline__ void svb16_stream(const uint8_t* __restrict__ comp, int64_t comp_total,
                                             const dbh_inflate_stream& s, int64_t total_out,
                                             uint8_t* __restrict__ out, int32_t* status_slot,
                                             int lane, const uint8_t* unpacked = nullptr,
                                             int64_t unpacked_bytes = 0) {
    namespace sv = dbh_svb16;
    static_assert(sv::kPerLane == kPerLane && sv::kLanes == 64, "one lane, sixteen values");
    // an output region outside the buffer is not written at all
    if (s.out_offset < 0 || s.out_bytes < 0 || (s.out_offset & 1) ||
        s.out_offset > total_out - s.out_bytes) {
        if (lane == 0) *status_slot = sv::kRefused;
        return;
    }
    int16_t* const dst = reinterpret_cast<int16_t*>(out + s.out_offset);
    const int64_t out_n = s.out_bytes / 2;
    bool bad = s.comp_offset < 0 || s.comp_bytes < 4 || s.comp_offset > comp_total - s.comp_bytes;
    int64_t written = 0;
    int refused = sv::kRefused;
    if (unpacked && !bad) {
        const int before = *status_slot;                   // (every lane reads it before lane 0 writes)
        if (before != 0) {
            bad = true;
            refused = before;
        }
    }
    const int64_t payload = unpacked ? unpacked_bytes : s.comp_bytes - 4;
    if (!bad) {
        const uint8_t* const src = comp + s.comp_offset;
        const uint32_t size = load_u32(src);
        const int64_t n = size / 2;
        int64_t key_bytes = 0, data_len = 0;
        bad = !sv::prefix_ok(size) || !sv::shape(n, payload, &key_bytes, &data_len);
        const uint8_t* const kbase = unpacked ? unpacked : src + 4;
        const uint8_t* const dbase = kbase + key_bytes;
        const int64_t keep = n < out_n ? n : out_n;
        const bool aligned16 = (s.out_offset & 15) == 0;
        int64_t doff = 0;                          // data bytes of the steps before (uniform)
        uint32_t carry = 0;                        // the running sample behind them (uniform)
        for (int64_t v0 = 0; !bad && v0 < n; v0 += sv::kStep) {
            const int64_t base = v0 + (int64_t)lane * kPerLane;
            const int valid = sv::lane_valid(n, base);
            uint32_t kb = 0;
            if (sv::lane_key_bytes(valid) > 0) kb = kbase[base / 8];
            if (sv::lane_key_bytes(valid) > 1) kb |= (uint32_t)kbase[base / 8 + 1] << 8;
            const uint32_t keys = sv::lane_keys(kb, valid);
            const uint32_t span = sv::lane_span(keys, valid);
            const uint32_t incl = wave_scan_inclusive(span);
            const uint32_t step_bytes = __builtin_amdgcn_readlane(incl, 63);
            const int64_t my = doff + (int64_t)(incl - span);
            const bool overrun = my + (int64_t)span > data_len;
            // the four groups: addresses first, then the loads, then the values
            const uint8_t* const mine = dbase + my;
            uint64_t grp[sv::kGroups];
#pragma unroll
            for (int g = 0; g < sv::kGroups; ++g)
                grp[g] = sv::group_used(valid, g) && !overrun ? load_u64(mine + sv::group_start(keys, g)) : 0ull;
            uint32_t run[kPerLane];
            const uint32_t sum = sv::lane_decode(keys, valid, grp, run);
            const uint32_t incl2 = wave_scan_inclusive(sum);
            const uint32_t prefix = carry + incl2 - sum;
            carry += __builtin_amdgcn_readlane(incl2, 63);
            doff += step_bytes;
            if (__builtin_amdgcn_ballot_w64(overrun) != 0) {
                bad = true;
                break;
            }
            // int16 stores: a lane's 16 samples are 32 consecutive bytes
            if (aligned16 && base + kPerLane <= keep) {
                uint32_t packed[8];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    packed[k] = ((prefix + run[2 * k]) & 0xFFFFu) | ((prefix + run[2 * k + 1]) << 16);
                uint4* q = reinterpret_cast<uint4*>(dst + base);
                q[0] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
                q[1] = make_uint4(packed[4], packed[5], packed[6], packed[7]);
            } else {
#pragma unroll
                for (int k = 0; k < kPerLane; ++k)
                    if (base + k < keep) dst[base + k] = (int16_t)(uint16_t)(prefix + run[k]);
            }
        }
        if (!bad && doff != data_len) bad = true;  // data that end before the stream does
        written = bad ? 0 : keep;
    }
    // zero-extension (a row shorter than asked for), or all of it for a refused stream
    for (int64_t k = written + lane; k < out_n; k += 64) dst[k] = 0;
    if ((s.out_bytes & 1) && lane == 0) out[s.out_offset + s.out_bytes - 1] = 0;   // (half a sample: no data)
    if (lane == 0) *status_slot = bad ? refused : 0;
}

// ---- HDF5's shuffle filter for int16, undone (DBH_INFLATE_ZLIB_SHUFFLE, DBH_INFLATE_STORED_SHUFFLE) ----
// The N shuffled bytes are the N/2 low bytes of the samples, then their N/2 high bytes.  One wave
// per stream, as everything in this kernel.

// samples [i0, i1) from the two planes: lane by lane up to the first 16-byte boundary of dst, then
// every lane 8 bytes of each plane, interleaved, as one 16-byte store, then the tail lane by lane
__device__ __forceinline__ void unshuffle_i16(const uint8_t* lo, const uint8_t* hi, uint8_t* dst,
                                              int64_t n, int lane) {
    int64_t head = (int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / 2;
    if (head > n) head = n;
    const int64_t body = (n - head) / 8;
    for (int64_t i = lane; i < head; i += 64) {
        const uint16_t v = (uint16_t)(lo[i] | ((unsigned)hi[i] << 8));
        *reinterpret_cast<uint16_t*>(dst + 2 * i) = v;
    }
    for (int64_t b = lane; b < body; b += 64) {
        const int64_t i = head + 8 * b;
        uint64_t l, h;
        __builtin_memcpy(&l, lo + i, 8);
        __builtin_memcpy(&h, hi + i, 8);
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t l2 = (uint32_t)(l >> (16 * k)) & 0xFFFFu, h2 = (uint32_t)(h >> (16 * k)) & 0xFFFFu;
            w[k] = (l2 & 0xFFu) | ((h2 & 0xFFu) << 8) | ((l2 >> 8) << 16) | ((h2 >> 8) << 24);
        }
        *reinterpret_cast<uint4*>(dst + 2 * i) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int64_t i = head + 8 * body + lane; i < n; i += 64) {
        const uint16_t v = (uint16_t)(lo[i] | ((unsigned)hi[i] << 8));
        *reinterpret_cast<uint16_t*>(dst + 2 * i) = v;
    }
}

// `slots`: the stream's token slots in the workspace (4 * out_bytes bytes at 4 * out_offset), dead
// once the inflate kernels are done with the stream.  DBH_INFLATE_ZLIB_SHUFFLE: they have left the
// N shuffled bytes in the stream's output region, their verdict in *status_slot, and in `ended` /
// `produced` whether the deflate data ended, and with how many bytes.
__device__ __forceinline__ void shuffle_stream(const uint8_t* __restrict__ comp, int64_t comp_total,
                                               const dbh_inflate_stream& s, int64_t total_out,
                                               uint8_t* out, int32_t* status_slot, int lane,
                                               uint8_t* work, int ended, int64_t produced) {
    // an output region outside the buffer is not written at all
    if (s.out_offset < 0 || s.out_bytes < 0 || (s.out_offset & 1) ||
        s.out_offset > total_out - s.out_bytes) {
        if (lane == 0) *status_slot = DBH_INFLATE_SHUFFLE_REFUSED;
        return;
    }
    uint8_t* const dst = out + s.out_offset;
    int status = DBH_INFLATE_SHUFFLE_REFUSED;
    int64_t written = 0;                           // bytes of dst that hold samples
    if (s.comp_offset >= 0 && s.comp_bytes >= 4 && s.comp_offset <= comp_total - s.comp_bytes) {
        const uint8_t* const src = comp + s.comp_offset;
        const int64_t n = (int64_t)load_u32(src);
        if (s.mode == DBH_INFLATE_STORED_SHUFFLE) {
            if (!(n & 1) && s.comp_bytes == 4 + n) {
                written = (n < s.out_bytes ? n : s.out_bytes) & ~(int64_t)1;
                unshuffle_i16(src + 4, src + 4 + n / 2, dst, written / 2, lane);
                status = 0;
            }
        } else if (!(n & 1) && n <= s.out_bytes) {
            const int before = *status_slot;       // (every lane reads it before lane 0 writes)
            if (before != 0) {
                status = before;                   // the zlib stage's own reason stays
            } else if (ended && produced == n) {
                // the region's bytes to the slots, coalesced; then back, de-interleaved
                uint8_t* const slots = work + 4 * s.out_offset;
                const int64_t whole = n & ~(int64_t)15;
                for (int64_t k = 16 * (int64_t)lane; k < whole; k += 1024) {
                    uint4 v;
                    __builtin_memcpy(&v, dst + k, 16);
                    __builtin_memcpy(slots + k, &v, 16);
                }
                for (int64_t k = whole + 2 * lane; k < n; k += 128)
                    *reinterpret_cast<uint16_t*>(slots + k) = *reinterpret_cast<const uint16_t*>(dst + k);
                // (the lanes of ONE wave: what they stored is what they load behind this - by the
                // order of accesses that go through one CU's L1, which is what a workgroup-scope
                // fence stands for in the default mode; a build with -mtgsplit, where the waves of
                // a workgroup may sit on different CUs, makes the fence do more, never less)
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                unshuffle_i16(slots, slots + n / 2, dst, n / 2, lane);
                written = n;
                status = 0;
            }
        }
    }
    // zero-extension, or all of it for a refused stream
    for (int64_t k = written + 2 * lane; k + 1 < s.out_bytes; k += 128)
        *reinterpret_cast<uint16_t*>(dst + k) = 0;
    if ((s.out_bytes & 1) && lane == 0) dst[s.out_bytes - 1] = 0;      // (half a sample: no data)
    if (lane == 0) *status_slot = status;
}

__global__ __launch_bounds__(64 * kWaves) void vbz_decode_kernel(
    const uint8_t* __restrict__ comp, int64_t comp_total,
    const dbh_inflate_stream* __restrict__ streams, int n_streams, int64_t total_out,
    uint8_t* out, int32_t* status_out, uint8_t* work, const char* produced0, const char* ended0,
    int64_t produced_stride) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = blockIdx.x * kWaves + wave; i < n_streams; i += gridDim.x * kWaves) {
        const dbh_inflate_stream s = streams[i];
        if (s.mode == DBH_INFLATE_VBZ_ZSTD || s.mode == DBH_INFLATE_SVB16_ZSTD) {
            // (a stream with no room in the workspace was refused by the zstd kernel: nothing is read)
            const int64_t have = *reinterpret_cast<const int64_t*>(produced0 + (int64_t)i * produced_stride);
            const bool placed = s.out_offset >= 0 && s.out_bytes >= 0 && s.out_offset <= total_out - s.out_bytes;
            if (s.mode == DBH_INFLATE_VBZ_ZSTD)
                vbz_stream(comp, comp_total, s, total_out, out, status_out + i, lane,
                           work + (placed ? 4 * s.out_offset : 0), placed ? have : 0);
            else
                svb16_stream(comp, comp_total, s, total_out, out, status_out + i, lane,
                             work + (placed ? 4 * s.out_offset : 0), placed ? have : 0);
            continue;
        }
        if (s.mode == DBH_INFLATE_SVB16) {
            svb16_stream(comp, comp_total, s, total_out, out, status_out + i, lane);
            continue;
        }
        if (s.mode == DBH_INFLATE_ZLIB_SHUFFLE || s.mode == DBH_INFLATE_STORED_SHUFFLE) {
            shuffle_stream(comp, comp_total, s, total_out, out, status_out + i, lane, work,
                           *reinterpret_cast<const int32_t*>(ended0 + (int64_t)i * produced_stride),
                           *reinterpret_cast<const int64_t*>(produced0 + (int64_t)i * produced_stride));
            continue;
        }
        if (s.mode != DBH_INFLATE_VBZ) continue;
        vbz_stream(comp, comp_total, s, total_out, out, status_out + i, lane);
    }
}

}  // namespace dbh_vbz_detail

extern "C" {
/* the GPU's svb16 decoder run on the host: same core, lanes as a loop (tests, tools) */
__attribute__((visibility("default"))) int dbh_svb16_decode_host(
    const uint8_t* stream, size_t stream_bytes, int64_t n, int16_t* out, int32_t* status) {
    if ((!stream && stream_bytes) || n < 0 || (!out && n) || !status) return 1;   // DBH_ERR_INVALID_ARGUMENT
    *status = dbh_svb16::decode_host(stream, (int64_t)stream_bytes, n, out);
    return 0;
}
}

// (dbh_inflate.hip's dbh_inflate_dev launches it; not part of the C ABI)
__attribute__((visibility("hidden"))) hipError_t dbh_vbz_launch(
    const uint8_t* comp_dev, int64_t comp_bytes, const dbh_inflate_stream* streams_dev,
    int n_streams, int64_t total_out_bytes, uint8_t* out_dev, int32_t* status_dev,
    uint8_t* work_dev, const char* produced0, const char* ended0, int64_t produced_stride,
    hipStream_t stream) {
    using namespace dbh_vbz_detail;
    const int blocks = (n_streams + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(vbz_decode_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)),
                       dim3(64 * kWaves), 0, stream, comp_dev, comp_bytes, streams_dev, n_streams,
                       total_out_bytes, out_dev, status_dev, work_dev, produced0, ended0,
                       produced_stride);
    return hipGetLastError();
}
