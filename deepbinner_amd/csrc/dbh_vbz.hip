// dbh_vbz.hip - the streamvbyte + zigzag + delta stage of ONT's VBZ filter (HDF5 filter 32020,
// version 0) ON THE GPU: streams of mode DBH_INFLATE_VBZ of dbh_inflate_dev (C ABI: the
// "compressed input" section of include/deepbinner_hip.h), launched in the same call as the
// inflate kernels, behind them on the same queue.  The loader's threads have undone the zstd stage
// (fast5_reader.cpp: f5_stream_open_raw, f5_load_batch_raw); a stream holds
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
// Self-checks as the host's (fast5_reader.cpp, vbz_unpack): an odd original_size, control bytes
// beyond the stream, data that would run past its end or that end before it: status != 0 and
// the stream's output all zeros; its neighbours are not touched.  Reads stay inside the stream's
// bytes plus the 3 bytes a 4-byte load of its last value may take beyond them (the compressed
// buffer is readable for 64 bytes beyond its end).  No LDS, no scalar stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/deepbinner_hip.h"

namespace dbh_vbz_detail {

constexpr int kWaves = 4;                  // streams per workgroup: one wave each
constexpr int kPerLane = 16;               // values per lane and step (4 control bytes)
constexpr int kStep = 64 * kPerLane;
constexpr int kRefused = 1;                // status of a stream that fails a self-check

// wave-wide inclusive prefix sum, modulo 2^32, on the DPP network (as dbh_inflate.hip's
// wave_scan_i32): within rows of 16 lanes by shifts, then each row's total to the rows behind it
__device__ __forceinline__ unsigned scan_u32(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);   // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);   // row_bcast:15
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);   // row_bcast:31
    return v;
}

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
            const uint32_t incl = scan_u32(span);
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
            const uint32_t incl2 = scan_u32(sum);
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

__global__ __launch_bounds__(64 * kWaves) void vbz_decode_kernel(
    const uint8_t* __restrict__ comp, int64_t comp_total,
    const dbh_inflate_stream* __restrict__ streams, int n_streams, int64_t total_out,
    uint8_t* __restrict__ out, int32_t* status_out, const uint8_t* work, const char* produced0,
    int64_t produced_stride) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = blockIdx.x * kWaves + wave; i < n_streams; i += gridDim.x * kWaves) {
        const dbh_inflate_stream s = streams[i];
        if (s.mode == DBH_INFLATE_VBZ_ZSTD) {
            // (a stream with no room in the workspace was refused by the zstd kernel: nothing is read)
            const int64_t have = *reinterpret_cast<const int64_t*>(produced0 + (int64_t)i * produced_stride);
            const bool placed = s.out_offset >= 0 && s.out_bytes >= 0 && s.out_offset <= total_out - s.out_bytes;
            vbz_stream(comp, comp_total, s, total_out, out, status_out + i, lane,
                       work + (placed ? 4 * s.out_offset : 0), placed ? have : 0);
            continue;
        }
        if (s.mode != DBH_INFLATE_VBZ) continue;
        vbz_stream(comp, comp_total, s, total_out, out, status_out + i, lane);
    }
}

}  // namespace dbh_vbz_detail

// (dbh_inflate.hip's dbh_inflate_dev launches it; not part of the C ABI)
__attribute__((visibility("hidden"))) hipError_t dbh_vbz_launch(
    const uint8_t* comp_dev, int64_t comp_bytes, const dbh_inflate_stream* streams_dev,
    int n_streams, int64_t total_out_bytes, uint8_t* out_dev, int32_t* status_dev,
    const uint8_t* work_dev, const char* produced0, int64_t produced_stride, hipStream_t stream) {
    using namespace dbh_vbz_detail;
    const int blocks = (n_streams + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(vbz_decode_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)),
                       dim3(64 * kWaves), 0, stream, comp_dev, comp_bytes, streams_dev, n_streams,
                       total_out_bytes, out_dev, status_dev, work_dev, produced0, produced_stride);
    return hipGetLastError();
}
