// dbh_wave.h — the scans and sums over a wave and over a workgroup that the decoders (dbh_inflate,
// dbh_vbz, dbh_zstd) and the training-data kernels (dbh_text, dbh_format, dbh_random, dbh_feed) share:
// a new kernel takes its scan from here.  Device functions only, as dbh_seam.h, and nothing for the
// host compiler: a file that is also compiled as plain C++ includes it behind __HIPCC__.  The
// forward, seam, general and DTW kernels keep reductions shaped to them.
#pragma once

#include <hip/hip_runtime.h>

namespace dbh_wave {

// Inclusive prefix sum over the wave's 64 lanes on the DPP network (no LDS round trips): within
// rows of 16 lanes by shifts, then each row's total handed on to the rows behind it.
// PRECONDITION, for every caller: all 64 lanes are active at the call (a lane that is off hands on
// nothing), so call it from wave-uniform control flow only.  Sums wrap modulo 2^32.
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T v) {
    static_assert(sizeof(T) == 4, "int or unsigned");
    v += (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);      // row_shr:1
    v += (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);      // row_shr:2
    v += (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);      // row_shr:4
    v += (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);      // row_shr:8
    v += (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);      // row_bcast:15 -> rows 1, 3
    v += (T)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);      // row_bcast:31 -> rows 2, 3
    return v;
}

// the same by shuffles: parse_lines of dbh_text.hip alone, whose compiled code is held to this form
__device__ __forceinline__ int wave_scan_inclusive_shfl(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int below = __shfl_up(v, d);
        if (lane >= d) v += below;
    }
    return v;
}

// a 32-bit value of the lane before (lane 0: its own)
template <typename T>
__device__ __forceinline__ T from_lane_before(T v) { return (T)__shfl_up((int)v, 1); }

// the sum over the wave's 64 lanes, in every lane: the butterfly (32-bit or 64-bit integers)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the highest value over the wave's 64 lanes and the lowest index that holds it, in every lane: the
// butterfly over (value, index) pairs.  The order is total - higher value, then lower index - so the
// result does not depend on which lane held what; a NaN wins no comparison (hand none in as a pick).
// All 64 lanes call it.
__device__ __forceinline__ void wave_best(float* value, int* index) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(*value, o);
        const int oi = __shfl_xor(*index, o);
        if (ov > *value || (ov == *value && oi < *index)) {
            *value = ov;
            *index = oi;
        }
    }
}

// This thread's exclusive prefix of `count` within its workgroup of kWaves waves, all of whose
// threads call it, and the workgroup's sum in *total.  wave_total: kWaves words of LDS, the
// caller's; one barrier here, between their writes and their reads - a caller that comes again (a
// loop) puts one of its own between this call's reads and the next call's writes.
template <int kWaves>
__device__ __forceinline__ int block_prefix(int count, int* wave_total, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_scan_inclusive(count);
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        before += k < wave ? wave_total[k] : 0;
        all += wave_total[k];
    }
    *total = all;
    return before + incl - count;
}

// inclusive prefix sum over the workgroup's kThreads threads, all of which call it, once
// (Hillis-Steele in LDS: part holds kThreads values, the caller's)
template <typename T, int kThreads>
__device__ __forceinline__ T block_scan_inclusive(T v, T* part) {
    const int t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const T below = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += below;
        __syncthreads();
    }
    return part[t];
}

// One trip of a prefix over values handed out kThreads at a time (the scan's window and event
// offsets, the live sessions' window list): this thread's exclusive prefix, the carry moved on by
// the trip's total.  All threads call it; `part` is free again on return.
template <int kThreads>
__device__ __forceinline__ long long prefix_trip(long long v, long long* part, long long* carry) {
    const long long incl = block_scan_inclusive<long long, kThreads>(v, part);
    const long long before = *carry + incl - v;
    *carry += part[kThreads - 1];
    __syncthreads();
    return before;
}

}  // namespace dbh_wave
