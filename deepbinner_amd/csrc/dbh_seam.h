// dbh_seam.h — the arithmetic of the two seams around the network, in ONE place for every kernel
// that needs it: in front, which samples of a read make a window (classify.py:337-349) and the
// constants of its z-normalisation (trim_signal.py:61-69); behind, make_sum_to_one and the barcode
// call of one read (classify.py:387-393, 285-295).  Used by the persistent forward kernel
// (dbh_forward.hip), the stand-alone normalise and merge kernels (dbh_kernels.hip) and the general
// path's front kernel (dbh_general.hip).  Device functions only: a kernel defined here would land in
// every translation unit that includes this file.
#ifndef DBH_SEAM_H
#define DBH_SEAM_H
#include <hip/hip_runtime.h>

namespace dbh {

// ---------------------------------------------------------------------------------------------
// make_sum_to_one + barcode call for one read held by a 32-lane group (lane c = class c):
// classify.py:387-393 in fp64 (what NumPy-1.x scalar promotion gave the reference) and
// classify.py:285-295 (ties to the lower class index: Python's stable sort with reverse=True).
// Shared by the stand-alone merge kernel and the forward kernel's fused single-step finish.
// ---------------------------------------------------------------------------------------------
// 64-bit / index moves inside a 16-lane row (DPP, no LDS round trip) for the reductions below.
template <int CTRL>
__device__ __forceinline__ int dpp_move_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double dpp_move_f64(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)dpp_move_i32<CTRL>((int)b);
    const unsigned hi = (unsigned)dpp_move_i32<CTRL>((int)(b >> 32));
    return __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
}

// The 32 lanes c = 0..31 of one read (two 16-lane rows) finish it: make_sum_to_one in fp64
// (classify.py:387-393), then the top-two call rule (classify.py:285-295; ties to the lower
// index).  Each all-reduce is four DPP steps inside the rows plus one v_permlane16_swap across
// them - five ds_bpermute rounds of 64-bit values apiece made this the slowest 3k cycles of a
// window.
template <class T, class Combine>
__device__ __forceinline__ T reduce32(T v, const Combine& combine) {
    v = combine(v, T::template moved<0xB1>(v));     // quad_perm [1,0,3,2]
    v = combine(v, T::template moved<0x4E>(v));     // quad_perm [2,3,0,1]
    v = combine(v, T::template moved<0x141>(v));    // row_half_mirror
    v = combine(v, T::template moved<0x140>(v));    // row_mirror
    T row0, row1;                                   // both rows' results, seen from both rows
    T::rows(v, &row0, &row1);
    return combine(row0, row1);
}
// v_permlane16_swap_b32 (gfx950): (x, x) -> {the even row's x in both rows of a pair, the odd
// row's x in both rows} - the cross-row step of a 32-lane reduction without an LDS round trip.
__device__ __forceinline__ void rows_i32(int x, int* even, int* odd) {
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
    *even = (int)r[0];
    *odd = (int)r[1];
}
__device__ __forceinline__ void rows_f64(double x, double* even, double* odd) {
    const long long b = __builtin_bit_cast(long long, x);
    int lo0, lo1, hi0, hi1;
    rows_i32((int)b, &lo0, &lo1);
    rows_i32((int)(b >> 32), &hi0, &hi1);
    *even = __builtin_bit_cast(double, (long long)(((unsigned long long)(unsigned)hi0 << 32) | (unsigned)lo0));
    *odd = __builtin_bit_cast(double, (long long)(((unsigned long long)(unsigned)hi1 << 32) | (unsigned)lo1));
}
struct RedF64 {
    double v;
    template <int CTRL>
    static __device__ __forceinline__ RedF64 moved(const RedF64& a) {
        return RedF64{dpp_move_f64<CTRL>(a.v)};
    }
    static __device__ __forceinline__ void rows(const RedF64& a, RedF64* even, RedF64* odd) {
        rows_f64(a.v, &even->v, &odd->v);
    }
};
struct RedBest {
    double v;
    int i;
    template <int CTRL>
    static __device__ __forceinline__ RedBest moved(const RedBest& a) {
        return RedBest{dpp_move_f64<CTRL>(a.v), dpp_move_i32<CTRL>(a.i)};
    }
    static __device__ __forceinline__ void rows(const RedBest& a, RedBest* even, RedBest* odd) {
        rows_f64(a.v, &even->v, &odd->v);
        rows_i32(a.i, &even->i, &odd->i);
    }
};

__device__ __forceinline__ void renormalise_and_call(float merged, int c, int n_classes,
                                                     double score_diff, float* probs_row,
                                                     int* call_out) {
    const bool valid = c < n_classes;
    double p = (double)merged;
    const double rest =
        reduce32(RedF64{(valid && c > 0) ? p : 0.0},
                 [](const RedF64& a, const RedF64& b) { return RedF64{a.v + b.v}; }).v;
    // (class 0 of this lane's half; the source lane made here: as a loop invariant its byte address
    // was kept in a register around the whole persistent loop - and spilled)
    int half_first;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(half_first));
    half_first = (half_first & 32) << 2;
    const long long p_bits = __builtin_bit_cast(long long, p);
    const unsigned p0_lo = (unsigned)__builtin_amdgcn_ds_bpermute(half_first, (int)(unsigned)p_bits);
    const unsigned p0_hi = (unsigned)__builtin_amdgcn_ds_bpermute(half_first, (int)(p_bits >> 32));
    const double p0 = __builtin_bit_cast(double, ((long long)p0_hi << 32) | (long long)p0_lo);
    const double factor = (1.0 - p0) / rest;
    if (c > 0) p = p * factor;
    if (valid) probs_row[c] = (float)p;

    const RedBest best = reduce32(RedBest{valid ? p : -1.0, c}, [](const RedBest& a, const RedBest& b) {
        return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
    });
    const double second =
        reduce32(RedF64{(valid && c != best.i) ? p : -1.0},
                 [](const RedF64& a, const RedF64& b) { return RedF64{fmax(a.v, b.v)}; }).v;
    if (c == 0) *call_out = (best.i != 0 && (best.v - second) >= score_diff) ? best.i : 0;
}

// Window w of a launch = (read w / steps, scan step w % steps).  Window indices fit 32 bits
// (n_windows is an int) and steps == 1 - whole reads, the classify path - needs no division at
// all; a 64-bit division is ~150 scalar instructions that every wave would run per window.
__device__ __forceinline__ void split_window(unsigned win, int steps, unsigned* read, int* step) {
    if (steps == 1) {
        *read = win;
        *step = 0;
    } else {
        *read = win / (unsigned)steps;
        *step = (int)(win - *read * (unsigned)steps);
    }
}

// Bounds of the window of `window` samples of scan step `step` inside a read of `len` samples
// (classify.py:337-349).
__device__ __forceinline__ void window_bounds(long long len, int step, int side, int window,
                                              long long* a, long long* b) {
    const long long sig_start = (long long)step * (window / 2);
    const long long sig_end = sig_start + window;
    if (side == 0) {
        *a = sig_start < len ? sig_start : len;
        *b = sig_end < len ? sig_end : len;
    } else {
        *a = len - sig_end > 0 ? len - sig_end : 0;
        *b = len - sig_start > 0 ? len - sig_start : 0;
    }
}

// z-normalisation constants from exact integer sums (trim_signal.py:61-69): x -> (x - mean) * inv
// with mean = sum(x)/n and inv = 1/std = n / sqrt(n*sum(x^2) - sum(x)^2), the radicand exact in
// int64; inv = 1 when std is 0 (the reference then only subtracts the mean).  Two fp64 divisions
// and one square root per window instead of a division per sample: fp64 division is ~20
// instructions at half rate, and stage A has nothing to hide them behind.  The product differs
// from the reference's quotient by at most one fp64 ulp before the cast to fp32 (the parity
// tests allow one fp32 ulp; every kernel that normalises shares this function, so they agree to
// the bit with each other).
__device__ __forceinline__ void mean_std(long long s1, long long s2, int cnt, double* mean,
                                         double* inv) {
    *mean = 0.0;
    *inv = 1.0;
    if (cnt > 0) {
        *mean = (double)s1 / (double)cnt;
        const long long num = (long long)cnt * s2 - s1 * s1;
        if (num > 0) *inv = (double)cnt / sqrt((double)num);
    }
}

}  // namespace dbh

#endif  // DBH_SEAM_H
