// dbh_occlude.hip — the device unit of `locate --occlude` (dbh_occlude.h; include/deepbinner_hip.h,
// "occlude"): from a side's locations to the windows of its three variants - the span blanked, all
// but the span blanked, a control stretch blanked - and from the variants' merged results to one
// record per read.  The rule is dbh_occlude_core.h's, the same lines for the threads here and for
// the CPU models below.
//
//   slice_kernel            one wave per window, four windows per workgroup: the general path's
//                           front without its convolution - dbh::window_bounds, the exact int64
//                           sums over the wave (dbh_wave::wave_sum), dbh::mean_std, the one fp64
//                           expression per value - so that a window handed to the layer chain as
//                           fp32 is the bits the chain slices for itself.
//   occlude_plan_kernel     one thread per read: location and length -> the three blank intervals,
//                           the invert and valid bits, the record's "no result" fields.
//   occlude_windows_kernel  one workgroup per read; its threads walk the steps * slots slots of the
//                           read's windows (dbo::blank_slot): a whole slot is one 16-byte load and
//                           three 16-byte stores, consecutive lanes on consecutive slots; the head
//                           and the tail of a row (L no multiple of 4) go position by position.
//   occlude_gather_kernel   one thread per read and variant: the unblanked call's class picked out
//                           of the variant's merged probabilities, and the variant's call.
//
// Every loop is bounded by steps * slots (or, in the slice, by L); no atomics, no LDS, nothing waits
// on another workgroup, and what is written for a read depends on that read alone.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dbh_occlude.h"
#include "dbh_occlude_core.h"
#include "dbh_seam.h"
#include "dbh_wave.h"

namespace dbh_occlude {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kPerLaunch = (int64_t)1 << 30;            // workgroups of one launch

__global__ __launch_bounds__(kThreads) void slice_kernel(
    const int16_t* __restrict__ samples, const long long* __restrict__ offsets, long long w0,
    long long n_windows, int steps, int L, int side, float* __restrict__ x) {
    const long long win = w0 + (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (win >= n_windows) return;                              // (whole waves)
    const long long read = win / steps;
    const int step = (int)(win - read * steps);
    const long long base = offsets[read];
    long long a, b;
    dbh::window_bounds(offsets[read + 1] - base, step, side, L, &a, &b);
    const int cnt = (int)(b - a);
    const int pad_left = side == DBH_SIDE_START ? 0 : L - cnt;
    const int16_t* src = samples + base + a;
    long long s1 = 0, s2 = 0;
    for (int k = lane; k < cnt; k += 64) {
        const long long v = src[k];
        s1 += v;
        s2 += v * v;
    }
    s1 = dbh_wave::wave_sum(s1);
    s2 = dbh_wave::wave_sum(s2);
    double mean, inv;
    dbh::mean_std(s1, s2, cnt, &mean, &inv);
    float* out = x + win * L;
    for (int i = lane; i < L; i += 64) {
        const int k = i - pad_left;
        out[i] = (k >= 0 && k < cnt) ? (float)(((double)src[k] - mean) * inv) : 0.f;
    }
}

__global__ __launch_bounds__(kThreads) void occlude_plan_kernel(
    const dbh_location* __restrict__ locations, const long long* __restrict__ offsets,
    long long n_reads, int steps, int L, int side, dbh_occlude_plan* __restrict__ plans,
    dbh_occlusion* __restrict__ occlusions) {
    const long long read = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (read >= n_reads) return;
    dbo::plan_read(locations[read], offsets[read + 1] - offsets[read], steps, L, side, plans + read,
                   occlusions + read);
}

__global__ __launch_bounds__(kThreads) void occlude_windows_kernel(
    const float* __restrict__ x, const long long* __restrict__ offsets,
    const dbh_occlude_plan* __restrict__ plans, long long read0, int steps, int L, int side,
    float* __restrict__ out0, float* __restrict__ out1, float* __restrict__ out2) {
    const long long read = read0 + blockIdx.x;
    const dbh_occlude_plan plan = plans[read];
    const long long n = offsets[read + 1] - offsets[read];
    const int slots = dbo::row_slots(L);
    const size_t first_row = (size_t)read * steps * L;
    for (int j = threadIdx.x; j < steps * slots; j += kThreads) {
        const int s = j / slots, k = j - s * slots;
        const size_t row = first_row + (size_t)s * L;
        float* const rows[dbo::kVariants] = {out0 + row, out1 + row, out2 + row};
        dbo::blank_slot(x + row, rows, plan, dbo::origin(n, s, L, side), n, L, k);
    }
}

__global__ __launch_bounds__(kThreads) void occlude_gather_kernel(
    const dbh_occlude_plan* __restrict__ plans, const float* __restrict__ probs,
    const float* __restrict__ vprobs, const int* __restrict__ vcalls, long long n_reads,
    long long stride, int C, dbh_occlusion* __restrict__ occlusions) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_reads * dbo::kVariants) return;
    const long long read = i / dbo::kVariants;
    const int v = (int)(i - read * dbo::kVariants);
    dbh_occlusion* o = occlusions + read;
    const int c = o->cls;                                      // (the plan's kernel wrote it)
    if (c <= 0 || c >= C) return;
    if (v == 0) o->p = probs[read * C + c];
    if (!((plans[read].valid >> v) & 1)) return;
    o->variant[v].call = vcalls[v * stride + read];
    o->variant[v].p = vprobs[(v * stride + read) * C + c];
}

}  // namespace

hipError_t slice(const int16_t* samples, const int64_t* offsets, int64_t n_reads, int steps, int L,
                 int side, float* x, hipStream_t stream) {
    const int64_t n_windows = n_reads * steps;
    for (int64_t w0 = 0; w0 < n_windows; w0 += 4 * kPerLaunch) {
        const int64_t n = std::min<int64_t>(4 * kPerLaunch, n_windows - w0);
        hipLaunchKernelGGL(slice_kernel, dim3((unsigned)((n + 3) / 4)), dim3(kThreads), 0, stream,
                           samples, (const long long*)offsets, (long long)w0, (long long)(w0 + n),
                           steps, L, side, x);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t plan(const dbh_location* locations, const int64_t* offsets, int64_t n_reads, int steps,
                int L, int side, dbh_occlude_plan* plans, dbh_occlusion* occlusions,
                hipStream_t stream) {
    for (int64_t r0 = 0; r0 < n_reads; r0 += kPerLaunch * kThreads) {
        const int64_t n = std::min<int64_t>(kPerLaunch * kThreads, n_reads - r0);
        hipLaunchKernelGGL(occlude_plan_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, stream, locations + r0,
                           (const long long*)(offsets + r0), (long long)n, steps, L, side,
                           plans + r0, occlusions + r0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t windows(const float* x, const int64_t* offsets, const dbh_occlude_plan* plans,
                   int64_t n_reads, int steps, int L, int side, float* const out[3],
                   hipStream_t stream) {
    for (int64_t r0 = 0; r0 < n_reads; r0 += kPerLaunch) {
        const int64_t n = std::min<int64_t>(kPerLaunch, n_reads - r0);
        // (the reads of a launch keep their numbers: every array is indexed from read 0)
        hipLaunchKernelGGL(occlude_windows_kernel, dim3((unsigned)n), dim3(kThreads), 0, stream, x,
                           (const long long*)offsets, plans, (long long)r0, steps, L, side, out[0],
                           out[1], out[2]);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t gather(const dbh_occlude_plan* plans, const float* probs, const float* vprobs,
                  const int32_t* vcalls, int64_t n_reads, int64_t stride, int n_classes,
                  dbh_occlusion* occlusions, hipStream_t stream) {
    const int64_t per_launch = kPerLaunch / dbo::kVariants * kThreads;      // reads
    for (int64_t r0 = 0; r0 < n_reads; r0 += per_launch) {
        const int64_t n = std::min<int64_t>(per_launch, n_reads - r0);
        hipLaunchKernelGGL(occlude_gather_kernel,
                           dim3((unsigned)((n * dbo::kVariants + kThreads - 1) / kThreads)),
                           dim3(kThreads), 0, stream, plans + r0, probs + r0 * n_classes,
                           vprobs + r0 * n_classes, (const int*)(vcalls + r0), (long long)n,
                           (long long)stride, n_classes, occlusions + r0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void plan_host(const dbh_location* locations, const int64_t* offsets, int64_t n_reads, int steps,
               int L, int side, dbh_occlude_plan* plans, dbh_occlusion* occlusions) {
    for (int64_t r = 0; r < n_reads; ++r)
        dbo::plan_read(locations[r], (long long)(offsets[r + 1] - offsets[r]), steps, L, side,
                       plans + r, occlusions + r);
}

void windows_host(const float* x, const int64_t* offsets, const dbh_occlude_plan* plans,
                  int64_t n_reads, int steps, int L, int side, float* const out[3]) {
    for (int64_t r = 0; r < n_reads; ++r) {
        const size_t first_row = (size_t)r * steps * L;
        float* const rows[dbo::kVariants] = {out[0] + first_row, out[1] + first_row,
                                             out[2] + first_row};
        dbo::blank_read(x + first_row, rows, plans[r], (long long)(offsets[r + 1] - offsets[r]),
                        steps, L, side);
    }
}

}  // namespace dbh_occlude
