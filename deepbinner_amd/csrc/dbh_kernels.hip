// dbh_kernels.hip — the device unit of the persistent path: the shipping build of the forward kernel
// and the three small seam kernels, with one host function each that launches it (dbh_kernels.h).
// The cycle-stamp build of the forward kernel is a unit of its own, dbh_timeline.hip.  The host code
// that prepares the launches is dbh_api.hip and dbh_probes.h.
//
// A kernel's instruction stream does not depend on which kernels share its unit, or on their
// order: every __device__ function these kernels call is __forceinline__, and cut at its ELF symbol's
// size dbh::dbh_forward_kernel is the same 15,365 instructions here, built alone, beside the
// timeline build or beside any other kernel (dbh_timeline::dbh_forward_kernel: 16,061 wherever it
// is built; DESIGN.md section 4, profiles/kernel_digest/).  After any rearrangement of the device
// code, check with  python tools/code_object.py --same OLD.so NEW.so
#include <hip/hip_runtime.h>

#include "../../include/deepbinner_hip.h"
#include "dbh_combine.h"
#include "dbh_kernels.h"
#define DBH_FORWARD_NS dbh
#define DBH_TIMELINE 0
#include "dbh_forward.hip"

// =============================================================================================
// Seam b2 as kernels of their own (the forward kernel does both itself when it is handed samples):
// on the arithmetic of dbh_seam.h, like it.
// =============================================================================================
namespace dbh {

// One block per (read, step): slice the window (classify.py:337-349), z-normalise it in fp64
// (trim_signal.py:61-69; the sums are exact integers), zero-pad right ('start') or left ('end')
// (classify.py:352-357) and emit fp32, which is what Keras casts the float64 input to.
__global__ __launch_bounds__(256) void dbh_normalise_kernel(
    const int16_t* __restrict__ samples, const long long* __restrict__ offsets, int steps,
    int side, float* __restrict__ windows) {
    __shared__ long long red[2][4];
    const long long read = blockIdx.x / steps;
    const int step = blockIdx.x - (int)(read * steps);
    const long long base = offsets[read];
    const long long len = offsets[read + 1] - base;
    long long a, b;
    window_bounds(len, step, side, kWindow, &a, &b);
    const int cnt = (int)(b - a);
    const int tid = threadIdx.x;
    const int16_t* src = samples + base + a;

    int v[4];
    long long s1 = 0, s2 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = tid + i * 256;
        v[i] = (k < cnt) ? (int)src[k] : 0;
        s1 += v[i];
        s2 += (long long)v[i] * v[i];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = s1;
        red[1][tid >> 6] = s2;
    }
    __syncthreads();
    s1 = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    s2 = red[1][0] + red[1][1] + red[1][2] + red[1][3];

    float* out = windows + (long long)blockIdx.x * kWindow;
    double mean, inv;
    mean_std(s1, s2, cnt, &mean, &inv);
    const int pad_left = (side == 0) ? 0 : kWindow - cnt;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = tid + i * 256;          // position in the source slice
        if (k < cnt) out[pad_left + k] = (float)(((double)v[i] - mean) * inv);
    }
    // zero padding: [cnt, 1024) for 'start', [0, 1024-cnt) for 'end'
    const int pad_begin = (side == 0) ? cnt : 0;
    const int pad_count = kWindow - cnt;
    for (int k = tid; k < pad_count; k += 256) out[pad_begin + k] = 0.f;
}

// 32 lanes per read: merge the per-step softmax vectors (classify.py:368-374: min for class 0,
// max for the barcodes), rescale the barcodes so the vector sums to one (classify.py:387-393,
// in fp64 like NumPy-1.x scalar promotion did) and make the call (classify.py:285-295).
__global__ __launch_bounds__(256) void dbh_merge_kernel(const float* __restrict__ wprobs,
                                                        long long n_reads, int steps,
                                                        int n_classes, double score_diff,
                                                        float* __restrict__ probs,
                                                        int* __restrict__ calls) {
    const long long read = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int c = threadIdx.x & 31;
    if (read >= n_reads) return;   // whole 32-lane groups exit together
    const bool valid = c < n_classes;
    float merged = 0.f;
    if (valid) {
        const float* src = wprobs + read * steps * n_classes + c;
        merged = src[0];
        for (int s = 1; s < steps; ++s) {
            const float v = src[(long long)s * n_classes];
            merged = (c == 0) ? fminf(merged, v) : fmaxf(merged, v);
        }
    }
    renormalise_and_call(merged, c, n_classes, score_diff, probs + read * n_classes,
                         calls + read);
}

}  // namespace dbh

extern "C" {      // (the kernel's symbol is unmangled)
namespace {
// classify.py:298-322 on call numbers (0 = 'none'), the rule of dbh_combine.h; one read per thread,
// 12 bytes of traffic each
__global__ void combine_calls_kernel(const int32_t* __restrict__ start_calls,
                                     const int32_t* __restrict__ end_calls, long long n, int mode,
                                     int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = dbh::combine_calls(start_calls[i], end_calls[i], mode);     // (dbh_combine.h)
}
}  // namespace
}  // extern "C"

// =============================================================================================
// The launches (dbh_kernels.h)
// =============================================================================================
namespace dbh_kernels {

hipError_t launch_forward(const dbh::ForwardArgs& a, unsigned grid, hipStream_t stream) {
    hipLaunchKernelGGL(dbh::dbh_forward_kernel, dim3(grid), dim3(dbh::kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t forward_attributes(hipFuncAttributes* attr) {
    return hipFuncGetAttributes(attr, (const void*)dbh::dbh_forward_kernel);
}

hipError_t launch_normalise(const int16_t* samples, const long long* offsets, int steps, int side,
                            float* windows_out, unsigned windows, hipStream_t stream) {
    hipLaunchKernelGGL(dbh::dbh_normalise_kernel, dim3(windows), dim3(256), 0, stream, samples,
                       offsets, steps, side, windows_out);
    return hipGetLastError();
}

hipError_t launch_merge(const float* wprobs, long long n_reads, int steps, int n_classes,
                        double score_diff, float* probs, int* calls, hipStream_t stream) {
    hipLaunchKernelGGL(dbh::dbh_merge_kernel, dim3((unsigned)((n_reads + 7) / 8)), dim3(256), 0,
                       stream, wprobs, n_reads, steps, n_classes, score_diff, probs, calls);
    return hipGetLastError();
}

hipError_t launch_combine(const int32_t* start_calls, const int32_t* end_calls, long long n, int mode,
                          int32_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(combine_calls_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       start_calls, end_calls, n, mode, out);
    return hipGetLastError();
}

}  // namespace dbh_kernels
