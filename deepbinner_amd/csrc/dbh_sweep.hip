// dbh_sweep.hip — the device unit of the sweep (dbh_sweep.h; include/deepbinner_hip.h, "sweep"):
// the calls of every scan size and every threshold out of ONE window pass at the largest scan size.
//
// Window s of a read is the same samples whatever the scan size (dbh_seam.h: window_bounds), and the
// merge over windows is a running min (class 0) / max (barcodes), so the merged vector after k
// windows is what a run at scan_size = k * L/2 merges.  The fold kernels walk the windows once and
// finish every prefix as the merge kernels finish the last: make_sum_to_one in fp64
// (classify.py:387-393), best class with ties to the lower index and the runner-up
// (classify.py:285-295).  What they keep per prefix is (best, best - second), from which the call at
// ANY threshold t is  best != 0 && margin >= t ? best : 0.
//
// Two forms, because the two merges sum the barcodes in different orders and a sweep has to agree
// with them to the bit:
//   fold32_kernel    32 lanes per read, the reductions of dbh_seam.h (reduce32: DPP inside the rows,
//                    v_permlane16_swap across them) in renormalise_and_call's order
//   fold256_kernel   one workgroup per read, the halving trees in LDS that dbh_general.hip's
//                    merge_kernel runs: both call dbh_trees.h's, one text
// The step itself - one window merged in, the prefix finished - is dbh_fold.h's, which the live
// sessions' resumable fold (dbh_live.hip) calls as well.
// One guard the merges do not have: a read whose barcodes are all zero (rest == 0) keeps them zero
// instead of 0 * (x / 0); class 0 is then the best class here as it is there, so no call changes, and
// the margin is a number.
//
// tally_kernel counts the outcomes: integers only, so the result depends on neither the launch shape
// nor on how the reads were split into calls.  early_kernel counts, from the same start track, what a
// live session would have decided early at every min_windows and threshold (dbh_early_core.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/deepbinner_hip.h"
#include "dbh_early_core.h"
#include "dbh_fold.h"
#include "dbh_sweep.h"

namespace dbh_sweep {
namespace {

constexpr int kThreads = 256;

// ---- 32 lanes per read (persistent models, C <= 32) ---------------------------------------------
// dbh_merge_kernel's shape: eight reads per workgroup, lane c = class c, whole 32-lane groups exit
// together; every reduction runs in control flow that is uniform over the group.
__global__ __launch_bounds__(kThreads) void fold32_kernel(const float* __restrict__ wprobs,
                                                          long long n_reads, int steps,
                                                          int n_classes, int* __restrict__ best,
                                                          double* __restrict__ margin) {
    using namespace dbh;
    const long long read = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int c = threadIdx.x & 31;
    if (read >= n_reads) return;
    const bool valid = c < n_classes;
    const float* src = wprobs + read * steps * n_classes + c;      // (read only where valid)
    float merged = 0.f;
    for (int s = 0; s < steps; ++s) {
        if (valid) merged = fold_merge(merged, src[(long long)s * n_classes], s == 0, c);
        int top;
        double lead;
        fold32_step(merged, valid, c, &top, &lead);                // (dbh_fold.h)
        if (c == 0) {
            best[read * steps + s] = top;
            margin[read * steps + s] = lead;
        }
    }
}

// ---- one workgroup per read (general models, C <= 256) ------------------------------------------
// dbh_trees.h's three halving trees, the very ones merge_kernel finishes a read with.
__global__ __launch_bounds__(kThreads) void fold256_kernel(const float* __restrict__ wprobs,
                                                           int steps, int C,
                                                           int* __restrict__ best,
                                                           double* __restrict__ margin) {
    __shared__ double rv[kThreads];
    __shared__ int ri[kThreads];
    __shared__ double first;
    const long long read = blockIdx.x;
    const int c = threadIdx.x;
    const bool valid = c < C;
    const float* src = wprobs + read * steps * C + c;              // (read only where valid)
    float merged = 0.f;
    for (int s = 0; s < steps; ++s) {
        if (valid) merged = dbh::fold_merge(merged, src[(long long)s * C], s == 0, c);
        int top;
        double lead;
        dbh::fold256_step<kThreads>(merged, valid, c, rv, ri, &first, &top, &lead);   // (dbh_fold.h)
        if (c == 0) {
            best[read * steps + s] = top;
            margin[read * steps + s] = lead;
        }
    }
}

// ---- the tally ----------------------------------------------------------------------------------
// Workgroup b = (chunk of 256 reads b / steps, prefix k = b % steps), one read per thread, which
// keeps its (best, margin) of both sides and its label in registers.  For every (threshold, mode) in
// turn the workgroup counts its reads in LDS and adds what is not zero to the caller's counts: a few
// global atomics per workgroup and cell, not one per read.  A `best` outside [0, C) is counted in
// no class.
__global__ __launch_bounds__(kThreads) void tally_kernel(
    const int* __restrict__ start_best, const double* __restrict__ start_margin,
    const int* __restrict__ end_best, const double* __restrict__ end_margin,
    const int* __restrict__ labels, long long n_reads, int steps, int C,
    const double* __restrict__ thresholds, int n_thresholds, unsigned long long* __restrict__ counts) {
    __shared__ unsigned hist[kMaxClasses + 3];
    const unsigned chunk = blockIdx.x / (unsigned)steps;
    const int k = (int)(blockIdx.x - chunk * (unsigned)steps);
    const int tid = threadIdx.x;
    const long long read = (long long)chunk * kThreads + tid;
    const bool live = read < n_reads;
    const bool both = start_best != nullptr && end_best != nullptr;
    const int modes = both ? 3 : 1;
    const int width = C + 3;
    int sb = 0, eb = 0, label = -1;
    double sm = 0.0, em = 0.0;
    if (live) {
        const long long at = read * steps + k;
        if (start_best) {
            sb = start_best[at];
            sm = start_margin[at];
        }
        if (end_best) {
            eb = end_best[at];
            em = end_margin[at];
        }
        if (labels) label = labels[read];
    }
    for (int t = 0; t < n_thresholds; ++t) {
        const double threshold = thresholds[t];
        const int s = (sb != 0 && sm >= threshold) ? sb : 0;
        const int e = (eb != 0 && em >= threshold) ? eb : 0;
        for (int mode = 0; mode < modes; ++mode) {
            for (int i = tid; i < width; i += kThreads) hist[i] = 0;
            __syncthreads();
            if (live) {
                int call;                       // combine_calls_kernel's rule (classify.py:298-322)
                if (!both) call = start_best ? s : e;
                else if (s == e) call = s;
                else if (mode == DBH_REQUIRE_BOTH) call = DBH_CALL_NONE;
                else if (e == DBH_CALL_NONE) call = s;
                else if (mode == DBH_REQUIRE_START) call = DBH_CALL_NONE;
                else call = (s == DBH_CALL_NONE) ? e : DBH_CALL_NONE;
                if ((unsigned)call < (unsigned)C) atomicAdd(&hist[call], 1u);
                if (label >= 0) atomicAdd(&hist[call == label ? C : (call != 0 ? C + 1 : C + 2)], 1u);
            }
            __syncthreads();
            unsigned long long* cell =
                counts + (((long long)k * n_thresholds + t) * modes + mode) * width;
            for (int i = tid; i < width; i += kThreads)
                if (hist[i]) atomicAdd(&cell[i], (unsigned long long)hist[i]);
            __syncthreads();
        }
    }
}

// ---- the early tally ----------------------------------------------------------------------------
// One workgroup per chunk of 256 reads, one read per thread, which keeps its label, length and end
// call in registers and walks its row of the start track.  Per threshold ONE pass over k from
// steps - 1 down to 0 keeps the first crossing at or behind k (dbh_early_core.h: step), which is the
// decision of min_windows = k + 1: the workgroup counts that cell in LDS - the calls, the eight
// columns (64-bit from the first add), the first kTile bins of the window and push histograms - and
// adds what is not zero to the caller's arrays; bins from kTile on follow tile by tile.  Every loop
// runs to a count the host passed, in control flow that is uniform over the workgroup.
constexpr int kTile = kThreads;         // histogram bins held in LDS at a time: one per thread

struct EarlySink {
    unsigned *calls_, *windows_, *pushes_;
    unsigned long long* early_;
    int width, pushes_end;
    __device__ void calls(int mode, int column) { atomicAdd(&calls_[mode * width + column], 1u); }
    __device__ void early(int column, long long value) {
        atomicAdd(&early_[column], (unsigned long long)value);
    }
    __device__ void window(int d) {
        if (d < kTile) atomicAdd(&windows_[d], 1u);
    }
    __device__ void push(long long r) {
        if (r < pushes_end) atomicAdd(&pushes_[r], 1u);
    }
};

// bins [base, base + kTile) of a histogram of `bins` bins: bin `mine` of every thread with `counts`
__device__ __forceinline__ void early_tile(unsigned* hist, bool counts, long long mine, int base,
                                           int bins, unsigned long long* out) {
    const int tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    if (counts && mine >= base && mine < (long long)base + kTile) atomicAdd(&hist[mine - base], 1u);
    __syncthreads();
    if (base + tid < bins && hist[tid]) atomicAdd(&out[base + tid], (unsigned long long)hist[tid]);
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void early_kernel(
    const int* __restrict__ start_best, const double* __restrict__ start_margin,
    const int* __restrict__ end_best, const double* __restrict__ end_margin,
    const int* __restrict__ labels, const long long* __restrict__ lengths, long long n_reads,
    int steps, int C, int input_size, long long chunk_samples,
    const double* __restrict__ thresholds, int n_thresholds, int P,
    unsigned long long* __restrict__ calls, unsigned long long* __restrict__ early,
    unsigned long long* __restrict__ windows, unsigned long long* __restrict__ pushes) {
    __shared__ unsigned h_calls[3 * (kMaxClasses + 3)];
    __shared__ unsigned h_windows[kTile], h_pushes[kTile];
    __shared__ unsigned long long h_early[dbh_early::kColumns];
    const int tid = threadIdx.x;
    const long long read = (long long)blockIdx.x * kThreads + tid;
    const bool live = read < n_reads;
    const bool both = end_best != nullptr, has_len = lengths != nullptr;
    const int modes = both ? 3 : 1, width = C + 3, n_calls = modes * width;
    const long long row = read * steps;
    int label = -1, eb = 0;
    double em = 0.0;
    long long len = 0;
    if (live) {
        if (labels) label = labels[read];
        if (both) {
            eb = end_best[row + steps - 1];
            em = end_margin[row + steps - 1];
        }
        if (has_len) len = lengths[read] > 0 ? lengths[read] : 0;      // (a negative length: 0)
    }
    EarlySink sink = {h_calls, h_windows, h_pushes, h_early, width, P < kTile ? P : kTile};
    for (int t = 0; t < n_thresholds; ++t) {
        const double threshold = thresholds[t];
        const int end_call = dbh_early::lead(eb, em, threshold) ? eb : 0;
        dbh_early::Crossing x = dbh_early::no_crossing();
        int final_call = 0;
        for (int k = steps - 1; k >= 0; --k) {
            if (live) dbh_early::step(&x, k, start_best[row + k], start_margin[row + k], threshold);
            if (k == steps - 1) final_call = x.call;
            for (int i = tid; i < n_calls; i += kThreads) h_calls[i] = 0;
            h_windows[tid] = 0;
            h_pushes[tid] = 0;
            if (tid < dbh_early::kColumns) h_early[tid] = 0;
            __syncthreads();
            if (live)
                dbh_early::count_read(sink, x, k, final_call, both, end_call, label, C, has_len, len,
                                      input_size, chunk_samples);
            __syncthreads();
            const long long cell = (long long)k * n_thresholds + t;
            unsigned long long* cell_windows = windows + cell * steps;
            unsigned long long* cell_pushes = has_len ? pushes + cell * P : nullptr;
            for (int i = tid; i < n_calls; i += kThreads)
                if (h_calls[i]) atomicAdd(&calls[cell * n_calls + i], (unsigned long long)h_calls[i]);
            if (tid < steps && h_windows[tid])
                atomicAdd(&cell_windows[tid], (unsigned long long)h_windows[tid]);
            if (has_len && tid < P && h_pushes[tid])
                atomicAdd(&cell_pushes[tid], (unsigned long long)h_pushes[tid]);
            if (tid < dbh_early::kColumns && h_early[tid])
                atomicAdd(&early[cell * dbh_early::kColumns + tid], h_early[tid]);
            __syncthreads();
            // the bins behind the first tile: windows from k's tile on (d >= k), every push tile
            const bool decided = live && x.d >= 0;
            for (int base = k / kTile * kTile < kTile ? kTile : k / kTile * kTile; base < steps;
                 base += kTile)
                early_tile(h_windows, decided, x.d, base, steps, cell_windows);
            if (has_len && P > kTile) {
                const long long r = decided ? dbh_early::push_of(x.d, input_size, len, chunk_samples) : 0;
                for (int base = kTile; base < P; base += kTile)
                    early_tile(h_pushes, decided, r - 1, base, P, cell_pushes);
            }
        }
    }
}

}  // namespace

// =============================================================================================
// The launches (dbh_sweep.h)
// =============================================================================================
hipError_t fold32(const float* wprobs, int64_t n_reads, int steps, int n_classes, int32_t* best,
                  double* margin, hipStream_t stream) {
    constexpr int64_t kReads = (int64_t)1 << 28;           // per launch: 2^25 workgroups
    for (int64_t r0 = 0; r0 < n_reads; r0 += kReads) {
        const int64_t n = std::min<int64_t>(kReads, n_reads - r0);
        hipLaunchKernelGGL(fold32_kernel, dim3((unsigned)((n + 7) / 8)), dim3(kThreads), 0, stream,
                           wprobs + r0 * steps * n_classes, (long long)n, steps, n_classes,
                           (int*)(best + r0 * steps), margin + r0 * steps);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t fold256(const float* wprobs, int64_t n_reads, int steps, int n_classes, int32_t* best,
                   double* margin, hipStream_t stream) {
    constexpr int64_t kReads = (int64_t)1 << 30;           // one workgroup per read
    for (int64_t r0 = 0; r0 < n_reads; r0 += kReads) {
        const int64_t n = std::min<int64_t>(kReads, n_reads - r0);
        hipLaunchKernelGGL(fold256_kernel, dim3((unsigned)n), dim3(kThreads), 0, stream,
                           wprobs + r0 * steps * n_classes, steps, n_classes,
                           (int*)(best + r0 * steps), margin + r0 * steps);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t tally(const int32_t* start_best, const double* start_margin, const int32_t* end_best,
                 const double* end_margin, const int32_t* labels, int64_t n_reads, int steps,
                 int n_classes, const double* thresholds, int n_thresholds,
                 unsigned long long* counts, hipStream_t stream) {
    // at most 2^30 workgroups per launch: chunks of 256 reads x steps prefixes
    const int64_t chunks_per_launch = std::max<int64_t>(1, ((int64_t)1 << 30) / steps);
    const int64_t reads_per_launch = chunks_per_launch * kThreads;
    for (int64_t r0 = 0; r0 < n_reads; r0 += reads_per_launch) {
        const int64_t n = std::min<int64_t>(reads_per_launch, n_reads - r0);
        const int64_t chunks = (n + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(tally_kernel, dim3((unsigned)(chunks * steps)), dim3(kThreads), 0, stream,
                           start_best ? (const int*)(start_best + r0 * steps) : nullptr,
                           start_margin ? start_margin + r0 * steps : nullptr,
                           end_best ? (const int*)(end_best + r0 * steps) : nullptr,
                           end_margin ? end_margin + r0 * steps : nullptr,
                           labels ? (const int*)(labels + r0) : nullptr, (long long)n, steps,
                           n_classes, thresholds, n_thresholds, counts);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t early_tally(const int32_t* start_best, const double* start_margin,
                       const int32_t* end_best, const double* end_margin, const int32_t* labels,
                       const int64_t* lengths, int64_t n_reads, int steps, int n_classes,
                       int input_size, int64_t chunk_samples, const double* thresholds,
                       int n_thresholds, int n_pushes, unsigned long long* calls,
                       unsigned long long* early, unsigned long long* windows,
                       unsigned long long* pushes, hipStream_t stream) {
    // at most 2^22 workgroups per launch: chunks of 256 reads
    constexpr int64_t reads_per_launch = ((int64_t)1 << 22) * kThreads;
    for (int64_t r0 = 0; r0 < n_reads; r0 += reads_per_launch) {
        const int64_t n = std::min<int64_t>(reads_per_launch, n_reads - r0);
        const int64_t chunks = (n + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(early_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, stream,
                           (const int*)(start_best + r0 * steps), start_margin + r0 * steps,
                           end_best ? (const int*)(end_best + r0 * steps) : nullptr,
                           end_margin ? end_margin + r0 * steps : nullptr,
                           labels ? (const int*)(labels + r0) : nullptr,
                           lengths ? (const long long*)(lengths + r0) : nullptr, (long long)n, steps,
                           n_classes, input_size, (long long)chunk_samples, thresholds, n_thresholds,
                           n_pushes, calls, early, windows, pushes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dbh_sweep
