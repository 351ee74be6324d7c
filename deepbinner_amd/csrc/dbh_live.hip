// dbh_live.hip — the device unit of the live sessions (dbh_live.h; include/deepbinner_hip.h, "live"):
// per sequencer channel the signal received so far and the fold over the windows that are complete,
// kept on the device between pushes.
//
//   append_kernel    one workgroup per chunk: the channel's record and gate through
//                    dbh_live_core.h's append (reset on BEGIN, the clip at cap, the counters, the
//                    windows this push made ready), the kept samples into the channel's row - 16
//                    bytes per thread where source and row are aligned alike (the host stages them
//                    so), single int16 values at the edges and otherwise.  Its pair form also
//                    stores the chunk's tail into the channel's ring, two spans at the wrap, by
//                    the same copy, and makes the end fold's record fresh at END
//   list_kernel      the exclusive prefix of the new-window counts: one workgroup walks the chunks
//                    1,024 at a time, dbh_wave.h's block scan per trip and a carry
//   front_kernel     one wave per listed window: find its chunk by binary search, cut
//                    [min(k h, n), min(k h + L, n)) from the channel's row, the scan's front rule
//                    (dbh_front.h, the text dbh_scan.hip's windows_kernel runs)
//   fold32_kernel    the resumable fold, 32 lanes per chunk (persistent models), and
//   fold256_kernel   one workgroup per chunk (general models): load merged and the record, fold
//                    this round's windows of the channel in order by dbh_fold.h's step - the
//                    sweep's - write the track, decide by dbh_live_core.h's folded(), store
//   end_front_kernel one wave per end window of every chunk that carried END (pair sessions):
//                    its m samples out of the ring through the wrap, the same front rule, padded
//                    in front; the forward pass and the fold kernels above take it from there,
//                    on the end model and the end side's record, merged vector and track
//   results_kernel   the record of every chunk's channel, IDLE for an idle chunk; its pair form
//                    the end record beside it (dbh_live_core.h's end_record: combine_calls)
//   yield_kernel     sessions with a yield policy: one workgroup per class sums, over the push's
//                    chunks, the samples and reads of the records that ended with that call (int64,
//                    dbh_wave.h's sum) and adds them to the session's yields
//   action_kernel    the lowest level over the balanced classes by a reduction, then a thread per
//                    chunk: the action record by dbh_live_core.h's action_of and the channel's
//                    action, which BEGIN (the chunk's flags) makes NONE again
//
// The forward pass between front and fold is what dbh_predict_dev launches, in rounds; a round may
// end in the middle of a channel's windows, the fold takes up where the record says.  Every loop is
// bounded by a count the host passed in; nothing waits on another workgroup.  A channel appears once
// in a push, so no two workgroups of a kernel touch one channel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/deepbinner_hip.h"
#include "dbh_fold.h"
#include "dbh_front.h"
#include "dbh_live.h"
#include "dbh_wave.h"

namespace dbh_live {
namespace {

constexpr int kThreads = 256;
constexpr int kPrefixThreads = 1024;
constexpr int kSearchDepth = 32;              // halvings of a range of at most 2^31 chunks

// ---- append -------------------------------------------------------------------------------------
// n samples src -> dst, all threads of the workgroup: 16 bytes per thread where src and dst agree
// modulo 16 bytes, single int16 values in front of dst's first 16-byte boundary, behind the last
// whole piece and where they do not agree
__device__ __forceinline__ void copy_span(int16_t* __restrict__ dst,
                                          const int16_t* __restrict__ src, long long n, int t) {
    long long head = (8 - (((unsigned long long)dst >> 1) & 7)) & 7;
    if (head > n) head = n;
    long long body = 0;                                        // 16-byte pieces behind the head
    if ((((unsigned long long)(src + head)) & 15) == 0) body = (n - head) / 8;
    for (long long j = t; j < head; j += kThreads) dst[j] = src[j];
    const int4* src16 = (const int4*)(src + head);
    int4* dst16 = (int4*)(dst + head);
    for (long long j = t; j < body; j += kThreads) dst16[j] = src16[j];
    for (long long j = head + body * 8 + t; j < n; j += kThreads) dst[j] = src[j];
}

template <bool kPair>
__global__ __launch_bounds__(kThreads) void append_kernel(State st, Shape shape, Pair pair,
                                                          const Chunk* __restrict__ chunks,
                                                          const int16_t* __restrict__ in,
                                                          int* __restrict__ first,
                                                          int* __restrict__ count) {
    const int i = blockIdx.x, t = threadIdx.x;
    const Chunk chunk = chunks[i];
    dbh_live_result r = st.rec[chunk.channel];                 // (every thread: the same words)
    Gate g = st.gate[chunk.channel];
    const Append a = append(&r, &g, chunk.flags, chunk.length, shape);
    __syncthreads();                                           // all have read what thread 0 writes
    if (t == 0) {
        first[i] = a.idle ? -1 : a.first;
        count[i] = a.count;
        if (!a.idle) {
            st.rec[chunk.channel] = r;
            st.gate[chunk.channel] = g;
            if (kPair && (chunk.flags & DBH_LIVE_END)) {       // the end fold starts from fresh
                dbh_live_result f = fresh_record();
                f.status = DBH_LIVE_PENDING;
                pair.end.rec[chunk.channel] = f;
            }
        }
    }
    // the row begins on a 16-byte boundary: the host stages src so that it agrees with at modulo 8
    if (a.keep > 0)
        copy_span(st.samples + (long long)chunk.channel * st.stride + a.at, in + chunk.src, a.keep, t);
    if (kPair && !a.idle) {                                    // whatever the start side's record says
        const Tail tail = tail_store(r.samples - chunk.length, chunk.length, pair.shape);
        int16_t* ring = pair.ring + (long long)chunk.channel * pair.stride;
        const int16_t* src = in + chunk.tail;
        copy_span(ring + tail.at, src, tail.head, t);
        copy_span(ring, src + tail.head, tail.keep - tail.head, t);      // behind the wrap
    }
}

// ---- the window list ----------------------------------------------------------------------------
__global__ __launch_bounds__(kPrefixThreads) void list_kernel(const int* __restrict__ count,
                                                              int n_chunks,
                                                              long long* __restrict__ win_offsets) {
    __shared__ long long part[kPrefixThreads];
    long long carry = 0;
    for (int base = 0; base < n_chunks; base += kPrefixThreads) {
        const int i = base + threadIdx.x;
        const long long before =
            dbh_wave::prefix_trip<kPrefixThreads>(i < n_chunks ? count[i] : 0, part, &carry);
        if (i < n_chunks) win_offsets[i] = before;
    }
    if (threadIdx.x == 0) win_offsets[n_chunks] = carry;
}

// ---- the front ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void front_kernel(State st, Shape shape,
                                                         const Chunk* __restrict__ chunks,
                                                         const int* __restrict__ first,
                                                         const long long* __restrict__ win_offsets,
                                                         int n_chunks, long long w0, long long n,
                                                         float* __restrict__ x) {
    const long long slot = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slot >= n) return;                                     // (whole waves)
    const long long g = w0 + slot;
    const int16_t* src = st.samples;
    long long m = 0;                                           // a window outside the list: zeros
    if (g >= win_offsets[0] && g < win_offsets[n_chunks]) {
        int lo = 0, hi = n_chunks;                             // win_offsets[lo] <= g < [hi]
        for (int d = 0; d < kSearchDepth && hi - lo > 1; ++d) {
            const int mid = lo + (hi - lo) / 2;
            if (win_offsets[mid] <= g) lo = mid; else hi = mid;
        }
        const long long k = first[lo] + (g - win_offsets[lo]);
        const int channel = chunks[lo].channel;
        const long long have = st.rec[channel].samples;
        if (first[lo] >= 0 && k < shape.steps) {               // (so b <= cap: inside the row)
            const long long a = k * shape.h < have ? k * shape.h : have;
            const long long b = k * shape.h + shape.L < have ? k * shape.h + shape.L : have;
            m = b - a;
            src = st.samples + (long long)channel * st.stride + a;
        }
    }
    dbh_front::window(src, m, shape.L, 0, lane, x + slot * shape.L);
}

// ---- the end windows (pair sessions) ------------------------------------------------------------
// where in the ring's row sample j of a window lies that begins at index `at`: through the wrap,
// once at the most (m <= cap)
struct RingAt {
    long long at, cap;
    __device__ __forceinline__ long long operator()(int j) const {
        const long long p = at + j;
        return p < cap ? p : p - cap;
    }
};

__global__ __launch_bounds__(kThreads) void end_front_kernel(State st, Pair pair,
                                                             const Chunk* __restrict__ chunks,
                                                             const long long* __restrict__ end_offsets,
                                                             int n_chunks, long long w0, long long n,
                                                             float* __restrict__ x) {
    const long long slot = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slot >= n) return;                                     // (whole waves)
    const long long g = w0 + slot;
    const int16_t* row = pair.ring;
    RingAt from{0, pair.shape.cap};
    long long m = 0;                                           // a window outside the list: zeros
    int pad = pair.shape.L;
    if (g >= end_offsets[0] && g < end_offsets[n_chunks]) {
        int lo = 0, hi = n_chunks;                             // end_offsets[lo] <= g < [hi]
        for (int d = 0; d < kSearchDepth && hi - lo > 1; ++d) {
            const int mid = lo + (hi - lo) / 2;
            if (end_offsets[mid] <= g) lo = mid; else hi = mid;
        }
        const long long s = g - end_offsets[lo];
        const int channel = chunks[lo].channel;
        if (s < pair.shape.steps) {                            // (so a >= n - cap: inside the ring)
            const EndWindow w = end_window(st.rec[channel].samples, (int)s, pair.shape);
            row = pair.ring + (long long)channel * pair.stride;
            from.at = w.at;
            m = w.m;
            pad = w.pad;
        }
    }
    dbh_front::window(row, m, pair.shape.L, pad, lane, x + slot * pair.shape.L, from);
}

// ---- the resumable fold -------------------------------------------------------------------------
struct FoldArgs {
    State st;
    Shape shape;
    const Chunk* chunks;                 // null: chunk i is channel i
    const long long* win_offsets;
    long long n_chunks, w0, n;
    const float* probs;                  // [n][C], listed window w0 first
};

// this chunk's windows of the round, [lo, hi) in list numbers; false: none
__device__ __forceinline__ bool round_share(const FoldArgs& a, long long chunk, long long* lo,
                                            long long* hi) {
    *lo = a.win_offsets[chunk] > a.w0 ? a.win_offsets[chunk] : a.w0;
    *hi = a.win_offsets[chunk + 1] < a.w0 + a.n ? a.win_offsets[chunk + 1] : a.w0 + a.n;
    return *lo < *hi;
}

// dbh_sweep.hip's fold32_kernel shape: eight chunks per workgroup, lane c = class c, whole 32-lane
// groups exit together, every reduction in control flow that is uniform over the group (the record
// is the same words in all 32 lanes)
__global__ __launch_bounds__(kThreads) void fold32_kernel(FoldArgs a) {
    const long long chunk = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int c = threadIdx.x & 31;
    if (chunk >= a.n_chunks) return;
    long long lo, hi;
    if (!round_share(a, chunk, &lo, &hi)) return;
    const long long channel = a.chunks ? a.chunks[chunk].channel : chunk;
    const int C = a.st.n_classes, steps = a.shape.steps;
    const bool valid = c < C;
    dbh_live_result r = a.st.rec[channel];
    float merged = valid ? a.st.merged[channel * C + c] : 0.f;
    for (long long g = lo; g < hi && r.windows >= 0 && may_fold(r, a.shape); ++g) {
        if (valid) merged = dbh::fold_merge(merged, a.probs[(g - a.w0) * C + c], r.windows == 0, c);
        int top;
        double lead;
        dbh::fold32_step(merged, valid, c, &top, &lead);
        if (c == 0) {
            a.st.best[channel * steps + r.windows] = top;
            a.st.margin[channel * steps + r.windows] = lead;
        }
        folded(&r, top, lead, a.shape);
    }
    if (valid) a.st.merged[channel * C + c] = merged;
    if (c == 0) a.st.rec[channel] = r;
}

// dbh_sweep.hip's fold256_kernel shape: one workgroup per chunk, thread c = class c, the trees of
// dbh_trees.h; the loop's bounds are the same words in every thread, so every barrier is met by all
__global__ __launch_bounds__(kThreads) void fold256_kernel(FoldArgs a) {
    __shared__ double rv[kThreads];
    __shared__ int ri[kThreads];
    __shared__ double first;
    const long long chunk = blockIdx.x;
    const int c = threadIdx.x;
    long long lo, hi;
    if (!round_share(a, chunk, &lo, &hi)) return;              // (the whole workgroup)
    const long long channel = a.chunks ? a.chunks[chunk].channel : chunk;
    const int C = a.st.n_classes, steps = a.shape.steps;
    const bool valid = c < C;
    dbh_live_result r = a.st.rec[channel];
    float merged = valid ? a.st.merged[channel * C + c] : 0.f;
    __syncthreads();                                           // all have read what thread 0 writes
    for (long long g = lo; g < hi && r.windows >= 0 && may_fold(r, a.shape); ++g) {
        if (valid) merged = dbh::fold_merge(merged, a.probs[(g - a.w0) * C + c], r.windows == 0, c);
        int top;
        double lead;
        dbh::fold256_step<kThreads>(merged, valid, c, rv, ri, &first, &top, &lead);
        if (c == 0) {
            a.st.best[channel * steps + r.windows] = top;
            a.st.margin[channel * steps + r.windows] = lead;
        }
        folded(&r, top, lead, a.shape);
    }
    if (valid) a.st.merged[channel * C + c] = merged;
    if (c == 0) a.st.rec[channel] = r;
}

// ---- results ------------------------------------------------------------------------------------
template <bool kPair>
__global__ __launch_bounds__(kThreads) void results_kernel(State st, Pair pair,
                                                           const Chunk* __restrict__ chunks,
                                                           const int* __restrict__ first,
                                                           int n_chunks,
                                                           dbh_live_result* __restrict__ results,
                                                           dbh_live_end_result* __restrict__ end_results) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_chunks) return;
    const int channel = chunks[i].channel;
    dbh_live_result r = st.rec[channel];
    if (kPair && end_results) {
        dbh_live_end_result e =
            end_record(r, st.gate[channel], pair.end.rec[channel], pair.combine_mode);
        if (first[i] < 0) e.status = DBH_LIVE_IDLE;
        end_results[i] = e;
    }
    if (first[i] < 0) r.status = DBH_LIVE_IDLE;
    results[i] = r;
}

// ---- the yield policy ---------------------------------------------------------------------------
// The sum over the workgroup's kThreads threads, in thread 0 (int64: a yield passes 2^32 within
// seconds of sequencing).  part: kThreads / 64 words of LDS; all threads call it, once.
__device__ __forceinline__ long long block_sum(long long v, long long* part) {
    v = dbh_wave::wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    long long sum = 0;
    for (int w = 0; w < kThreads / 64; ++w) sum += part[w];
    return sum;
}

// (a session's push has its chunk table, dbh_live_policy_dev the caller's two arrays)
__device__ __forceinline__ unsigned flags_of(const PolicyArgs& a, long long i) {
    return a.chunks ? a.chunks[i].flags : a.chunk_flags[i];
}

// One workgroup per class: its threads walk the push's chunks, each summing the records that ended
// with this class as their call; one sum over the workgroup, and thread 0 adds it to the session's
// yields.  Integer sums: the same bits in any order.
__global__ __launch_bounds__(kThreads) void yield_kernel(PolicyArgs a) {
    __shared__ long long part_samples[kThreads / 64], part_reads[kThreads / 64];
    const int c = blockIdx.x;
    long long samples = 0, reads = 0;
    for (long long i = threadIdx.x; i < a.n_chunks; i += kThreads) {
        const dbh_live_result r = a.records[i];
        if (yield_class(r, flags_of(a, i), a.n_classes) == c) {
            samples += r.samples;
            reads += 1;
        }
    }
    samples = block_sum(samples, part_samples);
    reads = block_sum(reads, part_reads);
    if (threadIdx.x == 0) {
        a.yield_samples[c] += samples;
        a.yield_reads[c] += reads;
    }
}

// Every workgroup finds the floor for itself - thread c the level of class c (n_classes <=
// kThreads), the lowest over the workgroup - then one thread per chunk: the action record by
// dbh_live_core.h's action_of, and the channel's action where the chunk is not idle.
__global__ __launch_bounds__(kThreads) void action_kernel(PolicyArgs a) {
    __shared__ long long part[kThreads / 64];
    const int t = threadIdx.x;
    long long lowest = kNoLevel;
    if (t < a.n_classes && balanced(a.weight[t])) lowest = level_of(a.yield_samples[t], a.weight[t]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const long long other = __shfl_xor(lowest, o);
        lowest = other < lowest ? other : lowest;
    }
    if ((t & 63) == 0) part[t >> 6] = lowest;
    __syncthreads();
    for (int w = 0; w < kThreads / 64; ++w) lowest = part[w] < lowest ? part[w] : lowest;
    const long long floor = floor_from(lowest);
    const long long i = (long long)blockIdx.x * kThreads + t;
    if (i >= a.n_chunks) return;
    const dbh_live_result r = a.records[i];
    const int channel = a.chunks ? a.chunks[i].channel : a.channels[i];
    const dbh_live_action act =
        action_of(r, flags_of(a, i), a.channel_action[channel], a.weight, a.n_classes,
                  (const int64_t*)a.yield_samples, floor, a.slack, a.undecided);
    a.actions[i] = act;
    if (r.status != DBH_LIVE_IDLE) a.channel_action[channel] = act.action;
}

}  // namespace

// =============================================================================================
// The launches (dbh_live.h)
// =============================================================================================
hipError_t append(const State& st, const Shape& shape, const Pair& pair, const Chunk* chunks,
                  const int16_t* in, int n_chunks, int32_t* first, int32_t* count,
                  hipStream_t stream) {
    if (pair.ring)
        hipLaunchKernelGGL(append_kernel<true>, dim3((unsigned)n_chunks), dim3(kThreads), 0, stream,
                           st, shape, pair, chunks, in, (int*)first, (int*)count);
    else
        hipLaunchKernelGGL(append_kernel<false>, dim3((unsigned)n_chunks), dim3(kThreads), 0, stream,
                           st, shape, pair, chunks, in, (int*)first, (int*)count);
    return hipGetLastError();
}

hipError_t window_list(const int32_t* count, int n_chunks, int64_t* win_offsets,
                       hipStream_t stream) {
    hipLaunchKernelGGL(list_kernel, dim3(1), dim3(kPrefixThreads), 0, stream, (const int*)count,
                       n_chunks, (long long*)win_offsets);
    return hipGetLastError();
}

hipError_t front(const State& st, const Shape& shape, const Chunk* chunks, const int32_t* first,
                 const int64_t* win_offsets, int n_chunks, int64_t w0, int64_t n, float* x,
                 hipStream_t stream) {
    hipLaunchKernelGGL(front_kernel, dim3((unsigned)((n + 3) / 4)), dim3(kThreads), 0, stream, st,
                       shape, chunks, (const int*)first, (const long long*)win_offsets, n_chunks,
                       (long long)w0, (long long)n, x);
    return hipGetLastError();
}

hipError_t fold(bool general, const State& st, const Shape& shape, const Chunk* chunks,
                const int64_t* win_offsets, int64_t n_chunks, int64_t w0, int64_t n,
                const float* probs, hipStream_t stream) {
    const FoldArgs a{st, shape, chunks, (const long long*)win_offsets, (long long)n_chunks,
                     (long long)w0, (long long)n, probs};
    if (general)
        hipLaunchKernelGGL(fold256_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(fold32_kernel, dim3((unsigned)((n_chunks + 7) / 8)), dim3(kThreads), 0,
                           stream, a);
    return hipGetLastError();
}

hipError_t end_front(const State& st, const Pair& pair, const Chunk* chunks,
                     const int64_t* end_offsets, int n_chunks, int64_t w0, int64_t n, float* x,
                     hipStream_t stream) {
    hipLaunchKernelGGL(end_front_kernel, dim3((unsigned)((n + 3) / 4)), dim3(kThreads), 0, stream,
                       st, pair, chunks, (const long long*)end_offsets, n_chunks, (long long)w0,
                       (long long)n, x);
    return hipGetLastError();
}

hipError_t results(const State& st, const Pair& pair, const Chunk* chunks, const int32_t* first,
                   int n_chunks, dbh_live_result* results, dbh_live_end_result* end_results,
                   hipStream_t stream) {
    const dim3 grid((unsigned)((n_chunks + kThreads - 1) / kThreads));
    if (pair.ring)
        hipLaunchKernelGGL(results_kernel<true>, grid, dim3(kThreads), 0, stream, st, pair, chunks,
                           (const int*)first, n_chunks, results, end_results);
    else
        hipLaunchKernelGGL(results_kernel<false>, grid, dim3(kThreads), 0, stream, st, pair, chunks,
                           (const int*)first, n_chunks, results, end_results);
    return hipGetLastError();
}

hipError_t policy(const PolicyArgs& args, hipStream_t stream) {
    static_assert(kMaxClasses <= kThreads, "action_kernel: thread c holds class c's level");
    hipLaunchKernelGGL(yield_kernel, dim3((unsigned)args.n_classes), dim3(kThreads), 0, stream, args);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(action_kernel, dim3((unsigned)((args.n_chunks + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace dbh_live
