// dbh_scan.hip — the device unit of the scan (dbh_scan.h; include/deepbinner_hip.h, "scan"): barcode
// signal looked for in EVERY window of a read, not only in the scan_size samples at its ends.
//
// A read of n samples has W(n) windows of L samples, one every h = L/2 (classify.py:337-357 carried
// on to the read's other end), so a batch of reads is ragged: window_offsets is the exclusive prefix
// of W over the reads, and a global window number finds its read there by binary search.
//
//   window_offsets_kernel   W per read from the sample offsets and their prefix: one workgroup walks
//                           the reads 1,024 at a time, dbh_wave.h's block scan per trip and a carry
//   windows_kernel          the ragged front: one wave per window - find the read, cut [a, b), the
//                           int64 sums S and Q over the wave (dbh_wave::wave_sum), the one fp64
//                           expression per value of DESIGN.md section 19, zero padding behind (side
//                           start) or in front (side end)
//   events_kernel           one wave per read, 64 consecutive windows per trip: a window fires its
//                           best class when that is a barcode and leads by the threshold; a run
//                           starts where a lane's firing class differs from the lane before it, its
//                           first window and its peak travel along the run by shuffles, and what a
//                           trip's last lane holds is carried into the next.  Run twice: a count
//                           pass, event_offsets_kernel's prefix over the reads, the write pass.
//
// Every loop is bounded by W, by the read count or by the search depth; nothing waits on another
// workgroup.  Events are integers and comparisons only (the peak is a maximum of the track's own
// values), so they depend on neither the launch shape nor on how the windows were split into chunks.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dbh_front.h"
#include "dbh_scan.h"
#include "dbh_wave.h"

namespace dbh_scan {
namespace {

constexpr int kThreads = 256;                 // four waves: four windows, or four reads
constexpr int kPrefixThreads = 1024;
constexpr int kSearchDepth = 64;              // halvings of a range of at most 2^63 reads

// one trip of a prefix over values handed out 1,024 at a time (dbh_wave.h)
__device__ __forceinline__ long long prefix_trip(long long v, long long* part, long long* carry) {
    return dbh_wave::prefix_trip<kPrefixThreads>(v, part, carry);
}

__global__ __launch_bounds__(kPrefixThreads) void window_offsets_kernel(
    const long long* __restrict__ offsets, long long n_reads, int L,
    long long* __restrict__ window_offsets) {
    __shared__ long long part[kPrefixThreads];
    long long carry = 0;
    for (long long base = 0; base < n_reads; base += kPrefixThreads) {
        const long long r = base + threadIdx.x;
        const long long w = r < n_reads ? window_count(offsets[r + 1] - offsets[r], L) : 0;
        const long long before = prefix_trip(w, part, &carry);
        if (r < n_reads) window_offsets[r] = before;
    }
    if (threadIdx.x == 0) window_offsets[n_reads] = carry;
}

__global__ __launch_bounds__(kPrefixThreads) void event_offsets_kernel(
    const int* __restrict__ counts, long long n_reads, long long* __restrict__ event_offsets,
    long long* __restrict__ n_events) {
    __shared__ long long part[kPrefixThreads];
    long long carry = 0;
    for (long long base = 0; base < n_reads; base += kPrefixThreads) {
        const long long r = base + threadIdx.x;
        const long long before = prefix_trip(r < n_reads ? counts[r] : 0, part, &carry);
        if (r < n_reads) event_offsets[r] = before;
    }
    if (threadIdx.x == 0) {
        event_offsets[n_reads] = carry;
        *n_events = carry;
    }
}

// ---- the ragged front (the rule itself: dbh_front.h, shared with dbh_live.hip) ------------------
__global__ __launch_bounds__(kThreads) void windows_kernel(
    const int16_t* __restrict__ samples, const long long* __restrict__ offsets,
    const long long* __restrict__ window_offsets, long long n_reads, int L, int side,
    long long first_window, long long n_windows, float* __restrict__ x) {
    const long long slot = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slot >= n_windows) return;                             // (whole waves)
    float* out = x + slot * L;
    const long long g = first_window + slot;
    long long a = 0, m = 0;                                    // the samples present: [a, a + m)
    if (g >= window_offsets[0] && g < window_offsets[n_reads]) {
        long long lo = 0, hi = n_reads;                        // window_offsets[lo] <= g < [hi]
        for (int d = 0; d < kSearchDepth && hi - lo > 1; ++d) {
            const long long mid = lo + (hi - lo) / 2;
            if (window_offsets[mid] <= g) lo = mid; else hi = mid;
        }
        const long long k = g - window_offsets[lo], h = L / 2;
        const long long n = offsets[lo + 1] - offsets[lo];
        long long b;
        if (side == DBH_SIDE_START) {
            a = k * h < n ? k * h : n;
            b = k * h + L < n ? k * h + L : n;
        } else {
            a = n - k * h - L > 0 ? n - k * h - L : 0;
            b = n - k * h > 0 ? n - k * h : 0;
        }
        m = b - a;
        a += offsets[lo];
    }
    const int pad = side == DBH_SIDE_START ? 0 : L - (int)m;   // zeros in front
    dbh_front::window(samples + a, m, L, pad, lane, out);
}

// ---- events -------------------------------------------------------------------------------------
__device__ __forceinline__ int firing_class(const int* best, const double* margin, long long at,
                                            double threshold, double* lead) {
    const int b = best[at];
    const double m = margin[at];
    *lead = m;
    return (b != 0 && m >= threshold) ? b : 0;
}

__global__ __launch_bounds__(kThreads) void events_kernel(
    const int* __restrict__ best, const double* __restrict__ margin,
    const long long* __restrict__ window_offsets, long long read0, long long n_reads,
    double threshold, int min_windows, int skip_windows, int write,
    const long long* __restrict__ event_offsets, dbh_scan_event* __restrict__ events,
    long long max_events, int* __restrict__ counts, int* __restrict__ interior) {
    const long long read = read0 + (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (read >= n_reads) return;                               // (whole waves)
    const long long w0 = window_offsets[read];
    const long long W = window_offsets[read + 1] - w0;
    long long out = write ? event_offsets[read] : 0;
    int carry_cls = 0, carry_first = 0, found = 0, inside = 0;
    double carry_peak = 0.0;
    for (long long t0 = 0; t0 < W; t0 += 64) {                 // (uniform over the wave)
        const long long k = t0 + lane;
        int cls = 0;
        double peak = 0.0;
        if (k < W) cls = firing_class(best, margin, w0 + k, threshold, &peak);
        int next = __shfl_down(cls, 1);
        if (lane == 63) {
            double unused;
            next = k + 1 < W ? firing_class(best, margin, w0 + k + 1, threshold, &unused) : 0;
        }
        int prev = dbh_wave::from_lane_before(cls);
        if (lane == 0) prev = carry_cls;
        // the run's first window: the latest run start at or before this lane, or the carried one
        int first = (cls != 0 && cls != prev) ? (int)k : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int below = __shfl_up(first, d);
            if (lane >= d && below > first) first = below;
        }
        if (cls == 0) first = -1;
        else if (first < 0) first = carry_first;
        // the highest margin of the run so far: a scan that stays inside the run
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double below = __shfl_up(peak, d);
            const int below_first = __shfl_up(first, d);
            if (lane >= d && cls != 0 && below_first == first) peak = fmax(peak, below);
        }
        if (cls != 0 && first < t0) peak = fmax(peak, carry_peak);
        const bool ends = cls != 0 && next != cls;             // (behind the last window: 0)
        const int emit = (ends && (int)k - first + 1 >= min_windows) ? 1 : 0;
        if (write) {
            const int incl = dbh_wave::wave_scan_inclusive(emit);
            const long long at = out + incl - emit;
            if (emit && at < max_events) {
                dbh_scan_event e;
                e.read = read;
                e.cls = cls;
                e.first = first;
                e.last = (int)k;
                e.reserved = 0;
                e.peak = peak;
                events[at] = e;
            }
            out += __shfl(incl, 63);
        } else {
            found += emit;
            inside += (emit && first >= skip_windows) ? 1 : 0;
        }
        carry_cls = __shfl(cls, 63);
        carry_first = __shfl(first, 63);
        carry_peak = __shfl(peak, 63);
    }
    if (!write) {
        found = dbh_wave::wave_sum(found);
        inside = dbh_wave::wave_sum(inside);
        if (lane == 0) {
            counts[read] = found;
            if (interior) interior[read] = inside;
        }
    }
}

}  // namespace

// =============================================================================================
// The launches (dbh_scan.h)
// =============================================================================================
hipError_t window_offsets(const int64_t* offsets, int64_t n_reads, int L, int64_t* window_offsets,
                          hipStream_t stream) {
    hipLaunchKernelGGL(window_offsets_kernel, dim3(1), dim3(kPrefixThreads), 0, stream,
                       (const long long*)offsets, (long long)n_reads, L, (long long*)window_offsets);
    return hipGetLastError();
}

hipError_t windows(const int16_t* samples, const int64_t* offsets, const int64_t* window_offsets,
                   int64_t n_reads, int L, int side, int64_t first_window, int64_t n_windows,
                   float* x, hipStream_t stream) {
    constexpr int64_t kPerLaunch = (int64_t)1 << 28;           // 2^26 workgroups
    for (int64_t w0 = 0; w0 < n_windows; w0 += kPerLaunch) {
        const int64_t n = std::min<int64_t>(kPerLaunch, n_windows - w0);
        hipLaunchKernelGGL(windows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(kThreads), 0, stream,
                           samples, (const long long*)offsets, (const long long*)window_offsets,
                           (long long)n_reads, L, side, (long long)(first_window + w0),
                           (long long)n, x + w0 * L);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// counts int32 [n_reads], then event_offsets int64 [n_reads + 1]
size_t events_workspace_bytes(int64_t n_reads) {
    return (((size_t)n_reads * sizeof(int32_t) + 255) & ~(size_t)255) +
           (size_t)(n_reads + 1) * sizeof(int64_t);
}

hipError_t events(const int32_t* best, const double* margin, const int64_t* window_offsets,
                  int64_t n_reads, double threshold, int min_windows, int skip_windows,
                  dbh_scan_event* events, int64_t max_events, int32_t* per_read_interior,
                  int64_t* n_events, void* workspace, hipStream_t stream) {
    int* counts = (int*)workspace;
    long long* event_offsets =
        (long long*)((char*)workspace + (((size_t)n_reads * sizeof(int32_t) + 255) & ~(size_t)255));
    constexpr int64_t kPerLaunch = (int64_t)1 << 28;
    for (int write = 0; write < 2; ++write) {
        for (int64_t r0 = 0; r0 < n_reads; r0 += kPerLaunch) {
            const int64_t n = std::min<int64_t>(kPerLaunch, n_reads - r0);
            // (the reads of a launch keep their numbers: every array is indexed from read 0)
            hipLaunchKernelGGL(events_kernel, dim3((unsigned)((n + 3) / 4)), dim3(kThreads), 0,
                               stream, (const int*)best, margin,
                               (const long long*)window_offsets, (long long)r0,
                               (long long)(r0 + n), threshold,
                               min_windows, skip_windows, write, event_offsets, events,
                               (long long)max_events, counts, (int*)per_read_interior);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        if (write == 0) {
            hipLaunchKernelGGL(event_offsets_kernel, dim3(1), dim3(kPrefixThreads), 0, stream,
                               counts, (long long)n_reads, event_offsets, (long long*)n_events);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace dbh_scan
