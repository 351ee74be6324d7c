// dbh_locate.hip — the device unit of `locate` (dbh_locate.h; include/deepbinner_hip.h, "locate"): from
// the evidence the general path's head leaves per window and cell (dbh_general.hip: head_kernel) and a
// side's calls to where in each read the call comes from.  The rule is dbh_locate_core.h's, the same
// lines for the wave here and for the CPU model below.
//
//   locate_kernel   one wave per read, four reads per workgroup.  The lanes walk the steps * cells
//                   values of the called class 64 at a time, each keeping its best (value, flat
//                   index); dbh_wave::wave_best folds the 64 picks - the order of the pick is total,
//                   so the fold gives what a serial loop gives; lane 0 then runs the span, the share
//                   and the sample range over the deciding window's cells (at most 128) and writes.
//
// Every loop is bounded by steps * cells or by cells; no atomics, nothing waits on another workgroup,
// and a read's location depends on that read's evidence alone - not on the batch it travels in.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dbh_locate.h"
#include "dbh_locate_core.h"
#include "dbh_wave.h"

namespace dbh_locate {
namespace {

constexpr int kThreads = 256;                 // four waves: four reads

__global__ __launch_bounds__(kThreads) void locate_kernel(
    const float* __restrict__ evidence, const int* __restrict__ calls,
    const long long* __restrict__ offsets, long long read0, long long n_reads, int steps, int cells,
    int C, int L, int side, dbh_location* __restrict__ locations) {
    const long long read = read0 + (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (read >= n_reads) return;                               // (whole waves)
    const int c = calls[read];
    if (!dbl::call_locates(c, C)) {                            // (uniform over the wave)
        if (lane == 0) locations[read] = dbl::no_location();
        return;
    }
    const float* ev = evidence + (size_t)read * steps * cells * C;
    dbl::Best best = dbl::best_none();
    const int n_values = steps * cells;
    for (int i = lane; i < n_values; i += 64) dbl::consider(&best, ev[(size_t)i * C + c], i);
    dbh_wave::wave_best(&best.v, &best.i);
    if (lane == 0)
        locations[read] = dbl::finish(ev, best, c, cells, C, L, side, offsets[read + 1] - offsets[read]);
}

}  // namespace

hipError_t locate(const float* evidence, const int32_t* calls, const int64_t* offsets,
                  int64_t n_reads, int steps, int cells, int n_classes, int input_size, int side,
                  dbh_location* locations, hipStream_t stream) {
    constexpr int64_t kPerLaunch = (int64_t)1 << 28;           // 2^26 workgroups
    for (int64_t r0 = 0; r0 < n_reads; r0 += kPerLaunch) {
        const int64_t n = std::min<int64_t>(kPerLaunch, n_reads - r0);
        // (the reads of a launch keep their numbers: every array is indexed from read 0)
        hipLaunchKernelGGL(locate_kernel, dim3((unsigned)((n + 3) / 4)), dim3(kThreads), 0, stream,
                           evidence, (const int*)calls, (const long long*)offsets, (long long)r0,
                           (long long)(r0 + n), steps, cells, n_classes, input_size, side, locations);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void locate_host(const float* evidence, const int32_t* calls, const int64_t* offsets,
                 int64_t n_reads, int steps, int cells, int n_classes, int input_size, int side,
                 dbh_location* locations) {
    for (int64_t r = 0; r < n_reads; ++r)
        locations[r] = dbl::locate_read(evidence + (size_t)r * steps * cells * n_classes, calls[r],
                                        steps, cells, n_classes, input_size, side,
                                        (long long)(offsets[r + 1] - offsets[r]));
}

}  // namespace dbh_locate
