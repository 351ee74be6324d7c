// dbh_random.hip - the synthetic no-barcode signals of `balance` made ON THE GPU (C ABI: the
// "random signals" section of include/deepbinner_hip.h).  What a value is:
// dbh_random_core.h; this file is the kernel that runs it, one workgroup per signal, and the host
// entry that runs the same core with loops (dbh_random_signals_host).
//
// random_signals  a workgroup takes signals blockIdx.x, blockIdx.x + gridDim.x, ...; every thread
//                 derives the signal's eight parameters itself (eight hashes), then the threads
//                 stride over the values.  flat, gaussian and perlin values need nothing else.  A
//                 multi_gaussian's segments are laid end to end, so a value's segment depends on
//                 the lengths in front of it: the workgroup draws 256 segments at a time, scans
//                 their lengths (dbh_wave.h: within a wave, four totals through LDS), keeps their
//                 starts, means and deviations in LDS, and each value finds its segment there by
//                 bisection.  256 segments cover 25,600 values at least, so the chunk loop runs
//                 input_size / 25,600 + 1 times at most.
// No atomics, nothing waits for another workgroup, and the result knows nothing of the launch
// geometry: first_signal only names which signals are wanted.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <stddef.h>
#include <stdint.h>

#include "dbh_random_core.h"

extern "C" {
/* the GPU's generator run on the host: same core, signals and values as loops; needs no device */
__attribute__((visibility("default"))) int dbh_random_signals_host(
    uint64_t seed, int64_t first_signal, int64_t n_signals, int input_size, int16_t* out_host) {
    const int st = dbr::check_arguments(first_signal, n_signals, input_size, out_host);
    if (st != 0) return st;
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    for (int64_t k = 0; k < n_signals; ++k)
        dbr::model_signal(lo, hi, (uint32_t)(first_signal + k), input_size, out_host + k * input_size);
    return 0;
}
}

#if defined(__HIPCC__)
#include "../../include/deepbinner_hip.h"
#include "dbh_owned.h"
#include "dbh_status.h"
#include "dbh_wave.h"

namespace dbh_random_detail {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kChunkSegments = kThreads;                 // one segment per thread and chunk
constexpr int kMaxBlocks = 1 << 16;

__global__ __launch_bounds__(kThreads) void random_signals(uint32_t lo, uint32_t hi, uint32_t first_signal,
                                                           int64_t n_signals, int32_t input_size,
                                                           int16_t* __restrict__ out) {
    __shared__ int32_t seg_start[kChunkSegments];
    __shared__ double seg_mean[kChunkSegments], seg_stdev[kChunkSegments];
    __shared__ int32_t wave_total[kWaves];
    const int t = threadIdx.x;
    for (int64_t k = blockIdx.x; k < n_signals; k += gridDim.x) {
        const uint32_t s = first_signal + (uint32_t)k;
        int16_t* row = out + k * input_size;
        const dbr::Signal g = dbr::signal_of(lo, hi, s);
        if (g.kind == dbr::kFlat) {
            for (int32_t i = t; i < input_size; i += kThreads) row[i] = (int16_t)g.level;
        } else if (g.kind == dbr::kGaussian) {
            for (int32_t i = t; i < input_size; i += kThreads)
                row[i] = dbr::gaussian_value(g.mean, g.stdev, dbr::normal(lo, hi, s, (uint32_t)i));
        } else if (g.kind == dbr::kPerlin) {
            for (int32_t i = t; i < input_size; i += kThreads)
                row[i] = dbr::perlin_value(g, lo, hi, s, (uint32_t)i);
        } else {
            // g.kind is the same in every thread of the workgroup: the barriers below are met by all
            const int32_t chunks = input_size / (kChunkSegments * dbr::kMinSegment) + 1;
            int32_t at = 0;                              // where this chunk's first segment starts
            for (int32_t chunk = 0; chunk < chunks && at < input_size; ++chunk) {
                const uint32_t segment = (uint32_t)(chunk * kChunkSegments + t);
                const int32_t length = dbr::segment_length(lo, hi, s, segment);
                int32_t total;
                seg_start[t] = at + dbh_wave::block_prefix<kWaves>(length, wave_total, &total);
                seg_mean[t] = dbr::segment_mean(lo, hi, s, segment);
                seg_stdev[t] = dbr::segment_stdev(lo, hi, s, segment);
                __syncthreads();
                const int32_t end = min(at + total, input_size);
                for (int32_t i = at + t; i < end; i += kThreads) {
                    // the last segment of the chunk that starts at or below i
                    int q = 0;
#pragma unroll
                    for (int half = kChunkSegments / 2; half >= 1; half >>= 1)
                        q += seg_start[q + half] <= i ? half : 0;
                    row[i] = dbr::gaussian_value(seg_mean[q], seg_stdev[q], dbr::normal(lo, hi, s, (uint32_t)i));
                }
                at += total;
                __syncthreads();                         // the tables are rewritten by the next chunk
            }
        }
    }
}

hipError_t launch(uint64_t seed, int64_t first_signal, int64_t n_signals, int input_size, int16_t* out_dev,
                  hipStream_t stream) {
    const unsigned grid = (unsigned)(n_signals < kMaxBlocks ? n_signals : kMaxBlocks);
    hipLaunchKernelGGL(random_signals, dim3(grid), dim3(kThreads), 0, stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)first_signal, n_signals, (int32_t)input_size, out_dev);
    return hipGetLastError();
}

}  // namespace dbh_random_detail

#define DBH_RANDOM_HIP(call) DBH_HIP_AS("dbh_random_signals", call)

extern "C" {

int dbh_random_signals_dev(uint64_t seed, int64_t first_signal, int64_t n_signals, int input_size,
                           int16_t* out_dev, dbh_stream stream) {
    const int st = dbr::check_arguments(first_signal, n_signals, input_size, out_dev);
    if (st != DBH_OK) return st;
    DBH_RANDOM_HIP(dbh_random_detail::launch(seed, first_signal, n_signals, input_size, out_dev,
                                             (hipStream_t)stream));
    return DBH_OK;
}

int dbh_random_signals(uint64_t seed, int64_t first_signal, int64_t n_signals, int input_size,
                       int16_t* out_host) {
    const int st = dbr::check_arguments(first_signal, n_signals, input_size, out_host);
    if (st != DBH_OK) return st;
    const size_t bytes = (size_t)n_signals * (size_t)input_size * sizeof(int16_t);
    dbh_owned::DeviceBlock block;
    DBH_RANDOM_HIP(block.reserve(bytes));
    DBH_RANDOM_HIP(dbh_random_detail::launch(seed, first_signal, n_signals, input_size,
                                             block.as<int16_t>(), 0));
    DBH_RANDOM_HIP(hipStreamSynchronize(0));
    DBH_RANDOM_HIP(hipMemcpy(out_host, block.get(), bytes, hipMemcpyDeviceToHost));
    return DBH_OK;
}

}
#endif
