// dbh_kernels.h — what the host code of libdeepbinner_hip.so (dbh_api.hip, dbh_probes.h) sees of
// the device units dbh_kernels.hip, dbh_timeline.hip (the forward kernel's cycle-stamp build) and
// dbh_lean.hip (its build without the debug stages, which production launches run): the
// forward kernel's arguments and launch shape, and one launch function per kernel.  No kernel
// symbol leaves its unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dbh {

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;

// Arguments of the forward kernel (one by-value struct = the kernel-argument segment).
struct ForwardArgs {
    const float* packed;         // packed parameters (dbh_layout.h)
    const float* x;              // seam b1: [n_windows][1024] normalised windows, or null
    float* probs;                // [n_windows][n_classes]
    float* debug_out;
    const int16_t* samples;      // seam b2: int16 signals, or null
    const long long* offsets;    //          read r = samples[offsets[r] .. offsets[r+1])
    int* calls;                  //          barcode calls (one scan step per read), or null
    float* tail_scratch;         // [grid][kTailBatch][16][48]: conv17 outputs parked per workgroup
    int* win_counter;            // null: workgroup b walks groups b, b + grid, ...; else every
                                 // workgroup takes its next group of windows off this counter;
                                 // [1] counts the workgroups that have finished (both 0 between
                                 // launches: the last workgroup of a launch resets them)
    long long* clock_out;        // [grid][4 + kPhaseMarks * kPhaseGroups] or null: shader clock and 100
                                 // MHz clock at a workgroup's start and end (dbh_forward_clock_read),
                                 // then the phase stamps of its first groups (dbh_forward_phases_read)
    double score_diff;
    long long read0, len_hint, hint_cap;     // dbh_model_set_read_length_hint
    long long n_windows;
    int n_classes, debug_stage, steps, side;
    // windows not yet handed out below which a workgroup asks for groups of 2 / of 1 instead of
    // kGroup (the end of a launch: dbh_forward_kernel)
    int chunk4_min_left, chunk2_min_left;
    int phases;                  // clock probe on: also keep the phase stamps (dbh_forward_phases_enable)
};

}  // namespace dbh

namespace dbh_timeline {
// Every build of dbh_forward.hip takes a ForwardArgs of its own namespace (DBH_FORWARD_NS), which
// is part of its kernel's mangled name; the cycle-stamp build's is the same fields.
struct ForwardArgs : dbh::ForwardArgs {};
}  // namespace dbh_timeline
namespace dbh_lean {
// (the lean build's: it never reads debug_stage, which its launches leave at -1)
struct ForwardArgs : dbh::ForwardArgs {};
}  // namespace dbh_lean

// The launches: each queues one kernel on `stream` and returns hipGetLastError().
namespace dbh_kernels {

// dbh::dbh_forward_kernel / dbh_timeline::dbh_forward_kernel / dbh_lean::dbh_forward_kernel: grid
// workgroups of dbh::kThreads.  launch_forward_lean is for production launches only (debug_stage
// < 0): the lean kernel has no debug stages, timing stops or tail behind every group.
hipError_t launch_forward(const dbh::ForwardArgs& a, unsigned grid, hipStream_t stream);
hipError_t launch_forward_timeline(const dbh::ForwardArgs& a, unsigned grid, hipStream_t stream);
hipError_t launch_forward_lean(const dbh::ForwardArgs& a, unsigned grid, hipStream_t stream);
// (dbh_forward_kernel_info: the full build's registers and LDS; the lean build's are the same)
hipError_t forward_attributes(hipFuncAttributes* attr);

// dbh::dbh_normalise_kernel: one block per window, windows <= 2^31 - 1
hipError_t launch_normalise(const int16_t* samples, const long long* offsets, int steps, int side,
                            float* windows_out, unsigned windows, hipStream_t stream);
// dbh::dbh_merge_kernel over n_reads reads
hipError_t launch_merge(const float* wprobs, long long n_reads, int steps, int n_classes,
                        double score_diff, float* probs, int* calls, hipStream_t stream);
// combine_calls_kernel over n reads
hipError_t launch_combine(const int32_t* start_calls, const int32_t* end_calls, long long n, int mode,
                          int32_t* out, hipStream_t stream);

}  // namespace dbh_kernels
