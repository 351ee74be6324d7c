// dbh_sweep.h — what the library's host code (dbh_api_sweep.hip) sees of dbh_sweep.hip: the
// fold over scan sizes in its two forms, the tally of outcomes and the early tally, one launch
// function each.  No kernel symbol leaves the unit.  The contract is include/deepbinner_hip.h's
// ("sweep").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dbh_sweep {

constexpr int kMaxClasses = 256;      // the general path's limit (dbh_general.h)

// best[read][k-1], margin[read][k-1] for k = 1 .. steps from wprobs[n_reads][steps][n_classes].
// fold32: 32 lanes per read, the sums in dbh_merge_kernel's order (n_classes <= 32); fold256: one
// workgroup per read, the sums in the general merge's order (n_classes <= 256).  Each queues its
// kernels on `stream` and returns hipGetLastError().
hipError_t fold32(const float* wprobs, int64_t n_reads, int steps, int n_classes, int32_t* best,
                  double* margin, hipStream_t stream);
hipError_t fold256(const float* wprobs, int64_t n_reads, int steps, int n_classes, int32_t* best,
                   double* margin, hipStream_t stream);

// Adds the outcomes of n_reads reads into counts[steps][n_thresholds][modes][n_classes + 3]
// (modes = 3 when both sides are given, else 1).  A side that is not given is two null pointers;
// labels may be null.
hipError_t tally(const int32_t* start_best, const double* start_margin, const int32_t* end_best,
                 const double* end_margin, const int32_t* labels, int64_t n_reads, int steps,
                 int n_classes, const double* thresholds, int n_thresholds,
                 unsigned long long* counts, hipStream_t stream);

// The early tally (dbh_early_core.h): adds what a live session would have decided at every
// min_windows 1 .. steps and every threshold into calls[steps][T][modes][n_classes + 3],
// early[steps][T][8], windows[steps][T][steps] and - with lengths - pushes[steps][T][n_pushes],
// n_pushes = pushes_bound(): one workgroup per 256 reads.  The end side, labels and lengths (with
// pushes) may be null; a negative length counts as 0.
hipError_t early_tally(const int32_t* start_best, const double* start_margin,
                       const int32_t* end_best, const double* end_margin, const int32_t* labels,
                       const int64_t* lengths, int64_t n_reads, int steps, int n_classes,
                       int input_size, int64_t chunk_samples, const double* thresholds,
                       int n_thresholds, int n_pushes, unsigned long long* calls,
                       unsigned long long* early, unsigned long long* windows,
                       unsigned long long* pushes, hipStream_t stream);

}  // namespace dbh_sweep
