// dbh_occlude.h — what the library's host code (dbh_api_locate.hip) sees of dbh_occlude.hip:
// the rule of `locate --occlude` over a batch of reads on the device, and the same rule on the host
// (the CPU models).  No kernel symbol leaves the unit.  The contract is include/deepbinner_hip.h's
// ("occlude").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/deepbinner_hip.h"

namespace dbh_occlude {

// x [n_reads][steps][L]: the side's windows of reads [0, n_reads) of `offsets`, sliced, normalised
// and zero-padded as the general path's front does it (dbh_seam.h: the same bounds, sums and
// constants, so the same bits).  One wave per window.
hipError_t slice(const int16_t* samples, const int64_t* offsets, int64_t n_reads, int steps, int L,
                 int side, float* x, hipStream_t stream);

// plans[n_reads] and occlusions[n_reads] (cls, control samples, the "no result" fields) from the
// locations and the reads' sample offsets [n_reads + 1] (only their differences are read)
hipError_t plan(const dbh_location* locations, const int64_t* offsets, int64_t n_reads, int steps,
                int L, int side, dbh_occlude_plan* plans, dbh_occlusion* occlusions,
                hipStream_t stream);

// out[v] [n_reads][steps][L], v = DBH_OCCLUDE_OUT, _ONLY, _CTRL: x with the variant's blank set
// stored as 0.0f
hipError_t windows(const float* x, const int64_t* offsets, const dbh_occlude_plan* plans,
                   int64_t n_reads, int steps, int L, int side, float* const out[3],
                   hipStream_t stream);

// the results of the variants into the occlusions: probs [n_reads][C] and the plans of the same
// reads; vprobs [3][stride][C] and vcalls [3][stride], stride >= n_reads, the merge's outputs of the
// three variant passes
hipError_t gather(const dbh_occlude_plan* plans, const float* probs, const float* vprobs,
                  const int32_t* vcalls, int64_t n_reads, int64_t stride, int n_classes,
                  dbh_occlusion* occlusions, hipStream_t stream);

// plan and windows over host arrays, read by read.  Every launch above queues on `stream` and
// returns: no allocation, no synchronisation.
void plan_host(const dbh_location* locations, const int64_t* offsets, int64_t n_reads, int steps,
               int L, int side, dbh_occlude_plan* plans, dbh_occlusion* occlusions);
void windows_host(const float* x, const int64_t* offsets, const dbh_occlude_plan* plans,
                  int64_t n_reads, int steps, int L, int side, float* const out[3]);

}  // namespace dbh_occlude
