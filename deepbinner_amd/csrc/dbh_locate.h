// dbh_locate.h — what the library's host code (dbh_api_locate.hip) sees of dbh_locate.hip: the
// rule of `locate` over a batch of reads on the device, and the same rule on the host (the CPU model).
// No kernel symbol leaves the unit.  The contract is include/deepbinner_hip.h's ("locate").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/deepbinner_hip.h"

namespace dbh_locate {

// locations[n_reads] from evidence [n_reads][steps][cells][C], the side's calls [n_reads] and the
// reads' sample offsets [n_reads + 1] (only their differences are read).  One launch per 2^28 reads,
// no allocation, no synchronisation.
hipError_t locate(const float* evidence, const int32_t* calls, const int64_t* offsets,
                  int64_t n_reads, int steps, int cells, int n_classes, int input_size, int side,
                  dbh_location* locations, hipStream_t stream);

// the same over host arrays, read by read
void locate_host(const float* evidence, const int32_t* calls, const int64_t* offsets,
                 int64_t n_reads, int steps, int cells, int n_classes, int input_size, int side,
                 dbh_location* locations);

}  // namespace dbh_locate
