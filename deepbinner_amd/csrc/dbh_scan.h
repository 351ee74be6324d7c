// dbh_scan.h — what the library's host code (dbh_api_scan.hip) sees of dbh_scan.hip: the
// window offsets of a batch of ragged reads, the front that cuts EVERY window of every read, and the
// pass from a per-window track to events, one launch function each.  No kernel symbol leaves the
// unit.  The contract is include/deepbinner_hip.h's ("scan").
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/deepbinner_hip.h"

namespace dbh_scan {

// W(n): windows of a read of n samples at input size L (host and device)
__host__ __device__ inline long long window_count(long long n, int L) {
    const long long h = L / 2;
    return n <= L ? 1 : (n - L + h - 1) / h + 1;
}

// window_offsets[n_reads + 1]: the exclusive prefix of W over the batch, the total behind it
hipError_t window_offsets(const int64_t* offsets, int64_t n_reads, int L, int64_t* window_offsets,
                          hipStream_t stream);

// x[n_windows][L] fp32: global windows [first_window, first_window + n_windows) of the batch, cut,
// normalised and padded.  A window outside the batch's windows is all zeros.
hipError_t windows(const int16_t* samples, const int64_t* offsets, const int64_t* window_offsets,
                   int64_t n_reads, int L, int side, int64_t first_window, int64_t n_windows,
                   float* x, hipStream_t stream);

// bytes of `workspace` for events() over n_reads reads
size_t events_workspace_bytes(int64_t n_reads);

// The events of a track (best, margin per global window): a count pass per read, the prefix over
// reads, the write pass.  events holds max_events entries; *n_events is the true total;
// per_read_interior (n_reads int32) may be null.
hipError_t events(const int32_t* best, const double* margin, const int64_t* window_offsets,
                  int64_t n_reads, double threshold, int min_windows, int skip_windows,
                  dbh_scan_event* events, int64_t max_events, int32_t* per_read_interior,
                  int64_t* n_events, void* workspace, hipStream_t stream);

}  // namespace dbh_scan
