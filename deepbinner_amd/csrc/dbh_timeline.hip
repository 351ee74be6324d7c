// dbh_timeline.hip — the forward kernel with the cycle stamps compiled in (tools/timeline.py), and
// the host function that launches it (dbh_kernels.h).  A unit of its own beside dbh_kernels.hip:
// the two builds of dbh_forward.hip share no code object and compile side by side.
#include <hip/hip_runtime.h>

#include "dbh_kernels.h"
#define DBH_FORWARD_NS dbh_timeline
#define DBH_TIMELINE 1
#include "dbh_forward.hip"

namespace dbh_kernels {

hipError_t launch_forward_timeline(const dbh::ForwardArgs& a, unsigned grid, hipStream_t stream) {
    hipLaunchKernelGGL(dbh_timeline::dbh_forward_kernel, dim3(grid), dim3(dbh::kThreads), 0, stream,
                       dbh_timeline::ForwardArgs{a});
    return hipGetLastError();
}

}  // namespace dbh_kernels
