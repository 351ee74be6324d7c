// dbh_lean.hip — the forward kernel as production launches run it: the same source with the debug
// stages, the 100 + k timing stops and tail_every_group folded away at compile time
// (DBH_FORWARD_DEBUG 0: debug_stage is the constant -1), and the host function that launches it
// (dbh_kernels.h).  A unit of its own beside dbh_kernels.hip and dbh_timeline.hip: the three builds
// of dbh_forward.hip share no code object and compile side by side.
#include <hip/hip_runtime.h>

#include "dbh_kernels.h"
#define DBH_FORWARD_NS dbh_lean
#define DBH_TIMELINE 0
#define DBH_FORWARD_DEBUG 0
#include "dbh_forward.hip"

namespace dbh_kernels {

hipError_t launch_forward_lean(const dbh::ForwardArgs& a, unsigned grid, hipStream_t stream) {
    hipLaunchKernelGGL(dbh_lean::dbh_forward_kernel, dim3(grid), dim3(dbh::kThreads), 0, stream,
                       dbh_lean::ForwardArgs{a});
    return hipGetLastError();
}

}  // namespace dbh_kernels
