// dbh_status.h — how a failed HIP call becomes a dbh_status in every unit that reports through
// dbh_last_error() (dbh_comm.hip and dbh_inflate.hip keep error strings, and macros, of their own).
#pragma once

#include <hip/hip_runtime.h>

namespace dbh_hip {
// dbh_api.hip: keeps "what: the error's text" for dbh_last_error(), maps the error to a dbh_status
__attribute__((visibility("hidden"))) int hip_fail(hipError_t e, const char* what);
}  // namespace dbh_hip

// return hip_fail's status where `call` fails, named as it is written (DBH_HIP) or by `what`
#define DBH_HIP_AS(what, call)                                              \
    do {                                                                    \
        const hipError_t e_ = (call);                                       \
        if (e_ != hipSuccess) return dbh_hip::hip_fail(e_, what);           \
    } while (0)
#define DBH_HIP(call) DBH_HIP_AS(#call, call)
