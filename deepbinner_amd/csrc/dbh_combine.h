// dbh_combine.h - combine_calls (classify.py:298-322) on call numbers (0 = 'none'), ONE text for
// dbh_kernels.hip's combine_calls_kernel (dbh_combine_calls_dev), the live sessions' end record
// (dbh_live.hip) and the host model of the live rules (live_model_check.cpp).  Plain integers: any
// compiler, host or device.
#pragma once

#include "../../include/deepbinner_hip.h"

#if defined(__HIPCC__)
#define DBH_COMBINE_FN __host__ __device__ __forceinline__
#else
#define DBH_COMBINE_FN inline
#endif

namespace dbh {

// mode: DBH_REQUIRE_EITHER / _START / _BOTH
DBH_COMBINE_FN int combine_calls(int s, int e, int mode) {
    if (s == e) return s;
    if (mode == DBH_REQUIRE_BOTH) return DBH_CALL_NONE;
    if (e == DBH_CALL_NONE) return s;
    if (mode == DBH_REQUIRE_START) return DBH_CALL_NONE;
    return (s == DBH_CALL_NONE) ? e : DBH_CALL_NONE;
}

}  // namespace dbh
