// dbh_front.h — the front rule of the scan (include/deepbinner_hip.h, "scan"),
// ONE text for dbh_scan.hip's windows_kernel and dbh_live.hip's front_kernel and end_front_kernel,
// whose windows have to agree to the bit: one wave takes the m samples present of a window, sums S and Q in int64 over its
// 64 lanes (dbh_wave::wave_sum), forms the exact D = m * Q - S * S, and writes the one fp64 expression
// per value, zeros behind it (or, `pad` zeros, in front).  Device functions only, as dbh_seam.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dbh_wave.h"

namespace dbh_front {

__device__ __forceinline__ float normalised(int16_t x, double mean, double sd) {
    const double d = (double)x - mean;
    return sd == 0.0 ? (float)d : (float)(d / sd);
}

// where in src sample j of a window lies: a plain row
struct Row {
    __device__ __forceinline__ int operator()(int j) const { return j; }
};

// All 64 lanes of a wave call it: src[0 .. m) -> out[0 .. L), the values at out[pad .. pad + m).
// `at` says where in src sample j lies: j itself (Row), or an index through a ring's wrap
// (dbh_live.hip's end windows).
template <typename At = Row>
__device__ __forceinline__ void window(const int16_t* __restrict__ src, long long m, int L, int pad,
                                       int lane, float* __restrict__ out, const At at = At{}) {
    long long s = 0, q = 0;
    for (int i = lane; i < m; i += 64) {
        const long long v = src[at(i)];
        s += v;
        q += v * v;
    }
    s = dbh_wave::wave_sum(s);
    q = dbh_wave::wave_sum(q);
    double mean = 0.0, sd = 0.0;
    if (m > 0) {
        const long long d = m * q - s * s;                     // m^2 * variance, exact: below 2^59
        mean = (double)s / (double)m;
        sd = sqrt((double)d) / (double)m;
    }
    for (int i = lane; i < L; i += 64) {
        const int j = i - pad;
        out[i] = (j >= 0 && j < m) ? normalised(src[at(j)], mean, sd) : 0.f;
    }
}

}  // namespace dbh_front
