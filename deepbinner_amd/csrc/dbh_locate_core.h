// dbh_locate_core.h - the rule of `locate` (include/deepbinner_hip.h, "locate"):
// from the evidence of a read's windows - [steps][cells][C] fp32, the post-ReLU conv1d_20 output whose
// mean over the cells is the class's logit - and the side's call c to WHERE the call comes from: the
// deciding window, its peak cell, the run of cells around the peak at half its height or more, that
// run's share of the window's evidence and the samples it covers.  The GPU's wave (dbh_locate.hip)
// and the CPU model (dbh_locate_host, same file; locate_model_check.cpp) compile these lines.
//
// The pick is a maximum with a total order - the higher value, among equals the lower flat index
// s * cells + p - so it does not depend on the order the cells are looked at: a wave's lanes and a
// serial loop agree.  It starts at (0, nothing): evidence is never negative, a NaN wins no '>' and
// equals nothing, and where no cell was taken (every one NaN) the pick is window 0, cell 0, peak 0.
#pragma once

#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/deepbinner_hip.h"

#if defined(__HIPCC__)
#define DBL_FN __host__ __device__ __forceinline__
#else
#define DBL_FN inline
#endif

namespace dbl {

constexpr int kCellSamples = 128;        // 2^7: one position of stage 7 (dbh_network.h: stage_lengths)
constexpr int kMaxCells = 128;           // len7 at L = 16384

struct Best {
    float v;
    int i;
};

DBL_FN Best best_none() { return Best{0.f, INT_MAX}; }

// does (v, i) come before (bv, bi)?  The one comparison of the pick.
DBL_FN bool wins(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

DBL_FN void consider(Best* b, float v, int i) {
    if (wins(v, i, b->v, b->i)) {
        b->v = v;
        b->i = i;
    }
}

DBL_FN dbh_location no_location() {
    dbh_location out;
    out.cls = 0;
    out.window = out.peak_cell = out.first_cell = out.last_cell = -1;
    out.peak = out.share = 0.f;
    out.reserved = 0;
    out.first_sample = out.end_sample = -1;
    return out;
}

DBL_FN bool call_locates(int c, int C) { return c > 0 && c < C; }

DBL_FN long long clip(long long v, long long n) { return v < 0 ? 0 : (v > n ? n : v); }

// ev: the read's evidence [steps][cells][C]; best: the pick over class c's steps * cells values;
// n: the read's samples.  Serial, over at most `cells` values of one window.
DBL_FN dbh_location finish(const float* ev, Best best, int c, int cells, int C, int L, int side,
                           long long n) {
    dbh_location out;
    const int flat = best.i == INT_MAX ? 0 : best.i;
    const int s = flat / cells, p = flat - s * cells;
    const float* row = ev + ((size_t)s * cells) * C + c;          // cell q at row[q * C]
    const float peak = best.i == INT_MAX ? 0.f : best.v;
    const float half = 0.5f * peak;
    int first = p, last = p;
    while (first > 0 && row[(size_t)(first - 1) * C] >= half) --first;
    while (last + 1 < cells && row[(size_t)(last + 1) * C] >= half) ++last;
    double part = 0.0, total = 0.0;
    for (int q = 0; q < cells; ++q) {
        const double v = (double)row[(size_t)q * C];
        total += v;                                              // (both sums in cell order)
        if (q >= first && q <= last) part += v;
    }
    out.cls = c;
    out.window = s;
    out.peak_cell = p;
    out.first_cell = first;
    out.last_cell = last;
    out.peak = peak;
    out.share = total == 0.0 ? 0.f : (float)(part / total);
    out.reserved = 0;
    // window positions [128 first, min(128 (last + 1), L)), from where the window begins in the read
    const long long h = L / 2;
    const long long o = side == DBH_SIDE_START ? (long long)s * h : n - (long long)s * h - L;
    const long long hi = (long long)kCellSamples * (last + 1);
    out.first_sample = clip(o + (long long)kCellSamples * first, n);
    out.end_sample = clip(o + (hi < L ? hi : (long long)L), n);
    if (out.end_sample < out.first_sample) out.end_sample = out.first_sample;
    return out;
}

// one read, serially: the CPU model
DBL_FN dbh_location locate_read(const float* ev, int c, int steps, int cells, int C, int L, int side,
                                long long n) {
    if (!call_locates(c, C)) return no_location();
    Best best = best_none();
    for (int i = 0; i < steps * cells; ++i) consider(&best, ev[(size_t)i * C + c], i);
    return finish(ev, best, c, cells, C, L, side, n);
}

}  // namespace dbl
