// dbh_occlude_core.h - the rule of `locate --occlude` (include/deepbinner_hip.h, "occlude"; DESIGN.md
// section 31): from a side's location to the three sets of read samples that are blanked - the span
// (OUT), everything the side's windows cover but the span (ONLY), an equally long stretch at the
// other end of what they cover (CTRL) - and from a plan to the blanked windows.  Blanking stores
// 0.0f, the value the zero pad of a short window has after normalisation; nothing is renormalised.
// The GPU's threads (dbh_occlude.hip) and the CPU models (dbh_occlude_plan_host,
// dbh_occlude_windows_host, same file; occlude_model_check.cpp) compile these lines.
//
// A window is walked in SLOTS of four positions: slot 0 is the head [0, head), slot k >= 1 covers
// [head + 4 (k - 1), head + 4 k), cut at L.  head is what brings the row's address to 16 bytes, so a
// whole slot is one 16-byte load and three 16-byte stores; where the four rows of a window (the
// input and the three variants) do not share their alignment, and in a cut slot, positions go one by
// one.  Which way a position went does not show in what is stored: copies and zeros.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/deepbinner_hip.h"

#if defined(__HIPCC__)
#define DBO_FN __host__ __device__ __forceinline__
#else
#define DBO_FN inline
#endif

namespace dbo {

constexpr int kVariants = 3;             // DBH_OCCLUDE_OUT, _ONLY, _CTRL

struct alignas(16) Four {
    float v[4];
};

struct Range {
    long long lo, hi;
};

// R: the read samples the side's `steps` windows cover
DBO_FN Range scanned(long long n, int steps, int L, int side) {
    const long long reach = (long long)(steps - 1) * (L / 2) + L;
    if (side == DBH_SIDE_START) return Range{0, reach < n ? reach : n};
    return Range{n - reach > 0 ? n - reach : 0, n};
}

// where window s begins in the read (the locate section's o); negative: zero pad in front
DBO_FN long long origin(long long n, int s, int L, int side) {
    const long long h = L / 2;
    return side == DBH_SIDE_START ? (long long)s * h : n - (long long)s * h - L;
}

DBO_FN float not_a_number() { return __builtin_nanf(""); }

// one read: the plan and the record with every "no result" field filled in
DBO_FN void plan_read(const dbh_location& loc, long long n, int steps, int L, int side,
                      dbh_occlude_plan* plan, dbh_occlusion* occ) {
    dbh_occlude_plan p;
    for (int v = 0; v < kVariants; ++v) p.first[v] = p.end[v] = 0;
    p.invert = p.valid = 0;
    p.reserved = 0;
    dbh_occlusion o;
    o.cls = loc.cls > 0 ? loc.cls : 0;
    o.p = not_a_number();
    for (int v = 0; v < kVariants; ++v) {
        o.variant[v].call = -1;
        o.variant[v].p = not_a_number();
    }
    o.ctrl_first = o.ctrl_end = -1;
    o.reserved[0] = o.reserved[1] = 0;
    const Range r = scanned(n, steps, L, side);
    // the span, held to R (a location of dbh_locate_dev lies inside it already)
    long long first = loc.first_sample, end = loc.end_sample;
    if (first < r.lo) first = r.lo;
    if (end > r.hi) end = r.hi;
    const long long m = end - first;
    if (loc.cls > 0 && m > 0) {
        p.first[DBH_OCCLUDE_OUT] = p.first[DBH_OCCLUDE_ONLY] = first;
        p.end[DBH_OCCLUDE_OUT] = p.end[DBH_OCCLUDE_ONLY] = end;
        p.invert = 1 << DBH_OCCLUDE_ONLY;
        p.valid = (1 << DBH_OCCLUDE_OUT) | (1 << DBH_OCCLUDE_ONLY);
        // the control: m samples at the end of R the span is further from (doubled midpoints)
        const bool span_in_front = first + end < r.lo + r.hi;
        const long long c_first = span_in_front ? r.hi - m : r.lo, c_end = c_first + m;
        if (c_end <= first || c_first >= end) {
            p.first[DBH_OCCLUDE_CTRL] = o.ctrl_first = c_first;
            p.end[DBH_OCCLUDE_CTRL] = o.ctrl_end = c_end;
            p.valid |= 1 << DBH_OCCLUDE_CTRL;
        }
    }
    *plan = p;
    *occ = o;
}

// is read sample t of a read of n samples blanked in variant v?  Never the pad (t outside [0, n)):
// it is 0 already.
DBO_FN bool blanked(const dbh_occlude_plan& p, int v, long long t, long long n) {
    if (t < 0 || t >= n) return false;
    const bool inside = t >= p.first[v] && t < p.end[v];
    return inside != (((p.invert >> v) & 1) != 0);
}

DBO_FN int row_slots(int L) { return (L + 3) / 4 + 1; }

// the positions in front of a row's first 16-byte boundary; L (no whole slot at all) where the four
// rows are not aligned alike
DBO_FN int row_head(const float* x, float* const* out, int L) {
    const uintptr_t a = (uintptr_t)x & 15;
    for (int v = 0; v < kVariants; ++v)
        if (((uintptr_t)out[v] & 15) != a) return L;
    return (int)(((16 - a) & 15) / 4);                       // (floats lie on 4 bytes)
}

// slot k of one window: x and out[v] are the window's rows, o its origin in the read
DBO_FN void blank_slot(const float* x, float* const* out, const dbh_occlude_plan& p, long long o,
                       long long n, int L, int k) {
    const int head = row_head(x, out, L);
    int a, b;
    if (head >= L) {                                          // (one by one, four to a slot)
        a = 4 * k;
        b = a + 4;
    } else {
        a = k == 0 ? 0 : head + 4 * (k - 1);
        b = k == 0 ? head : a + 4;
    }
    if (b > L) b = L;
    if (a >= b) return;
    if (head < L && b - a == 4) {
        const Four in = *(const Four*)(x + a);
        for (int v = 0; v < kVariants; ++v) {
            Four w = in;
            for (int j = 0; j < 4; ++j)
                if (blanked(p, v, o + a + j, n)) w.v[j] = 0.f;
            *(Four*)(out[v] + a) = w;
        }
        return;
    }
    for (int i = a; i < b; ++i)
        for (int v = 0; v < kVariants; ++v) out[v][i] = blanked(p, v, o + i, n) ? 0.f : x[i];
}

// one read's windows, serially: the CPU model
DBO_FN void blank_read(const float* x, float* const* out, const dbh_occlude_plan& p, long long n,
                       int steps, int L, int side) {
    const int slots = row_slots(L);
    for (int j = 0; j < steps * slots; ++j) {
        const int s = j / slots, k = j - s * slots;
        float* rows[kVariants];
        for (int v = 0; v < kVariants; ++v) rows[v] = out[v] + (size_t)s * L;
        blank_slot(x + (size_t)s * L, rows, p, origin(n, s, L, side), n, L, k);
    }
}

}  // namespace dbo
