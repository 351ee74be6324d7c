// occlude_model_check.cpp - the rule of `locate --occlude` (dbh_occlude_core.h: the lines the GPU's
// threads and the two _host entries compile) under AddressSanitizer + UBSan, as a program of its own
// (make occlude_asan): the planted spans of include/deepbinner_hip.h's "occlude" section, and the
// windows of every case in heap blocks of exactly steps * L floats per row set, at every offset of
// the input and of the variants from a 16-byte boundary, so that a read or a store one element
// outside them, or a 16-byte access that is not aligned, is caught.  Every case is also held
// against a plain loop over positions.  No device, no Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dbh_occlude_core.h"

namespace {

int failures = 0;

void fail(const char* what, long long a = 0, long long b = 0) {
    ++failures;
    std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
}

dbh_location location(int cls, long long first, long long end) {
    dbh_location loc;
    std::memset(&loc, 0, sizeof loc);
    loc.cls = cls;
    loc.first_sample = first;
    loc.end_sample = end;
    return loc;
}

// a block of `floats` floats that begins `shift` floats behind a 16-byte boundary and ends where
// the heap block ends
struct Block {
    char* raw;
    float* p;
    Block(size_t floats, int shift) {
        // (malloc gives 16-byte alignment)
        raw = (char*)std::malloc((size_t)shift * sizeof(float) + floats * sizeof(float));
        if (!raw) std::abort();
        p = (float*)raw + shift;
    }
    ~Block() { std::free(raw); }
};

void check_windows(const char* what, const dbh_occlude_plan& plan, long long n, int steps, int L,
                   int side) {
    const size_t floats = (size_t)steps * L;
    for (int shift_in = 0; shift_in < 4; ++shift_in) {
        for (int shift_out = 0; shift_out < 4; ++shift_out) {
            std::vector<float> x(floats);
            for (size_t i = 0; i < floats; ++i) x[i] = 1.f + (float)(i % 251);
            Block in(floats, shift_in), o0(floats, shift_out), o1(floats, shift_out),
                o2(floats, (shift_out + (shift_in == 3 ? 1 : 0)) % 4);
            std::memcpy(in.p, x.data(), floats * sizeof(float));
            float* const out[3] = {o0.p, o1.p, o2.p};
            dbo::blank_read(in.p, out, plan, n, steps, L, side);
            for (int s = 0; s < steps; ++s) {
                const long long o = dbo::origin(n, s, L, side);
                for (int i = 0; i < L; ++i) {
                    const long long t = o + i;
                    for (int v = 0; v < 3; ++v) {
                        bool blank = t >= 0 && t < n && t >= plan.first[v] && t < plan.end[v];
                        if ((plan.invert >> v) & 1)
                            blank = t >= 0 && t < n && !(t >= plan.first[v] && t < plan.end[v]);
                        const float want = blank ? 0.f : x[(size_t)s * L + i];
                        if (out[v][(size_t)s * L + i] != want) {
                            fail(what, s * 100000LL + i, v);
                            return;
                        }
                    }
                }
            }
        }
    }
}

void expect(const char* what, int steps, int L, int side, long long n, const dbh_location& loc,
            int valid, long long first, long long end, long long ctrl_first, long long ctrl_end) {
    dbh_occlude_plan plan;
    dbh_occlusion occ;
    dbo::plan_read(loc, n, steps, L, side, &plan, &occ);
    const bool ok = plan.valid == valid && plan.first[0] == first && plan.end[0] == end &&
                    plan.first[1] == first && plan.end[1] == end && occ.ctrl_first == ctrl_first &&
                    occ.ctrl_end == ctrl_end && plan.invert == (valid ? 2 : 0) &&
                    occ.cls == (loc.cls > 0 ? loc.cls : 0) && std::isnan(occ.p) &&
                    plan.first[2] == (valid & 4 ? ctrl_first : 0) &&
                    plan.end[2] == (valid & 4 ? ctrl_end : 0);
    if (!ok) fail(what, plan.valid, occ.ctrl_first);
    for (int v = 0; v < 3; ++v)
        if (occ.variant[v].call != -1 || !std::isnan(occ.variant[v].p)) fail(what, v, -1);
    check_windows(what, plan, n, steps, L, side);
}

}  // namespace

int main() {
    const int S = DBH_SIDE_START, E = DBH_SIDE_END;
    // start side, 2 steps of 1024: R = [0, 1536)
    expect("first sample", 2, 1024, S, 5000, location(3, 0, 128), 7, 0, 128, 1408, 1536);
    expect("last sample", 2, 1024, E, 5000, location(3, 4872, 5000), 7, 4872, 5000, 3464, 3592);
    expect("partly padded", 1, 1024, E, 300, location(2, 0, 44), 7, 0, 44, 256, 300);
    expect("wholly padded", 1, 1024, E, 300, location(2, 0, 0), 0, 0, 0, -1, -1);
    expect("midpoint on R's", 2, 1024, S, 5000, location(3, 512, 1024), 7, 512, 1024, 0, 512);
    expect("midpoint below", 2, 1024, S, 5000, location(3, 511, 1023), 7, 511, 1023, 1024, 1536);
    expect("control touches", 2, 1024, S, 5000, location(3, 0, 768), 7, 0, 768, 768, 1536);
    expect("control overlaps by one", 2, 1024, S, 1535, location(3, 0, 768), 3, 0, 768, -1, -1);
    expect("all of R", 2, 1024, S, 5000, location(3, 0, 1536), 3, 0, 1536, -1, -1);
    expect("no call", 2, 1024, S, 5000, location(0, -1, -1), 0, 0, 0, -1, -1);
    expect("held to R", 2, 1024, S, 5000, location(3, -7, 99999), 3, 0, 1536, -1, -1);
    // the scalar head and tail of the 16-byte path (L = 98), one cell with positions in none (160),
    // the smallest window, reads shorter than a window, an empty read, twelve steps
    expect("L 98 start", 3, 98, S, 131, location(1, 40, 77), 7, 40, 77, 94, 131);
    expect("L 98 end", 12, 98, E, 400, location(1, 395, 400), 7, 395, 400, 0, 5);
    expect("L 98 short", 2, 98, E, 33, location(1, 3, 30), 3, 3, 30, -1, -1);
    expect("L 160", 12, 160, S, 2000, location(12, 128, 256), 7, 128, 256, 912, 1040);
    expect("L 96 one step", 1, 96, E, 96, location(1, 0, 48), 7, 0, 48, 48, 96);
    expect("empty read", 2, 96, S, 0, location(1, 0, 0), 0, 0, 0, -1, -1);
    expect("one sample", 1, 96, E, 1, location(1, 0, 1), 3, 0, 1, -1, -1);
    std::printf("%s\n", failures ? "occlude_model_check: FAILED" : "occlude_model_check: ok");
    return failures ? 1 : 0;
}
