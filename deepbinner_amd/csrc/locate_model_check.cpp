// locate_model_check.cpp - the rule of `locate` (dbh_locate_core.h: the lines the GPU's wave and
// dbh_locate_host compile) under AddressSanitizer + UBSan, as a program of its own (make
// locate_asan): the planted cases of include/deepbinner_hip.h's "locate" section, each on evidence
// in a heap block of exactly steps * cells * C floats, so that a read one element outside it is
// caught.  Every case also states what the rule has to give.  No device, no Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dbh_locate_core.h"

namespace {

int failures = 0;

struct Case {
    int steps, cells, C, L, side, c;
    long long n;
    float* ev;                                             // exactly steps * cells * C floats
    Case(int steps_, int cells_, int C_, int L_, int side_, int c_, long long n_)
        : steps(steps_), cells(cells_), C(C_), L(L_), side(side_), c(c_), n(n_) {
        ev = (float*)std::calloc((size_t)steps * cells * C, sizeof(float));
        if (!ev) std::abort();
    }
    ~Case() { std::free(ev); }
    float& at(int s, int p) { return ev[((size_t)s * cells + p) * C + c]; }
    dbh_location run() const { return dbl::locate_read(ev, c, steps, cells, C, L, side, n); }
};

void expect(const char* what, const dbh_location& got, int window, int peak_cell, int first, int last,
            long long first_sample, long long end_sample) {
    const bool ok = got.window == window && got.peak_cell == peak_cell && got.first_cell == first &&
                    got.last_cell == last && got.first_sample == first_sample &&
                    got.end_sample == end_sample;
    if (!ok) {
        ++failures;
        std::printf("FAIL %s: window %d cell %d span %d-%d samples %lld-%lld\n", what, got.window,
                    got.peak_cell, got.first_cell, got.last_cell, (long long)got.first_sample,
                    (long long)got.end_sample);
    }
}

}  // namespace

int main() {
    {   // equal peaks in two windows: the lower window; equal cells: the lower cell
        Case k(3, 8, 13, 1024, DBH_SIDE_START, 5, 5000);
        k.at(2, 6) = k.at(1, 3) = k.at(1, 5) = 4.f;
        expect("equal peaks", k.run(), 1, 3, 3, 3, 512 + 384, 512 + 512);
    }
    {   // a neighbour at exactly half the peak is inside, one ulp below it outside
        Case k(2, 8, 2, 1024, DBH_SIDE_START, 1, 5000);
        k.at(0, 4) = 3.f;
        k.at(0, 3) = 1.5f;
        k.at(0, 5) = std::nextafterf(1.5f, 0.f);
        const dbh_location got = k.run();
        expect("half height", got, 0, 4, 3, 4, 384, 640);
        if (got.share != (float)(4.5 / (4.5 + (double)std::nextafterf(1.5f, 0.f)))) {
            ++failures;
            std::printf("FAIL share %.9g\n", got.share);
        }
    }
    {   // the peak in the first and in the last cell; one cell; the last class
        Case a(1, 8, 256, 1024, DBH_SIDE_START, 255, 4000), b(1, 8, 256, 1024, DBH_SIDE_START, 255, 4000);
        a.at(0, 0) = 1.f;
        b.at(0, 7) = 1.f;
        expect("first cell", a.run(), 0, 0, 0, 0, 0, 128);
        expect("last cell", b.run(), 0, 7, 7, 7, 896, 1024);
        Case one(24, 1, 2, 96, DBH_SIDE_END, 1, 700);
        one.at(23, 0) = 2.f;
        expect("one cell", one.run(), 23, 0, 0, 0, 0, 0);         // o = 700 - 23 * 48 - 96 < -96
    }
    {   // a span of the whole window; L = 1000: the last cell stops at L
        Case k(2, 8, 13, 1000, DBH_SIDE_START, 12, 3000);
        for (int p = 0; p < 8; ++p) k.at(1, p) = 1.f + 0.125f * p;
        expect("whole window", k.run(), 1, 7, 0, 7, 500, 1500);
    }
    {   // all-zero evidence: window 0, cell 0, every cell, share 0; no call: no location
        Case k(12, 63, 13, 8064, DBH_SIDE_START, 3, 100000);
        const dbh_location got = k.run();
        expect("all zero", got, 0, 0, 0, 62, 0, 8064);
        if (got.share != 0.f || got.peak != 0.f) ++failures;
        Case none(12, 63, 13, 8064, DBH_SIDE_START, 0, 100000);
        const dbh_location no = none.run();
        if (no.cls != 0 || no.window != -1 || no.first_sample != -1 || no.peak != 0.f) ++failures;
    }
    {   // a NaN is never the peak and ends a span
        Case k(1, 8, 13, 1024, DBH_SIDE_START, 1, 2000);
        k.at(0, 0) = NAN;
        k.at(0, 2) = 1.f;
        k.at(0, 1) = 1.f;
        k.at(0, 3) = NAN;
        expect("nan", k.run(), 0, 1, 1, 2, 128, 384);
        Case all(1, 2, 13, 256, DBH_SIDE_START, 1, 2000);
        all.at(0, 0) = all.at(0, 1) = NAN;
        expect("all nan", all.run(), 0, 0, 0, 0, 0, 128);
    }
    {   // an end-side read shorter than L: the span partly, then wholly, in the padding in front
        Case part(1, 8, 13, 1024, DBH_SIDE_END, 2, 300);            // o = -724: cell 5 is [-84, 44)
        part.at(0, 5) = 1.f;
        expect("partly padded", part.run(), 0, 5, 5, 5, 0, 44);
        Case whole(1, 8, 13, 1024, DBH_SIDE_END, 2, 300);           // cell 2 is [-468, -340)
        whole.at(0, 2) = 1.f;
        expect("wholly padded", whole.run(), 0, 2, 2, 2, 0, 0);
        Case behind(2, 8, 13, 1024, DBH_SIDE_START, 2, 300);        // start side, behind the read
        behind.at(1, 6) = 1.f;
        expect("behind the read", behind.run(), 1, 6, 6, 6, 300, 300);
        Case empty(1, 128, 4, 16384, DBH_SIDE_END, 3, 0);           // no samples at all
        empty.at(0, 127) = 1.f;
        expect("empty read", empty.run(), 0, 127, 127, 127, 0, 0);
    }
    std::printf("%s\n", failures ? "locate_model_check: FAILED" : "locate_model_check: ok");
    return failures ? 1 : 0;
}
