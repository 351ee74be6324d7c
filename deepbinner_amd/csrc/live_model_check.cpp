// live_model_check.cpp - the rules of a live session (dbh_live_core.h: the lines the GPU's threads,
// the session's host mirror and dbh_live_plan_host compile) under AddressSanitizer + UBSan, as a
// program of its own (make live_asan): the planning rule at every seam length of the read and under
// every chunking, the append clip at cap - 1, cap and cap + 1, the decision rules on planted tracks.
// A channel's row is a heap block of exactly cap samples, a chunk one of exactly its length, a track
// one of exactly steps entries, so that an access one element outside is caught.  Every case also
// states what the rule has to give.  No device, no Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dbh_live_core.h"

namespace {

int failures = 0;

void fail(const char* what, long long a, long long b, long long c) {
    ++failures;
    std::printf("FAIL %s: %lld %lld %lld\n", what, a, b, c);
}

template <typename T>
T* exactly(size_t count) {          // a heap block of exactly count elements (one of size 0: 1 byte)
    T* p = (T*)std::malloc(count ? count * sizeof(T) : 1);
    if (!p) std::abort();
    return p;
}

// the ready windows, said again without the division
int ready_by_counting(long long n, bool ended, int L, int steps) {
    if (ended) return steps;
    int k = 0;
    while (k < steps && (long long)k * (L / 2) + L <= n) ++k;
    return k;
}

// One read of `length` samples (sample j holds (int16)(j * 7 + 1)) delivered in chunks of `size`,
// END with the last chunk or alone in an empty chunk behind it: the row must hold the read's first
// min(length, cap) samples, every push's windows must be the counted ones, none twice, all by END.
void deliver(int L, int steps, long long length, long long size, bool end_alone) {
    const dbh_live::Shape s = dbh_live::shape_of(L, steps * (L / 2), 0.5, 1, 0);
    int16_t* row = exactly<int16_t>((size_t)s.cap);
    dbh_live_result r = dbh_live::fresh_record();
    dbh_live::Gate g{0, 0};
    long long sent = 0;
    int next_window = 0;
    bool first = true, ended = false;
    while (!ended) {
        const long long len = length - sent < size ? length - sent : size;
        const bool last = sent + len >= length;
        unsigned flags = first ? DBH_LIVE_BEGIN : 0;
        if (last && !(end_alone && len > 0)) flags |= DBH_LIVE_END;
        int16_t* chunk = exactly<int16_t>((size_t)len);
        for (long long j = 0; j < len; ++j) chunk[j] = (int16_t)((sent + j) * 7 + 1);
        const dbh_live::Append a = dbh_live::append(&r, &g, flags, len, s);
        if (a.idle) fail("idle inside a read", L, length, size);
        if (a.at + a.keep > s.cap || a.keep > len || a.keep < 0) fail("clip", a.at, a.keep, s.cap);
        if (a.keep > 0) std::memcpy(row + a.at, chunk, (size_t)a.keep * sizeof(int16_t));
        std::free(chunk);
        sent += len;
        ended = (flags & DBH_LIVE_END) != 0;
        const int ready = ready_by_counting(sent, ended, L, steps);
        if (r.samples != sent) fail("n", r.samples, sent, size);
        if (a.first != next_window || a.first + a.count != ready) fail("ready", a.first, a.count, ready);
        for (int j = 0; j < a.count; ++j) {
            if (!dbh_live::may_fold(r, s)) fail("may_fold", L, length, j);
            // the window's samples lie inside what the row holds
            const long long lo = (long long)r.windows * s.h < sent ? (long long)r.windows * s.h : sent;
            const long long hi = (long long)r.windows * s.h + L < sent ? (long long)r.windows * s.h + L : sent;
            if (hi > s.cap || lo > hi) fail("window bounds", lo, hi, s.cap);
            long long sum = 0;
            for (long long t = lo; t < hi; ++t) sum += row[t];
            (void)sum;
            dbh_live::folded(&r, 0, 1.0, s);
        }
        next_window = ready;
        first = false;
    }
    if (r.windows != steps || r.status != DBH_LIVE_FINAL || r.final_call != 0 || g.open || !g.ended)
        fail("final", r.windows, r.status, r.final_call);
    const long long kept = length < s.cap ? length : s.cap;
    for (long long j = 0; j < kept; ++j)
        if (row[j] != (int16_t)(j * 7 + 1)) {
            fail("row", L, length, j);
            break;
        }
    std::free(row);
}

void expect(const char* what, const dbh_live_result& r, int status, int call, int final_call,
            int windows, int decided_windows, long long decided_samples) {
    if (r.status != status || r.call != call || r.final_call != final_call || r.windows != windows ||
        r.decided_windows != decided_windows || r.decided_samples != decided_samples) {
        ++failures;
        std::printf("FAIL %s: status %d call %d final %d windows %d decided %d at %lld\n", what,
                    r.status, r.call, r.final_call, r.windows, r.decided_windows,
                    (long long)r.decided_samples);
    }
}

// one channel through plan_channel: chunks of one window's worth each, then END
void decide(const char* what, double score_diff, int min_windows, unsigned flags, const int* best,
            const double* margin, int steps, int status, int call, int final_call, int windows,
            int decided_windows) {
    const int L = 96, h = 48;
    const dbh_live::Shape s = dbh_live::shape_of(L, steps * h, score_diff, min_windows, flags);
    const int n_chunks = steps + 1;
    long long* lengths = exactly<long long>((size_t)n_chunks);
    unsigned* chunk_flags = exactly<unsigned>((size_t)n_chunks);
    int* track_best = exactly<int>((size_t)steps);
    double* track_margin = exactly<double>((size_t)steps);
    dbh_live_result* results = exactly<dbh_live_result>((size_t)n_chunks);
    int* new_windows = exactly<int>((size_t)n_chunks);
    for (int i = 0; i < n_chunks; ++i) {
        lengths[i] = i == 0 ? L : (i < steps ? h : 0);
        chunk_flags[i] = (i == 0 ? DBH_LIVE_BEGIN : 0) | (i == steps ? DBH_LIVE_END : 0);
    }
    std::memcpy(track_best, best, (size_t)steps * sizeof(int));
    std::memcpy(track_margin, margin, (size_t)steps * sizeof(double));
    dbh_live::plan_channel(s, lengths, chunk_flags, n_chunks, track_best, track_margin, results,
                           new_windows);
    const long long at = decided_windows ? L + (long long)(decided_windows - 1) * h : 0;
    expect(what, results[n_chunks - 1], status, call, final_call, windows, decided_windows, at);
    std::free(lengths);
    std::free(chunk_flags);
    std::free(track_best);
    std::free(track_margin);
    std::free(results);
    std::free(new_windows);
}

}  // namespace

int main() {
    const int shapes[2][2] = {{96, 12}, {1024, 4}};                // (L, steps) of the tests' models
    for (const auto& shape : shapes) {
        const int L = shape[0], steps = shape[1], h = L / 2;
        const long long cap = (long long)steps * h + h;
        const long long lengths[] = {0, 1, h - 1, L - 1, L, L + 1, L + h - 1, L + h,
                                     cap - 1, cap, cap + 1, 2 * cap};
        const long long sizes[] = {1, h - 1, h, h + 1, 3 * h, 1600, 4 * cap};
        for (long long length : lengths)
            for (long long size : sizes) {
                if (size == 1 && L != 96) continue;                // (one sample per chunk: small L)
                deliver(L, steps, length, size, false);
                deliver(L, steps, length, size, true);
            }
    }
    {   // a chunk on a channel with no read open changes nothing
        const dbh_live::Shape s = dbh_live::shape_of(96, 576, 0.5, 1, 0);
        dbh_live_result r = dbh_live::fresh_record();
        dbh_live::Gate g{0, 0};
        const dbh_live::Append a = dbh_live::append(&r, &g, DBH_LIVE_END, 500, s);
        if (!a.idle || a.keep != 0 || a.count != 0 || r.samples != 0 || g.open || g.ended)
            fail("idle", a.idle, a.keep, r.samples);
    }
    {   // the decision rules on planted tracks, four windows
        const int b[4] = {0, 3, 3, 5};
        const double m[4] = {0.9, 0.5, 0.7, 0.6};
        decide("equality decides", 0.5, 1, 0, b, m, 4, DBH_LIVE_FINAL, 3, 5, 4, 2);
        decide("one ulp more does not", 0.5000000000000001, 1, 0, b, m, 4, DBH_LIVE_FINAL, 3, 5, 4, 3);
        decide("min_windows holds it back", 0.5, 3, 0, b, m, 4, DBH_LIVE_FINAL, 3, 5, 4, 3);
        decide("min_windows = steps", 0.5, 4, 0, b, m, 4, DBH_LIVE_FINAL, 5, 5, 4, 4);
        decide("stop on decision", 0.5, 1, DBH_LIVE_STOP_ON_DECISION, b, m, 4, DBH_LIVE_DECIDED, 3, -1, 2, 2);
        decide("never", 0.95, 1, 0, b, m, 4, DBH_LIVE_FINAL, 0, 0, 4, 0);
        const int zero[4] = {0, 0, 0, 0};
        decide("class 0 never decides", 0.5, 1, 0, zero, m, 4, DBH_LIVE_FINAL, 0, 0, 4, 0);
    }
    {   // what creation refuses
        const struct { int L, scan, min_windows; unsigned flags; bool ok; } cases[] = {
            {96, 576, 1, 0, true},  {96, 576, 12, 1, true}, {96, 576, 13, 0, false},
            {96, 576, 0, 0, false}, {96, 500, 1, 0, false}, {96, 0, 1, 0, false},
            {96, -48, 1, 0, false}, {97, 576, 1, 0, false}, {96, 576, 1, 2, false}};
        for (const auto& c : cases)
            if (dbh_live::shape_ok(dbh_live::shape_of(c.L, c.scan, 0.5, c.min_windows, c.flags),
                                   c.scan) != c.ok)
                fail("shape_ok", c.L, c.scan, c.min_windows);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("live_model_check: ok\n");
    return 0;
}
