// live_model_check.cpp - the rules of a live session (dbh_live_core.h: the lines the GPU's threads,
// the session's host mirror and dbh_live_plan_host compile) under AddressSanitizer + UBSan, as a
// program of its own (make live_asan): the planning rule at every seam length of the read and under
// every chunking, the append clip at cap - 1, cap and cap + 1, the decision rules on planted tracks.
// A channel's row is a heap block of exactly cap samples, a chunk one of exactly its length, a track
// one of exactly steps entries, so that an access one element outside is caught.  Every case also
// states what the rule has to give.  The pair sessions' rules too: the tail ring (tail_store) and
// the end windows (end_window) at every read length 0 .. 3 cap_e + 7 of L = 96 under a set of
// chunkings - a ring of exactly cap_e samples and beside it who wrote each of them, so that every
// position an end window reads at END is one this read wrote and holds the right sample -, the
// host plan entry's form of the same (plan_tail), the end record and the combine rule.  The yield
// policy too (policy_ok, yield_class, level_of, floor_of, action_of, plan_policy_push): random push
// sequences on 1 to 300 channels and 2 to 256 classes with yields up to 2^50, in heap blocks of
// exactly the sizes given, against a plain loop written here.  No device, no Python.
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

// ---- the pair sessions' rules ----------------------------------------------------------------------
int16_t sample_of(long long read, long long p) { return (int16_t)(p * 7 + 1 + read * 131); }

// One channel, ring and who-wrote-it of exactly cap_e entries.  A read of `length` samples is
// delivered in chunks of the sizes `sizes[0 .. n_sizes)` in turn (0: an empty chunk), END with the
// last chunk or alone behind it.  stopped: the start side's record says DECIDED under
// STOP_ON_DECISION from the first chunk on - the ring must go on all the same.
struct RingChannel {
    dbh_live::Shape start, e;
    int16_t* ring;
    long long* who;                      // the position p of the sample at ring[i], and
    long long* whose;                    // the read that wrote it
    dbh_live_result r;
    dbh_live::Gate g;
    long long read;
};

void ring_push(RingChannel& c, long long len, unsigned flags, long long sent, bool stopped) {
    int16_t* chunk = exactly<int16_t>((size_t)len);
    if (flags & DBH_LIVE_BEGIN) ++c.read;
    for (long long j = 0; j < len; ++j) chunk[j] = sample_of(c.read, sent + j);
    const dbh_live::Append a = dbh_live::append(&c.r, &c.g, flags, len, c.start);
    if (stopped && !a.idle) {
        c.r.status = DBH_LIVE_DECIDED;
        c.r.call = 3;
        c.r.decided_windows = 1;
    }
    if (!a.idle) {
        const dbh_live::Tail t = dbh_live::tail_store(c.r.samples - len, len, c.e);
        if (t.keep < 0 || t.keep > len || t.keep > c.e.cap || t.from != len - t.keep || t.at < 0 ||
            t.at >= c.e.cap || t.head < 0 || t.head > t.keep || t.at + t.head > c.e.cap ||
            t.keep - t.head > t.at)
            fail("tail", t.at, t.keep, t.head);
        for (long long j = 0; j < t.keep; ++j) {                   // two spans at the wrap
            const long long i = j < t.head ? t.at + j : j - t.head;
            c.ring[i] = chunk[t.from + j];
            c.who[i] = c.r.samples - len + t.from + j;
            c.whose[i] = c.read;
        }
    } else if (len > 0 && (flags & DBH_LIVE_BEGIN)) {
        fail("idle with BEGIN", len, flags, 0);
    }
    std::free(chunk);
    if (a.idle || !(flags & DBH_LIVE_END)) return;
    const long long n = c.r.samples;
    for (int s = 0; s < c.e.steps; ++s) {
        const dbh_live::EndWindow w = dbh_live::end_window(n, s, c.e);
        const long long lo = n - ((long long)s * c.e.h + c.e.L), hi = n - (long long)s * c.e.h;
        if (w.a != (lo > 0 ? lo : 0) || w.a + w.m != (hi > 0 ? hi : 0) || w.m < 0 || w.m > c.e.L ||
            w.pad != c.e.L - w.m || w.at != w.a % c.e.cap || w.a < n - c.e.cap)
            fail("end window", n, s, w.a);
        for (long long j = 0; j < w.m; ++j) {
            const long long i = w.at + j < c.e.cap ? w.at + j : w.at + j - c.e.cap;
            if (c.whose[i] != c.read || c.who[i] != w.a + j || c.ring[i] != sample_of(c.read, w.a + j)) {
                fail("ring read", n, s, j);
                break;
            }
        }
    }
}

void deliver_tail(RingChannel& c, long long length, const long long* sizes, int n_sizes,
                  bool end_alone, bool stopped) {
    long long sent = 0;
    bool first = true, ended = false;
    for (int k = 0; !ended; ++k) {
        const long long size = sizes[k % n_sizes];
        const long long len = length - sent < size ? length - sent : size;
        const bool last = sent + len >= length && (size > 0 || length == 0 || k > 64);
        unsigned flags = first ? DBH_LIVE_BEGIN : 0;
        if (last && !(end_alone && len > 0)) flags |= DBH_LIVE_END;
        ring_push(c, len, flags, sent, stopped);
        sent += len;
        ended = (flags & DBH_LIVE_END) != 0;
        first = false;
    }
    if (c.r.samples != length || c.g.open || !c.g.ended) fail("tail n", c.r.samples, length, 0);
}

void tail_rules() {
    const int L = 96, steps = 12, h = L / 2;
    const unsigned stop = DBH_LIVE_STOP_ON_DECISION;
    RingChannel c;
    c.start = dbh_live::shape_of(L, steps * h, 0.5, 1, stop);
    c.e = dbh_live::shape_of(L, steps * h, 0.5, 1, 0);
    const long long cap = c.e.cap;
    c.ring = exactly<int16_t>((size_t)cap);
    c.who = exactly<long long>((size_t)cap);
    c.whose = exactly<long long>((size_t)cap);
    for (long long i = 0; i < cap; ++i) {
        c.ring[i] = 0;
        c.who[i] = c.whose[i] = -1;
    }
    c.r = dbh_live::fresh_record();
    c.g = dbh_live::Gate{0, 0};
    c.read = 0;
    // one channel all the way: every read follows another one's leftovers in the ring
    const long long whole[] = {4 * cap}, one[] = {1}, below[] = {h - 1}, half[] = {h}, above[] = {h + 1};
    const long long at_cap[] = {cap, h}, over_cap[] = {cap + 1, 7}, long_one[] = {2 * cap + 3, 5};
    const long long empties[] = {0, h + 5, 0, 0, 1600}, sequencer[] = {1600};
    const struct { const long long* sizes; int n; } chunkings[] = {
        {whole, 1}, {one, 1}, {below, 1}, {half, 1}, {above, 1}, {at_cap, 2}, {over_cap, 2},
        {long_one, 2}, {empties, 5}, {sequencer, 1}};
    for (long long length = 0; length <= 3 * cap + 7; ++length)
        for (const auto& ch : chunkings) {
            if (ch.sizes == one && length % 5 != 0 && length > L + 2) continue;   // (keeps it quick)
            deliver_tail(c, length, ch.sizes, ch.n, false, false);
            deliver_tail(c, length, ch.sizes, ch.n, true, length % 2 == 0);
        }
    {   // BEGIN inside a read, BEGIN|END on an empty chunk, a chunk with no read open
        ring_push(c, 2 * cap + 9, DBH_LIVE_BEGIN, 0, false);
        ring_push(c, 5, DBH_LIVE_BEGIN, 0, false);
        ring_push(c, 3, DBH_LIVE_END, 5, false);
        if (c.r.samples != 8) fail("BEGIN inside a read", c.r.samples, 8, 0);
        ring_push(c, 0, DBH_LIVE_BEGIN | DBH_LIVE_END, 0, false);
        if (c.r.samples != 0 || c.g.open) fail("BEGIN|END", c.r.samples, c.g.open, 0);
        const long long before = c.who[0];
        ring_push(c, 100, DBH_LIVE_END, 0, false);
        if (c.who[0] != before || c.r.samples != 0) fail("idle stores", c.who[0], before, 0);
    }
    {   // plan_tail, the host entry's form, against the same rules chunk by chunk
        const long long lengths[] = {2 * cap + 5, 0, 7, 100, 30, 0};
        const unsigned flags[] = {DBH_LIVE_BEGIN, DBH_LIVE_END, 0, DBH_LIVE_BEGIN, 0, DBH_LIVE_END};
        const int n = 6;
        long long* store = exactly<long long>(4 * n);
        long long* n_after = exactly<long long>(n);
        int* ends = exactly<int>(n);
        long long* windows = exactly<long long>((size_t)4 * n * steps);
        dbh_live::plan_tail(c.e, lengths, flags, n, store, n_after, ends, windows);
        const long long want_n[] = {2 * cap + 5, 2 * cap + 5, 2 * cap + 5, 100, 130, 130};
        const int want_ends[] = {0, 1, 0, 0, 0, 1};
        for (int i = 0; i < n; ++i)
            if (n_after[i] != want_n[i] || ends[i] != want_ends[i]) fail("plan_tail", i, n_after[i], ends[i]);
        if (store[0] != cap + 5 || store[1] != cap || store[2] != 5 || store[3] != cap - 5)
            fail("plan_tail store", store[0], store[1], store[2]);
        if (store[8] || store[9] || store[10] || store[11]) fail("plan_tail idle", 2, store[9], 0);
        const dbh_live::EndWindow w = dbh_live::end_window(130, 1, c.e);
        const long long* got = windows + 4 * (5 * steps + 1);
        if (got[0] != w.a || got[1] != w.m || got[2] != w.pad || got[3] != w.at || w.a != 0 || w.m != 82)
            fail("plan_tail window", got[0], got[1], got[2]);
        std::free(store);
        std::free(n_after);
        std::free(ends);
        std::free(windows);
    }
    std::free(c.ring);
    std::free(c.who);
    std::free(c.whose);
}

void end_records() {
    // the combine rule: the reference's truth table (tests/test_combine_calls.py:27-51)
    const struct { int mode, s, e, want; } table[] = {
        {DBH_REQUIRE_EITHER, 1, 2, 0}, {DBH_REQUIRE_EITHER, 4, 4, 4}, {DBH_REQUIRE_EITHER, 5, 0, 5},
        {DBH_REQUIRE_EITHER, 0, 7, 7}, {DBH_REQUIRE_EITHER, 0, 0, 0}, {DBH_REQUIRE_START, 1, 2, 0},
        {DBH_REQUIRE_START, 4, 4, 4},  {DBH_REQUIRE_START, 5, 0, 5},  {DBH_REQUIRE_START, 0, 7, 0},
        {DBH_REQUIRE_START, 0, 0, 0},  {DBH_REQUIRE_BOTH, 1, 2, 0},   {DBH_REQUIRE_BOTH, 4, 4, 4},
        {DBH_REQUIRE_BOTH, 5, 0, 0},   {DBH_REQUIRE_BOTH, 0, 7, 0},   {DBH_REQUIRE_BOTH, 0, 0, 0}};
    for (const auto& row : table)
        if (dbh::combine_calls(row.s, row.e, row.mode) != row.want) fail("combine", row.mode, row.s, row.e);
    dbh_live_result r = dbh_live::fresh_record(), f = dbh_live::fresh_record();
    dbh_live::Gate g{0, 0};
    dbh_live_end_result o = dbh_live::end_record(r, g, f, DBH_REQUIRE_EITHER);
    if (o.status != DBH_LIVE_IDLE || o.end_call != -1 || o.start_call != -1 || o.read_call != -1 ||
        o.end_windows != 0 || o.samples != 0)
        fail("end record, no read", o.status, o.end_call, o.samples);
    r.status = DBH_LIVE_DECIDED;                                   // open, decided early, not ended
    r.call = 3;
    r.samples = 5000;
    g.open = 1;
    f.status = DBH_LIVE_FINAL;                                     // (the read before this one)
    f.final_call = 9;
    o = dbh_live::end_record(r, g, f, DBH_REQUIRE_EITHER);
    if (o.status != DBH_LIVE_PENDING || o.end_call != -1 || o.read_call != -1 || o.samples != 5000)
        fail("end record, pending", o.status, o.end_call, o.samples);
    g.open = 0;                                                    // ended behind a stop: the early call
    g.ended = 1;
    f.final_call = 0;
    f.best = 4;
    f.windows = 12;
    f.margin = 0.25;
    o = dbh_live::end_record(r, g, f, DBH_REQUIRE_EITHER);
    if (o.status != DBH_LIVE_FINAL || o.start_call != 3 || o.end_call != 0 || o.read_call != 3 ||
        o.end_best != 4 || o.end_windows != 12 || o.end_margin != 0.25)
        fail("end record, stopped", o.start_call, o.end_call, o.read_call);
    r.status = DBH_LIVE_FINAL;                                     // FINAL: the final call goes in
    r.final_call = 0;
    f.final_call = 7;
    o = dbh_live::end_record(r, g, f, DBH_REQUIRE_EITHER);
    if (o.start_call != 0 || o.end_call != 7 || o.read_call != 7) fail("end record, final", o.start_call, o.end_call, o.read_call);
    o = dbh_live::end_record(r, g, f, DBH_REQUIRE_START);
    if (o.read_call != 0) fail("end record, require start", o.start_call, o.end_call, o.read_call);
}

// ---- the yield policy ---------------------------------------------------------------------------
unsigned long long rng_state = 34;
unsigned long long draw(unsigned long long below) {                 // (a 64-bit LCG's high bits)
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return below ? (rng_state >> 20) % below : 0;
}

// One random session: n_pushes pushes of up to n_channels chunks through plan_policy_push, and the
// same said again as a plain loop - yields first, then the lowest level, then chunk by chunk.
void policy_session(int n_channels, int n_classes, int n_pushes) {
    int32_t* weight = exactly<int32_t>((size_t)n_classes);
    const int kinds[] = {-1, 0, 1, 2, 7, 1 << 20};
    for (int c = 0; c < n_classes; ++c) weight[c] = c ? kinds[draw(6)] : -1;
    const long long slack = draw(3) == 0 ? 0 : (draw(2) ? 5 : 1LL << 40);
    const int undecided = draw(2) ? DBH_LIVE_ACTION_KEEP : DBH_LIVE_ACTION_EJECT;
    if (!dbh_live::policy_ok(weight, n_classes, slack, undecided)) fail("policy_ok", n_classes, slack, 0);
    int64_t* ys = exactly<int64_t>((size_t)n_classes);
    int64_t* yr = exactly<int64_t>((size_t)n_classes);
    int64_t* want_ys = exactly<int64_t>((size_t)n_classes);
    int64_t* want_yr = exactly<int64_t>((size_t)n_classes);
    for (int c = 0; c < n_classes; ++c) {
        ys[c] = want_ys[c] = draw(4) ? (int64_t)draw((1ULL << 50) + 1) : (int64_t)(1LL << 50);
        yr[c] = want_yr[c] = (int64_t)draw(1000);
    }
    int32_t* standing = exactly<int32_t>((size_t)n_channels);
    int32_t* want_standing = exactly<int32_t>((size_t)n_channels);
    for (int ch = 0; ch < n_channels; ++ch) standing[ch] = want_standing[ch] = DBH_LIVE_ACTION_NONE;
    std::vector<int> order((size_t)n_channels);
    for (int ch = 0; ch < n_channels; ++ch) order[(size_t)ch] = ch;
    for (int p = 0; p < n_pushes; ++p) {
        const size_t n = (size_t)draw((unsigned long long)n_channels + 1);
        for (size_t i = 0; i < n; ++i)                              // n distinct channels
            std::swap(order[i], order[i + (size_t)draw((unsigned long long)n_channels - i)]);
        int32_t* channels = exactly<int32_t>(n);
        uint32_t* flags = exactly<uint32_t>(n);
        dbh_live_result* records = exactly<dbh_live_result>(n);
        dbh_live_action* actions = exactly<dbh_live_action>(n);
        for (size_t i = 0; i < n; ++i) {
            channels[i] = order[i];
            flags[i] = (uint32_t)draw(4);
            dbh_live_result r = dbh_live::fresh_record();
            r.status = (int32_t)draw(4);
            r.samples = (int64_t)draw(1ULL << 34);
            if (r.status != DBH_LIVE_PENDING && draw(4)) {
                r.call = (int32_t)draw((unsigned long long)n_classes);
                r.decided_windows = r.call ? 1 : 0;
            }
            records[i] = r;
        }
        dbh_live::plan_policy_push(weight, n_classes, slack, undecided, channels, flags, records,
                                   (long long)n, standing, ys, yr, actions);
        // ... and plainly
        for (size_t i = 0; i < n; ++i)
            if ((flags[i] & DBH_LIVE_END) && records[i].status != DBH_LIVE_IDLE) {
                want_ys[records[i].call] += records[i].samples;
                want_yr[records[i].call] += 1;
            }
        bool any = false;
        long long floor = 0;
        for (int c = 0; c < n_classes; ++c)
            if (weight[c] >= 1 && (!any || want_ys[c] / weight[c] < floor)) {
                floor = want_ys[c] / weight[c];
                any = true;
            }
        for (size_t i = 0; i < n; ++i) {
            const dbh_live_result& r = records[i];
            int was = (flags[i] & DBH_LIVE_BEGIN) ? DBH_LIVE_ACTION_NONE : want_standing[channels[i]];
            dbh_live_action w{was, 0, 0, 0, 0, 0};
            if (r.status != DBH_LIVE_IDLE && was == DBH_LIVE_ACTION_NONE) {
                if (r.decided_windows > 0) {
                    const int wt = weight[r.call];
                    const long long level = wt >= 1 ? want_ys[r.call] / wt : 0;
                    w.klass = r.call;
                    w.level = level;
                    w.floor = floor;
                    if (wt == -1) { w.action = DBH_LIVE_ACTION_KEEP; w.reason = DBH_LIVE_REASON_WEIGHT_KEEP; }
                    else if (wt == 0) { w.action = DBH_LIVE_ACTION_EJECT; w.reason = DBH_LIVE_REASON_WEIGHT_EJECT; }
                    else if (level > floor + slack) { w.action = DBH_LIVE_ACTION_EJECT; w.reason = DBH_LIVE_REASON_OVER_LEVEL; }
                    else { w.action = DBH_LIVE_ACTION_KEEP; w.reason = DBH_LIVE_REASON_BALANCED; }
                } else if (r.status == DBH_LIVE_FINAL) {
                    w.action = undecided;
                    w.reason = DBH_LIVE_REASON_UNDECIDED;
                    w.floor = floor;
                }
            }
            if (r.status != DBH_LIVE_IDLE) want_standing[channels[i]] = w.action;
            if (std::memcmp(&w, &actions[i], sizeof w) != 0)
                fail("action", p, (long long)i, actions[i].action * 10 + w.action);
        }
        if (std::memcmp(ys, want_ys, (size_t)n_classes * sizeof(int64_t)) != 0 ||
            std::memcmp(yr, want_yr, (size_t)n_classes * sizeof(int64_t)) != 0)
            fail("yields", p, n_classes, n_channels);
        if (std::memcmp(standing, want_standing, (size_t)n_channels * sizeof(int32_t)) != 0)
            fail("standing actions", p, n_classes, n_channels);
        std::free(channels);
        std::free(flags);
        std::free(records);
        std::free(actions);
    }
    for (void* q : {(void*)weight, (void*)ys, (void*)yr, (void*)want_ys, (void*)want_yr,
                    (void*)standing, (void*)want_standing})
        std::free(q);
}

}  // namespace

int main() {
    tail_rules();
    end_records();
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
    {   // the yield policy: the sizes at the edges, then random ones
        const int edges[][2] = {{1, 2}, {300, 256}, {1, 256}, {300, 2}, {64, 13}};
        for (const auto& e : edges) policy_session(e[0], e[1], 12);
        for (int trial = 0; trial < 60; ++trial)
            policy_session(1 + (int)draw(300), 2 + (int)draw(255), 1 + (int)draw(20));
        // what set_policy refuses
        const int32_t good[3] = {-1, 1, 0}, kept0[3] = {0, 1, 0}, low[3] = {-1, -2, 0},
                      high[3] = {-1, (1 << 20) + 1, 0};
        if (!dbh_live::policy_ok(good, 3, 0, DBH_LIVE_ACTION_KEEP)) fail("policy_ok good", 0, 0, 0);
        if (dbh_live::policy_ok(kept0, 3, 0, DBH_LIVE_ACTION_KEEP) ||
            dbh_live::policy_ok(low, 3, 0, DBH_LIVE_ACTION_KEEP) ||
            dbh_live::policy_ok(high, 3, 0, DBH_LIVE_ACTION_KEEP) ||
            dbh_live::policy_ok(good, 3, -1, DBH_LIVE_ACTION_KEEP) ||
            dbh_live::policy_ok(good, 3, 0, DBH_LIVE_ACTION_NONE) ||
            dbh_live::policy_ok(good, 0, 0, DBH_LIVE_ACTION_KEEP) ||
            dbh_live::policy_ok(nullptr, 3, 0, DBH_LIVE_ACTION_KEEP))
            fail("policy_ok refuses", 0, 0, 0);
        // a yield_class outside the model's classes adds nothing; level_of of an unbalanced class is 0
        dbh_live_result r = dbh_live::fresh_record();
        r.status = DBH_LIVE_FINAL;
        r.call = 3;
        if (dbh_live::yield_class(r, DBH_LIVE_END, 3) != -1 || dbh_live::yield_class(r, DBH_LIVE_END, 4) != 3 ||
            dbh_live::yield_class(r, DBH_LIVE_BEGIN, 4) != -1)
            fail("yield_class", 0, 0, 0);
        if (dbh_live::level_of(1LL << 50, -1) != 0 || dbh_live::level_of(1LL << 50, 0) != 0 ||
            dbh_live::level_of((1LL << 50) + 7, 1 << 20) != (1LL << 30))
            fail("level_of", 0, 0, 0);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("live_model_check: ok\n");
    return 0;
}
