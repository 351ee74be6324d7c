// dbh_live_core.h - the rules of a live session (include/deepbinner_hip.h, "live"; DESIGN.md section
// 32) that are integers and comparisons: which windows of a channel are ready, what of a chunk is
// stored, what a folded window does to the channel's record, and - for a pair session - the tail
// ring, the end windows and the end record; for a session with a yield policy, what a barcode has
// yielded, its level and the keep / eject action.  The GPU's threads (dbh_live.hip),
// the session's host mirror (dbh_api_live.hip: it knows every push's window count without reading the
// device back) and the CPU model (dbh_live_plan_host; live_model_check.cpp) compile these lines.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/deepbinner_hip.h"
#include "dbh_combine.h"

#if defined(__HIPCC__)
#define DBLIVE_FN __host__ __device__ __forceinline__
#else
#define DBLIVE_FN inline
#endif

namespace dbh_live {

// the shape of a session: L = input size, h = L / 2, cap = scan_size + h
struct Shape {
    int L, h, steps;
    long long cap;
    double score_diff;
    int min_windows;
    unsigned flags;                      // DBH_LIVE_STOP_ON_DECISION
};

DBLIVE_FN Shape shape_of(int input_size, int scan_size, double score_diff, int min_windows,
                         unsigned flags) {
    Shape s;
    s.L = input_size;
    s.h = input_size / 2;
    s.steps = s.h > 0 ? scan_size / s.h : 0;
    s.cap = (long long)scan_size + s.h;
    s.score_diff = score_diff;
    s.min_windows = min_windows;
    s.flags = flags;
    return s;
}

// what creation takes: even L, scan_size a positive multiple of h, 1 <= min_windows <= steps, the
// one flag bit, a threshold that is a number
DBLIVE_FN bool shape_ok(const Shape& s, int scan_size) {
    return s.L >= 2 && s.L % 2 == 0 && scan_size > 0 && s.steps >= 1 &&
           (long long)s.steps * s.h == scan_size && s.min_windows >= 1 && s.min_windows <= s.steps &&
           (s.flags & ~(unsigned)DBH_LIVE_STOP_ON_DECISION) == 0 && s.score_diff == s.score_diff;
}

// a channel apart from its record: is a read open, has it ended
struct Gate {
    int open, ended;
};

DBLIVE_FN dbh_live_result fresh_record() {
    dbh_live_result r;
    r.status = DBH_LIVE_IDLE;
    r.call = 0;
    r.final_call = -1;
    r.windows = 0;
    r.decided_windows = 0;
    r.best = 0;
    r.margin = 0.0;
    r.samples = 0;
    r.decided_samples = 0;
    return r;
}

// windows 0 .. ready - 1 of a read of n samples can run: k h + L <= n, or every one behind END
DBLIVE_FN int ready_windows(long long n, int ended, const Shape& s) {
    if (ended) return s.steps;
    if (n < s.L) return 0;
    const long long w = (n - s.L) / s.h + 1;
    return w < s.steps ? (int)w : s.steps;
}

// stores and runs nothing more
DBLIVE_FN bool stopped(const dbh_live_result& r, const Shape& s) {
    return r.status == DBH_LIVE_FINAL ||
           (r.status == DBH_LIVE_DECIDED && (s.flags & DBH_LIVE_STOP_ON_DECISION) != 0);
}

// What one chunk does: the first `keep` of its samples go to [at, at + keep) of the channel's
// buffer, and windows [first, first + count) have to run.  idle: nothing changed.
struct Append {
    long long at, keep;
    int first, count, idle;
};

// reset on BEGIN, append, set ended on END - in this order
DBLIVE_FN Append append(dbh_live_result* r, Gate* g, unsigned chunk_flags, long long length,
                        const Shape& s) {
    Append a;
    a.at = a.keep = 0;
    a.first = a.count = a.idle = 0;
    if (chunk_flags & DBH_LIVE_BEGIN) {
        *r = fresh_record();
        r->status = DBH_LIVE_PENDING;
        g->open = 1;
        g->ended = 0;
    } else if (!g->open) {
        a.idle = 1;
        return a;
    }
    const bool stop = stopped(*r, s);
    a.at = r->samples < s.cap ? r->samples : s.cap;            // the clip at cap
    a.keep = stop ? 0 : (length < s.cap - a.at ? length : s.cap - a.at);
    r->samples += length;
    if (chunk_flags & DBH_LIVE_END) {
        g->ended = 1;
        g->open = 0;
    }
    a.first = r->windows;
    a.count = stop ? 0 : ready_windows(r->samples, g->ended, s) - r->windows;
    return a;
}

// may window r->windows be folded?  (under STOP_ON_DECISION the fold ends behind the deciding one)
DBLIVE_FN bool may_fold(const dbh_live_result& r, const Shape& s) {
    return r.windows < s.steps && !stopped(r, s);
}

// window k = r->windows was folded and the prefix ends in (best, margin)
DBLIVE_FN void folded(dbh_live_result* r, int best, double margin, const Shape& s) {
    const int k = r->windows;
    r->windows = k + 1;
    r->best = best;
    r->margin = margin;
    const bool leads = best != 0 && margin >= s.score_diff;
    if (r->decided_windows == 0 && k + 1 >= s.min_windows && leads) {
        r->call = best;
        r->decided_windows = k + 1;
        r->decided_samples = r->samples;
        r->status = DBH_LIVE_DECIDED;
    }
    if (r->windows == s.steps) {
        r->status = DBH_LIVE_FINAL;
        r->final_call = leads ? best : 0;
    }
}

// One channel through n_chunks pushes on the host: window k folds to (track_best[k],
// track_margin[k]).  results[i]: the record behind push i; new_windows[i] (may be null): the
// windows that push folded.
DBLIVE_FN void plan_channel(const Shape& s, const long long* lengths, const unsigned* chunk_flags,
                            long long n_chunks, const int* track_best, const double* track_margin,
                            dbh_live_result* results, int* new_windows) {
    dbh_live_result r = fresh_record();
    Gate g;
    g.open = g.ended = 0;
    for (long long i = 0; i < n_chunks; ++i) {
        const Append a = append(&r, &g, chunk_flags[i], lengths[i], s);
        int done = 0;
        for (int j = 0; j < a.count && may_fold(r, s); ++j, ++done)
            folded(&r, track_best[r.windows], track_margin[r.windows], s);
        results[i] = r;
        if (a.idle) results[i].status = DBH_LIVE_IDLE;
        if (new_windows) new_windows[i] = done;
    }
}

// =============================================================================================
// The end side of a pair session.  `e` is the END model's shape: L_e, h_e,
// steps_e, cap_e = scan_size + h_e; its score_diff is the session's, min_windows 1, flags 0.
// =============================================================================================

// The tail ring: sample p of a read (counted from BEGIN) lives at ring[p % cap_e].  A chunk of
// `length` samples arriving at n stores its last `keep` = min(length, cap_e): the chunk's samples
// [from, length) go to ring positions at, at + 1, .. through the wrap - `head` of them up to the
// row's end, the others from ring[0] on.  Every chunk of an open read stores, whatever the start
// side's record says; BEGIN resets nothing here.
struct Tail {
    long long from, keep, at, head;
};

DBLIVE_FN Tail tail_store(long long n, long long length, const Shape& e) {
    Tail t;
    t.keep = length < e.cap ? length : e.cap;
    t.from = length - t.keep;
    t.at = (n + t.from) % e.cap;
    t.head = t.keep < e.cap - t.at ? t.keep : e.cap - t.at;
    return t;
}

// End window s of a read of n samples, known at END (call_batch with side == 'end',
// classify.py:343-357): samples [a, a + m), the values at out[pad .. L_e), zeros in front; sample
// a + j is ring[(at + j) % cap_e].  Window steps_e - 1 reaches back to n - cap_e at the most.
struct EndWindow {
    long long a, m, at;
    int pad;
};

DBLIVE_FN EndWindow end_window(long long n, int s, const Shape& e) {
    EndWindow w;
    const long long lo = n - ((long long)s * e.h + e.L), hi = n - (long long)s * e.h;
    w.a = lo > 0 ? lo : 0;
    w.m = (hi > 0 ? hi : 0) - w.a;
    w.at = w.a % e.cap;
    w.pad = e.L - (int)w.m;
    return w;
}

// what the start side gives combine_calls: the final call, or - stopped on a decision - the early one
DBLIVE_FN int start_side_call(const dbh_live_result& r) {
    return r.status == DBH_LIVE_FINAL ? r.final_call : r.call;
}

DBLIVE_FN dbh_live_end_result fresh_end_record() {
    dbh_live_end_result r;
    r.status = DBH_LIVE_IDLE;
    r.end_call = r.start_call = r.read_call = -1;
    r.end_best = 0;
    r.end_windows = 0;
    r.end_margin = 0.0;
    r.samples = 0;
    return r;
}

// The end record of a channel from its start record `r`, its gate and the end fold's record `f`
// (a dbh_live_result folded from fresh over the steps_e end windows: FINAL behind them).
DBLIVE_FN dbh_live_end_result end_record(const dbh_live_result& r, const Gate& g,
                                         const dbh_live_result& f, int combine_mode) {
    dbh_live_end_result o = fresh_end_record();
    if (r.status == DBH_LIVE_IDLE) return o;                   // no read yet
    o.status = DBH_LIVE_PENDING;
    o.samples = r.samples;
    if (!g.ended || f.status != DBH_LIVE_FINAL) return o;
    o.status = DBH_LIVE_FINAL;
    o.end_call = f.final_call;
    o.start_call = start_side_call(r);
    o.read_call = dbh::combine_calls(o.start_call, o.end_call, combine_mode);
    o.end_best = f.best;
    o.end_windows = f.windows;
    o.end_margin = f.margin;
    return o;
}

// One channel's ring and end windows through n_chunks pushes on the host.  Per chunk i:
// store[i] = (from, keep, at, head) of tail_store (zeros for an idle chunk), n_after[i] = n behind
// it; a chunk that carries END on an open read has ends[i] = 1 and windows[4 (i steps_e + s) ..] =
// (a, m, pad, at) of end window s (the other chunks' entries are not written).
DBLIVE_FN void plan_tail(const Shape& e, const long long* lengths,
                         const unsigned* chunk_flags, long long n_chunks, long long* store,
                         long long* n_after, int* ends, long long* windows) {
    dbh_live_result r = fresh_record();
    Gate g;
    g.open = g.ended = 0;
    for (long long i = 0; i < n_chunks; ++i) {
        const Append a = append(&r, &g, chunk_flags[i], lengths[i], e);    // (gate and n only)
        Tail t;
        t.from = t.keep = t.at = t.head = 0;
        if (!a.idle) t = tail_store(r.samples - lengths[i], lengths[i], e);
        store[4 * i] = t.from;
        store[4 * i + 1] = t.keep;
        store[4 * i + 2] = t.at;
        store[4 * i + 3] = t.head;
        n_after[i] = r.samples;
        ends[i] = !a.idle && (chunk_flags[i] & DBH_LIVE_END) != 0;
        if (!ends[i]) continue;
        for (int s = 0; s < e.steps; ++s) {
            const EndWindow w = end_window(r.samples, s, e);
            long long* out = windows + 4 * (i * e.steps + s);
            out[0] = w.a;
            out[1] = w.m;
            out[2] = w.pad;
            out[3] = w.at;
        }
    }
}

// =============================================================================================
// Yield policies: keep or eject a read by what its barcode has yielded so
// far.  Integers only - int64 wherever a yield or a level passes.
// =============================================================================================

// weight -1: always kept, outside the balance; 0: always ejected; 1 .. 1 << 20: balanced by share
DBLIVE_FN bool balanced(int weight) { return weight >= 1; }

// what dbh_live_set_policy takes: a weight per class of -1 .. 1 << 20, class 0 kept, slack >= 0,
// KEEP or EJECT for a read that ends undecided
DBLIVE_FN bool policy_ok(const int32_t* weight, int n_classes, long long slack, int undecided) {
    if (!weight || n_classes < 1 || slack < 0) return false;
    if (undecided != DBH_LIVE_ACTION_KEEP && undecided != DBH_LIVE_ACTION_EJECT) return false;
    if (weight[0] != -1) return false;
    for (int c = 0; c < n_classes; ++c)
        if (weight[c] < -1 || weight[c] > DBH_LIVE_MAX_WEIGHT) return false;
    return true;
}

// the class whose yield a chunk's record adds to: its call where the chunk carried END on an open
// read (an idle chunk's record reports IDLE), else -1
DBLIVE_FN int yield_class(const dbh_live_result& r, unsigned chunk_flags, int n_classes) {
    if (r.status == DBH_LIVE_IDLE || !(chunk_flags & DBH_LIVE_END)) return -1;
    return r.call >= 0 && r.call < n_classes ? r.call : -1;
}

// a balanced class's level: its yield by its share, rounded down (0 where the class is not balanced)
DBLIVE_FN long long level_of(long long yield_samples, int weight) {
    return balanced(weight) ? yield_samples / weight : 0;
}

// (no balanced class: floor_of's start value, turned into 0 by floor_from)
constexpr long long kNoLevel = INT64_MAX;
DBLIVE_FN long long floor_from(long long lowest) { return lowest == kNoLevel ? 0 : lowest; }

// the lowest level of the balanced classes, 0 if there is none (the kernel: a reduction instead)
DBLIVE_FN long long floor_of(const int32_t* weight, const int64_t* yield_samples, int n_classes) {
    long long lowest = kNoLevel;
    for (int c = 0; c < n_classes; ++c)
        if (balanced(weight[c])) {
            const long long level = level_of(yield_samples[c], weight[c]);
            if (level < lowest) lowest = level;
        }
    return floor_from(lowest);
}

DBLIVE_FN dbh_live_action standing_action(int action) {
    dbh_live_action a;
    a.action = action;
    a.reason = DBH_LIVE_REASON_NONE;
    a.klass = a.reserved = 0;
    a.level = a.floor = 0;
    return a;
}

// The action record of one chunk behind the push's yields.  `standing`: the channel's action in
// front of this push; BEGIN makes it NONE.  An action that stands, an idle chunk and a read that is
// neither decided nor FINAL report what stands and nothing else.
DBLIVE_FN dbh_live_action action_of(const dbh_live_result& r, unsigned chunk_flags, int standing,
                                    const int32_t* weight, int n_classes,
                                    const int64_t* yield_samples, long long floor, long long slack,
                                    int undecided) {
    if (chunk_flags & DBH_LIVE_BEGIN) standing = DBH_LIVE_ACTION_NONE;
    dbh_live_action a = standing_action(standing);
    if (r.status == DBH_LIVE_IDLE || standing != DBH_LIVE_ACTION_NONE) return a;
    if (r.decided_windows > 0) {
        const int c = r.call;
        if (c < 0 || c >= n_classes) return a;                 // (not a call of this model)
        a.klass = c;
        a.floor = floor;
        a.level = level_of(yield_samples[c], weight[c]);
        if (weight[c] == -1) {
            a.action = DBH_LIVE_ACTION_KEEP;
            a.reason = DBH_LIVE_REASON_WEIGHT_KEEP;
        } else if (weight[c] == 0) {
            a.action = DBH_LIVE_ACTION_EJECT;
            a.reason = DBH_LIVE_REASON_WEIGHT_EJECT;
        } else if (a.level - floor > slack) {                  // (level >= floor >= 0: no overflow)
            a.action = DBH_LIVE_ACTION_EJECT;
            a.reason = DBH_LIVE_REASON_OVER_LEVEL;
        } else {
            a.action = DBH_LIVE_ACTION_KEEP;
            a.reason = DBH_LIVE_REASON_BALANCED;
        }
    } else if (r.status == DBH_LIVE_FINAL) {
        a.floor = floor;
        a.action = undecided;
        a.reason = DBH_LIVE_REASON_UNDECIDED;
    }
    return a;
}

// One push on the host: the yields of its ENDs, then the floor, then every chunk's action - the
// order the two kernels run in.  channel_action [channels named], the two yields: in and out.
DBLIVE_FN void plan_policy_push(const int32_t* weight, int n_classes, long long slack, int undecided,
                                const int32_t* channels, const uint32_t* chunk_flags,
                                const dbh_live_result* records, long long n_chunks,
                                int32_t* channel_action, int64_t* yield_samples,
                                int64_t* yield_reads, dbh_live_action* actions) {
    for (long long i = 0; i < n_chunks; ++i) {
        const int c = yield_class(records[i], chunk_flags[i], n_classes);
        if (c < 0) continue;
        yield_samples[c] += records[i].samples;
        yield_reads[c] += 1;
    }
    const long long floor = floor_of(weight, yield_samples, n_classes);
    for (long long i = 0; i < n_chunks; ++i) {
        actions[i] = action_of(records[i], chunk_flags[i], channel_action[channels[i]], weight,
                               n_classes, yield_samples, floor, slack, undecided);
        if (records[i].status != DBH_LIVE_IDLE) channel_action[channels[i]] = actions[i].action;
    }
}

}  // namespace dbh_live
