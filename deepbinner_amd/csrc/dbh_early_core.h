// dbh_early_core.h - the live decision read out of a sweep's track (include/deepbinner_hip.h,
// "early tally"): what a live session with min_windows = m and score_diff = t
// would have called, at which window, in which push and with how many samples received, for EVERY
// m and t - integers and comparisons over the start track (best[k], margin[k]) and the read's
// length.  The GPU's threads (dbh_sweep.hip: early_kernel), the host entry (dbh_sweep_early_host)
// and the stand-alone check (early_model_check.cpp) compile these lines.
//
// L = input size, h = L / 2, steps windows, cap = (steps + 1) h, c = chunk_samples, len = the
// read's length.  A replay delivers the read in R = max(1, ceil(len / c)) pushes; push r (from 1)
// brings it to min(r c, len) samples and the last one carries END.  Window d is folded in push
// min(ceil((d h + L) / c), R): the first that holds its last sample, or the END.
#pragma once

#include <stdint.h>

#include "dbh_combine.h"

#if defined(__HIPCC__)
#define DBEARLY_FN __host__ __device__ __forceinline__
#else
#define DBEARLY_FN inline
#endif

namespace dbh_early {

constexpr int kColumns = 8;            // early[..][8]
constexpr int kMaxPushes = 4096;       // P above this is refused
enum Column { kDecided = 0, kAgree, kChanged, kLost, kLate, kWindows, kSamples, kLength };

// dbh_live::folded's comparison; a NaN margin leads nowhere
DBEARLY_FN bool lead(int best, double margin, double t) { return best != 0 && margin >= t; }

DBEARLY_FN long long ceil_div(long long a, long long b) { return a / b + (a % b != 0); }

// P: the push in which a read's last window is folded at the latest, ceil(cap / c)
DBEARLY_FN long long pushes_bound(int input_size, long long scan_size, long long chunk_samples) {
    return ceil_div(scan_size + input_size / 2, chunk_samples);
}

// the pushes of a read of len samples
DBEARLY_FN long long read_pushes(long long len, long long c) {
    const long long r = ceil_div(len, c);
    return r < 1 ? 1 : r;
}

// the push (from 1) in which window d of a read of len samples is folded
DBEARLY_FN long long push_of(int d, int input_size, long long len, long long c) {
    const long long q = ceil_div((long long)d * (input_size / 2) + input_size, c);
    const long long last = read_pushes(len, c);
    return q < last ? q : last;
}

// min(r c, len) without forming r c where it could pass int64: r < R means r c < len
DBEARLY_FN long long samples_at(long long r, long long len, long long c) {
    return r >= read_pushes(len, c) ? len : r * c;
}

// The first crossing at or behind window k, kept while k walks DOWN from steps - 1 to 0: behind
// step(k, ..) the state says what a session with min_windows = k + 1 decides.  One pass gives every m.
struct Crossing {
    int d, call;                         // d: the deciding window, -1 = never; call = best[d], 0 = never
};

DBEARLY_FN Crossing no_crossing() {
    Crossing x;
    x.d = -1;
    x.call = 0;
    return x;
}

DBEARLY_FN void step(Crossing* x, int k, int best, double margin, double t) {
    if (lead(best, margin, t)) {
        x->d = k;
        x->call = best;
    }
}

// What one read adds to the cell (m = k + 1, t): `x` behind step(k), final_call (the state behind
// step(steps - 1): a never-decided read has 0), the end side's call at t (both: combine under the
// three modes), label (< 0: unknown), len (has_len: lengths were given; push and samples are then
// counted).  The sink takes   calls(mode, column), early(column, value), window(d), push(r - 1).
template <class Sink>
DBEARLY_FN void count_read(Sink& sink, const Crossing& x, int k, int final_call, bool both,
                           int end_call, int label, int n_classes, bool has_len, long long len,
                           int input_size, long long c) {
    const int modes = both ? 3 : 1;
    for (int mode = 0; mode < modes; ++mode) {
        const int call = both ? dbh::combine_calls(x.call, end_call, mode) : x.call;
        if ((unsigned)call < (unsigned)n_classes) sink.calls(mode, call);
        if (label >= 0)
            sink.calls(mode, call == label ? n_classes : (call != 0 ? n_classes + 1 : n_classes + 2));
    }
    if (x.d < 0) return;
    sink.early(kDecided, 1);
    if (x.call == final_call) sink.early(kAgree, 1);
    else if (final_call != 0) sink.early(kChanged, 1);
    else sink.early(kLost, 1);
    if (x.d > k) sink.early(kLate, 1);
    sink.early(kWindows, (long long)x.d + 1);
    sink.window(x.d);
    if (!has_len) return;
    const long long r = push_of(x.d, input_size, len, c);
    sink.early(kSamples, samples_at(r, len, c));
    sink.early(kLength, len);
    sink.push(r - 1);
}

// the shape both tally entries and the host entry take
DBEARLY_FN bool shape_ok(long long n_reads, int steps, int n_classes, int input_size,
                         long long chunk_samples, int n_thresholds) {
    if (n_reads < 0 || steps < 1 || n_classes < 2 || n_classes > 256 || input_size < 2 ||
        input_size % 2 != 0 || chunk_samples < 1 || n_thresholds < 1)
        return false;
    return pushes_bound(input_size, (long long)steps * (input_size / 2), chunk_samples) <= kMaxPushes;
}

// The host's sink: the four arrays of one (m, t) cell, added to directly.
struct HostCell {
    int64_t *c, *e, *w, *p;
    int width;
    void calls(int mode, int column) { c[(long long)mode * width + column] += 1; }
    void early(int column, long long value) { e[column] += value; }
    void window(int d) { w[d] += 1; }
    void push(long long r) { if (p) p[r] += 1; }
};

// dbh_sweep_early_host: every read through the rule on the host, no device.  Arguments checked by
// the caller (shape_ok, the pointers, no negative length).
inline void tally_host(const int32_t* sb, const double* sm, const int32_t* eb, const double* em,
                       const int32_t* labels, const int64_t* lengths, long long n_reads, int steps,
                       int n_classes, int input_size, long long c, const double* thresholds,
                       int n_thresholds, int64_t* calls, int64_t* early, int64_t* windows,
                       int64_t* pushes) {
    const bool both = eb != nullptr;
    const int modes = both ? 3 : 1, width = n_classes + 3;
    const long long P = pushes_bound(input_size, (long long)steps * (input_size / 2), c);
    for (long long i = 0; i < n_reads; ++i) {
        const long long row = i * steps;
        for (int t = 0; t < n_thresholds; ++t) {
            const double threshold = thresholds[t];
            const int end_call =
                both && lead(eb[row + steps - 1], em[row + steps - 1], threshold) ? eb[row + steps - 1] : 0;
            Crossing x = no_crossing();
            int final_call = 0;
            for (int k = steps - 1; k >= 0; --k) {
                step(&x, k, sb[row + k], sm[row + k], threshold);
                if (k == steps - 1) final_call = x.call;
                const long long cell = (long long)k * n_thresholds + t;
                HostCell sink = {calls + cell * modes * width, early + cell * kColumns,
                                 windows + cell * steps, pushes ? pushes + cell * P : nullptr, width};
                count_read(sink, x, k, final_call, both, end_call, labels ? labels[i] : -1, n_classes,
                           lengths != nullptr, lengths ? lengths[i] : 0, input_size, c);
            }
        }
    }
}

}  // namespace dbh_early
