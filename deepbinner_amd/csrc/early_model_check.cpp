// early_model_check.cpp - the early tally's rule (dbh_early_core.h: the lines the GPU's threads and
// dbh_sweep_early_host compile) under AddressSanitizer + UBSan, as a program of its own (make
// early_asan): tally_host over random tracks whose margins sit on the thresholds, at every shape of
// a list - one step and many, 2 to 256 classes, chunks of one sample, of cap and of 2^62, reads of
// no sample and of 2^33 + 1 - with every input and every one of the four arrays a heap block of
// exactly its size, so that an access one element outside is caught, against a plain loop written
// here: per read, per setting, the first leading window from m - 1 on by a forward search, the push
// by counting pushes.  No device, no Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "dbh_early_core.h"

namespace {

int failures = 0;

template <typename T>
T* exactly(size_t count) {          // a heap block of exactly count elements (one of size 0: 1 byte)
    T* p = (T*)std::calloc(count ? count * sizeof(T) : 1, 1);
    if (!p) std::abort();
    return p;
}

unsigned long long state = 0x9E3779B97F4A7C15ull;
unsigned long long draw() {         // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return state * 0x2545F4914F6CDD1Dull;
}

int combine_plain(int s, int e, int mode) {             // classify.py:298-322, said again
    if (s == e) return s;
    if (mode == 2 || (mode == 1 && e != 0)) return 0;
    if (e == 0) return s;
    return s == 0 ? e : 0;
}

struct Case {
    int L, steps, C, T;
    long long n, c;
    bool both, labelled, lengths;
};

void run(const Case& k) {
    const int h = k.L / 2, width = k.C + 3, modes = k.both ? 3 : 1;
    const long long cap = (long long)(k.steps + 1) * h;
    const long long P = dbh_early::pushes_bound(k.L, (long long)k.steps * h, k.c);
    if (P != (cap + (k.c - 1)) / k.c && k.c < (1ll << 40)) ++failures;
    const size_t per_side = (size_t)k.n * k.steps, cells = (size_t)k.steps * k.T;
    double* thresholds = exactly<double>((size_t)k.T);
    for (int t = 0; t < k.T; ++t) thresholds[t] = (t + 1.0) / (k.T + 1.0);
    int32_t* best[2];
    double* margin[2];
    for (int side = 0; side < 2; ++side) {
        best[side] = exactly<int32_t>(per_side);
        margin[side] = exactly<double>(per_side);
        for (size_t i = 0; i < per_side; ++i) {
            best[side][i] = (int32_t)(draw() % (unsigned)(k.C + 2)) - 1;       // -1 .. C
            const double t = thresholds[draw() % (unsigned)k.T];
            const unsigned pick = (unsigned)(draw() % 6);
            margin[side][i] = pick == 0   ? 0.0
                              : pick == 1 ? std::nextafter(t, 0.0)
                              : pick == 2 ? t
                              : pick == 3 ? std::nextafter(t, 1.0)
                              : pick == 4 ? 1.0
                                          : std::numeric_limits<double>::quiet_NaN();
        }
    }
    int32_t* labels = exactly<int32_t>((size_t)k.n);
    int64_t* lengths = exactly<int64_t>((size_t)k.n);
    for (long long i = 0; i < k.n; ++i) {
        labels[i] = (int32_t)(draw() % (unsigned)(k.C + 1)) - 1;
        const unsigned pick = (unsigned)(draw() % 5);
        lengths[i] = pick == 0   ? 0
                     : pick == 1 ? (long long)(draw() % (unsigned long long)(3 * cap))
                     : pick == 2 ? cap
                     : pick == 3 ? (1ll << 33) + 1
                                 : (long long)(draw() % (unsigned long long)(k.L + 1));
    }
    const size_t sizes[4] = {cells * modes * width, cells * dbh_early::kColumns, cells * k.steps,
                             k.lengths ? cells * (size_t)P : 0};
    int64_t *got[4], *want[4];
    for (int a = 0; a < 4; ++a) {
        got[a] = exactly<int64_t>(sizes[a]);
        want[a] = exactly<int64_t>(sizes[a]);
    }
    dbh_early::tally_host(best[0], margin[0], k.both ? best[1] : nullptr,
                          k.both ? margin[1] : nullptr, k.labelled ? labels : nullptr,
                          k.lengths ? lengths : nullptr, k.n, k.steps, k.C, k.L, k.c, thresholds, k.T,
                          got[0], got[1], got[2], k.lengths ? got[3] : nullptr);
    // the plain loop
    for (long long i = 0; i < k.n; ++i)
        for (int m = 1; m <= k.steps; ++m)
            for (int t = 0; t < k.T; ++t) {
                const double th = thresholds[t];
                const int32_t* b = best[0] + i * k.steps;
                const double* g = margin[0] + i * k.steps;
                int d = -1;
                for (int w = m - 1; w < k.steps && d < 0; ++w)
                    if (b[w] != 0 && g[w] >= th) d = w;
                const int last = k.steps - 1;
                const int final_call = (b[last] != 0 && g[last] >= th) ? b[last] : 0;
                const int call = d < 0 ? 0 : b[d];
                int end_call = 0;
                if (k.both) {
                    const int32_t eb = best[1][i * k.steps + last];
                    if (eb != 0 && margin[1][i * k.steps + last] >= th) end_call = eb;
                }
                const size_t cell = (size_t)(m - 1) * k.T + t;
                for (int mode = 0; mode < modes; ++mode) {
                    const int read_call = k.both ? combine_plain(call, end_call, mode) : call;
                    int64_t* row = want[0] + (cell * modes + mode) * width;
                    if (read_call >= 0 && read_call < k.C) row[read_call] += 1;
                    if (k.labelled && labels[i] >= 0)
                        row[read_call == labels[i] ? k.C : (read_call != 0 ? k.C + 1 : k.C + 2)] += 1;
                }
                if (d < 0) continue;
                int64_t* e = want[1] + cell * dbh_early::kColumns;
                e[0] += 1;
                e[1] += call == final_call;
                e[2] += final_call != 0 && final_call != call;
                e[3] += final_call == 0;
                e[4] += d + 1 > m;
                e[5] += d + 1;
                want[2][cell * k.steps + d] += 1;
                if (!k.lengths) continue;
                const long long len = lengths[i], need = (long long)d * h + k.L;
                long long r = 0, have = 0;                   // pushes until the window is whole or END
                for (;;) {
                    ++r;
                    const bool end = len - have <= k.c;      // this push carries END
                    have = end ? len : have + k.c;
                    if (end || have >= need) break;
                }
                e[6] += have;
                e[7] += len;
                if (r < 1 || r > P) {
                    ++failures;
                    std::printf("FAIL push %lld outside 1 .. %lld\n", r, P);
                    continue;
                }
                want[3][cell * (size_t)P + (size_t)(r - 1)] += 1;
            }
    for (int a = 0; a < 4; ++a) {
        if (std::memcmp(got[a], want[a], sizes[a] * sizeof(int64_t)) != 0) {
            ++failures;
            std::printf("FAIL array %d: L %d steps %d C %d T %d n %lld c %lld both %d\n", a, k.L,
                        k.steps, k.C, k.T, k.n, k.c, (int)k.both);
        }
        std::free(got[a]);
        std::free(want[a]);
    }
    std::free(labels);
    std::free(lengths);
    std::free(thresholds);
    for (int side = 0; side < 2; ++side) {
        std::free(best[side]);
        std::free(margin[side]);
    }
}

}  // namespace

int main() {
    int cases = 0;
    const int shapes[][2] = {{96, 1}, {96, 4}, {96, 12}, {1024, 4}, {1024, 12}, {96, 65}, {2, 3}};
    for (const auto& shape : shapes) {
        const int L = shape[0], steps = shape[1], h = L / 2;
        const long long cap = (long long)(steps + 1) * h;
        const long long chunks[] = {1, h - 1, h + 1, 1600, cap, 1ll << 62};
        for (long long c : chunks) {
            if (c < 1 || !dbh_early::shape_ok(1, steps, 2, L, c, 1)) continue;
            for (int C : {2, 13, 256})
                for (int T : {1, 3})
                    for (int flags = 0; flags < 8; ++flags) {
                        run(Case{L, steps, C, T, 1 + (long long)(draw() % 40), c, (flags & 1) != 0,
                                 (flags & 2) != 0, (flags & 4) != 0});
                        ++cases;
                    }
        }
    }
    // what the entries refuse
    if (dbh_early::shape_ok(1, 3, 5, 9000, 4, 1) || dbh_early::shape_ok(1, 0, 5, 96, 4, 1) ||
        dbh_early::shape_ok(-1, 3, 5, 96, 4, 1) || dbh_early::shape_ok(1, 3, 5, 95, 4, 1) ||
        dbh_early::shape_ok(1, 3, 257, 96, 4, 1) || dbh_early::shape_ok(1, 3, 5, 96, 0, 1) ||
        dbh_early::shape_ok(1, 3, 5, 96, 4, 0) || !dbh_early::shape_ok(0, 3, 5, 96, 4, 1))
        ++failures;
    // the arithmetic at the edge of int64: a read of 2^62 samples in chunks of 2^62 - 1 and of 1
    if (dbh_early::samples_at(1, 1ll << 62, (1ll << 62) - 1) != (1ll << 62) - 1 ||
        dbh_early::samples_at(2, 1ll << 62, (1ll << 62) - 1) != (1ll << 62) ||
        dbh_early::push_of(3, 96, 1ll << 62, 1) != 240 || dbh_early::push_of(0, 96, 0, 1600) != 1 ||
        dbh_early::pushes_bound(96, 192, 1ll << 62) != 1)
        ++failures;
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
