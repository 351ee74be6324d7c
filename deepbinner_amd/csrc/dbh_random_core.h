// dbh_random_core.h - the synthetic no-barcode signals of `balance` (reference balance.py:164-193):
// what value i of signal s is, as a function of (seed, s, i, input_size) alone.  The kernel
// (dbh_random.hip) and the CPU model (dbh_random_signals_host, same file) are both compiled from
// this header.  C ABI: the "random signals" section of include/deepbinner_hip.h, which carries the
// contract in full; tests/random_signal_reference.py restates it in NumPy.
//
// The hash is dbh_train.h's (mix32, dropout_bits), restated here because this header is also
// compiled as plain C++ with no HIP headers in reach; layers 11..14 are this file's (dbh_feed.h
// keeps the list).  All arithmetic is fp64, one IEEE operation per written operation, left to
// right - every unit that includes this header is built without contraction.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DBR_FN __host__ __device__ __forceinline__
#else
#define DBR_FN inline
#endif

namespace dbr {

constexpr uint32_t kLayerSignal = 11, kLayerSegment = 12, kLayerDraw = 13, kLayerGradient = 14;
constexpr int kFlat = 0, kGaussian = 1, kMultiGaussian = 2, kPerlin = 3;
constexpr int kMaxInput = 1 << 20;
constexpr int64_t kMaxValues = (int64_t)1 << 30;
constexpr int kMinSegment = 100, kSegmentSpan = 401;    // a segment holds 100..500 values

DBR_FN uint32_t mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

// 24 bits of (seed, layer, signal, position, channel): dbh_train.h's dropout_bits
DBR_FN uint32_t bits(uint32_t seed_lo, uint32_t seed_hi, uint32_t layer, uint32_t signal,
                     uint32_t position, uint32_t channel) {
    uint32_t h = mix32(seed_lo + layer * 0x9e3779b9u);
    h = mix32(h ^ seed_hi);
    h = mix32(h + signal);
    h = mix32(h ^ (position * 256u + channel));
    return h >> 8;
}

DBR_FN double unit(uint32_t b) { return (double)b / 16777216.0; }
DBR_FN double mean_of(uint32_t b) { return 300.0 + 300.0 * unit(b); }
DBR_FN double stdev_of(uint32_t b) { return 10.0 + 490.0 * unit(b); }

struct Signal {
    int kind, level, octaves;
    double mean, stdev, step, start, factor;
};

DBR_FN Signal signal_of(uint32_t lo, uint32_t hi, uint32_t s) {
    Signal g;
    g.kind = (int)(bits(lo, hi, kLayerSignal, s, 0u, 0u) % 4u);
    g.level = (int)(bits(lo, hi, kLayerSignal, s, 0u, 1u) % 1001u);
    g.mean = mean_of(bits(lo, hi, kLayerSignal, s, 0u, 2u));
    g.stdev = stdev_of(bits(lo, hi, kLayerSignal, s, 0u, 3u));
    g.octaves = 1 + (int)(bits(lo, hi, kLayerSignal, s, 0u, 4u) % 4u);
    g.step = 0.001 + 0.039 * unit(bits(lo, hi, kLayerSignal, s, 0u, 5u));
    g.start = unit(bits(lo, hi, kLayerSignal, s, 0u, 6u));
    g.factor = 10.0 + 290.0 * unit(bits(lo, hi, kLayerSignal, s, 0u, 7u));
    return g;
}

// the standard normal draw of value i: the trainer's Box-Muller (dbh_trainer.hip, noise_kernel)
DBR_FN double normal(uint32_t lo, uint32_t hi, uint32_t s, uint32_t i) {
    const uint32_t b1 = bits(lo, hi, kLayerDraw, s, i, 0u);
    const uint32_t b2 = bits(lo, hi, kLayerDraw, s, i, 1u);
    const double u1 = ((double)b1 + 1.0) / 16777216.0;
    const double u2 = (double)b2 / 16777216.0;
    const double radius = sqrt(-2.0 * log(u1));
    return radius * cos(6.283185307179586 * u2);
}

// truncation toward zero; every value lies far inside int16
DBR_FN int16_t gaussian_value(double mean, double stdev, double z) {
    return (int16_t)(int32_t)(mean + stdev * z);
}

DBR_FN int32_t segment_length(uint32_t lo, uint32_t hi, uint32_t s, uint32_t k) {
    return kMinSegment + (int32_t)(bits(lo, hi, kLayerSegment, s, k, 0u) % (uint32_t)kSegmentSpan);
}
DBR_FN double segment_mean(uint32_t lo, uint32_t hi, uint32_t s, uint32_t k) {
    return mean_of(bits(lo, hi, kLayerSegment, s, k, 1u));
}
DBR_FN double segment_stdev(uint32_t lo, uint32_t hi, uint32_t s, uint32_t k) {
    return stdev_of(bits(lo, hi, kLayerSegment, s, k, 2u));
}

DBR_FN double gradient(uint32_t lo, uint32_t hi, uint32_t s, uint32_t j, uint32_t k) {
    return 2.0 * unit(bits(lo, hi, kLayerGradient, s, j, k)) - 1.0;
}

// gradient noise over `octaves` octaves at x = start + i * step, hashed gradients at the integers
DBR_FN int16_t perlin_value(const Signal& g, uint32_t lo, uint32_t hi, uint32_t s, uint32_t i) {
    const double x = g.start + (double)i * g.step;
    double sum = 0.0, weights = 0.0, amplitude = 1.0, scale = 1.0;
    for (int k = 0; k < 4; ++k) {
        if (k < g.octaves) {
            const double xk = x * scale;
            const double jf = floor(xk);
            const double t = xk - jf;
            const uint32_t j = (uint32_t)jf;
            const double f = t * t * t * (t * (t * 6.0 - 15.0) + 10.0);
            const double a = gradient(lo, hi, s, j, (uint32_t)k) * t;
            const double b = gradient(lo, hi, s, j + 1u, (uint32_t)k) * (t - 1.0);
            const double n = a + f * (b - a);
            sum = sum + amplitude * 2.0 * n;
            weights = weights + amplitude;
        }
        amplitude = amplitude * 0.5;
        scale = scale * 2.0;
    }
    return (int16_t)(int32_t)(g.mean + g.factor * (sum / weights));
}

// the argument errors of the three entries, before any work: dbh_status values
inline int check_arguments(int64_t first_signal, int64_t n_signals, int input_size, const void* out) {
    if (!out || n_signals < 1 || input_size < 1 || first_signal < 0) return 1;
    if (n_signals > ((int64_t)1 << 32) || first_signal > ((int64_t)1 << 32) - n_signals) return 1;
    if (input_size > kMaxInput || n_signals > kMaxValues / input_size) return 5;
    return 0;
}

// ---- the CPU model: signals one after another, a multi_gaussian's segments walked in order --------
inline void model_signal(uint32_t lo, uint32_t hi, uint32_t s, int32_t input_size, int16_t* row) {
    const Signal g = signal_of(lo, hi, s);
    if (g.kind == kFlat) {
        for (int32_t i = 0; i < input_size; ++i) row[i] = (int16_t)g.level;
    } else if (g.kind == kGaussian) {
        for (int32_t i = 0; i < input_size; ++i)
            row[i] = gaussian_value(g.mean, g.stdev, normal(lo, hi, s, (uint32_t)i));
    } else if (g.kind == kMultiGaussian) {
        int32_t at = 0;
        for (uint32_t k = 0; at < input_size; ++k) {
            const int32_t length = segment_length(lo, hi, s, k);
            const double mean = segment_mean(lo, hi, s, k), stdev = segment_stdev(lo, hi, s, k);
            const int32_t end = length < input_size - at ? at + length : input_size;
            for (int32_t i = at; i < end; ++i)
                row[i] = gaussian_value(mean, stdev, normal(lo, hi, s, (uint32_t)i));
            at = end;
        }
    } else {
        for (int32_t i = 0; i < input_size; ++i) row[i] = perlin_value(g, lo, hi, s, (uint32_t)i);
    }
}

}  // namespace dbr
