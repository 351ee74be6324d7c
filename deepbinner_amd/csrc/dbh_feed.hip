// dbh_feed.hip — training data resident on the device, and batches assembled from it there
// (dbh_feed.h; include/deepbinner_hip.h, "training: device-fed batches"):
//   window_stats   once per data set: a window's sum and sum of squares in int64 (exact, so no
//                  order of summation exists), its mean and standard deviation from them in fp64.
//                  One wave per window, reduced by shuffles.
//   assemble       one workgroup per batch slot: gather the slot's window, normalise it, and where
//                  the slot's draw says so augment it (the reference's modify_signal,
//                  train_network.py:170-193: a quarter of the positions written twice, a quarter
//                  dropped).  Which positions: the `half` first and the next `half` in the order of
//                  (key, position).  Ranks are never formed - a position's fate depends only on
//                  which side of the two boundary pairs it lies.  A boundary's 24-bit key is
//                  found bit by bit from the top, one count over the workgroup per bit, both
//                  boundaries in one round; its position is that of the one element with that
//                  key, or, where keys are equal, found by the same search over 14 bits.  Then
//                  a prefix sum of the copies per position, the source position of every output
//                  in LDS, and coalesced stores.
// Everything is integer work up to the one fp64 expression per value: no atomics, and nothing that
// depends on the launch geometry.  tests/feed_reference.py restates it in NumPy, bit for bit.
#include "dbh_feed.h"

#include "../../include/deepbinner_hip.h"
#include "dbh_general.h"
#include "dbh_host_layout.h"
#include "dbh_owned.h"
#include "dbh_status.h"
#include "dbh_train.h"
#include "dbh_wave.h"

#include <cmath>
#include <new>
#include <vector>

struct dbh_dataset {
    dbh_feed::View view;
    dbh_owned::DeviceBlock block;
};

const dbh_feed::View* dbh_dataset_view(const dbh_dataset* ds) { return ds ? &ds->view : nullptr; }

namespace dbh_feed {
namespace {

constexpr int kStatThreads = 64;
constexpr int kThreads = 1024;                               // assemble: 16 waves
constexpr int kWaves = kThreads / 64;
constexpr int kPer = dbh_gen::kMaxInput / kThreads;          // positions per thread, at most
constexpr int kKeyBits = 24, kIndexBits = 14;
constexpr uint32_t kNoKey = 0xffffffffu;                     // a register that holds no position
static_assert(dbh_gen::kMaxInput == 1 << kIndexBits, "a position fits kIndexBits");

__global__ __launch_bounds__(kStatThreads) void window_stats(const int16_t* __restrict__ x,
                                                             long long n, int L,
                                                             double* __restrict__ mean,
                                                             double* __restrict__ std) {
    for (long long w = blockIdx.x; w < n; w += gridDim.x) {
        const int16_t* p = x + w * L;
        long long s = 0, q = 0;
        for (int i = threadIdx.x; i < L; i += kStatThreads) {
            const long long v = p[i];
            s += v;
            q += v * v;
        }
        s = dbh_wave::wave_sum(s);
        q = dbh_wave::wave_sum(q);
        if (threadIdx.x == 0) {
            const long long d = (long long)L * q - s * s;    // L^2 * variance, exact: below 2^59
            mean[w] = (double)s / (double)L;
            std[w] = sqrt((double)d) / (double)L;
        }
    }
}

__device__ inline float normalised(int16_t x, double mean, double sd) {
    const double d = (double)x - mean;
    return sd == 0.0 ? (float)d : (float)(d / sd);
}

// the sum of a word over the workgroup: shuffles within a wave, one LDS word per wave, one barrier
// (the word buffers alternate with the round, so that a round's words outlive its readers)
__device__ inline uint32_t block_sum(uint32_t v, uint32_t (*words)[kWaves], int round, int tid) {
    v = dbh_wave::wave_sum(v);
    uint32_t* buf = words[round & 1];
    if ((tid & 63) == 0) buf[tid >> 6] = v;
    __syncthreads();
    uint32_t all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) all += buf[w];
    return all;
}

// twice below the first boundary (k1, i1), never from there to below the second, once otherwise
__device__ inline int copies_of(uint32_t key, uint32_t i, uint32_t k1, uint32_t i1, uint32_t k2,
                                uint32_t i2) {
    if (key < k1 || (key == k1 && i < i1)) return 2;
    if (key < k2 || (key == k2 && i < i2)) return 0;
    return 1;
}

__global__ __launch_bounds__(kThreads) void assemble_kernel(View ds, const long long* __restrict__ indices,
                                                            long long first, int half,
                                                            uint32_t threshold, uint32_t seed_lo,
                                                            uint32_t seed_hi, float* __restrict__ x_out,
                                                            int* __restrict__ labels_out) {
    __shared__ unsigned short source[dbh_gen::kMaxInput];    // per output: the position it copies
    __shared__ uint32_t counts[2][kWaves];
    __shared__ int totals[kWaves];
    const long long slot = blockIdx.x;
    const int tid = threadIdx.x, L = ds.input_size;
    const long long idx = indices ? indices[slot] : first + slot;
    float* out = x_out + slot * L;
    if (idx < 0 || idx >= ds.n) {
        for (int i = tid; i < L; i += kThreads) out[i] = NAN;
        if (tid == 0) labels_out[slot] = -1;
        return;
    }
    const int16_t* src = ds.samples + idx * L;
    const double mean = ds.mean[idx], sd = ds.std[idx];
    if (tid == 0) labels_out[slot] = ds.labels[idx];
    const bool augmented =
        dbh_train::dropout_bits(seed_lo, seed_hi, kLayerChance, (uint32_t)slot, 0u, 0u) < threshold;
    if (!augmented) {
        for (int i = tid; i < L; i += kThreads) out[i] = normalised(src[i], mean, sd);
        return;
    }

    // this thread's positions: base .. base + per - 1, their keys in registers
    const int per = (L + kThreads - 1) / kThreads, base = tid * per;
    uint32_t key[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = base + j;
        key[j] = kNoKey;
        if (j < per && i < L)
            key[j] = dbh_train::dropout_bits(seed_lo, seed_hi, kLayerKey, (uint32_t)slot, (uint32_t)i, 0u);
    }
    // The boundary of rank r in the order of (key, position) is the largest (k, i) with
    // count((key, position) < (k, i)) <= r.  Its key first, bit by bit from the top: both
    // boundaries in one round, two counts of at most 2^14 in one word.
    const uint32_t rank1 = (uint32_t)half, rank2 = 2u * (uint32_t)half;
    int round = 0;
    uint32_t k1 = 0, k2 = 0;
    for (int bit = kKeyBits - 1; bit >= 0; --bit) {
        const uint32_t c1 = k1 | (1u << bit), c2 = k2 | (1u << bit);
        uint32_t below = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            if (j >= per) break;
            below += (key[j] < c1 ? 1u : 0u) + (key[j] < c2 ? 0x10000u : 0u);
        }
        const uint32_t all = block_sum(below, counts, round++, tid);
        if ((all & 0xffffu) <= rank1) k1 = c1;
        if ((all >> 16) <= rank2) k2 = c2;
    }
    // how many keys lie below each boundary's, and how many share it
    uint32_t lower = 0, equal = 0, where = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        if (j >= per) break;
        lower += (key[j] < k1 ? 1u : 0u) + (key[j] < k2 ? 0x10000u : 0u);
        equal += (key[j] == k1 ? 1u : 0u) + (key[j] == k2 ? 0x10000u : 0u);
        where += (key[j] == k1 ? (uint32_t)(base + j) : 0u) + (key[j] == k2 ? (uint32_t)(base + j) << 16 : 0u);
    }
    lower = block_sum(lower, counts, round++, tid);
    equal = block_sum(equal, counts, round++, tid);
    uint32_t i1 = 0, i2 = 0;
    if (equal == 0x10001u) {
        // no other position has either boundary's key: the boundaries are those two positions
        where = block_sum(where, counts, round++, tid);
        i1 = where & 0xffffu;
        i2 = where >> 16;
    } else {
        // equal keys rank by position: the same search over the positions that share the key
        const uint32_t need1 = rank1 - (lower & 0xffffu), need2 = rank2 - (lower >> 16);
        for (int bit = kIndexBits - 1; bit >= 0; --bit) {
            const uint32_t c1 = i1 | (1u << bit), c2 = i2 | (1u << bit);
            uint32_t below = 0;
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                if (j >= per) break;
                const uint32_t i = (uint32_t)(base + j);
                below += (key[j] == k1 && i < c1 ? 1u : 0u) + (key[j] == k2 && i < c2 ? 0x10000u : 0u);
            }
            const uint32_t all = block_sum(below, counts, round++, tid);
            if ((all & 0xffffu) <= need1) i1 = c1;
            if ((all >> 16) <= need2) i2 = c2;
        }
    }
    // copies per position, their exclusive prefix sum in position order
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        if (j >= per) break;
        if (key[j] != kNoKey) mine += copies_of(key[j], (uint32_t)(base + j), k1, i1, k2, i2);
    }
    int total;
    int at = dbh_wave::block_prefix<kWaves>(mine, totals, &total);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        if (j >= per) break;
        if (key[j] == kNoKey) continue;
        const int copies = copies_of(key[j], (uint32_t)(base + j), k1, i1, k2, i2);
        for (int k = 0; k < copies; ++k, ++at)
            if (at < L) source[at] = (unsigned short)(base + j);
    }
    __syncthreads();
    for (int i = tid; i < L; i += kThreads) out[i] = normalised(src[source[i]], mean, sd);
}

int check_batch(const dbh_dataset* ds, int64_t n_windows, double augmentation, uint32_t* threshold) {
    if (!ds || n_windows < 1 || !augment_threshold(augmentation, threshold))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_windows > dbh_train::kMaxBatchSamples / ds->view.input_size) return DBH_ERR_UNSUPPORTED;
    return DBH_OK;
}

}  // namespace

bool augment_threshold(double augmentation, uint32_t* threshold) {
    if (!(augmentation >= 1.0)) return false;
    *threshold = (uint32_t)std::floor((1.0 - 1.0 / augmentation) * 16777216.0);
    return true;
}

hipError_t assemble(const View& ds, const int64_t* indices_dev, int64_t first, int64_t n_windows,
                    uint32_t threshold, uint64_t seed, float* x_dev, int32_t* labels_dev,
                    hipStream_t stream) {
    // L / 4 rounded half to even, as Python's round() does (train_network.py:171-174)
    const int L = ds.input_size, q = L / 4, r = L % 4;
    const int half = r < 2 ? q : (r == 2 ? q + (q & 1) : q + 1);
    hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)n_windows), dim3(kThreads), 0, stream, ds,
                       (const long long*)indices_dev, (long long)first, half, threshold,
                       (uint32_t)seed, (uint32_t)(seed >> 32), x_dev, (int*)labels_dev);
    return hipGetLastError();
}

}  // namespace dbh_feed

// ---- C ABI (include/deepbinner_hip.h, "training: device-fed batches") ----------------------------
using namespace dbh_feed;

extern "C" {

int dbh_epoch_order(uint64_t seed, int64_t pass, int64_t n, int64_t* order) {
    if (!order || n < 1 || pass < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n > ((int64_t)1 << 31)) return DBH_ERR_UNSUPPORTED;
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    const uint32_t position = (uint32_t)(pass & ((1 << kIndexBits) - 1));
    auto key = [=](int64_t i) {
        return dbh_train::dropout_bits(lo, hi, kLayerOrder, (uint32_t)i, position, 0u);
    };
    // a stable sort by 24-bit keys: two counting passes of 12 bits, the lower first
    constexpr int kDigit = 12, kBuckets = 1 << kDigit;
    std::vector<int64_t> tmp, start;
    try {
        tmp.resize((size_t)n);
        start.assign(kBuckets + 1, 0);
    } catch (const std::bad_alloc&) {
        return DBH_ERR_OUT_OF_MEMORY;
    }
    for (int64_t i = 0; i < n; ++i) start[(key(i) & (kBuckets - 1)) + 1] += 1;
    for (int b = 0; b < kBuckets; ++b) start[b + 1] += start[b];
    for (int64_t i = 0; i < n; ++i) tmp[(size_t)start[key(i) & (kBuckets - 1)]++] = i;
    start.assign(kBuckets + 1, 0);
    for (int64_t i = 0; i < n; ++i) start[(key(i) >> kDigit) + 1] += 1;
    for (int b = 0; b < kBuckets; ++b) start[b + 1] += start[b];
    for (int64_t j = 0; j < n; ++j) order[start[key(tmp[(size_t)j]) >> kDigit]++] = tmp[(size_t)j];
    return DBH_OK;
}

int dbh_dataset_create(const int16_t* samples_host, const int32_t* labels_host, int64_t n,
                       int input_size, int n_classes, dbh_dataset** ds) {
    if (!dbh_gen::geometry_ok(input_size, n_classes)) return DBH_ERR_UNSUPPORTED;
    if (!samples_host || !labels_host || !ds || n < 1) return DBH_ERR_INVALID_ARGUMENT;
    if (n > 0x7fffffff) return DBH_ERR_UNSUPPORTED;
    for (int64_t i = 0; i < n; ++i)
        if (labels_host[i] < 0 || labels_host[i] >= n_classes) return DBH_ERR_INVALID_ARGUMENT;
    dbh_dataset* d = new (std::nothrow) dbh_dataset;
    if (!d) return DBH_ERR_OUT_OF_MEMORY;
    const size_t s_bytes = (size_t)n * input_size * sizeof(int16_t), l_bytes = (size_t)n * sizeof(int32_t);
    int16_t* samples;
    int32_t* labels;
    double *mean, *sd;
    hipError_t e = d->block.carve([&](dbh_host::Carve& c) {
        d->view.samples = samples = c.take<int16_t>((size_t)n * input_size);
        d->view.labels = labels = c.take<int32_t>((size_t)n);
        d->view.mean = mean = c.take<double>((size_t)n);
        d->view.std = sd = c.take<double>((size_t)n);
    });
    if (e == hipSuccess) e = hipMemcpy(samples, samples_host, s_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(labels, labels_host, l_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)(n < 65536 ? n : 65536);
        hipLaunchKernelGGL(window_stats, dim3(grid), dim3(kStatThreads), 0, 0, samples, (long long)n,
                           input_size, mean, sd);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        delete d;
        return dbh_hip::hip_fail(e, "dbh_dataset_create");
    }
    d->view.n = n;
    d->view.input_size = input_size;
    d->view.n_classes = n_classes;
    *ds = d;
    return DBH_OK;
}

int dbh_dataset_destroy(dbh_dataset* ds) {
    if (ds) {
        (void)hipDeviceSynchronize();      // a queued batch may still read the block
        delete ds;
    }
    return DBH_OK;
}

int dbh_dataset_count(const dbh_dataset* ds, int64_t* n) {
    if (!ds || !n) return DBH_ERR_INVALID_ARGUMENT;
    *n = ds->view.n;
    return DBH_OK;
}

int dbh_dataset_batch_dev(const dbh_dataset* ds, const int64_t* indices_dev, int64_t n_windows,
                          double augmentation, uint64_t seed, float* x_dev, int32_t* labels_dev,
                          dbh_stream stream) {
    uint32_t threshold = 0;
    const int st = check_batch(ds, n_windows, augmentation, &threshold);
    if (st != DBH_OK) return st;
    if (!indices_dev || !x_dev || !labels_dev) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(assemble(ds->view, indices_dev, 0, n_windows, threshold, seed, x_dev, labels_dev,
                     (hipStream_t)stream));
    return DBH_OK;
}

int dbh_dataset_batch(const dbh_dataset* ds, const int64_t* indices_host, int64_t n_windows,
                      double augmentation, uint64_t seed, float* x_host, int32_t* labels_host) {
    uint32_t threshold = 0;
    const int st = check_batch(ds, n_windows, augmentation, &threshold);
    if (st != DBH_OK) return st;
    if (!indices_host || !x_host || !labels_host) return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_windows; ++i)
        if (indices_host[i] < 0 || indices_host[i] >= ds->view.n) return DBH_ERR_INVALID_ARGUMENT;
    const size_t i_bytes = (size_t)n_windows * sizeof(int64_t), l_bytes = (size_t)n_windows * sizeof(int32_t);
    const size_t x_bytes = (size_t)n_windows * ds->view.input_size * sizeof(float);
    int64_t* indices;
    int32_t* labels;
    float* x;
    auto lay_out = [&](dbh_host::Carve& c) {
        indices = c.take<int64_t>((size_t)n_windows);
        labels = c.take<int32_t>((size_t)n_windows);
        x = c.take<float>((size_t)n_windows * ds->view.input_size);
    };
    dbh_owned::DeviceBlock block;
    DBH_HIP(block.carve(lay_out));
    DBH_HIP(hipMemcpyAsync(indices, indices_host, i_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(assemble(ds->view, indices, 0, n_windows, threshold, seed, x, labels, 0));
    DBH_HIP(hipStreamSynchronize(0));
    DBH_HIP(hipMemcpy(x_host, x, x_bytes, hipMemcpyDeviceToHost));
    DBH_HIP(hipMemcpy(labels_host, labels, l_bytes, hipMemcpyDeviceToHost));
    return DBH_OK;
}

}  // extern "C"
