// dbh_trainer.hip — the training step's second half and the trainer that keeps a model's training
// state on the device (include/deepbinner_hip.h, "a resident trainer"):
//   noise_kernel    GaussianNoise (reference network_architecture.py:25): Box-Muller in fp64 from two
//                   draws of dbh_train.h's hash, layer number 0, one rounding to fp32
//   update_kernel   one pass over the blob: Keras 2.1.4's Nadam (train_network.py:53-55) on the
//                   trainable elements, BatchNormalization's moving average on the others, in fp64.
//                   Which is which comes from dbh_network.h's table (BlobMap below).  The elements
//                   of frozen blocks it neither reads nor writes.
// Every element is a function of its own index: no atomics, no reduction, nothing that depends on
// the launch geometry.  The library is built with -ffp-contract=off, so each operation below is the
// IEEE operation it is written as, and NumPy on the host gives the same bits
// (tests/train_step_reference.py).
#include "../../include/deepbinner_hip.h"
#include "dbh_feed.h"
#include "dbh_general.h"
#include "dbh_host_layout.h"
#include "dbh_network.h"
#include "dbh_owned.h"
#include "dbh_status.h"
#include "dbh_train.h"

#include <cmath>
#include <new>
#include <vector>

namespace {

using namespace dbh_net;
using dbh_host::blocks_for;

constexpr int kThreads = 256;
constexpr uint64_t kStepStride = 0x9E3779B97F4A7C15ull;    // step_seed = seed + t0 * kStepStride
constexpr int64_t kMaxNoiseSamples = dbh_train::kMaxBatchSamples;

// ---- noise --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void noise_kernel(const float* __restrict__ x, long long total,
                                                         int input_size, float noise_std,
                                                         uint32_t seed_lo, uint32_t seed_hi,
                                                         float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const float v = x[idx];
    if (noise_std == 0.f) {          // bit for bit: no arithmetic (x + 0 would turn -0 into +0)
        out[idx] = v;
        return;
    }
    const long long window = idx / input_size;
    const uint32_t position = (uint32_t)(idx - window * input_size);
    const uint32_t b1 = dbh_train::dropout_bits(seed_lo, seed_hi, 0u, (uint32_t)window, position, 0u);
    const uint32_t b2 = dbh_train::dropout_bits(seed_lo, seed_hi, 0u, (uint32_t)window, position, 1u);
    const double u1 = ((double)b1 + 1.0) / 16777216.0;
    const double u2 = (double)b2 / 16777216.0;
    const double radius = sqrt(-2.0 * log(u1));
    const double z = radius * cos(6.283185307179586 * u2);
    out[idx] = (float)((double)v + (double)noise_std * z);
}

// ---- update -------------------------------------------------------------------------------------
// Where the batch normalisations lie in a blob of this class count: bn[j] = blob_bn(j), bn[kNumBn] =
// the blob's end.  Layer j holds gamma, beta, moving mean, moving variance, a quarter of its floats
// each; its batch statistics (mean then variance) start at half its distance from bn[0].
// Frozen blocks (dbh_train.h): the convolutions' elements below frozen_floats and the whole of the
// first frozen_bn batch normalisations are left as they are - not read, not written.
struct BlobMap {
    int bn[kNumBn + 1];
    int frozen_floats, frozen_bn;
};

BlobMap blob_map(int n_classes, int frozen_blocks) {
    BlobMap map;
    for (int j = 0; j <= kNumBn; ++j) map.bn[j] = (int)blob_bn(j, n_classes);
    map.frozen_floats = (int)blob_kernel(dbh_train::frozen_convs(frozen_blocks), n_classes);
    map.frozen_bn = frozen_blocks;
    return map;
}

__global__ __launch_bounds__(kThreads) void update_kernel(float* __restrict__ params,
                                                          const float* __restrict__ grads,
                                                          float* __restrict__ m_blob,
                                                          float* __restrict__ v_blob,
                                                          const float* __restrict__ stats,
                                                          BlobMap map, dbh_nadam_coefficients k) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= map.bn[kNumBn] || i < map.frozen_floats) return;
    if (i >= map.bn[0]) {
        int begin = map.bn[0], end = map.bn[1], layer = 0;
#pragma unroll
        for (int j = 1; j < kNumBn; ++j)
            if (i >= map.bn[j]) {
                begin = map.bn[j];
                end = map.bn[j + 1];
                layer = j;
            }
        if (layer < map.frozen_bn) return;
        const int channels = (end - begin) / 4;
        const int within = i - begin;
        if (within >= 2 * channels) {
            // moving mean (third quarter) or moving variance (fourth): the batch's value lies at the
            // same distance behind the layer's first statistic
            const double old = (double)params[i];
            const double batch = (double)stats[(begin - map.bn[0]) / 2 + (within - 2 * channels)];
            const double step = (old - batch) * (1.0 - k.bn_momentum);
            params[i] = (float)(old - step);
            return;
        }
    }
    const double p = (double)params[i], g = (double)grads[i];
    const double g_prime = g / (1.0 - k.sched_new);
    const double m_keep = k.beta_1 * (double)m_blob[i];
    const double m_add = (1.0 - k.beta_1) * g;
    const double m = m_keep + m_add;
    const double m_prime = m / (1.0 - k.sched_next);
    const double v_keep = k.beta_2 * (double)v_blob[i];
    const double gg = g * g;
    const double v_add = (1.0 - k.beta_2) * gg;
    const double v = v_keep + v_add;
    const double v_prime = v / (1.0 - k.beta_2_t);
    const double from_g = (1.0 - k.mu_t) * g_prime;
    const double from_m = k.mu_t1 * m_prime;
    const double bar = from_g + from_m;
    const double denom = sqrt(v_prime) + k.epsilon;
    const double scaled = k.lr * bar;
    const double move = scaled / denom;
    m_blob[i] = (float)m;
    v_blob[i] = (float)v;
    params[i] = (float)(p - move);
}

// ---- host ---------------------------------------------------------------------------------------
const dbh_trainer_options kDefaults = {
    (double)0.002f, (double)0.9f, (double)0.999f, 1e-7, 0.004, 0.99, 0.15f, 0.02f, 0,
};

bool in_unit(double v, bool closed) { return v >= 0.0 && (closed ? v <= 1.0 : v < 1.0); }

int check_options(const dbh_trainer_options& o) {
    if (!in_unit((double)o.dropout_rate, false) || !(o.noise_std >= 0.f) || !in_unit(o.bn_momentum, true))
        return DBH_ERR_INVALID_ARGUMENT;
    return DBH_OK;
}

int check_noise(int64_t n_windows, int input_size, float noise_std) {
    if (n_windows < 1 || input_size < 1 || !(noise_std >= 0.f)) return DBH_ERR_INVALID_ARGUMENT;
    if (input_size > dbh_gen::kMaxInput || n_windows > kMaxNoiseSamples / input_size)
        return DBH_ERR_UNSUPPORTED;
    return DBH_OK;
}

int check_update(int64_t n_floats, int n_classes, const dbh_nadam_coefficients* k) {
    if (n_classes < dbh_gen::kMinClasses || n_classes > dbh_gen::kMaxClasses) return DBH_ERR_UNSUPPORTED;
    if (n_floats != param_count(n_classes)) return DBH_ERR_BAD_WEIGHTS;
    if (!k || !in_unit(k->bn_momentum, true)) return DBH_ERR_INVALID_ARGUMENT;
    return DBH_OK;
}

hipError_t launch_noise(const float* x, int64_t n_windows, int input_size, float noise_std,
                        uint64_t seed, float* out, hipStream_t stream) {
    const long long total = (long long)n_windows * input_size;
    hipLaunchKernelGGL(noise_kernel, dim3(blocks_for(total, kThreads)), dim3(kThreads), 0, stream, x, total,
                       input_size, noise_std, (uint32_t)seed, (uint32_t)(seed >> 32), out);
    return hipGetLastError();
}

hipError_t launch_update(float* params, const float* grads, float* m, float* v, const float* stats,
                         int n_classes, const dbh_nadam_coefficients& k, int frozen_blocks,
                         hipStream_t stream) {
    hipLaunchKernelGGL(update_kernel, dim3(blocks_for(param_count(n_classes), kThreads)), dim3(kThreads), 0,
                       stream, params, grads, m, v, stats, blob_map(n_classes, frozen_blocks), k);
    return hipGetLastError();
}

}  // namespace

// One block on the device, carved once: the four blobs, the statistics, a batch's windows as given
// and with their noise, its labels, the loss and the count (and an evaluation's totals behind
// them), dbh_gradients' workspace, a batch's sample indices.
struct dbh_trainer {
    dbh_trainer_options options;
    int n_classes = 0, input_size = 0;
    int64_t n_floats = 0, max_windows = 0;
    int64_t iterations = 0;
    double m_schedule = 1.0;
    int frozen_blocks = 0;           // an option of the run (dbh_trainer_set_frozen), not of the state
    dbh_owned::DeviceBlock block;
    float *weights = nullptr, *m = nullptr, *v = nullptr, *grads = nullptr, *stats = nullptr;
    float *x_in = nullptr, *x_noisy = nullptr;
    int32_t* labels = nullptr;
    double* loss = nullptr;          // the count follows it: int64 at loss + 1; an evaluation's
                                     // loss sum and count at loss + 2 and loss + 3
    void* workspace = nullptr;
    int64_t* indices = nullptr;

    size_t blob_bytes() const { return (size_t)n_floats * sizeof(float); }

    hipError_t allocate() {
        return block.carve([this](dbh_host::Carve& c) {
            weights = c.take<float>((size_t)n_floats);
            m = c.take<float>((size_t)n_floats);
            v = c.take<float>((size_t)n_floats);
            grads = c.take<float>((size_t)n_floats);
            stats = c.take<float>(dbh_train::kStatsFloats);
            x_in = c.take<float>((size_t)max_windows * input_size);
            x_noisy = c.take<float>((size_t)max_windows * input_size);
            labels = c.take<int32_t>((size_t)max_windows);
            loss = c.take<double>(4);
            workspace = c.take<char>(dbh_train::workspace_bytes(n_classes, input_size, max_windows));
            indices = c.take<int64_t>((size_t)max_windows);
        });
    }

    int check_step(int64_t n_windows) const {
        if (n_windows < 1) return DBH_ERR_INVALID_ARGUMENT;
        if (n_windows > max_windows) return DBH_ERR_UNSUPPORTED;
        return DBH_OK;
    }

    // noise, gradients, update: queued on `stream`; the host's part of the state moves on at once
    hipError_t queue_step(const float* x, const int32_t* step_labels, int64_t n_windows,
                          double* mean_loss, int64_t* n_correct, hipStream_t stream) {
        const uint64_t step_seed = options.seed + (uint64_t)iterations * kStepStride;
        dbh_nadam_coefficients k;
        (void)dbh_nadam_schedule(iterations, m_schedule, &options, &k);
        hipError_t e = launch_noise(x, n_windows, input_size, options.noise_std, step_seed, x_noisy, stream);
        if (e == hipSuccess)
            e = dbh_train::gradients(weights, n_classes, input_size, x_noisy, step_labels, n_windows,
                                     options.dropout_rate, step_seed, mean_loss, n_correct, grads,
                                     stats, workspace, stream, frozen_blocks);
        if (e == hipSuccess)
            e = launch_update(weights, grads, m, v, stats, n_classes, k, frozen_blocks, stream);
        if (e == hipSuccess) {
            iterations += 1;
            m_schedule = k.sched_new;
        }
        return e;
    }

    // what a data-set entry checks before any device work
    int check_dataset(const dbh_feed::View* ds, int64_t n_windows, double augmentation,
                      uint32_t* threshold) const {
        if (!ds || !dbh_feed::augment_threshold(augmentation, threshold)) return DBH_ERR_INVALID_ARGUMENT;
        if (ds->input_size != input_size || ds->n_classes != n_classes) return DBH_ERR_UNSUPPORTED;
        return check_step(n_windows);
    }

    // augment (into x_in and labels), then the step: one step seed for all of it
    hipError_t queue_dataset_step(const dbh_feed::View& ds, const int64_t* indices_dev,
                                  int64_t n_windows, uint32_t threshold, double* mean_loss,
                                  int64_t* n_correct, hipStream_t stream) {
        const uint64_t step_seed = options.seed + (uint64_t)iterations * kStepStride;
        const hipError_t e = dbh_feed::assemble(ds, indices_dev, 0, n_windows, threshold, step_seed,
                                                x_in, labels, stream);
        return e == hipSuccess ? queue_step(x_in, labels, n_windows, mean_loss, n_correct, stream) : e;
    }
};

extern "C" {

int dbh_trainer_default_options(dbh_trainer_options* options) {
    if (!options) return DBH_ERR_INVALID_ARGUMENT;
    *options = kDefaults;
    return DBH_OK;
}

int dbh_nadam_schedule(int64_t t0, double m_schedule, const dbh_trainer_options* hyper,
                       dbh_nadam_coefficients* k) {
    if (!k || t0 < 0) return DBH_ERR_INVALID_ARGUMENT;
    const dbh_trainer_options& o = hyper ? *hyper : kDefaults;
    const double t = (double)t0 + 1.0;
    k->lr = o.lr;
    k->beta_1 = o.beta_1;
    k->beta_2 = o.beta_2;
    k->epsilon = o.epsilon;
    k->mu_t = o.beta_1 * (1.0 - 0.5 * std::pow(0.96, t * o.schedule_decay));
    k->mu_t1 = o.beta_1 * (1.0 - 0.5 * std::pow(0.96, (t + 1.0) * o.schedule_decay));
    k->sched_new = m_schedule * k->mu_t;
    k->sched_next = k->sched_new * k->mu_t1;
    k->beta_2_t = std::pow(o.beta_2, t);
    k->bn_momentum = o.bn_momentum;
    return DBH_OK;
}

int dbh_train_noise_dev(const float* x_dev, int64_t n_windows, int input_size, float noise_std,
                        uint64_t seed, float* out_dev, dbh_stream stream) {
    const int st = check_noise(n_windows, input_size, noise_std);
    if (st != DBH_OK) return st;
    if (!x_dev || !out_dev) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(launch_noise(x_dev, n_windows, input_size, noise_std, seed, out_dev,
                         (hipStream_t)stream));
    return DBH_OK;
}

int dbh_train_noise(const float* x_host, int64_t n_windows, int input_size, float noise_std,
                    uint64_t seed, float* out_host) {
    const int st = check_noise(n_windows, input_size, noise_std);
    if (st != DBH_OK) return st;
    if (!x_host || !out_host) return DBH_ERR_INVALID_ARGUMENT;
    const size_t bytes = (size_t)n_windows * input_size * sizeof(float);
    dbh_owned::DeviceBlock block;
    DBH_HIP(block.reserve(bytes));
    float* d = block.as<float>();
    DBH_HIP(hipMemcpyAsync(d, x_host, bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(launch_noise(d, n_windows, input_size, noise_std, seed, d, 0));
    DBH_HIP(hipStreamSynchronize(0));
    DBH_HIP(hipMemcpy(out_host, d, bytes, hipMemcpyDeviceToHost));
    return DBH_OK;
}

int dbh_nadam_update_frozen_dev(float* params_dev, const float* grads_dev, float* m_dev,
                                float* v_dev, const float* batch_stats_dev, int64_t n_floats,
                                int n_classes, const dbh_nadam_coefficients* coefficients,
                                dbh_stream stream, int frozen_blocks) {
    const int st = check_update(n_floats, n_classes, coefficients);
    if (st != DBH_OK) return st;
    if (!params_dev || !grads_dev || !m_dev || !v_dev || !batch_stats_dev ||
        !dbh_train::frozen_ok(frozen_blocks))
        return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(launch_update(params_dev, grads_dev, m_dev, v_dev, batch_stats_dev, n_classes,
                          *coefficients, frozen_blocks, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_nadam_update_dev(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev,
                         const float* batch_stats_dev, int64_t n_floats, int n_classes,
                         const dbh_nadam_coefficients* coefficients, dbh_stream stream) {
    return dbh_nadam_update_frozen_dev(params_dev, grads_dev, m_dev, v_dev, batch_stats_dev, n_floats,
                                       n_classes, coefficients, stream, 0);
}

int dbh_nadam_update_frozen(float* params_host, const float* grads_host, float* m_host,
                            float* v_host, const float* batch_stats_host, int64_t n_floats,
                            int n_classes, const dbh_nadam_coefficients* coefficients,
                            int frozen_blocks) {
    const int st = check_update(n_floats, n_classes, coefficients);
    if (st != DBH_OK) return st;
    if (!params_host || !grads_host || !m_host || !v_host || !batch_stats_host ||
        !dbh_train::frozen_ok(frozen_blocks))
        return DBH_ERR_INVALID_ARGUMENT;
    const size_t bytes = (size_t)n_floats * sizeof(float);
    const size_t s_bytes = dbh_train::kStatsFloats * sizeof(float);
    float *p, *g, *m, *v, *s;
    auto lay_out = [&](dbh_host::Carve& c) {
        p = c.take<float>((size_t)n_floats);
        g = c.take<float>((size_t)n_floats);
        m = c.take<float>((size_t)n_floats);
        v = c.take<float>((size_t)n_floats);
        s = c.take<float>(dbh_train::kStatsFloats);
    };
    dbh_owned::DeviceBlock block;
    DBH_HIP(block.carve(lay_out));
    DBH_HIP(hipMemcpyAsync(p, params_host, bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(g, grads_host, bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(m, m_host, bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(v, v_host, bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(s, batch_stats_host, s_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(launch_update(p, g, m, v, s, n_classes, *coefficients, frozen_blocks, 0));
    DBH_HIP(hipStreamSynchronize(0));
    DBH_HIP(hipMemcpy(params_host, p, bytes, hipMemcpyDeviceToHost));
    DBH_HIP(hipMemcpy(m_host, m, bytes, hipMemcpyDeviceToHost));
    DBH_HIP(hipMemcpy(v_host, v, bytes, hipMemcpyDeviceToHost));
    return DBH_OK;
}

int dbh_nadam_update(float* params_host, const float* grads_host, float* m_host, float* v_host,
                     const float* batch_stats_host, int64_t n_floats, int n_classes,
                     const dbh_nadam_coefficients* coefficients) {
    return dbh_nadam_update_frozen(params_host, grads_host, m_host, v_host, batch_stats_host, n_floats,
                                   n_classes, coefficients, 0);
}

int dbh_trainer_create(const float* weights_host, int64_t n_floats, int n_classes, int input_size,
                       int64_t max_windows, const dbh_trainer_options* options,
                       dbh_trainer** trainer) {
    if (!dbh_gen::geometry_ok(input_size, n_classes)) return DBH_ERR_UNSUPPORTED;
    if (n_floats != param_count(n_classes)) return DBH_ERR_BAD_WEIGHTS;
    const dbh_trainer_options& o = options ? *options : kDefaults;
    if (max_windows < 1 || !weights_host || !trainer || check_options(o) != DBH_OK)
        return DBH_ERR_INVALID_ARGUMENT;
    if (max_windows > dbh_train::kMaxBatchSamples / input_size) return DBH_ERR_UNSUPPORTED;
    dbh_trainer* t = new (std::nothrow) dbh_trainer;
    if (!t) return DBH_ERR_OUT_OF_MEMORY;
    t->options = o;
    t->n_classes = n_classes;
    t->input_size = input_size;
    t->n_floats = n_floats;
    t->max_windows = max_windows;
    hipError_t e = t->allocate();
    if (e == hipSuccess) e = hipMemcpy(t->weights, weights_host, t->blob_bytes(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(t->m, 0, t->blob_bytes());
    if (e == hipSuccess) e = hipMemset(t->v, 0, t->blob_bytes());
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        delete t;
        return dbh_hip::hip_fail(e, "dbh_trainer_create");
    }
    *trainer = t;
    return DBH_OK;
}

int dbh_trainer_destroy(dbh_trainer* trainer) {
    if (trainer) {
        (void)hipDeviceSynchronize();      // a queued step may still use the block
        delete trainer;
    }
    return DBH_OK;
}

int dbh_trainer_step_dev(dbh_trainer* trainer, const float* x_dev, const int32_t* labels_dev,
                         int64_t n_windows, double* mean_loss_dev, int64_t* n_correct_dev,
                         dbh_stream stream) {
    if (!trainer || !x_dev || !labels_dev || !mean_loss_dev || !n_correct_dev)
        return DBH_ERR_INVALID_ARGUMENT;
    const int st = trainer->check_step(n_windows);
    if (st != DBH_OK) return st;
    DBH_HIP(trainer->queue_step(x_dev, labels_dev, n_windows, mean_loss_dev, n_correct_dev,
                                (hipStream_t)stream));
    return DBH_OK;
}

int dbh_trainer_step(dbh_trainer* trainer, const float* x_host, const int32_t* labels_host,
                     int64_t n_windows, double* mean_loss, int64_t* n_correct) {
    if (!trainer || !x_host || !labels_host || !mean_loss || !n_correct) return DBH_ERR_INVALID_ARGUMENT;
    const int st = trainer->check_step(n_windows);
    if (st != DBH_OK) return st;
    for (int64_t i = 0; i < n_windows; ++i)
        if (labels_host[i] < 0 || labels_host[i] >= trainer->n_classes) return DBH_ERR_INVALID_ARGUMENT;
    dbh_trainer& t = *trainer;
    DBH_HIP(hipMemcpyAsync(t.x_in, x_host, (size_t)n_windows * t.input_size * sizeof(float),
                           hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(t.labels, labels_host, (size_t)n_windows * sizeof(int32_t),
                           hipMemcpyHostToDevice, 0));
    DBH_HIP(t.queue_step(t.x_in, t.labels, n_windows, t.loss, (int64_t*)(t.loss + 1), 0));
    DBH_HIP(hipStreamSynchronize(0));
    struct { double loss; int64_t correct; } out;
    DBH_HIP(hipMemcpy(&out, t.loss, sizeof(out), hipMemcpyDeviceToHost));
    *mean_loss = out.loss;
    *n_correct = out.correct;
    return DBH_OK;
}

int dbh_trainer_get_weights(dbh_trainer* trainer, float* weights_host, int64_t n_floats) {
    if (!trainer || !weights_host) return DBH_ERR_INVALID_ARGUMENT;
    if (n_floats != trainer->n_floats) return DBH_ERR_BAD_WEIGHTS;
    DBH_HIP(hipDeviceSynchronize());
    DBH_HIP(hipMemcpy(weights_host, trainer->weights, trainer->blob_bytes(), hipMemcpyDeviceToHost));
    return DBH_OK;
}

int dbh_trainer_get_state(dbh_trainer* trainer, float* m_host, float* v_host, int64_t n_floats,
                          int64_t* iterations, double* m_schedule) {
    if (!trainer || !m_host || !v_host || !iterations || !m_schedule) return DBH_ERR_INVALID_ARGUMENT;
    if (n_floats != trainer->n_floats) return DBH_ERR_BAD_WEIGHTS;
    DBH_HIP(hipDeviceSynchronize());
    DBH_HIP(hipMemcpy(m_host, trainer->m, trainer->blob_bytes(), hipMemcpyDeviceToHost));
    DBH_HIP(hipMemcpy(v_host, trainer->v, trainer->blob_bytes(), hipMemcpyDeviceToHost));
    *iterations = trainer->iterations;
    *m_schedule = trainer->m_schedule;
    return DBH_OK;
}

int dbh_trainer_set_state(dbh_trainer* trainer, const float* m_host, const float* v_host,
                          int64_t n_floats, int64_t iterations, double m_schedule) {
    if (!trainer || !m_host || !v_host || iterations < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_floats != trainer->n_floats) return DBH_ERR_BAD_WEIGHTS;
    DBH_HIP(hipDeviceSynchronize());
    DBH_HIP(hipMemcpy(trainer->m, m_host, trainer->blob_bytes(), hipMemcpyHostToDevice));
    DBH_HIP(hipMemcpy(trainer->v, v_host, trainer->blob_bytes(), hipMemcpyHostToDevice));
    trainer->iterations = iterations;
    trainer->m_schedule = m_schedule;
    return DBH_OK;
}

int dbh_trainer_iterations(dbh_trainer* trainer, int64_t* iterations) {
    if (!trainer || !iterations) return DBH_ERR_INVALID_ARGUMENT;
    *iterations = trainer->iterations;
    return DBH_OK;
}

// (a step's launches carry the count they were queued with: no wait is needed here)
int dbh_trainer_set_frozen(dbh_trainer* trainer, int frozen_blocks) {
    if (!trainer || !dbh_train::frozen_ok(frozen_blocks)) return DBH_ERR_INVALID_ARGUMENT;
    trainer->frozen_blocks = frozen_blocks;
    return DBH_OK;
}

int dbh_trainer_get_frozen(dbh_trainer* trainer, int* frozen_blocks) {
    if (!trainer || !frozen_blocks) return DBH_ERR_INVALID_ARGUMENT;
    *frozen_blocks = trainer->frozen_blocks;
    return DBH_OK;
}

int dbh_trainer_step_dataset_dev(dbh_trainer* trainer, const dbh_dataset* ds,
                                 const int64_t* indices_dev, int64_t n_windows, double augmentation,
                                 double* mean_loss_dev, int64_t* n_correct_dev, dbh_stream stream) {
    if (!trainer || !indices_dev || !mean_loss_dev || !n_correct_dev) return DBH_ERR_INVALID_ARGUMENT;
    uint32_t threshold = 0;
    const int st = trainer->check_dataset(dbh_dataset_view(ds), n_windows, augmentation, &threshold);
    if (st != DBH_OK) return st;
    DBH_HIP(trainer->queue_dataset_step(*dbh_dataset_view(ds), indices_dev, n_windows,
                                        threshold, mean_loss_dev, n_correct_dev,
                                        (hipStream_t)stream));
    return DBH_OK;
}

int dbh_trainer_step_dataset(dbh_trainer* trainer, const dbh_dataset* ds, const int64_t* indices_host,
                             int64_t n_windows, double augmentation, double* mean_loss,
                             int64_t* n_correct) {
    if (!trainer || !indices_host || !mean_loss || !n_correct) return DBH_ERR_INVALID_ARGUMENT;
    uint32_t threshold = 0;
    const dbh_feed::View* view = dbh_dataset_view(ds);
    const int st = trainer->check_dataset(view, n_windows, augmentation, &threshold);
    if (st != DBH_OK) return st;
    for (int64_t i = 0; i < n_windows; ++i)
        if (indices_host[i] < 0 || indices_host[i] >= view->n) return DBH_ERR_INVALID_ARGUMENT;
    dbh_trainer& t = *trainer;
    DBH_HIP(hipMemcpyAsync(t.indices, indices_host, (size_t)n_windows * sizeof(int64_t),
                           hipMemcpyHostToDevice, 0));
    DBH_HIP(t.queue_dataset_step(*view, t.indices, n_windows, threshold, t.loss,
                                 (int64_t*)(t.loss + 1), 0));
    DBH_HIP(hipStreamSynchronize(0));
    struct { double loss; int64_t correct; } out;
    DBH_HIP(hipMemcpy(&out, t.loss, sizeof(out), hipMemcpyDeviceToHost));
    *mean_loss = out.loss;
    *n_correct = out.correct;
    return DBH_OK;
}

int dbh_trainer_evaluate_dataset(dbh_trainer* trainer, const dbh_dataset* ds, int64_t first,
                                 int64_t count, double* loss_sum, int64_t* n_correct,
                                 double* window_loss_host) {
    const dbh_feed::View* view = dbh_dataset_view(ds);
    if (!trainer || !view || !loss_sum || !n_correct || count < 1 || first < 0 ||
        first > view->n || count > view->n - first)
        return DBH_ERR_INVALID_ARGUMENT;
    if (view->input_size != trainer->input_size || view->n_classes != trainer->n_classes)
        return DBH_ERR_UNSUPPORTED;
    dbh_trainer& t = *trainer;
    dbh_owned::DeviceBlock per_window;
    if (window_loss_host) DBH_HIP(per_window.reserve((size_t)count * sizeof(double)));
    double* totals = t.loss + 2;
    DBH_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(double), 0));
    // file order, unaugmented (threshold 0), chunk by chunk through the step's own buffers
    for (int64_t done = 0; done < count; done += t.max_windows) {
        const int64_t n = count - done < t.max_windows ? count - done : t.max_windows;
        DBH_HIP(dbh_feed::assemble(*view, nullptr, first + done, n, 0u, 0, t.x_in, t.labels, 0));
        DBH_HIP(dbh_train::evaluate(t.weights, t.n_classes, t.input_size, t.x_in, t.labels, n,
                                    totals, (int64_t*)(totals + 1),
                                    window_loss_host ? per_window.as<double>() + done : nullptr,
                                    t.workspace, 0));
    }
    DBH_HIP(hipStreamSynchronize(0));
    struct { double loss; int64_t correct; } out;
    DBH_HIP(hipMemcpy(&out, totals, sizeof(out), hipMemcpyDeviceToHost));
    if (window_loss_host)
        DBH_HIP(hipMemcpy(window_loss_host, per_window.get(), (size_t)count * sizeof(double),
                          hipMemcpyDeviceToHost));
    *loss_sum = out.loss;
    *n_correct = out.correct;
    return DBH_OK;
}

}  // extern "C"
