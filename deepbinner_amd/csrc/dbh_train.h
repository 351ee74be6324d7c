// dbh_train.h — the training step's first half (dbh_train.hip): training-mode forward pass,
// categorical cross-entropy and the gradient of the mean loss with respect to every trainable
// parameter of a Deepbinner network (reference network_architecture.py:18-95, compiled as in
// train_network.py:53-55), for any geometry dbh_gen::geometry_ok accepts.  DESIGN.md section 17.
//
// The input windows are taken as given: the reference's GaussianNoise(0.02) layer
// (network_architecture.py:25) is the caller's to add to x (dbh_trainer.hip); it is not part of this call.
//
// Dropout (rate, inverted, behind each batch normalisation) keeps an element by a stateless
// function of (seed, dropout layer 1..7, window, position, channel), 32-bit integers throughout:
//
//     mix(h):  h ^= h >> 16;  h *= 0x7feb352d;  h ^= h >> 15;  h *= 0x846ca68b;  h ^= h >> 16
//     h = mix(seed_lo + layer * 0x9e3779b9)         seed_lo, seed_hi: the halves of the 64-bit seed
//     h = mix(h ^ seed_hi)
//     h = mix(h + window)
//     h = mix(h ^ (position * 256 + channel))
//     kept  <=>  (h >> 8) >= floor(rate * 2^24)
//
// A kept element is multiplied by (float)(1 / (1 - rate)), which is exactly 1 at rate 0, where the
// threshold is 0 and everything is kept.  Nothing in it knows the launch geometry.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dbh_network.h"

namespace dbh_train {

// The limit of one call: n_windows * input_size <= kMaxBatchSamples (256 windows of 1,024 samples
// are a quarter of it, 20 of 16,384 a third).  Batch statistics are per call, so a batch is never
// split; the workspace grows by about 1.3 KB per sample (dbh_gradients_workspace_bytes).
constexpr int64_t kMaxBatchSamples = (int64_t)1 << 20;
constexpr int kBnTotal = dbh_net::bn_channel_offset(dbh_net::kNumBn);   // 480 channels, BN 1..7
constexpr int kStatsFloats = 2 * kBnTotal; // batch mean then batch variance per layer

__host__ __device__ inline uint32_t mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

__host__ __device__ inline uint32_t dropout_bits(uint32_t seed_lo, uint32_t seed_hi, uint32_t layer,
                                                 uint32_t window, uint32_t position,
                                                 uint32_t channel) {
    uint32_t h = mix32(seed_lo + layer * 0x9e3779b9u);
    h = mix32(h ^ seed_hi);
    h = mix32(h + window);
    h = mix32(h ^ (position * 256u + channel));
    return h >> 8;
}

size_t workspace_bytes(int n_classes, int input_size, int64_t n_windows);

// Frozen blocks: block j = 1..7 ends at batch normalisation j, so it holds
// the convolutions that read stage j - 1 (dbh_network.h: in == j - 1) and that normalisation.  With
// the first f blocks frozen, the first frozen_convs(f) = 0, 1, 4, 7, 9, 16, 17, 19 convolutions and
// batch_normalization_1 .. f take no gradient and no update; the head (conv1d_20) is never frozen.
constexpr int kMaxFrozenBlocks = dbh_net::kNumBn;
constexpr int frozen_convs(int frozen_blocks) {
    int n = 0;
    for (int i = 0; i < dbh_net::kNumConvs; ++i) n += dbh_net::kConvs[i].in < frozen_blocks ? 1 : 0;
    return n;
}
static_assert(frozen_convs(0) == 0 && frozen_convs(4) == 9 && frozen_convs(kMaxFrozenBlocks) == 19,
              "blocks follow the stages of dbh_network.h");
inline bool frozen_ok(int frozen_blocks) { return frozen_blocks >= 0 && frozen_blocks <= kMaxFrozenBlocks; }

// Everything on the device, queued on `stream`, nothing synchronised.  weights: the canonical blob
// (16-byte aligned); grads: the same layout, moving-statistics slots zero; stats: kStatsFloats.
// frozen_blocks (0 .. kMaxFrozenBlocks, the caller's to check): the forward pass is the same; the
// backward pass ends at the first trainable convolution's weight gradient, without that layer's
// data gradient, and the frozen tensors' slots of grads are zero like the moving-statistics slots.
hipError_t gradients(const float* weights, int n_classes, int input_size, const float* x,
                     const int32_t* labels, int64_t n_windows, float dropout_rate, uint64_t seed,
                     double* mean_loss, int64_t* n_correct, float* grads, float* stats,
                     void* workspace, hipStream_t stream, int frozen_blocks);

// The same forward pass in Keras's test phase: the blob's moving statistics in place of the batch's,
// no dropout, nothing written to the weights.  Queued, not synchronised.  The losses are ADDED, in
// window order, to *loss_sum, the hits to *n_correct (zero them in front of a set's first chunk);
// window_loss (n_windows doubles) may be null.  The workspace is workspace_bytes()'.
hipError_t evaluate(const float* weights, int n_classes, int input_size, const float* x,
                    const int32_t* labels, int64_t n_windows, double* loss_sum, int64_t* n_correct,
                    double* window_loss, void* workspace, hipStream_t stream);

}  // namespace dbh_train
