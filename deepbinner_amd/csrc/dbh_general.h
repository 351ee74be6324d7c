// dbh_general.h — the general forward path of libdeepbinner_hip.so (dbh_general.hip): Deepbinner
// networks of any supported input size L and class count C, layer by layer through device memory.
// The persistent kernel (dbh_forward.hip) keeps the shipped geometry (L = 1024, C <= 32); a model
// created with DBH_MODEL_GENERAL, or of any other geometry, runs here ("General models").
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dbh_pack.h"

namespace dbh_gen {

constexpr int kMinInput = 96;          // the global average needs one position
constexpr int kMaxInput = 16384;
constexpr int kMinClasses = 2;
constexpr int kMaxClasses = 256;

inline bool geometry_ok(int input_size, int n_classes) {
    return input_size >= kMinInput && input_size <= kMaxInput && input_size % 2 == 0 &&
           n_classes >= kMinClasses && n_classes <= kMaxClasses;
}

struct Net : dbh_pack::GeneralOffsets {      // (where the pieces of d_params lie)
    int L = 0, C = 0;
    int len[8] = {};               // dbh_net::stage_lengths(L)
    float* d_params = nullptr;     // packed weights (device): dbh_pack::pack_general
    int64_t chunk = 0;             // windows per pass through the layer chain
    size_t act_floats = 0;         // activation floats per window of a chunk
};

// canonical blob (model_format.py order) -> packed device weights; the geometry is checked by
// the caller.  Returns a HIP error (hipSuccess on success).
hipError_t create(const float* canon, int n_classes, int input_size, Net* net);
void destroy(Net* net);

// device bytes of the activations for a call of n_windows windows (at most one chunk's worth)
size_t activation_bytes(const Net& net, int64_t n_windows);

// Softmax probabilities [n_windows][C] of windows given either as fp32 [n_windows][L] (x != null:
// dbh_predict) or sliced from int16 reads (x == null: window w = read w / steps, scan step
// w % steps, normalised and zero-padded as classify.py:330-357 does).  act: activation_bytes().
// evidence (null: not wanted): [n_windows][len[7]][C], the post-ReLU conv1d_20 output per position
// whose mean over the positions is the logit; the probabilities are the same bits with and without.
hipError_t forward(const Net& net, const float* x, const int16_t* samples, const int64_t* offsets,
                   int steps, int side, int64_t n_windows, float* probs, float* evidence, void* act,
                   hipStream_t stream);

// merge + make_sum_to_one + top-2 call for C <= 256 (the contract of dbh_merge_calls_dev)
hipError_t merge(const float* wprobs, int64_t n_reads, int steps, int n_classes,
                 double score_diff, float* probs, int32_t* calls, hipStream_t stream);

}  // namespace dbh_gen
