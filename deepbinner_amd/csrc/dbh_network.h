// dbh_network.h — the Deepbinner network (reference network_architecture.py:18-95), once: what the
// persistent kernel's layout (dbh_layout.h), both weight packers (dbh_pack.h), the general path
// (dbh_general.hip) and the training step (dbh_train.hip) have to agree on.  Plain C++17, no HIP:
// host code, device code and a g++ program (oracle/api_host_test.cpp, through which
// tests/test_api_host.py holds it to model_format.py, the specification) read the same lines.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIP__
#define DBH_NET_HD __host__ __device__
#else
#define DBH_NET_HD
#endif

namespace dbh_net {

constexpr int kNumConvs = 20;
constexpr int kNumBn = 7;

// conv1d_1..20 (index = Keras layer number - 1).  cout 0: the class count (see cout()).  in, out:
// the stages, as indices into len[] of stage_lengths(), whose lengths the convolution reads and
// produces - the two strided layers step to the next stage themselves, every other step is the
// MaxPooling1D(2) behind conv1d_4, 7, 9, the concatenation of conv1d_10, 11, 13, 16, and conv1d_19.
struct Conv { int k, cin, cout, stride, in, out; };
constexpr Conv kConvs[kNumConvs] = {
    {3, 1, 48, 2, 0, 1},                                               // conv1d_1
    {3, 48, 48, 1, 1, 1},  {3, 48, 48, 1, 1, 1}, {3, 48, 48, 1, 1, 1}, // conv1d_2..4
    {1, 48, 16, 1, 2, 2},  {3, 16, 48, 1, 2, 2}, {3, 48, 48, 1, 2, 2}, // conv1d_5..7
    {3, 48, 48, 1, 3, 3},  {3, 48, 48, 1, 3, 3},                       // conv1d_8, 9
    {1, 48, 48, 1, 4, 4},  {1, 48, 48, 1, 4, 4},                       // conv1d_10, 11 (inception)
    {1, 48, 16, 1, 4, 4},  {3, 16, 48, 1, 4, 4},                       // conv1d_12, 13
    {1, 48, 16, 1, 4, 4},  {3, 16, 48, 1, 4, 4}, {3, 48, 48, 1, 4, 4}, // conv1d_14..16
    {3, 192, 48, 2, 5, 6},                                             // conv1d_17
    {3, 48, 48, 1, 6, 6},  {3, 48, 48, 1, 6, 6},                       // conv1d_18, 19
    {1, 48, 0, 1, 7, 7},                                               // conv1d_20
};
constexpr int cout(int i, int n_classes) { return kConvs[i].cout ? kConvs[i].cout : n_classes; }

// batch_normalization_1..7 (and the dropouts behind them): number j normalises the tensor of stage
// j - conv1d_1's output, the pooled tensors, conv1d_17's output - for the convolutions with in == j
constexpr int kBnChannels[kNumBn] = {48, 48, 48, 48, 192, 48, 48};
constexpr double kBnEps = 1e-3;            // model_format.BN_EPSILON
// channels of the batch normalisations before number j (j = kNumBn: of all)
constexpr int bn_channel_offset(int j) {
    int at = 0;
    for (int i = 0; i < j; ++i) at += kBnChannels[i];
    return at;
}

// positions of a window of L samples at every stage (TensorFlow's rules: a strided SAME
// convolution rounds up, a 'valid' pool of two rounds down)
DBH_NET_HD constexpr void stage_lengths(int L, int len[8]) {
    len[0] = L;
    len[1] = (L + 1) / 2;                                  // conv1d_1
    for (int i = 2; i <= 5; ++i) len[i] = len[i - 1] / 2;  // four pools
    len[6] = (len[5] + 1) / 2;                             // conv1d_17
    len[7] = len[6] / 2;                                   // the last pool
}

// SAME padding on the left of a convolution (TensorFlow: the odd one goes right)
DBH_NET_HD constexpr int same_pad_left(int k, int stride, int lin, int lout) {
    const int total = (lout - 1) * stride + k - lin;
    return total > 0 ? total / 2 : 0;
}

// The canonical blob (model_format.py: "flat blob layout"), in floats: per convolution its kernel
// [k][C_in][C_out] then its bias; then per batch normalisation gamma, beta, moving mean, moving
// variance, C floats each.
constexpr size_t blob_kernel(int i, int n_classes) {
    size_t at = 0;
    for (int j = 0; j < i; ++j) at += (size_t)(kConvs[j].k * kConvs[j].cin + 1) * cout(j, n_classes);
    return at;
}
constexpr size_t blob_bias(int i, int n_classes) { return blob_kernel(i + 1, n_classes) - cout(i, n_classes); }
constexpr size_t blob_bn(int j, int n_classes) {
    return blob_kernel(kNumConvs, n_classes) + (size_t)4 * bn_channel_offset(j);
}
constexpr int64_t param_count(int n_classes) { return (int64_t)blob_bn(kNumBn, n_classes); }

// A batch normalisation at inference as y = x * scale + shift, in fp64.  (The library is built with
// -ffp-contract=off: the bits of the packed images depend on these two lines as they are written.)
struct BnFold { double scale, shift; };
inline BnFold bn_fold(float gamma, float beta, float mean, float var) {
    const double scale = (double)gamma / std::sqrt((double)var + kBnEps);
    return {scale, (double)beta - (double)mean * scale};
}

}  // namespace dbh_net

#undef DBH_NET_HD
