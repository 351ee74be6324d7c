// dbh_pack.h — both weight packers of libdeepbinner_hip.so, as host-only code: the canonical blob
// (dbh_network.h: blob_kernel / blob_bias / blob_bn) into the persistent kernel's image
// (dbh_layout.h) and into the general path's (dbh_general.hip: conv_kernel).  Nothing but index
// arithmetic and the fp64 folds, so oracle/api_host_test.cpp compiles this very header with g++ and
// tests/test_api_host.py holds both images, bit for bit, to tests/golden/packed_digests.txt.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#include "dbh_layout.h"
#include "dbh_network.h"

namespace dbh_pack {

// a batch normalisation of the blob (gamma, beta, mean, var: c_n each) as scale and shift x unit
inline void fold_bn(const float* q, int c_n, float* scale, float* shift, float unit) {
    for (int c = 0; c < c_n; ++c) {
        const dbh_net::BnFold f = dbh_net::bn_fold(q[c], q[c_n + c], q[2 * c_n + c], q[3 * c_n + c]);
        scale[c] = (float)f.scale;
        shift[c] = (float)f.shift * unit;
    }
}

// canonical blob -> the persistent kernel's packed buffer (layout: dbh_layout.h)
inline void pack_persistent(const float* w, int n_classes, std::vector<float>& packed) {
    using namespace dbh;
    namespace net = dbh_net;
    packed.assign(kPackedFloats, 0.f);
    // BN2 (scale s, shift t per channel of conv1d_4's pooled output) is folded into conv1d_5, a 1x1
    // convolution with no padding to get in the way: W5'[c][o] = W5[c][o] s[c], b5'[o] = b5[o] +
    // sum_c W5[c][o] t[c] - exact algebra, in fp64 here; the forward kernel feeds conv1d_5 the
    // pooled values as they are (dbh_forward.hip: stage_b_chain)
    net::BnFold fold[48];
    const float* bn2 = w + net::blob_bn(1, n_classes);
    for (int c = 0; c < 48; ++c) fold[c] = net::bn_fold(bn2[c], bn2[48 + c], bn2[96 + c], bn2[144 + c]);
    static_assert(kBnChannels[1] == 48 && kConv[4].cin == 48 && kConv[4].taps == 1, "");
    for (int i = 0; i < kNumConvs; ++i) {
        const int k = kConv[i].taps, cin = kConv[i].cin, cout = net::cout(i, n_classes);
        const float* kernel = w + net::blob_kernel(i, n_classes);      // [k][cin][cout]
        const float* bias = w + net::blob_bias(i, n_classes);
        float* dst = packed.data() + weight_offset(i);
        if (i == 0) {
            // conv1d_1 stays [tap][cout]: one value per lane and channel group, read once per workgroup
            for (int tap = 0; tap < 3; ++tap)
                for (int c = 0; c < cout; ++c) dst[tap * 48 + c] = kernel[(tap * cin) * cout + c];
        } else {
            // One matrix per tap, or the Winograd matrices V = G g of F(2,3) / F(4,3), computed in
            // fp64; each in fragment order.
            const int wino = kConv[i].wino, mats = wino == 4 ? 6 : wino == 2 ? 4 : k;
            const int sp_n = cin / 8, nt = kConv[i].cout_pad / 16;
            const bool by_tile = wino == 4 || wino2_by_tile(i);
            static const double G23[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
            static const double G43[6][3] = {{1. / 4, 0, 0},  {-1. / 6, -1. / 6, -1. / 6},  {-1. / 6, 1. / 6, -1. / 6},
                                             {1. / 24, 1. / 12, 1. / 6}, {1. / 24, -1. / 12, 1. / 6}, {0, 0, 1}};
            for (int m = 0; m < mats; ++m)
                for (int sp = 0; sp < sp_n; ++sp)
                    for (int t = 0; t < nt; ++t)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 2; ++e) {
                                // (conv1d_2's k-steps walk the channels in the order conv1d_1's
                                // transposed MFMAs leave them in registers: dbh_layout.h)
                                const int ci = frag_cin(i, sp, lane >> 4, e);
                                const int co = 16 * t + (lane & 15);
                                float v = 0.f;
                                if (co < cout && !wino) {
                                    v = kernel[((size_t)m * cin + ci) * cout + co];
                                } else if (co < cout) {
                                    const double* G = wino == 4 ? G43[m] : G23[m];
                                    double sum = 0.0;
                                    for (int tap = 0; tap < 3; ++tap)
                                        sum += G[tap] * (double)kernel[((size_t)tap * cin + ci) * cout + co];
                                    v = (float)sum;
                                }
                                if (i == 4) v = (float)((double)v * fold[ci].scale);   // BN2's scale
                                // Matrix-major [m][sp][t][lane][e], or by N tile (F(4,3), and the
                                // F(2,3) layers of wino2_by_tile): [t][sp][m >> 1][lane][m & 1][e],
                                // so that one 16-byte LDS read fetches the fragments of two
                                // matrices for two k-steps.
                                const size_t idx =
                                    by_tile ? (((((size_t)t * sp_n + sp) * (mats / 2) + (m >> 1)) * 64 + lane) * 2 + (m & 1)) * 2 + e
                                            : ((((size_t)m * sp_n + sp) * nt + t) * 64 + lane) * 2 + e;
                                dst[idx] = v;
                            }
        }
        float* bdst = packed.data() + bias_offset(i);
        for (int c = 0; c < cout; ++c) bdst[c] = bias[c] * kActScale;      // (exact: a power of two)
        if (i == 4)       // ... and BN2's shift, through conv1d_5's weights, in its bias
            for (int c = 0; c < cout; ++c) {
                double extra = 0.0;
                for (int ci = 0; ci < cin; ++ci) extra += (double)kernel[(size_t)ci * cout + c] * fold[ci].shift;
                bdst[c] = (float)(((double)bias[c] + extra) * (double)kActScale);
            }
    }
    for (int i = 0; i < kNumBn; ++i)
        fold_bn(w + net::blob_bn(i, n_classes), kBnChannels[i], packed.data() + bn_scale_offset(i),
                packed.data() + bn_shift_offset(i), kActScale);
}

// where the pieces of the general image lie (floats), each 16-byte aligned
struct GeneralOffsets {
    size_t w_off[dbh_net::kNumConvs] = {}, b_off[dbh_net::kNumConvs] = {};
    size_t sc_off[dbh_net::kNumBn] = {}, sh_off[dbh_net::kNumBn] = {};
};

// canonical blob -> the general path's image: per convolution its kernel in fragment order
// [tap][cin / 16][cout / 16][lane][4] (conv1d_1 and conv1d_20 as stored) then its bias, then the
// batch normalisations' scale and shift
inline std::vector<float> pack_general(const float* canon, int n_classes, GeneralOffsets* off) {
    namespace net = dbh_net;
    std::vector<float> packed;
    auto take = [&](size_t count) {
        const size_t at = packed.size();
        packed.resize(at + ((count + 3) & ~(size_t)3), 0.f);
        return at;
    };
    for (int i = 0; i < net::kNumConvs; ++i) {
        const int k = net::kConvs[i].k, cin = net::kConvs[i].cin, cout = net::cout(i, n_classes);
        const float* kernel = canon + net::blob_kernel(i, n_classes);     // [k][cin][cout]
        const float* bias = canon + net::blob_bias(i, n_classes);
        off->w_off[i] = take((size_t)k * cin * cout);
        float* dst = packed.data() + off->w_off[i];
        if (i == 0 || i == net::kNumConvs - 1) {
            std::copy(kernel, kernel + (size_t)k * cin * cout, dst);    // as stored
        } else {
            const int G = cin / 16, NT = cout / 16;
            for (int t = 0; t < k; ++t)
                for (int g = 0; g < G; ++g)
                    for (int nt = 0; nt < NT; ++nt)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 4; ++j) {
                                const int ci = 16 * g + 4 * (lane >> 4) + j;
                                const int co = 16 * nt + (lane & 15);
                                dst[((((size_t)t * G + g) * NT + nt) * 64 + lane) * 4 + j] =
                                    kernel[((size_t)t * cin + ci) * cout + co];
                            }
        }
        off->b_off[i] = take((size_t)cout);
        std::copy(bias, bias + cout, packed.data() + off->b_off[i]);
    }
    for (int i = 0; i < net::kNumBn; ++i) {
        off->sc_off[i] = take((size_t)net::kBnChannels[i]);
        off->sh_off[i] = take((size_t)net::kBnChannels[i]);
        fold_bn(canon + net::blob_bn(i, n_classes), net::kBnChannels[i], packed.data() + off->sc_off[i],
                packed.data() + off->sh_off[i], 1.f);
    }
    return packed;
}

}  // namespace dbh_pack
