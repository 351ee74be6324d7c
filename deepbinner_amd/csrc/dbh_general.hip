// dbh_general.hip — the general forward path (dbh_general.h): any even input size L in
// [96, 16384] and any class count C in [2, 256], fp32 throughout.
//
// The network (reference network_architecture.py:18-95) runs layer by layer over a chunk of
// windows, activations channels-last [window][position][channel] in device memory:
//   front      slice + z-normalise each window (or take it as given) and conv1d_1 on the VALU
//   conv       every other convolution as an implicit GEMM on v_mfma_f32_16x16x4_f32:
//              M = windows x output positions, N = C_out, K = taps x C_in; the preceding batch
//              normalisation applied to the input as it is loaded (taps in the SAME padding stay
//              zero: TensorFlow pads the normalised tensor), bias + ReLU and the following
//              max-pool in the epilogue; the four inception branches write their channel slices
//              of one 192-channel buffer (pool(concat) = concat(pool))
//   head       conv1d_20 + ReLU + global average + softmax, one workgroup per window
// No atomics and no cross-window arithmetic: a window's result does not depend on the chunk,
// the batch or the stream it travels in.
#include "dbh_general.h"
#include "dbh_seam.h"
#include "dbh_trees.h"

#include <algorithm>
#include <cmath>

namespace dbh_gen {
namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kRowTiles = 2;                       // 16-row M tiles per wave
constexpr int kRowsPerBlock = 4 * 16 * kRowTiles;  // four waves
constexpr size_t kChunkBudget = (size_t)128 << 20; // activation bytes per chunk (about)
constexpr int kMaxL7 = kMaxInput / 128;            // positions reaching the head at L = 16384

// input transform of a convolution, applied as its operand is loaded
enum { kInPlain = 0, kInBn = 1, kInAvgBn = 2 };

// ---- front: slice + normalise (+ given fp32 windows) and conv1d_1 (k 3, stride 2, 1 -> 48) ---
// The persistent path's arithmetic (dbh_seam.h: window bounds, exact integer sums, fp64 constants), so
// that the windows agree with it and with classify.py:330-357.
__global__ __launch_bounds__(kThreads) void front_kernel(
    const float* __restrict__ x, const int16_t* __restrict__ samples,
    const long long* __restrict__ offsets, int steps, int side, long long w0, int L, int L1,
    const float* __restrict__ w1, const float* __restrict__ b1, float* __restrict__ y) {
    __shared__ long long red[2][kThreads / 64];
    __shared__ float wts[4 * 48];
    const int tid = threadIdx.x;
    const long long win = w0 + blockIdx.x;
    if (tid < 3 * 48) wts[tid] = w1[tid];
    else if (tid < 4 * 48) wts[tid] = b1[tid - 3 * 48];

    const int16_t* src = nullptr;
    int cnt = 0, pad_left = 0;
    double mean = 0.0, inv = 1.0;
    if (!x) {
        const long long read = win / steps;
        const int step = (int)(win - read * steps);
        const long long base = offsets[read];
        const long long len = offsets[read + 1] - base;
        long long a, b;
        dbh::window_bounds(len, step, side, L, &a, &b);
        cnt = (int)(b - a);
        pad_left = side == 0 ? 0 : L - cnt;
        src = samples + base + a;
        long long s1 = 0, s2 = 0;
        for (int k = tid; k < cnt; k += kThreads) {
            const long long v = src[k];
            s1 += v;
            s2 += v * v;
        }
        for (int off = 32; off >= 1; off >>= 1) {
            s1 += __shfl_xor(s1, off);
            s2 += __shfl_xor(s2, off);
        }
        if ((tid & 63) == 0) {
            red[0][tid >> 6] = s1;
            red[1][tid >> 6] = s2;
        }
        __syncthreads();
        s1 = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        s2 = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        dbh::mean_std(s1, s2, cnt, &mean, &inv);
    } else {
        __syncthreads();
    }
    const float* xw = x ? x + win * L : nullptr;
    auto value = [&](int i) -> float {          // window sample i; 0 in the padding
        if (i >= L) return 0.f;                  // conv1d_1's SAME padding (one on the right)
        if (xw) return xw[i];
        const int k = i - pad_left;
        return (k >= 0 && k < cnt) ? (float)(((double)src[k] - mean) * inv) : 0.f;
    };
    float* out = y + (long long)blockIdx.x * L1 * 48;
    for (int idx = tid; idx < L1 * 48; idx += kThreads) {
        const int p = idx / 48, c = idx - p * 48;
        float s = 0.f;
        s = fmaf(value(2 * p), wts[c], s);
        s = fmaf(value(2 * p + 1), wts[48 + c], s);
        s = fmaf(value(2 * p + 2), wts[96 + c], s);
        s += wts[144 + c];
        out[idx] = s > 0.f ? s : 0.f;
    }
}

// ---- convolution as an implicit GEMM ---------------------------------------------------------
struct ConvArgs {
    const float* x;        // [n_win][lin][in_stride]
    const float* w;        // fragment order [tap][cin / 16][cout / 16][lane][4]
    const float* bias;     // [cout]
    const float* sc;       // BN scale / shift of the input channels (kInBn, kInAvgBn)
    const float* sh;
    float* y;              // [n_win][lconv (/2 if pooled)][out_stride], channels from out_off
    long long n_win;
    int lin, in_stride, lconv, out_stride, out_off;
};

// One wave: kRowTiles x 16 output rows (window, position) x all C_out.  Lane l loads the four
// input channels 16g + 4(l >> 4) .. +3 of row l & 15 as one float4 and feeds them to four MFMAs
// (k-step j takes element j): the k order is permuted the same way in the packed weights.
// Pooled layers compute only the 2 * (lconv / 2) positions the 'valid' pool reads, so output row
// pairs (2i, 2i + 1) sit in one lane's accumulator (rows 4(l >> 4) .. +3).
template <int K, int S, int CIN, int COUT, int IN, bool POOL>
__global__ __launch_bounds__(kThreads) void conv_kernel(ConvArgs a) {
    static_assert(CIN % 16 == 0 && COUT % 16 == 0, "channel counts come in 16s");
    static_assert(IN != kInAvgBn || K == 1, "the average pool feeds a 1x1 convolution");
    constexpr int G = CIN / 16, NT = COUT / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int lrows = POOL ? (a.lconv & ~1) : a.lconv;
    const long long M = a.n_win * lrows;
    const long long m_base = ((long long)blockIdx.x * 4 + wave) * (16 * kRowTiles);
    if (m_base >= M) return;
    const int pad_l = dbh_net::same_pad_left(K, S, a.lin, a.lconv);

    long long row_base[kRowTiles];
    int ipos[kRowTiles];
    bool ok[kRowTiles];
#pragma unroll
    for (int mt = 0; mt < kRowTiles; ++mt) {
        const long long m = m_base + mt * 16 + r;
        ok[mt] = m < M;
        const long long win = ok[mt] ? m / lrows : 0;
        const int pos = ok[mt] ? (int)(m - win * lrows) : 0;
        row_base[mt] = win * a.lin;
        ipos[mt] = pos * S - pad_l;
    }
    floatx4 acc[kRowTiles][NT];
#pragma unroll
    for (int mt = 0; mt < kRowTiles; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (int t = 0; t < K; ++t) {
        for (int g = 0; g < G; ++g) {
            const int c0 = 16 * g + 4 * q;
            floatx4 scale = {1.f, 1.f, 1.f, 1.f}, shift = {0.f, 0.f, 0.f, 0.f};
            if (IN != kInPlain) {
                scale = *(const floatx4*)(a.sc + c0);
                shift = *(const floatx4*)(a.sh + c0);
            }
            floatx4 av[kRowTiles];
#pragma unroll
            for (int mt = 0; mt < kRowTiles; ++mt) {
                const int ip = ipos[mt] + t;
                const bool valid = ok[mt] && ip >= 0 && ip < a.lin;
                floatx4 v = {0.f, 0.f, 0.f, 0.f};
                if (IN == kInAvgBn) {
                    // AveragePooling1D(3, 1, 'same') of the normalised input: valid taps only
                    if (valid) {
                        float n = 0.f;
                        for (int d = -1; d <= 1; ++d) {
                            const int jp = ip + d;
                            if (jp < 0 || jp >= a.lin) continue;
                            const floatx4 u = *(const floatx4*)(a.x + (row_base[mt] + jp) * a.in_stride + c0);
                            v += u * scale + shift;
                            n += 1.f;
                        }
                        v = v / n;
                    }
                } else if (valid) {
                    v = *(const floatx4*)(a.x + (row_base[mt] + ip) * a.in_stride + c0);
                    if (IN == kInBn) v = v * scale + shift;
                }
                av[mt] = v;
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const floatx4 bv = *(const floatx4*)(a.w + ((((size_t)t * G + g) * NT + nt) * 64 + lane) * 4);
#pragma unroll
                for (int mt = 0; mt < kRowTiles; ++mt) {
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][0], bv[0], acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][1], bv[1], acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][2], bv[2], acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][3], bv[3], acc[mt][nt], 0, 0, 0);
                }
            }
        }
    }
    // epilogue: D row 4q + i, column r of each tile
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = 16 * nt + r;
        const float b = a.bias[n];
#pragma unroll
        for (int mt = 0; mt < kRowTiles; ++mt) {
            const long long m0 = m_base + mt * 16 + 4 * q;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float s = acc[mt][nt][i] + b;
                v[i] = s > 0.f ? s : 0.f;
            }
            if (POOL) {
                // m is even exactly where the position is (lrows is even): pooled row m / 2
#pragma unroll
                for (int i = 0; i < 4; i += 2)
                    if (m0 + i < M)
                        a.y[((m0 + i) >> 1) * a.out_stride + a.out_off + n] = fmaxf(v[i], v[i + 1]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (m0 + i < M) a.y[(m0 + i) * a.out_stride + a.out_off + n] = v[i];
            }
        }
    }
}

// ---- head: BN7 -> conv1d_20 (1x1, 48 -> C) + ReLU -> global average -> softmax ----------------
// EVIDENCE: the post-ReLU value of every position and class, whose mean is the logit, is stored as
// well - ev [window][l7][C], coalesced over the class threads (include/deepbinner_hip.h, "locate").
// The sum and the softmax are the same lines either way: the probabilities do not change by a bit.
template <bool EVIDENCE>
__global__ __launch_bounds__(kThreads) void head_kernel(const float* __restrict__ x, int l7,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ bias,
                                                        const float* __restrict__ sc,
                                                        const float* __restrict__ sh, int C,
                                                        long long w0, float* __restrict__ probs,
                                                        float* __restrict__ ev) {
    __shared__ float xs[kMaxL7 * 48];
    __shared__ float red[kThreads];
    const int tid = threadIdx.x;
    const float* src = x + (long long)blockIdx.x * l7 * 48;
    for (int i = tid; i < l7 * 48; i += kThreads) {
        const int c = i % 48;
        xs[i] = src[i] * sc[c] + sh[c];
    }
    __syncthreads();
    const bool valid = tid < C;
    float logit = -INFINITY;
    if (valid) {
        float sum = 0.f;
        for (int p = 0; p < l7; ++p) {
            float s = 0.f;
            for (int ci = 0; ci < 48; ++ci) s = fmaf(xs[p * 48 + ci], w[ci * C + tid], s);
            s += bias[tid];
            sum += s > 0.f ? s : 0.f;
            if (EVIDENCE) ev[((w0 + blockIdx.x) * l7 + p) * C + tid] = s > 0.f ? s : 0.f;
        }
        logit = sum / (float)l7;
    }
    // softmax over the block; fixed reduction trees
    red[tid] = logit;
    __syncthreads();
    for (int half = kThreads / 2; half >= 1; half >>= 1) {
        if (tid < half) red[tid] = fmaxf(red[tid], red[tid + half]);
        __syncthreads();
    }
    const float mx = red[0];
    __syncthreads();
    const float e = valid ? expf(logit - mx) : 0.f;
    red[tid] = e;
    __syncthreads();
    for (int half = kThreads / 2; half >= 1; half >>= 1) {
        if (tid < half) red[tid] += red[tid + half];
        __syncthreads();
    }
    if (valid) probs[(w0 + blockIdx.x) * C + tid] = e / red[0];
}

// ---- merge for C <= 256: one workgroup per read ----------------------------------------------
// classify.py:368-374 (min for class 0, max for the barcodes), make_sum_to_one in fp64
// (classify.py:387-393) and the top-2 call (classify.py:285-295; ties go to the lower class, as
// the reference's stable sort gives them).
__global__ __launch_bounds__(kThreads) void merge_kernel(const float* __restrict__ wprobs,
                                                         int steps, int C, double score_diff,
                                                         float* __restrict__ probs,
                                                         int* __restrict__ calls) {
    __shared__ double rv[kThreads];
    __shared__ int ri[kThreads];
    const long long read = blockIdx.x;
    const int c = threadIdx.x;
    const bool valid = c < C;
    float merged = 0.f;
    if (valid) {
        const float* src = wprobs + read * steps * C + c;
        merged = src[0];
        for (int s = 1; s < steps; ++s) {
            const float v = src[(long long)s * C];
            merged = c == 0 ? fminf(merged, v) : fmaxf(merged, v);
        }
    }
    double p = (double)merged;
    const double rest = dbh::tree_sum<kThreads>(rv, c, (valid && c > 0) ? p : 0.0);
    if (c == 0) rv[0] = p;
    __syncthreads();
    const double p0 = rv[0];
    __syncthreads();
    if (c > 0) p = p * ((1.0 - p0) / rest);
    if (valid) probs[read * C + c] = (float)p;
    // best: highest probability, lowest class among equals; then the runner-up (dbh_trees.h)
    int best;
    const double best_v = dbh::tree_best<kThreads>(rv, ri, c, valid ? p : -1.0, &best);
    const double second = dbh::tree_max<kThreads>(rv, c, (valid && c != best) ? p : -1.0);
    if (c == 0) calls[read] = (best != 0 && (best_v - second) >= score_diff) ? best : 0;
}

// ---- host ------------------------------------------------------------------------------------
// Convolution LAYER (0-based) of dbh_network.h's table, which gives its shapes and lengths.  IN: how
// its input is transformed as it is loaded (kInBn, kInAvgBn: by the batch normalisation of its
// input stage); POOL: whether the max-pool follows.
template <int LAYER, int IN, bool POOL>
hipError_t conv(const Net& net, const float* x, float* y, int out_stride, int out_off,
                int64_t n_win, hipStream_t stream) {
    constexpr dbh_net::Conv kL = dbh_net::kConvs[LAYER];
    const float* p = net.d_params;
    constexpr bool bn = IN != kInPlain;      // batch normalisation kL.in, 0-based kL.in - 1
    const ConvArgs a = {x, p + net.w_off[LAYER], p + net.b_off[LAYER],
                        bn ? p + net.sc_off[kL.in - 1] : nullptr, bn ? p + net.sh_off[kL.in - 1] : nullptr,
                        y, n_win, net.len[kL.in], kL.cin, net.len[kL.out], out_stride, out_off};
    const long long rows = (long long)n_win * (POOL ? (a.lconv & ~1) : a.lconv);
    if (rows == 0) return hipSuccess;
    const long long blocks = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL((conv_kernel<kL.k, kL.stride, kL.cin, kL.cout, IN, POOL>),
                       dim3((unsigned)blocks), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t create(const float* canon, int n_classes, int input_size, Net* net) {
    Net n;
    n.L = input_size;
    n.C = n_classes;
    dbh_net::stage_lengths(input_size, n.len);
    const std::vector<float> packed = dbh_pack::pack_general(canon, n_classes, &n);
    // activations per window: two ping-pong buffers of conv1d_1's size, the inception's 16- and
    // 48-channel intermediates, the 192-channel concat, two buffers for conv1d_17 .. conv1d_19
    n.act_floats = (size_t)2 * n.len[1] * 48 + (size_t)n.len[4] * 64 + (size_t)n.len[5] * 192 +
                   (size_t)2 * n.len[6] * 48;
    n.chunk = std::max<int64_t>(1, std::min<int64_t>(4096, (int64_t)(kChunkBudget / (n.act_floats * 4))));
    hipError_t e = hipMalloc((void**)&n.d_params, packed.size() * sizeof(float));
    if (e != hipSuccess) return e;
    e = hipMemcpy(n.d_params, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(n.d_params);
        return e;
    }
    *net = n;
    return hipSuccess;
}

void destroy(Net* net) {
    if (net->d_params) (void)hipFree(net->d_params);
    net->d_params = nullptr;
}

size_t activation_bytes(const Net& net, int64_t n_windows) {
    const int64_t w = std::min<int64_t>(std::max<int64_t>(n_windows, 1), net.chunk);
    return (size_t)w * net.act_floats * sizeof(float);
}

hipError_t forward(const Net& net, const float* x, const int16_t* samples, const int64_t* offsets,
                   int steps, int side, int64_t n_windows, float* probs, float* evidence, void* act,
                   hipStream_t stream) {
    const int* len = net.len;
    for (int64_t w0 = 0; w0 < n_windows; w0 += net.chunk) {
        const int64_t n = std::min<int64_t>(net.chunk, n_windows - w0);
        float* P = (float*)act;
        float* Q = P + (size_t)n * len[1] * 48;
        float* T = Q + (size_t)n * len[1] * 48;           // [n][len4][16] then [n][len4][48]
        float* T48 = T + (size_t)n * len[4] * 16;
        float* Cc = T + (size_t)n * len[4] * 64;
        float* F1 = Cc + (size_t)n * len[5] * 192;
        float* F2 = F1 + (size_t)n * len[6] * 48;
        hipLaunchKernelGGL(front_kernel, dim3((unsigned)n), dim3(kThreads), 0, stream, x,
                           samples, (const long long*)offsets, steps, side, (long long)w0,
                           net.L, len[1], net.d_params + net.w_off[0],
                           net.d_params + net.b_off[0], P);
        hipError_t e = hipGetLastError();
        // stage B: BN1 -> conv2 -> conv3 -> conv4 -> pool
        if (e == hipSuccess) e = conv<1, kInBn, false>(net, P, Q, 48, 0, n, stream);
        if (e == hipSuccess) e = conv<2, kInPlain, false>(net, Q, P, 48, 0, n, stream);
        if (e == hipSuccess) e = conv<3, kInPlain, true>(net, P, Q, 48, 0, n, stream);
        // stage C: BN2 -> conv5 -> conv6 -> conv7 -> pool
        if (e == hipSuccess) e = conv<4, kInBn, false>(net, Q, P, 16, 0, n, stream);
        if (e == hipSuccess) e = conv<5, kInPlain, false>(net, P, Q, 48, 0, n, stream);
        if (e == hipSuccess) e = conv<6, kInPlain, true>(net, Q, P, 48, 0, n, stream);
        // stage D: BN3 -> conv8 -> conv9 -> pool
        if (e == hipSuccess) e = conv<7, kInBn, false>(net, P, Q, 48, 0, n, stream);
        if (e == hipSuccess) e = conv<8, kInPlain, true>(net, Q, P, 48, 0, n, stream);
        // stage E: the inception block on BN4(P), each branch pooled into its slice of Cc
        if (e == hipSuccess) e = conv<9, kInAvgBn, true>(net, P, Cc, 192, 0, n, stream);
        if (e == hipSuccess) e = conv<10, kInBn, true>(net, P, Cc, 192, 48, n, stream);
        if (e == hipSuccess) e = conv<11, kInBn, false>(net, P, T, 16, 0, n, stream);
        if (e == hipSuccess) e = conv<12, kInPlain, true>(net, T, Cc, 192, 96, n, stream);
        if (e == hipSuccess) e = conv<13, kInBn, false>(net, P, T, 16, 0, n, stream);
        if (e == hipSuccess) e = conv<14, kInPlain, false>(net, T, T48, 48, 0, n, stream);
        if (e == hipSuccess) e = conv<15, kInPlain, true>(net, T48, Cc, 192, 144, n, stream);
        // stage F: BN5 -> conv17 (stride 2)
        if (e == hipSuccess) e = conv<16, kInBn, false>(net, Cc, F1, 48, 0, n, stream);
        // stage G: BN6 -> conv18 -> conv19 -> pool
        if (e == hipSuccess) e = conv<17, kInBn, false>(net, F1, F2, 48, 0, n, stream);
        if (e == hipSuccess) e = conv<18, kInPlain, true>(net, F2, F1, 48, 0, n, stream);
        // head: BN7 -> conv20 -> ReLU -> mean -> softmax
        if (e == hipSuccess) {
            hipLaunchKernelGGL(evidence ? head_kernel<true> : head_kernel<false>, dim3((unsigned)n),
                               dim3(kThreads), 0, stream, F1, len[7], net.d_params + net.w_off[19],
                               net.d_params + net.b_off[19], net.d_params + net.sc_off[6],
                               net.d_params + net.sh_off[6], net.C, (long long)w0, probs, evidence);
            e = hipGetLastError();
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t merge(const float* wprobs, int64_t n_reads, int steps, int n_classes,
                 double score_diff, float* probs, int32_t* calls, hipStream_t stream) {
    for (int64_t r0 = 0; r0 < n_reads; r0 += (int64_t)1 << 30) {
        const int64_t n = std::min<int64_t>((int64_t)1 << 30, n_reads - r0);
        hipLaunchKernelGGL(merge_kernel, dim3((unsigned)n), dim3(kThreads), 0, stream,
                           wprobs + r0 * steps * n_classes, steps, n_classes, score_diff,
                           probs + r0 * n_classes, (int*)(calls + r0));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dbh_gen
