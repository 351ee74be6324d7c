// dbh_train.hip — loss and weight gradients of one batch (dbh_train.h).
//
// Layer by layer through device memory, activations channels-last [window][position][channel],
// stored in fp32.  The matrix pipe forms short sums in fp32 (16 channels of a tap; 64 rows of a
// weight gradient); what adds those, every sum over the batch, the batch-norm backward bracket and
// the head run in fp64: tests hold each tensor to four times the error of plain fp32 arithmetic,
// and over few elements (BN7 at the minimum input normalises three) plain fp32 is not reliably there.  What the forward pass keeps for the backward
// pass: every convolution's input as it consumed it (the batch-normalised, dropped-out tensors h1..h7
// and the ReLU outputs a2..a19, which double as the ReLU masks and the pool choices), the inputs of
// the batch normalisations (a1, the pooled tensors, a17) with their batch mean and 1 / std.
//   conv_gemm     forward convolution, and data gradient, as an implicit GEMM on
//                 v_mfma_f32_16x16x4_f32 in conv_kernel's register layout (dbh_general.hip).  Both
//                 read the canonical kernel [k][C_in][C_out] where it lies: the forward B fragment is
//                 four loads of 16 consecutive C_out, the data gradient's - the transposed kernel -
//                 one float4 of four consecutive C_out.  No second weight image is packed.
//   wgrad         weight gradient: C_in x C_out tiles per tap with (window, position) as the
//                 contraction, one partial sum per wave in a workspace, summed in wave order by
//                 reduce_partials (fp64).
//   col_sums      per-channel sums over all rows (batch-norm mean, variance, backward sums; bias
//                 gradients): one fp64 partial per workgroup, summed in workgroup order.
// No atomics: every sum has one order, fixed by the shapes alone.
#include "dbh_train.h"

#include "../../include/deepbinner_hip.h"
#include "dbh_general.h"
#include "dbh_host_layout.h"
#include "dbh_network.h"
#include "dbh_owned.h"
#include "dbh_status.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace dbh_train {
namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kRowTiles = 2;
constexpr int kRowsPerBlock = 4 * 16 * kRowTiles;
constexpr int kMaxPartials = 256;          // partial sums per reduction, at most
constexpr int kMaxL7 = dbh_gen::kMaxInput / 128;

using namespace dbh_net;      // the network: dbh_network.h
using dbh_host::blocks_for;
using dbh_host::Carve;

struct Drop {
    uint32_t seed_lo, seed_hi, layer, threshold;
    float scale;
};

__device__ inline float drop_factor(const Drop& d, long long window, int position, int channel) {
    const uint32_t bits = dropout_bits(d.seed_lo, d.seed_hi, d.layer, (uint32_t)window,
                                       (uint32_t)position, (uint32_t)channel);
    return bits >= d.threshold ? d.scale : 0.f;
}

// ---- conv1d_1 (k 3, stride 2, 1 -> 48) on the VALU ---------------------------------------------
__global__ __launch_bounds__(kThreads) void conv1_forward(const float* __restrict__ x,
                                                          const float* __restrict__ w,
                                                          long long n_win, int L, int L1, int pad_l,
                                                          float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_win * L1 * 48) return;
    const int c = (int)(idx % 48);
    const long long row = idx / 48;
    const long long win = row / L1;
    const int p = (int)(row - win * L1);
    float s = 0.f;
    for (int t = 0; t < 3; ++t) {
        const int i = 2 * p - pad_l + t;
        const float v = (i >= 0 && i < L) ? x[win * L + i] : 0.f;
        s = fmaf(v, w[t * 48 + c], s);
    }
    s += w[144 + c];
    y[idx] = s > 0.f ? s : 0.f;
}

// its weight and bias gradients: per workgroup 4 x 48 fp64 partials (three taps, the bias) - the
// order of conv1d_1's slots in the blob
__global__ __launch_bounds__(kThreads) void conv1_wgrad(const float* __restrict__ x,
                                                        const float* __restrict__ dz,
                                                        long long rows, int L, int L1, int pad_l,
                                                        long long rows_per_block,
                                                        double* __restrict__ part) {
    __shared__ double red[4][kThreads];
    const int tid = threadIdx.x;
    const int c = tid % 48, rl = tid / 48;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (rl < 5) {
        for (long long row = r0 + rl; row < r1; row += 5) {
            const long long win = row / L1;
            const int p = (int)(row - win * L1);
            const double g = (double)dz[row * 48 + c];
            for (int t = 0; t < 3; ++t) {
                const int i = 2 * p - pad_l + t;
                if (i >= 0 && i < L) s[t] += (double)x[win * L + i] * g;
            }
            s[3] += g;
        }
    }
    for (int q = 0; q < 4; ++q) red[q][tid] = s[q];
    __syncthreads();
    if (tid < 192) {
        const int q = tid / 48, cc = tid % 48;
        double sum = 0.0;
        for (int k = 0; k < 5; ++k) sum += red[q][k * 48 + cc];
        part[(long long)blockIdx.x * 192 + tid] = sum;
    }
}

// ---- convolution and data gradient as an implicit GEMM -----------------------------------------
struct GemmArgs {
    const float* a;        // [n_win][la][a_stride], channels from a_off
    const float* w;        // the layer's canonical kernel [k][cin][cout]
    const float* bias;     // forward: [cout]
    const float* mask;     // data gradient: the ReLU output the result passes back through (or null)
    float* y;              // [n_win][ly][y_stride], channels from y_off (mask: same indexing)
    long long n_win;
    int la, a_stride, a_off, ly, y_stride, y_off;
    int k, stride, pad_l, cin, cout;   // of the convolution as the forward pass runs it
    int accumulate;        // data gradient: add to y (the inception branches share one input)
};

// One wave: kRowTiles x 16 rows (window, position) x all CN output channels, contraction over
// taps x CA channels.  Forward: row = output position, tap t reads input position
// p * stride - pad_l + t.  Data gradient: row = input position i, tap t reads output position
// (i + pad_l - t) / stride where that is whole (the stride-2 layers scatter by parity).
template <int CA, int CN, bool DGRAD>
__global__ __launch_bounds__(kThreads) void conv_gemm(GemmArgs a) {
    static_assert(CA % 16 == 0 && CN % 16 == 0, "channel counts come in 16s");
    constexpr int G = CA / 16, NT = CN / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const long long M = a.n_win * a.ly;
    const long long m_base = ((long long)blockIdx.x * 4 + wave) * (16 * kRowTiles);
    if (m_base >= M) return;

    long long row_base[kRowTiles];
    int pos[kRowTiles];
    bool ok[kRowTiles];
#pragma unroll
    for (int mt = 0; mt < kRowTiles; ++mt) {
        const long long m = m_base + mt * 16 + r;
        ok[mt] = m < M;
        const long long win = ok[mt] ? m / a.ly : 0;
        pos[mt] = ok[mt] ? (int)(m - win * a.ly) : 0;
        row_base[mt] = win * a.la;
    }
    // The matrix pipe sums one tap's 16 channels (four k-steps) in fp32; those short sums are added
    // in fp64, so a value's rounding does not grow with taps x channels.
    double acc[kRowTiles][NT][4];
#pragma unroll
    for (int mt = 0; mt < kRowTiles; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[mt][nt][i] = 0.0;

    for (int t = 0; t < a.k; ++t) {
        for (int g = 0; g < G; ++g) {
            const int c0 = 16 * g + 4 * q;
            floatx4 av[kRowTiles];
#pragma unroll
            for (int mt = 0; mt < kRowTiles; ++mt) {
                int ip;
                bool valid = ok[mt];
                if (DGRAD) {
                    const int u = pos[mt] + a.pad_l - t;
                    ip = u / a.stride;
                    valid = valid && u >= 0 && ip * a.stride == u && ip < a.la;
                } else {
                    ip = pos[mt] * a.stride - a.pad_l + t;
                    valid = valid && ip >= 0 && ip < a.la;
                }
                floatx4 v = {0.f, 0.f, 0.f, 0.f};
                if (valid) v = *(const floatx4*)(a.a + (row_base[mt] + ip) * a.a_stride + a.a_off + c0);
                av[mt] = v;
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                floatx4 bv;
                if (DGRAD) {
                    // B[k = c_out 16g + 4q + j][n = c_in 16nt + r]: four consecutive c_out
                    bv = *(const floatx4*)(a.w + ((size_t)t * a.cin + 16 * nt + r) * a.cout + c0);
                } else {
                    // B[k = c_in 16g + 4q + j][n = c_out 16nt + r]
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        bv[j] = a.w[((size_t)t * a.cin + c0 + j) * a.cout + 16 * nt + r];
                }
#pragma unroll
                for (int mt = 0; mt < kRowTiles; ++mt) {
                    floatx4 c = {0.f, 0.f, 0.f, 0.f};
                    c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][0], bv[0], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][1], bv[1], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][2], bv[2], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][3], bv[3], c, 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[mt][nt][i] += (double)c[i];
                }
            }
        }
    }
    // epilogue: D row 4q + i, column r of each tile
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = 16 * nt + r;
        const double b = DGRAD ? 0.0 : (double)a.bias[n];
#pragma unroll
        for (int mt = 0; mt < kRowTiles; ++mt) {
            const long long m0 = m_base + mt * 16 + 4 * q;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (m0 + i >= M) continue;
                const long long at = (m0 + i) * a.y_stride + a.y_off + n;
                float v = (float)(acc[mt][nt][i] + b);
                if (DGRAD) {
                    if (a.mask && !(a.mask[at] > 0.f)) v = 0.f;
                    if (a.accumulate) v = a.y[at] + v;
                } else {
                    v = v > 0.f ? v : 0.f;
                }
                a.y[at] = v;
            }
        }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------
struct WgradArgs {
    const float* x;        // the convolution's input as consumed [n_win][lx][x_stride] from x_off
    const float* dz;       // gradient at its pre-activation [n_win][lz][z_stride] from z_off
    float* part;           // [waves][k * cin * cout], canonical kernel order
    long long rows, rows_per_wave;
    int lx, x_stride, x_off, lz, z_stride, z_off;
    int k, stride, pad_l, cin, cout;
};

// grid (workgroups, taps x C_in / 16).  A = x^T (16 input channels x 4 rows), B = dz (4 rows x 16
// output channels): lane (r, q) supplies x[row q][channel r] and dz[row q][channel r].  Every wave
// writes its tile, rows or none, so that the reduction reads no stale partial.
template <int NT>
__global__ __launch_bounds__(kThreads) void wgrad(WgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int G = a.cin / 16;
    const int t = blockIdx.y / G, g = blockIdx.y - t * G;
    const long long p = (long long)blockIdx.x * 4 + wave;
    const long long r0 = p * a.rows_per_wave;
    const long long r1 = r0 + a.rows_per_wave < a.rows ? r0 + a.rows_per_wave : a.rows;
    // 64 rows (16 k-steps) at a time in the matrix pipe's fp32, those sums added in fp64
    floatx4 acc[NT];
    double sum[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        acc[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) sum[nt][i] = 0.0;
    }
    int steps = 0;
    for (long long base = r0; base < r1; base += 4) {
        const long long row = base + q;
        const bool ok = row < r1;
        const long long win = ok ? row / a.lz : 0;
        const int o = ok ? (int)(row - win * a.lz) : 0;
        const int ip = o * a.stride - a.pad_l + t;
        float xv = 0.f;
        if (ok && ip >= 0 && ip < a.lx)
            xv = a.x[(win * a.lx + ip) * a.x_stride + a.x_off + 16 * g + r];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float zv = 0.f;
            if (ok) zv = a.dz[row * a.z_stride + a.z_off + 16 * nt + r];
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv, zv, acc[nt], 0, 0, 0);
        }
        if (++steps == 16 || base + 4 >= r1) {
            steps = 0;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sum[nt][i] += (double)acc[nt][i];
                acc[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    float* dst = a.part + p * ((long long)a.k * a.cin * a.cout);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            dst[((size_t)t * a.cin + 16 * g + 4 * q + i) * a.cout + 16 * nt + r] = (float)sum[nt][i];
}

// out[i] = sum over p = 0 .. n_part - 1, in that order, of part[p * pstride + i]
template <typename T>
__global__ __launch_bounds__(kThreads) void reduce_partials(const T* __restrict__ part, int n_part,
                                                            long long pstride, long long n,
                                                            float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int p = 0; p < n_part; ++p) s += (double)part[p * pstride + i];
    out[i] = (float)s;
}

// ---- per-channel sums over rows -------------------------------------------------------------------
enum { kColSum = 0, kColVar = 1, kColBnBwd = 2 };
struct ColArgs {
    const float* a;        // [rows][stride], channels from off
    long long rows, rows_per_block;
    int C, stride, off;
    const double* mean;    // kColVar, kColBnBwd: the batch mean and 1 / std, fp64
    const double* istd;
    const float* x;        // kColBnBwd: the batch normalisation's input [rows][C]
    int len;               // positions per window (dropout counters)
    Drop drop;
    double* part;          // [workgroups][2][C]
};

template <int MODE>
__global__ __launch_bounds__(kThreads) void col_sums(ColArgs a) {
    __shared__ double red[2][kThreads];
    const int tid = threadIdx.x;
    const int lanes = kThreads / a.C;
    const int c = tid % a.C, rl = tid / a.C;
    const long long r0 = (long long)blockIdx.x * a.rows_per_block;
    const long long r1 = r0 + a.rows_per_block < a.rows ? r0 + a.rows_per_block : a.rows;
    double s0 = 0.0, s1 = 0.0;
    if (rl < lanes) {
        for (long long row = r0 + rl; row < r1; row += lanes) {
            const float v = a.a[row * a.stride + a.off + c];
            if (MODE == kColSum) {
                s0 += (double)v;
            } else if (MODE == kColVar) {
                const double d = (double)v - a.mean[c];
                s0 += d * d;
            } else {
                const long long win = row / a.len;
                const float g = v * drop_factor(a.drop, win, (int)(row - win * a.len), c);
                const double xh = ((double)a.x[row * a.C + c] - a.mean[c]) * a.istd[c];
                s0 += (double)g;
                s1 += (double)g * xh;
            }
        }
    }
    red[0][tid] = s0;
    red[1][tid] = s1;
    __syncthreads();
    if (tid < a.C) {
        double t0 = 0.0, t1 = 0.0;
        for (int k = 0; k < lanes; ++k) {
            t0 += red[0][k * a.C + tid];
            t1 += red[1][k * a.C + tid];
        }
        a.part[((long long)blockIdx.x * 2) * a.C + tid] = t0;
        a.part[((long long)blockIdx.x * 2 + 1) * a.C + tid] = t1;
    }
}

__global__ void finish_mean(const double* __restrict__ part, int n_part, int C, double rows,
                            double* __restrict__ mean_d) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int p = 0; p < n_part; ++p) s += part[((long long)p * 2) * C + c];
    mean_d[c] = s / rows;
}

// biased variance; stats: mean at [c], variance at [C + c]
__global__ void finish_var(const double* __restrict__ part, int n_part, int C, double rows,
                           const double* __restrict__ mean, double* __restrict__ istd,
                           float* __restrict__ stats) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int p = 0; p < n_part; ++p) s += part[((long long)p * 2) * C + c];
    const double var = s / rows;
    istd[c] = 1.0 / sqrt(var + kBnEps);
    stats[c] = (float)mean[c];
    stats[C + c] = (float)var;
}

// sums[c] = sum g (beta's gradient), sums[C + c] = sum g * xhat (gamma's)
__global__ void finish_bn_backward(const double* __restrict__ part, int n_part, int C,
                                   float* __restrict__ dgamma, float* __restrict__ dbeta,
                                   double* __restrict__ sums) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int p = 0; p < n_part; ++p) {
        s0 += part[((long long)p * 2) * C + c];
        s1 += part[((long long)p * 2 + 1) * C + c];
    }
    sums[c] = s0;
    sums[C + c] = s1;
    dbeta[c] = (float)s0;
    dgamma[c] = (float)s1;
}

// ---- elementwise ----------------------------------------------------------------------------------
// h = dropout(gamma * xhat + beta)
__global__ __launch_bounds__(kThreads) void bn_apply(const float* __restrict__ x, long long total,
                                                     int C, int len, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta,
                                                     const double* __restrict__ mean,
                                                     const double* __restrict__ istd, Drop drop,
                                                     float* __restrict__ h) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long row = idx / C;
    const long long win = row / len;
    const float xh = (float)(((double)x[idx] - mean[c]) * istd[c]);
    const float y = xh * gamma[c] + beta[c];
    h[idx] = y * drop_factor(drop, win, (int)(row - win * len), c);
}

// dx = gamma / std * (g - mean(g) - xhat * mean(g * xhat)), g = dropout'(dh).  The bracket cancels
// (over few elements almost wholly: with two, to eps / (var + eps) of g), so it is formed in fp64.
__global__ __launch_bounds__(kThreads) void bn_backward_apply(
    const float* __restrict__ dh, const float* __restrict__ x, long long total, int C, int len,
    const float* __restrict__ gamma, const double* __restrict__ mean,
    const double* __restrict__ istd, const double* __restrict__ sums, double inv_rows, Drop drop,
    float* __restrict__ dx) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long row = idx / C;
    const long long win = row / len;
    const double g = (double)(dh[idx] * drop_factor(drop, win, (int)(row - win * len), c));
    const double xh = ((double)x[idx] - mean[c]) * istd[c];
    const double t = g - sums[c] * inv_rows - xh * (sums[C + c] * inv_rows);
    dx[idx] = (float)(((double)gamma[c] * istd[c]) * t);
}

// MaxPooling1D(2), 'valid'
__global__ __launch_bounds__(kThreads) void pool_forward(const float* __restrict__ a, long long n_win,
                                                         int li, int lo, int C,
                                                         float* __restrict__ p) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_win * lo * C) return;
    const int c = (int)(idx % C);
    const long long row = idx / C;
    const long long win = row / lo;
    const int j = (int)(row - win * lo);
    const float* src = a + ((win * li + 2 * j) * C + c);
    p[idx] = fmaxf(src[0], src[C]);
}

// gradient at a convolution's pre-activation from the gradient behind its ReLU (POOL: behind the
// max-pool that follows; a tie goes to the first of the pair, a dropped last position gets 0)
template <bool POOL>
__global__ __launch_bounds__(kThreads) void relu_pool_backward(const float* __restrict__ g,
                                                               const float* __restrict__ a,
                                                               long long n_win, int li, int lo,
                                                               int C, float* __restrict__ dz) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_win * li * C) return;
    float v;
    if (POOL) {
        const int c = (int)(idx % C);
        const long long row = idx / C;
        const long long win = row / li;
        const int pos = (int)(row - win * li);
        const int j = pos >> 1;
        v = 0.f;
        if (j < lo) {
            const float* src = a + ((win * li + 2 * j) * C + c);
            const bool first = src[0] >= src[C];
            if (((pos & 1) == 0) == first) v = g[(win * lo + j) * C + c];
        }
    } else {
        v = g[idx];
    }
    dz[idx] = a[idx] > 0.f ? v : 0.f;
}

// AveragePooling1D(3, 1, 'same'): the sum of the valid taps (left, middle, right) by their count
__global__ __launch_bounds__(kThreads) void avg_forward(const float* __restrict__ x, long long n_win,
                                                        int len, int C, float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_win * len * C) return;
    const long long row = idx / C;
    const int pos = (int)(row % len);
    float s = 0.f, n = 0.f;
    for (int d = -1; d <= 1; ++d) {
        if (pos + d < 0 || pos + d >= len) continue;
        s += x[idx + (long long)d * C];
        n += 1.f;
    }
    y[idx] = s / n;
}

// dx[i] += sum over outputs j = i - 1 .. i + 1 of g[j] / count(j)
__global__ __launch_bounds__(kThreads) void avg_backward_add(const float* __restrict__ g,
                                                             long long n_win, int len, int C,
                                                             float* __restrict__ dx) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n_win * len * C) return;
    const long long row = idx / C;
    const int pos = (int)(row % len);
    float s = 0.f;
    for (int d = -1; d <= 1; ++d) {
        const int j = pos + d;
        if (j < 0 || j >= len) continue;
        const float n = 1.f + (j > 0 ? 1.f : 0.f) + (j < len - 1 ? 1.f : 0.f);
        s += g[idx + (long long)d * C] / n;
    }
    dx[idx] += s;
}

// ---- head: conv1d_20 + ReLU, global average, softmax, loss -------------------------------------
// One workgroup per window.  dz: first conv1d_20's ReLU output, then, in place, the gradient at its
// pre-activation: (softmax - onehot) / (n_windows * l7) where the ReLU let the value through.
__global__ __launch_bounds__(kThreads) void head_forward(
    const float* __restrict__ h, int l7, const float* __restrict__ w, const float* __restrict__ bias,
    int C, const int* __restrict__ labels, double inv_windows, float* __restrict__ dz,
    double* __restrict__ loss, int* __restrict__ correct) {
    __shared__ float hs[kMaxL7 * 48];
    __shared__ double red[kThreads];
    __shared__ int redi[kThreads];
    const int tid = threadIdx.x;
    const long long win = blockIdx.x;
    const float* src = h + win * l7 * 48;
    for (int i = tid; i < l7 * 48; i += kThreads) hs[i] = src[i];
    __syncthreads();
    const bool valid = tid < C;
    float* z = dz + win * l7 * C;
    double logit = 0.0;             // fp64 from the fp32 inputs: softmax - onehot cancels
    if (valid) {
        double sum = 0.0;
        for (int p = 0; p < l7; ++p) {
            double s = 0.0;
            for (int ci = 0; ci < 48; ++ci) s += (double)hs[p * 48 + ci] * (double)w[ci * C + tid];
            s += (double)bias[tid];
            s = s > 0.0 ? s : 0.0;
            z[p * C + tid] = (float)s;
            sum += s;
        }
        logit = sum / (double)l7;
    }
    // argmax, the lowest index among equals
    red[tid] = valid ? logit : -INFINITY;
    redi[tid] = tid;
    __syncthreads();
    for (int half = kThreads / 2; half >= 1; half >>= 1) {
        if (tid < half) {
            const double o = red[tid + half];
            const int oi = redi[tid + half];
            if (o > red[tid] || (o == red[tid] && oi < redi[tid])) {
                red[tid] = o;
                redi[tid] = oi;
            }
        }
        __syncthreads();
    }
    const double mx = red[0];
    const int best = redi[0];
    __syncthreads();
    const double e = valid ? exp(logit - mx) : 0.0;
    red[tid] = e;
    __syncthreads();
    for (int half = kThreads / 2; half >= 1; half >>= 1) {
        if (tid < half) red[tid] += red[tid + half];
        __syncthreads();
    }
    const double se = red[0];
    const int label = labels[win];
    // (a label outside [0, C) reaches this kernel only through the _dev entry: its loss is NaN)
    if (tid == 0) {
        if (label < 0 || label >= C) loss[win] = NAN;
        correct[win] = best == label ? 1 : 0;
    }
    if (valid && tid == label) loss[win] = (mx + log(se)) - logit;
    if (valid) {
        const double prob = e / se;
        const float dl = (float)((prob - (tid == label ? 1.0 : 0.0)) * inv_windows / (double)l7);
        for (int p = 0; p < l7; ++p) z[p * C + tid] = z[p * C + tid] > 0.f ? dl : 0.f;
    }
}

__global__ void finish_loss(const double* __restrict__ loss, const int* __restrict__ correct,
                            long long n_win, double* __restrict__ mean_loss,
                            long long* __restrict__ n_correct) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    long long k = 0;
    for (long long i = 0; i < n_win; ++i) {
        s += loss[i];
        k += correct[i];
    }
    *mean_loss = s / (double)n_win;
    *n_correct = k;
}

// ---- inference phase (evaluate) ---------------------------------------------------------------------
// mean and 1 / std of a batch normalisation from the blob's moving statistics, as finish_var forms
// 1 / std from a batch variance
__global__ void moving_stats(const float* __restrict__ moving_mean,
                             const float* __restrict__ moving_var, int C,
                             double* __restrict__ mean, double* __restrict__ istd) {
    const int c = threadIdx.x;
    if (c >= C) return;
    mean[c] = (double)moving_mean[c];
    istd[c] = 1.0 / sqrt((double)moving_var[c] + kBnEps);
}

// running totals over the chunks of a set: the losses added in window order by one thread
__global__ void add_losses(const double* __restrict__ loss, const int* __restrict__ correct,
                           long long n_win, double* __restrict__ loss_sum,
                           long long* __restrict__ n_correct, double* __restrict__ window_loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = *loss_sum;
    long long k = *n_correct;
    for (long long i = 0; i < n_win; ++i) {
        s += loss[i];
        k += correct[i];
        if (window_loss) window_loss[i] = loss[i];
    }
    *loss_sum = s;
    *n_correct = k;
}

// conv1d_20's kernel gradient: grid (48 * C / 256, partials), fp64 partials [partial][48][C]
__global__ __launch_bounds__(kThreads) void head_wgrad(const float* __restrict__ h,
                                                       const float* __restrict__ dz, long long rows,
                                                       long long rows_per_block, int C,
                                                       double* __restrict__ part) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= 48 * C) return;
    const int ci = e / C, c = e - ci * C;
    const long long r0 = (long long)blockIdx.y * rows_per_block;
    const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    double s = 0.0;
    for (long long row = r0; row < r1; ++row) s += (double)h[row * 48 + ci] * (double)dz[row * C + c];
    part[(long long)blockIdx.y * 48 * C + e] = s;
}

__global__ __launch_bounds__(kThreads) void head_dgrad(const float* __restrict__ dz,
                                                       const float* __restrict__ w, long long rows,
                                                       int C, float* __restrict__ dh) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= rows * 48) return;
    const int ci = (int)(idx % 48);
    const long long row = idx / 48;
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)dz[row * C + c] * (double)w[ci * C + c];
    dh[idx] = (float)s;
}

// ---- host -------------------------------------------------------------------------------------------
struct Geometry {
    int L, C, len[8];
    Geometry(int input_size, int n_classes) : L(input_size), C(n_classes) { stage_lengths(L, len); }
};

// the workspace, carved in one order by workspace_bytes(), gradients() and evaluate()
struct Buffers {
    float *a1, *h1, *a2, *a3, *a4, *p4, *h2, *a5, *a6, *a7, *p7, *h3, *a8, *a9, *p9, *h4;
    float *avg, *a12, *a14, *a15, *cc, *pcc, *h5, *a17, *h6, *a18, *a19, *p19, *h7, *dz20;
    float *gA, *gB, *gE, *gD, *g48, *g16, *gavg;
    double *mean, *istd, *sums;
    double* loss;
    int* correct;
    void* part;
    size_t part_bytes;
    Buffers(Carve& ws, const Geometry& g, int64_t n) {
        const int* len = g.len;
        auto f = [&](int l, int c) { return ws.take<float>((size_t)n * l * c); };
        a1 = f(len[1], 48); h1 = f(len[1], 48); a2 = f(len[1], 48); a3 = f(len[1], 48);
        a4 = f(len[1], 48); p4 = f(len[2], 48); h2 = f(len[2], 48);
        a5 = f(len[2], 16); a6 = f(len[2], 48); a7 = f(len[2], 48); p7 = f(len[3], 48);
        h3 = f(len[3], 48); a8 = f(len[3], 48); a9 = f(len[3], 48); p9 = f(len[4], 48);
        h4 = f(len[4], 48); avg = f(len[4], 48); a12 = f(len[4], 16); a14 = f(len[4], 16);
        a15 = f(len[4], 48); cc = f(len[4], 192); pcc = f(len[5], 192); h5 = f(len[5], 192);
        a17 = f(len[6], 48); h6 = f(len[6], 48); a18 = f(len[6], 48); a19 = f(len[6], 48);
        p19 = f(len[7], 48); h7 = f(len[7], 48); dz20 = f(len[7], g.C);
        gA = f(len[1], 48); gB = f(len[1], 48); gE = f(len[4], 192); gD = f(len[4], 48);
        g48 = f(len[4], 48); g16 = f(len[4], 16); gavg = f(len[4], 48);
        mean = ws.take<double>(kBnTotal);
        istd = ws.take<double>(kBnTotal);
        sums = ws.take<double>(2 * 192);
        loss = ws.take<double>((size_t)n);
        correct = ws.take<int>((size_t)n);
        // the largest set of partial sums: conv1d_17's kernel per wave, or conv1d_20's in fp64
        part_bytes = std::max((size_t)kMaxPartials * 3 * 192 * 48 * sizeof(float),
                              (size_t)kMaxPartials * 48 * dbh_gen::kMaxClasses * sizeof(double));
        part = ws.take<char>(part_bytes);
    }
};

// rows split over at most kMaxPartials parts of at least `least` rows, a multiple of `unit`
inline long long rows_per_part(long long rows, long long least, long long unit) {
    long long per = (rows + kMaxPartials - 1) / kMaxPartials;
    per = std::max(per, least);
    return (per + unit - 1) / unit * unit;
}

struct Run {
    const Geometry& g;
    const Buffers& b;
    const float* w;
    float* grads;
    float* stats;
    int64_t n;
    Drop drop;
    hipStream_t stream;
    bool inference = false;    // Keras's test phase: the blob's moving statistics, no dropout
    hipError_t err = hipSuccess;

    bool ok() {
        if (err == hipSuccess) err = hipGetLastError();
        return err == hipSuccess;
    }
    Drop drop_of(int bn) const {
        Drop d = drop;
        d.layer = (uint32_t)bn + 1;
        return d;
    }

    template <int CA, int CN, bool DGRAD>
    void gemm(int layer, const float* a, int la, int a_stride, int a_off, float* y, int ly,
              int y_stride, int y_off, const float* mask, bool accumulate) {
        if (!ok()) return;
        const Conv& l = kConvs[layer];
        GemmArgs ga;
        ga.a = a;
        ga.w = w + blob_kernel(layer, g.C);
        ga.bias = w + blob_bias(layer, g.C);
        ga.mask = mask;
        ga.y = y;
        ga.n_win = n;
        ga.la = la; ga.a_stride = a_stride; ga.a_off = a_off;
        ga.ly = ly; ga.y_stride = y_stride; ga.y_off = y_off;
        ga.k = l.k; ga.stride = l.stride; ga.cin = l.cin; ga.cout = l.cout;
        // forward: a is the input (la) and y the output (ly); data gradient: the other way round
        ga.pad_l = DGRAD ? same_pad_left(l.k, l.stride, ly, la) : same_pad_left(l.k, l.stride, la, ly);
        ga.accumulate = accumulate ? 1 : 0;
        const long long rows = (long long)n * ly;
        hipLaunchKernelGGL((conv_gemm<CA, CN, DGRAD>), dim3((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)),
                           dim3(kThreads), 0, stream, ga);
    }
    // forward convolution of `layer`: x [n][lin][cin at x_off of x_stride] -> y
    void conv(int layer, const float* x, int lin, float* y, int lout, int y_stride = 0, int y_off = 0) {
        const Conv& l = kConvs[layer];
        if (y_stride == 0) y_stride = l.cout;
        if (l.cin == 48 && l.cout == 48) gemm<48, 48, false>(layer, x, lin, 48, 0, y, lout, y_stride, y_off, nullptr, false);
        else if (l.cin == 48 && l.cout == 16) gemm<48, 16, false>(layer, x, lin, 48, 0, y, lout, y_stride, y_off, nullptr, false);
        else if (l.cin == 16 && l.cout == 48) gemm<16, 48, false>(layer, x, lin, 16, 0, y, lout, y_stride, y_off, nullptr, false);
        else gemm<192, 48, false>(layer, x, lin, 192, 0, y, lout, y_stride, y_off, nullptr, false);
    }
    // everything a convolution owes the backward pass, given the gradient dz at its pre-activation
    // ([n][lout][z_stride] from z_off): bias and kernel gradients, and (dx != null) the gradient at
    // its input, through the ReLU of the layer that produced it where `mask` names that output
    void conv_backward(int layer, const float* x, int lin, const float* dz, int lout, int z_stride,
                       int z_off, float* dx, const float* mask, bool accumulate) {
        const Conv& l = kConvs[layer];
        const long long rows = (long long)n * lout;
        bias_grad(dz, rows, l.cout, z_stride, z_off, grads + blob_bias(layer, g.C));
        if (!ok()) return;
        WgradArgs wa;
        wa.x = x; wa.dz = dz; wa.part = (float*)b.part;
        wa.rows = rows;
        wa.rows_per_wave = rows_per_part(rows, 64, 4);
        wa.lx = lin; wa.x_stride = l.cin; wa.x_off = 0;
        wa.lz = lout; wa.z_stride = z_stride; wa.z_off = z_off;
        wa.k = l.k; wa.stride = l.stride; wa.cin = l.cin; wa.cout = l.cout;
        wa.pad_l = same_pad_left(l.k, l.stride, lin, lout);
        const long long waves = (rows + wa.rows_per_wave - 1) / wa.rows_per_wave;
        const unsigned wgs = (unsigned)((waves + 3) / 4);
        const dim3 grid(wgs, (unsigned)(l.k * (l.cin / 16)));
        if (l.cout == 48) hipLaunchKernelGGL((wgrad<3>), grid, dim3(kThreads), 0, stream, wa);
        else hipLaunchKernelGGL((wgrad<1>), grid, dim3(kThreads), 0, stream, wa);
        if (!ok()) return;
        const long long count = (long long)l.k * l.cin * l.cout;
        hipLaunchKernelGGL((reduce_partials<float>), dim3(blocks_for(count, kThreads)), dim3(kThreads), 0, stream,
                           (const float*)b.part, (int)(wgs * 4), count, count, grads + blob_kernel(layer, g.C));
        if (!dx) return;
        // the data gradient's contraction runs over cout, its output over cin
        if (l.cin == 48 && l.cout == 48) gemm<48, 48, true>(layer, dz, lout, z_stride, z_off, dx, lin, 48, 0, mask, accumulate);
        else if (l.cin == 48 && l.cout == 16) gemm<16, 48, true>(layer, dz, lout, z_stride, z_off, dx, lin, 48, 0, mask, accumulate);
        else if (l.cin == 16 && l.cout == 48) gemm<48, 16, true>(layer, dz, lout, z_stride, z_off, dx, lin, 16, 0, mask, accumulate);
        else gemm<48, 192, true>(layer, dz, lout, z_stride, z_off, dx, lin, 192, 0, mask, accumulate);
    }
    unsigned col_launch(ColArgs& ca) {
        ca.rows_per_block = rows_per_part(ca.rows, 64, 1);
        ca.part = (double*)b.part;
        return (unsigned)((ca.rows + ca.rows_per_block - 1) / ca.rows_per_block);
    }
    void bias_grad(const float* dz, long long rows, int C, int stride, int off, float* out) {
        if (!ok()) return;
        ColArgs ca = {};
        ca.a = dz; ca.rows = rows; ca.C = C; ca.stride = stride; ca.off = off;
        const unsigned parts = col_launch(ca);
        hipLaunchKernelGGL((col_sums<kColSum>), dim3(parts), dim3(kThreads), 0, stream, ca);
        if (!ok()) return;
        hipLaunchKernelGGL((reduce_partials<double>), dim3(blocks_for(C, kThreads)), dim3(kThreads), 0, stream,
                           (const double*)b.part, (int)parts, (long long)2 * C, (long long)C, out);
    }
    // batch normalisation `bn` and its dropout: x [n][len][C] -> h
    void bn_forward(int bn, const float* x, int len, float* h) {
        if (!ok()) return;
        const int C = kBnChannels[bn];
        const long long rows = (long long)n * len;
        const size_t so = bn_channel_offset(bn);
        const float* gamma = w + blob_bn(bn, g.C);
        if (inference) {
            hipLaunchKernelGGL(moving_stats, dim3(1), dim3(kThreads), 0, stream, gamma + 2 * C,
                               gamma + 3 * C, C, b.mean + so, b.istd + so);
        } else {
            ColArgs ca = {};
            ca.a = x; ca.rows = rows; ca.C = C; ca.stride = C; ca.off = 0;
            const unsigned parts = col_launch(ca);
            hipLaunchKernelGGL((col_sums<kColSum>), dim3(parts), dim3(kThreads), 0, stream, ca);
            hipLaunchKernelGGL(finish_mean, dim3(1), dim3(kThreads), 0, stream, (const double*)b.part,
                               (int)parts, C, (double)rows, b.mean + so);
            ca.mean = b.mean + so;
            hipLaunchKernelGGL((col_sums<kColVar>), dim3(parts), dim3(kThreads), 0, stream, ca);
            hipLaunchKernelGGL(finish_var, dim3(1), dim3(kThreads), 0, stream, (const double*)b.part,
                               (int)parts, C, (double)rows, (const double*)(b.mean + so), b.istd + so,
                               stats + 2 * so);
        }
        if (!ok()) return;
        hipLaunchKernelGGL(bn_apply, dim3(blocks_for(rows * C, kThreads)), dim3(kThreads), 0, stream, x,
                           rows * C, C, len, gamma, gamma + C, (const double*)(b.mean + so),
                           (const double*)(b.istd + so), drop_of(bn), h);
    }
    // dh: gradient at the dropout's output -> dx: at the batch normalisation's input x
    void bn_backward(int bn, const float* dh, const float* x, int len, float* dx) {
        if (!ok()) return;
        const int C = kBnChannels[bn];
        const long long rows = (long long)n * len;
        const size_t so = bn_channel_offset(bn);
        ColArgs ca = {};
        ca.a = dh; ca.rows = rows; ca.C = C; ca.stride = C; ca.off = 0;
        ca.x = x; ca.mean = b.mean + so; ca.istd = b.istd + so; ca.len = len;
        ca.drop = drop_of(bn);
        const unsigned parts = col_launch(ca);
        hipLaunchKernelGGL((col_sums<kColBnBwd>), dim3(parts), dim3(kThreads), 0, stream, ca);
        float* dgamma = grads + blob_bn(bn, g.C);
        hipLaunchKernelGGL(finish_bn_backward, dim3(1), dim3(kThreads), 0, stream,
                           (const double*)b.part, (int)parts, C, dgamma, dgamma + C, b.sums);
        if (!ok()) return;
        hipLaunchKernelGGL(bn_backward_apply, dim3(blocks_for(rows * C, kThreads)), dim3(kThreads), 0, stream,
                           dh, x, rows * C, C, len, w + blob_bn(bn, g.C), (const double*)(b.mean + so),
                           (const double*)(b.istd + so), (const double*)b.sums, 1.0 / (double)rows,
                           drop_of(bn), dx);
    }
    void pool(const float* a, int li, int lo, int C, float* p) {
        if (!ok() || lo == 0) return;
        hipLaunchKernelGGL(pool_forward, dim3(blocks_for((long long)n * lo * C, kThreads)), dim3(kThreads), 0,
                           stream, a, (long long)n, li, lo, C, p);
    }
    void unpool(bool pooled, const float* gr, const float* a, int li, int lo, int C, float* dz) {
        if (!ok()) return;
        const dim3 grid(blocks_for((long long)n * li * C, kThreads));
        if (pooled)
            hipLaunchKernelGGL((relu_pool_backward<true>), grid, dim3(kThreads), 0, stream, gr, a,
                               (long long)n, li, lo, C, dz);
        else
            hipLaunchKernelGGL((relu_pool_backward<false>), grid, dim3(kThreads), 0, stream, gr, a,
                               (long long)n, li, lo, C, dz);
    }
};

// The forward pass, from the windows to each window's loss and hit (b.loss, b.correct): the half that
// gradients() and evaluate() share.  r.inference chooses the phase.
void forward(Run& r, const float* x, const int32_t* labels) {
    const Geometry& g = r.g;
    const Buffers& b = r.b;
    const int* len = g.len;
    const int64_t n = r.n;
    const int C = g.C;
    if (r.ok())
        hipLaunchKernelGGL(conv1_forward, dim3(blocks_for(n * len[1] * 48, kThreads)), dim3(kThreads), 0,
                           r.stream, x, r.w + blob_kernel(0, g.C), (long long)n, g.L, len[1],
                           same_pad_left(3, 2, g.L, len[1]), b.a1);
    r.bn_forward(0, b.a1, len[1], b.h1);
    r.conv(1, b.h1, len[1], b.a2, len[1]);
    r.conv(2, b.a2, len[1], b.a3, len[1]);
    r.conv(3, b.a3, len[1], b.a4, len[1]);
    r.pool(b.a4, len[1], len[2], 48, b.p4);
    r.bn_forward(1, b.p4, len[2], b.h2);
    r.conv(4, b.h2, len[2], b.a5, len[2]);
    r.conv(5, b.a5, len[2], b.a6, len[2]);
    r.conv(6, b.a6, len[2], b.a7, len[2]);
    r.pool(b.a7, len[2], len[3], 48, b.p7);
    r.bn_forward(2, b.p7, len[3], b.h3);
    r.conv(7, b.h3, len[3], b.a8, len[3]);
    r.conv(8, b.a8, len[3], b.a9, len[3]);
    r.pool(b.a9, len[3], len[4], 48, b.p9);
    r.bn_forward(3, b.p9, len[4], b.h4);
    if (r.ok())
        hipLaunchKernelGGL(avg_forward, dim3(blocks_for(n * len[4] * 48, kThreads)), dim3(kThreads), 0, r.stream,
                           (const float*)b.h4, (long long)n, len[4], 48, b.avg);
    r.conv(9, b.avg, len[4], b.cc, len[4], 192, 0);
    r.conv(10, b.h4, len[4], b.cc, len[4], 192, 48);
    r.conv(11, b.h4, len[4], b.a12, len[4]);
    r.conv(12, b.a12, len[4], b.cc, len[4], 192, 96);
    r.conv(13, b.h4, len[4], b.a14, len[4]);
    r.conv(14, b.a14, len[4], b.a15, len[4]);
    r.conv(15, b.a15, len[4], b.cc, len[4], 192, 144);
    r.pool(b.cc, len[4], len[5], 192, b.pcc);
    r.bn_forward(4, b.pcc, len[5], b.h5);
    r.conv(16, b.h5, len[5], b.a17, len[6]);
    r.bn_forward(5, b.a17, len[6], b.h6);
    r.conv(17, b.h6, len[6], b.a18, len[6]);
    r.conv(18, b.a18, len[6], b.a19, len[6]);
    r.pool(b.a19, len[6], len[7], 48, b.p19);
    r.bn_forward(6, b.p19, len[7], b.h7);
    if (r.ok())
        hipLaunchKernelGGL(head_forward, dim3((unsigned)n), dim3(kThreads), 0, r.stream,
                           (const float*)b.h7, len[7], r.w + blob_kernel(19, g.C), r.w + blob_bias(19, g.C),
                           C, (const int*)labels, 1.0 / (double)n, b.dz20, b.loss, b.correct);
}

}  // namespace

size_t workspace_bytes(int n_classes, int input_size, int64_t n_windows) {
    const Geometry g(input_size, n_classes);
    Carve ws(nullptr);
    const Buffers b(ws, g, n_windows);
    (void)b;
    return ws.used;
}

hipError_t gradients(const float* weights, int n_classes, int input_size, const float* x,
                     const int32_t* labels, int64_t n_windows, float dropout_rate, uint64_t seed,
                     double* mean_loss, int64_t* n_correct, float* grads, float* stats,
                     void* workspace, hipStream_t stream, int frozen_blocks) {
    const Geometry g(input_size, n_classes);
    Carve ws(workspace);
    const Buffers b(ws, g, n_windows);
    const int* len = g.len;
    const int64_t n = n_windows;
    const int C = n_classes;

    Drop drop;
    drop.seed_lo = (uint32_t)seed;
    drop.seed_hi = (uint32_t)(seed >> 32);
    drop.layer = 0;
    drop.threshold = (uint32_t)((double)dropout_rate * 16777216.0);
    drop.scale = (float)(1.0 / (1.0 - (double)dropout_rate));
    Run r{g, b, weights, grads, stats, n, drop, stream};

    // the moving-statistics slots and the frozen tensors' stay zero; everything else is written below
    r.err = hipMemsetAsync(grads, 0, (size_t)dbh_net::param_count(C) * sizeof(float), stream);

    forward(r, x, labels);
    if (r.ok())
        hipLaunchKernelGGL(finish_loss, dim3(1), dim3(64), 0, stream, (const double*)b.loss,
                           (const int*)b.correct, (long long)n, mean_loss, (long long*)n_correct);

    // ---- backward ----------------------------------------------------------------------------
    // With f blocks frozen the pass ends at the first trainable convolutions: their weight and bias
    // gradients, no data gradient into the frozen part.  What runs is launched as at f = 0.
    const int f = frozen_blocks;
    const long long rows7 = (long long)n * len[7];
    r.bias_grad(b.dz20, rows7, C, C, 0, grads + blob_bias(19, g.C));
    if (r.ok()) {
        const long long per = rows_per_part(rows7, 16, 1);
        const unsigned parts = (unsigned)((rows7 + per - 1) / per);
        hipLaunchKernelGGL(head_wgrad, dim3(blocks_for(48 * C, kThreads), parts), dim3(kThreads), 0, stream,
                           (const float*)b.h7, (const float*)b.dz20, rows7, per, C, (double*)b.part);
        hipLaunchKernelGGL((reduce_partials<double>), dim3(blocks_for(48 * C, kThreads)), dim3(kThreads), 0,
                           stream, (const double*)b.part, (int)parts, (long long)48 * C,
                           (long long)48 * C, grads + blob_kernel(19, g.C));
        if (f < 7)
            hipLaunchKernelGGL(head_dgrad, dim3(blocks_for(rows7 * 48, kThreads)), dim3(kThreads), 0, stream,
                               (const float*)b.dz20, weights + blob_kernel(19, g.C), rows7, C, b.gA);
    }
    if (f < 7) {    // stage G
        r.bn_backward(6, b.gA, b.p19, len[7], b.gB);
        r.unpool(true, b.gB, b.a19, len[6], len[7], 48, b.gA);
        r.conv_backward(18, b.a18, len[6], b.gA, len[6], 48, 0, b.gB, b.a18, false);
        r.conv_backward(17, b.h6, len[6], b.gB, len[6], 48, 0, f < 6 ? b.gA : nullptr, nullptr, false);
    }
    if (f < 6) {    // stage F
        r.bn_backward(5, b.gA, b.a17, len[6], b.gB);
        r.unpool(false, b.gB, b.a17, len[6], len[6], 48, b.gA);
        r.conv_backward(16, b.h5, len[5], b.gA, len[6], 48, 0, f < 5 ? b.gB : nullptr, nullptr, false);
    }
    if (f < 5) {    // stage E: the four branches' data gradients add in gD
        float* const gD = f < 4 ? b.gD : nullptr;
        r.bn_backward(4, b.gB, b.pcc, len[5], b.gA);
        r.unpool(true, b.gA, b.cc, len[4], len[5], 192, b.gE);
        r.conv_backward(15, b.a15, len[4], b.gE, len[4], 192, 144, b.g48, b.a15, false);
        r.conv_backward(14, b.a14, len[4], b.g48, len[4], 48, 0, b.g16, b.a14, false);
        r.conv_backward(13, b.h4, len[4], b.g16, len[4], 16, 0, gD, nullptr, false);
        r.conv_backward(12, b.a12, len[4], b.gE, len[4], 192, 96, b.g16, b.a12, false);
        r.conv_backward(11, b.h4, len[4], b.g16, len[4], 16, 0, gD, nullptr, true);
        r.conv_backward(10, b.h4, len[4], b.gE, len[4], 192, 48, gD, nullptr, true);
        r.conv_backward(9, b.avg, len[4], b.gE, len[4], 192, 0, gD ? b.gavg : nullptr, nullptr, false);
        if (gD && r.ok())
            hipLaunchKernelGGL(avg_backward_add, dim3(blocks_for(n * len[4] * 48, kThreads)), dim3(kThreads), 0,
                               stream, (const float*)b.gavg, (long long)n, len[4], 48, b.gD);
    }
    if (f < 4) {    // stage D
        r.bn_backward(3, b.gD, b.p9, len[4], b.gA);
        r.unpool(true, b.gA, b.a9, len[3], len[4], 48, b.gB);
        r.conv_backward(8, b.a8, len[3], b.gB, len[3], 48, 0, b.gA, b.a8, false);
        r.conv_backward(7, b.h3, len[3], b.gA, len[3], 48, 0, f < 3 ? b.gB : nullptr, nullptr, false);
    }
    if (f < 3) {    // stage C
        r.bn_backward(2, b.gB, b.p7, len[3], b.gA);
        r.unpool(true, b.gA, b.a7, len[2], len[3], 48, b.gB);
        r.conv_backward(6, b.a6, len[2], b.gB, len[2], 48, 0, b.gA, b.a6, false);
        r.conv_backward(5, b.a5, len[2], b.gA, len[2], 48, 0, b.gB, b.a5, false);
        r.conv_backward(4, b.h2, len[2], b.gB, len[2], 16, 0, f < 2 ? b.gA : nullptr, nullptr, false);
    }
    if (f < 2) {    // stage B
        r.bn_backward(1, b.gA, b.p4, len[2], b.gB);
        r.unpool(true, b.gB, b.a4, len[1], len[2], 48, b.gA);
        r.conv_backward(3, b.a3, len[1], b.gA, len[1], 48, 0, b.gB, b.a3, false);
        r.conv_backward(2, b.a2, len[1], b.gB, len[1], 48, 0, b.gA, b.a2, false);
        r.conv_backward(1, b.h1, len[1], b.gA, len[1], 48, 0, f < 1 ? b.gB : nullptr, nullptr, false);
    }
    if (f < 1) {    // stage A: conv1d_1 has one input channel and needs no data gradient
        r.bn_backward(0, b.gB, b.a1, len[1], b.gA);
        r.unpool(false, b.gA, b.a1, len[1], len[1], 48, b.gB);
        if (r.ok()) {
            const long long rows = (long long)n * len[1];
            const long long per = rows_per_part(rows, 64, 1);
            const unsigned parts = (unsigned)((rows + per - 1) / per);
            hipLaunchKernelGGL(conv1_wgrad, dim3(parts), dim3(kThreads), 0, stream, x,
                               (const float*)b.gB, rows, g.L, len[1], same_pad_left(3, 2, g.L, len[1]), per,
                               (double*)b.part);
            hipLaunchKernelGGL((reduce_partials<double>), dim3(1), dim3(kThreads), 0, stream,
                               (const double*)b.part, (int)parts, (long long)192, (long long)192, grads);
        }
    }
    r.ok();
    return r.err;
}

hipError_t evaluate(const float* weights, int n_classes, int input_size, const float* x,
                    const int32_t* labels, int64_t n_windows, double* loss_sum, int64_t* n_correct,
                    double* window_loss, void* workspace, hipStream_t stream) {
    const Geometry g(input_size, n_classes);
    Carve ws(workspace);
    const Buffers b(ws, g, n_windows);
    const Drop keep_all = {0u, 0u, 0u, 0u, 1.f};
    Run r{g, b, weights, nullptr, nullptr, n_windows, keep_all, stream, true};
    forward(r, x, labels);
    if (r.ok())
        hipLaunchKernelGGL(add_losses, dim3(1), dim3(64), 0, stream, (const double*)b.loss,
                           (const int*)b.correct, (long long)n_windows, loss_sum,
                           (long long*)n_correct, window_loss);
    r.ok();
    return r.err;
}

}  // namespace dbh_train

// ---- C ABI (include/deepbinner_hip.h, "training") ------------------------------------------------
namespace {

int check_arguments(int64_t n_floats, int n_classes, int input_size, int64_t n_windows,
                    float dropout_rate) {
    if (!dbh_gen::geometry_ok(input_size, n_classes)) return DBH_ERR_UNSUPPORTED;
    if (n_floats != dbh_net::param_count(n_classes)) return DBH_ERR_BAD_WEIGHTS;
    if (n_windows < 1 || !(dropout_rate >= 0.f && dropout_rate < 1.f)) return DBH_ERR_INVALID_ARGUMENT;
    if (n_windows > dbh_train::kMaxBatchSamples / input_size) return DBH_ERR_UNSUPPORTED;
    return DBH_OK;
}

}  // namespace

extern "C" {

int dbh_gradients_max_windows(int input_size, int64_t* n_windows) {
    if (!n_windows || input_size < 1) return DBH_ERR_INVALID_ARGUMENT;
    *n_windows = dbh_train::kMaxBatchSamples / input_size;
    return DBH_OK;
}

int dbh_gradients_workspace_bytes(int n_classes, int input_size, int64_t n_windows, size_t* bytes) {
    if (!bytes) return DBH_ERR_INVALID_ARGUMENT;
    const int st = check_arguments(dbh_gen::geometry_ok(input_size, n_classes)
                                       ? dbh_net::param_count(n_classes) : 0,
                                   n_classes, input_size, n_windows, 0.f);
    if (st != DBH_OK) return st;
    *bytes = dbh_train::workspace_bytes(n_classes, input_size, n_windows);
    return DBH_OK;
}

int dbh_gradients_frozen_dev(const float* weights_dev, int64_t n_floats, int n_classes,
                             int input_size, const float* x_dev, const int32_t* labels_dev,
                             int64_t n_windows, float dropout_rate, uint64_t seed,
                             double* mean_loss_dev, int64_t* n_correct_dev, float* grads_dev,
                             float* batch_stats_dev, void* workspace_dev, dbh_stream stream,
                             int frozen_blocks) {
    const int st = check_arguments(n_floats, n_classes, input_size, n_windows, dropout_rate);
    if (st != DBH_OK) return st;
    if (!dbh_train::frozen_ok(frozen_blocks)) return DBH_ERR_INVALID_ARGUMENT;
    if (!weights_dev || !x_dev || !labels_dev || !mean_loss_dev || !n_correct_dev || !grads_dev ||
        !batch_stats_dev || !workspace_dev || ((uintptr_t)weights_dev & 15))
        return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(dbh_train::gradients(weights_dev, n_classes, input_size, x_dev, labels_dev,
                                 n_windows, dropout_rate, seed, mean_loss_dev, n_correct_dev,
                                 grads_dev, batch_stats_dev, workspace_dev,
                                 (hipStream_t)stream, frozen_blocks));
    return DBH_OK;
}

int dbh_gradients_dev(const float* weights_dev, int64_t n_floats, int n_classes, int input_size,
                      const float* x_dev, const int32_t* labels_dev, int64_t n_windows,
                      float dropout_rate, uint64_t seed, double* mean_loss_dev,
                      int64_t* n_correct_dev, float* grads_dev, float* batch_stats_dev,
                      void* workspace_dev, dbh_stream stream) {
    return dbh_gradients_frozen_dev(weights_dev, n_floats, n_classes, input_size, x_dev, labels_dev,
                                    n_windows, dropout_rate, seed, mean_loss_dev, n_correct_dev,
                                    grads_dev, batch_stats_dev, workspace_dev, stream, 0);
}

int dbh_evaluate_dev(const float* weights_dev, int64_t n_floats, int n_classes, int input_size,
                     const float* x_dev, const int32_t* labels_dev, int64_t n_windows,
                     double* loss_sum_dev, int64_t* n_correct_dev, double* window_loss_dev,
                     void* workspace_dev, dbh_stream stream) {
    const int st = check_arguments(n_floats, n_classes, input_size, n_windows, 0.f);
    if (st != DBH_OK) return st;
    if (!weights_dev || !x_dev || !labels_dev || !loss_sum_dev || !n_correct_dev || !workspace_dev ||
        ((uintptr_t)weights_dev & 15))
        return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(dbh_train::evaluate(weights_dev, n_classes, input_size, x_dev, labels_dev,
                                n_windows, loss_sum_dev, n_correct_dev, window_loss_dev,
                                workspace_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_evaluate(const float* weights_host, int64_t n_floats, int n_classes, int input_size,
                 const float* x_host, const int32_t* labels_host, int64_t n_windows,
                 double* loss_sum, int64_t* n_correct, double* window_loss_host) {
    const int st = check_arguments(n_floats, n_classes, input_size, n_windows, 0.f);
    if (st != DBH_OK) return st;
    if (!weights_host || !x_host || !labels_host || !loss_sum || !n_correct)
        return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_windows; ++i)
        if (labels_host[i] < 0 || labels_host[i] >= n_classes) return DBH_ERR_INVALID_ARGUMENT;

    const size_t w_bytes = (size_t)n_floats * sizeof(float);
    const size_t x_bytes = (size_t)n_windows * input_size * sizeof(float);
    const size_t l_bytes = (size_t)n_windows * sizeof(int32_t);
    const size_t wl_bytes = (size_t)n_windows * sizeof(double);
    // one block: weights, windows, labels, the totals, the windows' losses, the workspace
    float *w, *x;
    int32_t* labels;
    double *totals, *window_loss;      // (the totals: the loss, the count as int64 behind it)
    char* work;
    auto lay_out = [&](dbh_host::Carve& c) {
        w = c.take<float>((size_t)n_floats);
        x = c.take<float>((size_t)n_windows * input_size);
        labels = c.take<int32_t>((size_t)n_windows);
        totals = c.take<double>(2);
        window_loss = c.take<double>((size_t)n_windows);
        work = c.take<char>(dbh_train::workspace_bytes(n_classes, input_size, n_windows));
    };
    dbh_owned::DeviceBlock block;
    DBH_HIP(block.carve(lay_out));
    DBH_HIP(hipMemcpyAsync(w, weights_host, w_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(x, x_host, x_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(labels, labels_host, l_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemsetAsync(totals, 0, 16, 0));
    DBH_HIP(dbh_train::evaluate(w, n_classes, input_size, x, labels, n_windows, totals,
                                (int64_t*)(totals + 1), window_loss, work, 0));
    DBH_HIP(hipStreamSynchronize(0));
    struct { double loss; int64_t correct; } out;
    DBH_HIP(hipMemcpy(&out, totals, sizeof(out), hipMemcpyDeviceToHost));
    if (window_loss_host)
        DBH_HIP(hipMemcpy(window_loss_host, window_loss, wl_bytes, hipMemcpyDeviceToHost));
    *loss_sum = out.loss;
    *n_correct = out.correct;
    return DBH_OK;
}

int dbh_gradients_frozen(const float* weights_host, int64_t n_floats, int n_classes, int input_size,
                         const float* x_host, const int32_t* labels_host, int64_t n_windows,
                         float dropout_rate, uint64_t seed, double* mean_loss, int64_t* n_correct,
                         float* grads_host, float* batch_stats_host, int frozen_blocks) {
    const int st = check_arguments(n_floats, n_classes, input_size, n_windows, dropout_rate);
    if (st != DBH_OK) return st;
    if (!dbh_train::frozen_ok(frozen_blocks)) return DBH_ERR_INVALID_ARGUMENT;
    if (!weights_host || !x_host || !labels_host || !mean_loss || !n_correct || !grads_host ||
        !batch_stats_host)
        return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_windows; ++i)
        if (labels_host[i] < 0 || labels_host[i] >= n_classes) return DBH_ERR_INVALID_ARGUMENT;

    const size_t w_bytes = (size_t)n_floats * sizeof(float);
    const size_t x_bytes = (size_t)n_windows * input_size * sizeof(float);
    const size_t l_bytes = (size_t)n_windows * sizeof(int32_t);
    const size_t s_bytes = dbh_train::kStatsFloats * sizeof(float);
    // one block: weights, gradients, windows, labels, statistics, loss and count, the workspace
    float *w, *grads, *x, *stats;
    int32_t* labels;
    double* loss;                      // (the count as int64 behind it)
    char* work;
    auto lay_out = [&](dbh_host::Carve& c) {
        w = c.take<float>((size_t)n_floats);
        grads = c.take<float>((size_t)n_floats);
        x = c.take<float>((size_t)n_windows * input_size);
        labels = c.take<int32_t>((size_t)n_windows);
        stats = c.take<float>(dbh_train::kStatsFloats);
        loss = c.take<double>(2);
        work = c.take<char>(dbh_train::workspace_bytes(n_classes, input_size, n_windows));
    };
    dbh_owned::DeviceBlock block;
    DBH_HIP(block.carve(lay_out));
    DBH_HIP(hipMemcpyAsync(w, weights_host, w_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(x, x_host, x_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(labels, labels_host, l_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(dbh_train::gradients(w, n_classes, input_size, x, labels, n_windows, dropout_rate, seed,
                                 loss, (int64_t*)(loss + 1), grads, stats, work, 0, frozen_blocks));
    DBH_HIP(hipStreamSynchronize(0));
    // results reach the caller's buffers only once the whole call has succeeded
    struct { double loss; int64_t correct; } out;
    DBH_HIP(hipMemcpy(&out, loss, sizeof(out), hipMemcpyDeviceToHost));
    DBH_HIP(hipMemcpy(grads_host, grads, w_bytes, hipMemcpyDeviceToHost));
    DBH_HIP(hipMemcpy(batch_stats_host, stats, s_bytes, hipMemcpyDeviceToHost));
    *mean_loss = out.loss;
    *n_correct = out.correct;
    return DBH_OK;
}

int dbh_gradients(const float* weights_host, int64_t n_floats, int n_classes, int input_size,
                  const float* x_host, const int32_t* labels_host, int64_t n_windows,
                  float dropout_rate, uint64_t seed, double* mean_loss, int64_t* n_correct,
                  float* grads_host, float* batch_stats_host) {
    return dbh_gradients_frozen(weights_host, n_floats, n_classes, input_size, x_host, labels_host,
                                n_windows, dropout_rate, seed, mean_loss, n_correct, grads_host,
                                batch_stats_host, 0);
}

}  // extern "C"
