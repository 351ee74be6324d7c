// libdeepbinner_dtw.so - semi-global dynamic time warping for MI355X (gfx950 only).
// C ABI: include/deepbinner_dtw.h (replaces the reference's deepbinner/dtw/dtw.cpp:58-151).
//
// One wavefront per (reference signal, query signal) pair.  The query runs across the lanes, C
// consecutive columns per lane; lane l works on reference row s - l at step s, so that the value it
// needs from its left neighbour (row i of column chunk l - 1) was produced one step earlier and
// moves over with one DPP wave shift - no LDS, no barrier.  The C costs of a lane's chunk stay in
// registers from row to row.  Queries longer than 64 * 16 columns are done in panels, the last
// column of a panel handed to the next through a per-pair edge buffer.
//
// What goes to HBM is the direction of every cell, 2 bits, packed per lane and step into one
// word ([panel][step][lane], 4 bytes, one coalesced store per step): 0.25 - 1 byte per cell,
// written once.  The walk back
// runs in the same kernel: the wave fetches the words of 64 rows of the current column chunk at
// once (one per lane) and steps through them with v_readlane until the path leaves that tile.
//
// Arithmetic as in dtw.cpp, in fp64 and without contraction (-ffp-contract=off): cost = best of
// (diagonal, left, up) + (ref[i] - query[j])^2, the diagonal winning ties, an exact left/up tie
// going LEFT (the reference draws rand() there, dtw.cpp:40-45).
//
// Beside dtw_kernel: the kernels of prep's signal stage (dtw_rescaled_batch, dtw_locate_batch) -
// normalise, the line fit between two passes of dtw_kernel, the verdict on slope and fit, the
// first hit of a group - which keep the rescaled DTW and prep's scans on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/deepbinner_dtw.h"

namespace {

constexpr int kLanes = 64;
enum : unsigned { NIL = 0, DIAGONAL = 1, LEFT = 2, UP = 3 };

struct PairJob {
    int64_t ref_off, query_off;   // first sample in refs / queries
    int64_t path_off;             // first direction word of this pair (in words of the launch)
    int64_t edge_off;             // first double of its 2 * ref_len edge buffer (multi-panel only)
    int64_t align_off;            // first int of its alignment
    int32_t ref_len, query_len;
    int32_t pair, pad;
};

using Word = uint32_t;   // 2 bits per cell, at most 16 cells per lane

// lane l <- lane l - 1 (DPP wave_shr:1); lane 0 receives 0
__device__ __forceinline__ double from_left_lane(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x138, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x138, 0xF, 0xF, false);
    return __builtin_bit_cast(double,
                              (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// v_min_f64 as it is: llvm.minnum would first canonicalise both inputs (IEEE mode, signalling
// NaNs), two more instructions on the dependent chain of every cell
__device__ __forceinline__ double min_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// the double held by lane `lane` (uniform), for every lane
__device__ __forceinline__ double lane_value(double v, int lane) {
    const long long b = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ Word word_of_lane(Word w, int lane) {
    return (Word)__builtin_amdgcn_readlane((int)w, lane);
}

template <int C>
__global__ __launch_bounds__(kLanes) void dtw_kernel(
    const PairJob* __restrict__ jobs, const double* __restrict__ refs,
    const double* __restrict__ queries, Word* __restrict__ path,
    double* __restrict__ edges, double* __restrict__ distances, int32_t* __restrict__ positions,
    int32_t* __restrict__ path_lengths, int32_t* __restrict__ alignment) {
    constexpr int kPanel = kLanes * C;
    // only the widest variant ever sees a query of more than one panel (cells_per_lane): the
    // narrower ones drop the edge-column hand-over from their step altogether
    constexpr bool kMultiPanel = (C == 16);
    const PairJob job = jobs[blockIdx.x];
    const int lane = threadIdx.x;
    const int R = job.ref_len, Q = job.query_len;
    const double* ref = refs + job.ref_off;
    const double* query = queries + job.query_off;
    Word* words = path + job.path_off;
    double* edge = edges + job.edge_off;
    const int panels = (Q + kPanel - 1) / kPanel;
    // direction words are stored by STEP, [panel][s][lane] with s = row + lane: the 64 lanes of a
    // step then write 64 consecutive words (by row they would hit 64 different cache lines)
    const size_t kSteps = (size_t)R + kLanes - 1;
    const int last_lane = ((Q - 1) % kPanel) / C;
    const int last_c = __builtin_amdgcn_readfirstlane((Q - 1) % C);

    // ---- the fill (dtw.cpp:68-111) ----------------------------------------------------------
    double best = DBL_MAX;
    int best_i = 0;
    for (int p = 0; p < panels; ++p) {
        const int j0 = p * kPanel + lane * C;
        // cost[] holds the row above; +inf above row 0 (and in diag_in) makes the general rule
        // pick LEFT along the top row, which is what dtw.cpp:81-87 fills in there
        double q[C], cost[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            q[c] = (j0 + c < Q) ? query[j0 + c] : 0.0;
            cost[c] = HUGE_VAL;
        }
        const double* edge_in = edge + (size_t)((p + 1) & 1) * R;   // what panel p - 1 wrote
        double* edge_out = edge + (size_t)(p & 1) * R;
        const bool tracks_end = (p == panels - 1) && (lane == last_lane);
        const bool first_column = (j0 == 0);
        double newest_last = 0.0;    // cost of my last column in my newest row
        double diag_in = HUGE_VAL;   // left neighbour's last column one row up
        // Lane l needs ref[s - l] at step s - what lane l - 1 had one step earlier, so the
        // reference value travels along the lanes like the costs do and only lane 0 takes in a new
        // one per step.  Those come 64 at a time: one coalesced load per 64 steps, issued 64 steps
        // ahead, handed out with v_readlane - a load per step would put its latency on every
        // step.  The edge column of the previous panel reaches lane 0 the same way.
        auto block_at = [&](const double* base, int first) {
            const int at = first + lane;
            return (at < R) ? base[at] : 0.0;
        };
        double ref_block = block_at(ref, 0), ref_ahead = 0.0;
        double edge_block = 0.0, edge_ahead = 0.0;
        if constexpr (kMultiPanel) edge_block = (p > 0) ? block_at(edge_in, 0) : 0.0;
        double r = 0.0;
        for (int s = 0; s < R + kLanes - 1; ++s) {
            const int i = s - lane;
            const int k = s % kLanes;
            if (k == 0) {
                ref_ahead = block_at(ref, s + kLanes);
                if constexpr (kMultiPanel)
                    if (p > 0) edge_ahead = block_at(edge_in, s + kLanes);
            }
            double left_in = from_left_lane(newest_last);
            r = from_left_lane(r);
            const double ref_s = lane_value(ref_block, k);
            if (lane == 0) r = ref_s;
            if constexpr (kMultiPanel) {
                const double edge_s = lane_value(edge_block, k);
                if (lane == 0 && p > 0) left_in = edge_s;
            }
            if (k == kLanes - 1) {
                ref_block = ref_ahead;
                if constexpr (kMultiPanel) edge_block = edge_ahead;
            }
            if (i < 0 || i >= R) continue;
            double left = left_in, diag = diag_in;
            Word word = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                // dtw.cpp:29-46 without branches: the cost to come from is min(diag, left, top);
                // DIAGONAL iff that is the diagonal (it wins ties), else UP iff top < left
                const double top = cost[c];
                const double d = r - q[c];
                const double from = min_f64(left, min_f64(diag, top));
                unsigned dir = (from == diag) ? DIAGONAL : ((top < left) ? UP : LEFT);
                double value = from + d * d;
                if (c == 0 && first_column) {   // dtw.cpp:68-78: the query may start anywhere
                    value = 0.0;
                    dir = NIL;
                }
                word |= dir << (2 * c);
                diag = top;
                left = value;
                cost[c] = value;
            }
            words[((size_t)p * kSteps + s) * kLanes + lane] = word;
            newest_last = cost[C - 1];
            diag_in = left_in;
            if constexpr (kMultiPanel)
                if (lane == kLanes - 1 && p + 1 < panels) edge_out[i] = newest_last;
            if (tracks_end && i >= 1) {    // dtw.cpp:113-122: first smallest over rows 1..R-1
                const double v = cost[last_c];   // uniform index: s_set_gpr_idx + v_mov
                if (v < best) {
                    best = v;
                    best_i = i;
                }
            }
        }
        __threadfence();    // the edge column (and, last time round, the words) for other lanes
    }
    best = __shfl(best, last_lane);
    best_i = __shfl(best_i, last_lane);

    // ---- the walk back (dtw.cpp:124-145) ----------------------------------------------------
    int32_t* out = alignment ? alignment + job.align_off : nullptr;
    int i = best_i, j = Q - 1, n = 0;
    for (;;) {
        const int p = j / kPanel, chunk = (j % kPanel) / C;
        const int tile_top = i;
        const int row = tile_top - lane;
        Word mine = 0;
        if (row >= 0) mine = words[((size_t)p * kSteps + row + chunk) * kLanes + chunk];
        bool done = false;
        for (;;) {
            if (out && lane == 0) {
                out[2 * n] = i;
                out[2 * n + 1] = j;
            }
            ++n;
            if (j == 0) {
                done = true;
                break;
            }
            const Word w = word_of_lane(mine, __builtin_amdgcn_readfirstlane(tile_top - i));
            const unsigned dir = (unsigned)(w >> (2 * (j % C))) & 3u;
            if (dir != LEFT) --i;
            if (dir != UP) --j;
            if (tile_top - i >= kLanes || j / C != p * kLanes + chunk) break;
        }
        if (done) break;
    }
    if (lane == 0) {
        distances[job.pair] = best;
        positions[2 * job.pair] = i;
        positions[2 * job.pair + 1] = best_i;
        path_lengths[job.pair] = n;
    }
}

// ------------------------------------------------------------------------------------------------
// prep's signal stage (include/deepbinner_dtw.h, "Rescaled DTW" and "Locate"): what runs between
// and around two passes of dtw_kernel so that nothing has to cross to the host in between.

// One block per read: int16 region -> fp64, ((double)x - mean) / std, or (double)x - mean where
// std is 0.  mean and std are the whole trimmed read's, formed by the host from exact integer sums.
__global__ __launch_bounds__(256) void normalise_kernel(
    const int16_t* __restrict__ samples, const int64_t* __restrict__ region_offsets,
    const double* __restrict__ mean_std, double* __restrict__ out) {
    const int64_t first = region_offsets[blockIdx.x], last = region_offsets[blockIdx.x + 1];
    const double mean = mean_std[2 * (size_t)blockIdx.x], sd = mean_std[2 * (size_t)blockIdx.x + 1];
    for (int64_t k = first + threadIdx.x; k < last; k += 256) {
        const double centred = (double)samples[k] - mean;
        out[k] = (sd > 0.0) ? centred / sd : centred;
    }
}

// One wave per pair, between the passes: the line y = m x + b through (query[j], ref[i]) over the
// alignment pass 1 left on the device, and the pair's own rescaled query.  Summation order (the
// header fixes it): lane l adds path entries l, l + 64, ... in stored order (from the alignment's
// END backwards) into its four partial sums, starting from +0.0; the totals start from +0.0 and
// take the 64 partials in lane order.  x * x and x * y are rounded before they are added.
__global__ __launch_bounds__(kLanes) void fit_kernel(
    const PairJob* __restrict__ first_pass, const PairJob* __restrict__ second_pass,
    const double* __restrict__ refs, const double* __restrict__ queries,
    const int32_t* __restrict__ alignment, const int32_t* __restrict__ path_lengths,
    double* __restrict__ rescaled, double* __restrict__ slopes, int32_t* __restrict__ bad_fit) {
    const PairJob job = first_pass[blockIdx.x];
    const int lane = threadIdx.x;
    const double* ref = refs + job.ref_off;
    const double* query = queries + job.query_off;
    double* out = rescaled + second_pass[blockIdx.x].query_off;
    const int2* pairs = reinterpret_cast<const int2*>(alignment + job.align_off);
    const int n = path_lengths[job.pair];
    double sx = 0.0, sy = 0.0, sxx = 0.0, sxy = 0.0;
    for (int k = lane; k < n; k += kLanes) {
        const int2 ij = pairs[k];
        const double y = ref[ij.x], x = query[ij.y];
        sx += x;
        sy += y;
        sxx += x * x;
        sxy += x * y;
    }
    double Sx = 0.0, Sy = 0.0, Sxx = 0.0, Sxy = 0.0;
    for (int l = 0; l < kLanes; ++l) {
        Sx += lane_value(sx, l);
        Sy += lane_value(sy, l);
        Sxx += lane_value(sxx, l);
        Sxy += lane_value(sxy, l);
    }
    const double count = (double)n;
    const double denominator = count * Sxx - Sx * Sx;
    // a constant query (or sums that left the finite range): no line, the query stays as it is
    // and the verdict makes the distance +inf
    const bool bad = !(denominator != 0.0 && fabs(denominator) <= DBL_MAX);
    double m = 1.0, b = 0.0;
    if (!bad) {
        m = (count * Sxy - Sx * Sy) / denominator;
        b = (Sy - m * Sx) / count;
    }
    for (int j = lane; j < job.query_len; j += kLanes) {
        const double scaled = m * query[j];
        out[j] = bad ? query[j] : scaled + b;
    }
    if (lane == 0) {
        slopes[job.pair] = bad ? __builtin_nan("") : m;
        bad_fit[job.pair] = bad ? 1 : 0;
    }
}

// One thread per pair, after pass 2: a slope outside 0.75 .. 1.333 (reference
// dtw_semi_global.py:91-93) or a fit that could not be made turns the distance into +inf; a
// skipped job (empty window) gets +inf, positions -1 and a NaN slope.
__global__ __launch_bounds__(256) void verdict_kernel(
    int64_t n, const int32_t* __restrict__ ref_lengths, const int32_t* __restrict__ bad_fit,
    double* __restrict__ slopes, double* __restrict__ distances, int32_t* __restrict__ positions) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    if (ref_lengths[k] == 0) {
        distances[k] = HUGE_VAL;
        positions[2 * k] = positions[2 * k + 1] = -1;
        slopes[k] = __builtin_nan("");
        return;
    }
    const double m = slopes[k];
    if (bad_fit[k] || m < 0.75 || m > 1.333) distances[k] = HUGE_VAL;
}

// One thread per group: its first job, in job order, with a finite distance <= threshold.
__global__ __launch_bounds__(256) void select_kernel(
    int64_t n_groups, const int64_t* __restrict__ group_offsets,
    const double* __restrict__ distances, double threshold, int32_t* __restrict__ hits) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    int32_t hit = -1;
    for (int64_t k = group_offsets[g]; k < group_offsets[g + 1]; ++k) {
        const double d = distances[k];
        if (d <= threshold && d < HUGE_VAL) {
            hit = (int32_t)k;
            break;
        }
    }
    hits[g] = hit;
}

// ------------------------------------------------------------------------------------------------
thread_local std::string g_error;

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        const hipError_t e = hipMalloc(&ptr, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
};

struct Context {
    std::mutex lock;
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t begin = nullptr, end = nullptr;
    DeviceBuffer refs, queries, jobs, path, edges, distances, positions, lengths, alignment;
    // the resident entries (dtw_rescaled_batch, dtw_locate_batch) only
    DeviceBuffer second_jobs, first_alignment, rescaled, slopes, bad_fit, ref_lengths, samples,
        region_offsets, mean_std, group_offsets, hits;
    double last_ms = 0.0;
    int64_t last_cells = 0;
};
Context g_ctx;

#define DTW_HIP(call)                                                                    \
    do {                                                                                 \
        const hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) {                                                          \
            g_error = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            return DTW_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

int prepare(Context& ctx) {
    int device = 0, count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        g_error = "no HIP device";
        return DTW_ERR_NO_DEVICE;
    }
    DTW_HIP(hipGetDevice(&device));
    if (ctx.device != device) {
        hipDeviceProp_t prop;
        DTW_HIP(hipGetDeviceProperties(&prop, device));
        if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
            g_error = std::string("built for gfx950, device is ") + prop.gcnArchName;
            return DTW_ERR_NO_DEVICE;
        }
        // first use, or the caller switched devices: buffers of the other device are dropped
        for (DeviceBuffer* b : {&ctx.refs, &ctx.queries, &ctx.jobs, &ctx.path, &ctx.edges,
                                &ctx.distances, &ctx.positions, &ctx.lengths, &ctx.alignment,
                                &ctx.second_jobs, &ctx.first_alignment, &ctx.rescaled, &ctx.slopes,
                                &ctx.bad_fit, &ctx.ref_lengths, &ctx.samples, &ctx.region_offsets,
                                &ctx.mean_std, &ctx.group_offsets, &ctx.hits})
            *b = DeviceBuffer{};
        ctx.device = device;
        DTW_HIP(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
        DTW_HIP(hipEventCreate(&ctx.begin));
        DTW_HIP(hipEventCreate(&ctx.end));
    }
    return DTW_OK;
}

size_t path_budget_bytes() {
    if (const char* text = std::getenv("DEEPBINNER_DTW_PATH_BYTES")) {
        const long long v = std::atoll(text);
        if (v > 0) return (size_t)v;
    }
    return (size_t)8 << 30;
}

int cells_per_lane(int query_len) {
    // longer queries than 64 * 16 columns go in panels of that width: measured faster than 32
    // columns per lane, which leaves room for two waves per SIMD only
    for (int c : {4, 8})
        if (query_len <= kLanes * c) return c;
    return 16;
}

template <int C>
void launch(Context& ctx, int n, int32_t* alignment) {
    hipLaunchKernelGGL(dtw_kernel<C>, dim3(n), dim3(kLanes), 0, ctx.stream,
                       (const PairJob*)ctx.jobs.ptr, (const double*)ctx.refs.ptr,
                       (const double*)ctx.queries.ptr, (Word*)ctx.path.ptr,
                       (double*)ctx.edges.ptr, (double*)ctx.distances.ptr,
                       (int32_t*)ctx.positions.ptr, (int32_t*)ctx.lengths.ptr, alignment);
}

// One launch: jobs of one lane width whose direction words fit the budget.
int run_group(Context& ctx, int c, std::vector<PairJob>& jobs, bool want_alignment) {
    const int panel = kLanes * c;
    // the longest first: the tail of the launch is then made of the short ones
    std::sort(jobs.begin(), jobs.end(), [](const PairJob& a, const PairJob& b) {
        return (int64_t)a.ref_len * a.query_len > (int64_t)b.ref_len * b.query_len;
    });
    size_t words = 0, edge_doubles = 0;
    for (PairJob& job : jobs) {
        const int panels = (job.query_len + panel - 1) / panel;
        job.path_off = (int64_t)words;
        words += (size_t)panels * ((size_t)job.ref_len + kLanes - 1) * kLanes;
        job.edge_off = (int64_t)edge_doubles;
        if (panels > 1) edge_doubles += (size_t)2 * job.ref_len;
    }
    DTW_HIP(ctx.path.reserve(std::max<size_t>(words * sizeof(Word), 8)));
    DTW_HIP(ctx.edges.reserve(std::max<size_t>(edge_doubles * sizeof(double), 8)));
    DTW_HIP(ctx.jobs.reserve(jobs.size() * sizeof(PairJob)));
    DTW_HIP(hipMemcpyAsync(ctx.jobs.ptr, jobs.data(), jobs.size() * sizeof(PairJob),
                           hipMemcpyHostToDevice, ctx.stream));
    int32_t* alignment = want_alignment ? (int32_t*)ctx.alignment.ptr : nullptr;
    DTW_HIP(hipEventRecord(ctx.begin, ctx.stream));
    switch (c) {
        case 4: launch<4>(ctx, (int)jobs.size(), alignment); break;
        case 8: launch<8>(ctx, (int)jobs.size(), alignment); break;
        default: launch<16>(ctx, (int)jobs.size(), alignment); break;
    }
    DTW_HIP(hipGetLastError());
    DTW_HIP(hipEventRecord(ctx.end, ctx.stream));
    DTW_HIP(hipStreamSynchronize(ctx.stream));
    float ms = 0.f;
    DTW_HIP(hipEventElapsedTime(&ms, ctx.begin, ctx.end));
    ctx.last_ms += ms;
    for (const PairJob& job : jobs) ctx.last_cells += (int64_t)job.ref_len * job.query_len;
    return DTW_OK;
}

int run_batch(Context& ctx, const double* refs, const int64_t* ref_offsets, const double* queries,
              const int64_t* query_offsets, int64_t n_pairs, double* distances, int32_t* positions,
              int32_t* path_lengths, int32_t* alignment) {
    const int64_t n_ref = ref_offsets[n_pairs] - ref_offsets[0];
    const int64_t n_query = query_offsets[n_pairs] - query_offsets[0];
    const size_t align_ints = (size_t)2 * (size_t)(ref_offsets[n_pairs] + query_offsets[n_pairs]);
    ctx.last_ms = 0.0;
    ctx.last_cells = 0;
    DTW_HIP(ctx.refs.reserve((size_t)n_ref * sizeof(double)));
    DTW_HIP(ctx.queries.reserve((size_t)n_query * sizeof(double)));
    DTW_HIP(ctx.distances.reserve((size_t)n_pairs * sizeof(double)));
    DTW_HIP(ctx.positions.reserve((size_t)n_pairs * 2 * sizeof(int32_t)));
    DTW_HIP(ctx.lengths.reserve((size_t)n_pairs * sizeof(int32_t)));
    if (alignment) DTW_HIP(ctx.alignment.reserve(align_ints * sizeof(int32_t)));
    DTW_HIP(hipMemcpyAsync(ctx.refs.ptr, refs + ref_offsets[0], (size_t)n_ref * sizeof(double),
                           hipMemcpyHostToDevice, ctx.stream));
    DTW_HIP(hipMemcpyAsync(ctx.queries.ptr, queries + query_offsets[0],
                           (size_t)n_query * sizeof(double), hipMemcpyHostToDevice, ctx.stream));

    const size_t budget = path_budget_bytes();
    for (int c : {4, 8, 16}) {
        std::vector<PairJob> group;
        size_t bytes = 0;
        for (int64_t p = 0; p <= n_pairs; ++p) {
            size_t need = 0;
            if (p < n_pairs) {
                const int64_t r = ref_offsets[p + 1] - ref_offsets[p];
                const int64_t q = query_offsets[p + 1] - query_offsets[p];
                if (cells_per_lane((int)q) != c) continue;
                const int64_t panels = (q + kLanes * c - 1) / (kLanes * c);
                need = (size_t)panels * (size_t)(r + kLanes - 1) * kLanes * sizeof(Word);
                if (!group.empty() && bytes + need > budget) {
                    const int st = run_group(ctx, c, group, alignment != nullptr);
                    if (st != DTW_OK) return st;
                    group.clear();
                    bytes = 0;
                }
                PairJob job{};
                job.ref_off = ref_offsets[p] - ref_offsets[0];
                job.query_off = query_offsets[p] - query_offsets[0];
                job.align_off = 2 * (ref_offsets[p] + query_offsets[p]);
                job.ref_len = (int32_t)r;
                job.query_len = (int32_t)q;
                job.pair = (int32_t)p;
                group.push_back(job);
                bytes += need;
            } else if (!group.empty()) {
                const int st = run_group(ctx, c, group, alignment != nullptr);
                if (st != DTW_OK) return st;
            }
        }
    }
    DTW_HIP(hipMemcpyAsync(distances, ctx.distances.ptr, (size_t)n_pairs * sizeof(double),
                           hipMemcpyDeviceToHost, ctx.stream));
    DTW_HIP(hipMemcpyAsync(positions, ctx.positions.ptr, (size_t)n_pairs * 2 * sizeof(int32_t),
                           hipMemcpyDeviceToHost, ctx.stream));
    DTW_HIP(hipMemcpyAsync(path_lengths, ctx.lengths.ptr, (size_t)n_pairs * sizeof(int32_t),
                           hipMemcpyDeviceToHost, ctx.stream));
    DTW_HIP(hipStreamSynchronize(ctx.stream));
    if (alignment) {
        const size_t first = (size_t)2 * (size_t)(ref_offsets[0] + query_offsets[0]);
        DTW_HIP(hipMemcpyAsync(alignment + first, (const int32_t*)ctx.alignment.ptr + first,
                               (align_ints - first) * sizeof(int32_t), hipMemcpyDeviceToHost,
                               ctx.stream));
        DTW_HIP(hipStreamSynchronize(ctx.stream));
    }
    return DTW_OK;
}

// ---- the resident entries ----------------------------------------------------------------------
// A pair of the rescaled DTW: where its reference and its query lie in ctx.refs / ctx.queries, and
// where its pass-2 alignment goes.  ref_len == 0: a skipped job (dtw_locate_batch's empty window).
struct ResidentPair {
    int64_t ref_off, query_off, align_off;
    int32_t ref_len, query_len;
};

// One part: pairs of one lane width whose direction words fit the budget.  A pair's pass 1, fit
// and pass 2 are all in its part; the direction words, the edge columns and the pass-1 alignments
// are the part's and are used again by the next part, in stream order.
struct Part {
    int c;
    size_t first, count;   // its jobs in the two job arrays
};

template <int C>
void launch_pass(Context& ctx, const Part& part, const PairJob* jobs, const double* queries,
                 int32_t* alignment) {
    hipLaunchKernelGGL(dtw_kernel<C>, dim3((unsigned)part.count), dim3(kLanes), 0, ctx.stream,
                       jobs + part.first, (const double*)ctx.refs.ptr, queries,
                       (Word*)ctx.path.ptr, (double*)ctx.edges.ptr, (double*)ctx.distances.ptr,
                       (int32_t*)ctx.positions.ptr, (int32_t*)ctx.lengths.ptr, alignment);
}

void launch_pass(Context& ctx, const Part& part, const PairJob* jobs, const double* queries,
                 int32_t* alignment) {
    switch (part.c) {
        case 4: launch_pass<4>(ctx, part, jobs, queries, alignment); break;
        case 8: launch_pass<8>(ctx, part, jobs, queries, alignment); break;
        default: launch_pass<16>(ctx, part, jobs, queries, alignment); break;
    }
}

// What plan_rescaled works out and queue_rescaled launches.  The job arrays are copied to the
// device asynchronously, so the plan is the caller's and lives until the caller has synchronised.
struct ResidentPlan {
    std::vector<Part> parts;
    std::vector<PairJob> first_jobs, second_jobs;   // pass 1 and pass 2, part after part
    std::vector<int32_t> ref_lengths;
    size_t n_pairs = 0;
    bool want_alignment = false;
};

// Cuts the pairs into parts, sizes every buffer the launches need (once: nothing is allocated
// between the launches) and queues the upload of the job arrays.
int plan_rescaled(Context& ctx, const std::vector<ResidentPair>& pairs, bool want_alignment,
                  size_t alignment_ints, ResidentPlan& plan) {
    const size_t n = pairs.size();
    const size_t budget = path_budget_bytes();
    std::vector<Part>& parts = plan.parts;
    std::vector<PairJob>& first_jobs = plan.first_jobs;
    std::vector<PairJob>& second_jobs = plan.second_jobs;
    std::vector<int32_t>& ref_lengths = plan.ref_lengths;
    plan.n_pairs = n;
    plan.want_alignment = want_alignment;
    parts.clear();
    ref_lengths.assign(n, 0);
    size_t rescaled_doubles = 0, max_words = 0, max_edges = 0, max_first_alignment = 0;
    std::vector<int64_t> rescaled_off(n);
    for (size_t p = 0; p < n; ++p) {
        ref_lengths[p] = pairs[p].ref_len;
        rescaled_off[p] = (int64_t)rescaled_doubles;
        if (pairs[p].ref_len > 0) rescaled_doubles += (size_t)pairs[p].query_len;
    }
    first_jobs.clear();
    ctx.last_ms = 0.0;
    ctx.last_cells = 0;
    for (int c : {4, 8, 16}) {
        const int panel = kLanes * c;
        auto close_part = [&](size_t first) {
            if (first == first_jobs.size()) return;
            // the longest first, as run_group has them
            std::sort(first_jobs.begin() + first, first_jobs.end(),
                      [](const PairJob& a, const PairJob& b) {
                          return (int64_t)a.ref_len * a.query_len > (int64_t)b.ref_len * b.query_len;
                      });
            size_t words = 0, edge_doubles = 0, align_ints = 0;
            for (size_t k = first; k < first_jobs.size(); ++k) {
                PairJob& job = first_jobs[k];
                const int panels = (job.query_len + panel - 1) / panel;
                job.path_off = (int64_t)words;
                words += (size_t)panels * ((size_t)job.ref_len + kLanes - 1) * kLanes;
                job.edge_off = (int64_t)edge_doubles;
                if (panels > 1) edge_doubles += (size_t)2 * job.ref_len;
                job.align_off = (int64_t)align_ints;
                align_ints += (size_t)2 * ((size_t)job.ref_len + job.query_len);
            }
            max_words = std::max(max_words, words);
            max_edges = std::max(max_edges, edge_doubles);
            max_first_alignment = std::max(max_first_alignment, align_ints);
            parts.push_back(Part{c, first, first_jobs.size() - first});
        };
        size_t first = first_jobs.size(), bytes = 0;
        for (size_t p = 0; p < n; ++p) {
            const ResidentPair& pair = pairs[p];
            if (pair.ref_len == 0 || cells_per_lane(pair.query_len) != c) continue;
            const size_t panels = ((size_t)pair.query_len + panel - 1) / panel;
            const size_t need = panels * ((size_t)pair.ref_len + kLanes - 1) * kLanes * sizeof(Word);
            if (first != first_jobs.size() && bytes + need > budget) {
                close_part(first);
                first = first_jobs.size();
                bytes = 0;
            }
            PairJob job{};
            job.ref_off = pair.ref_off;
            job.query_off = pair.query_off;
            job.ref_len = pair.ref_len;
            job.query_len = pair.query_len;
            job.pair = (int32_t)p;
            first_jobs.push_back(job);
            bytes += need;
            ctx.last_cells += (int64_t)2 * pair.ref_len * pair.query_len;
        }
        close_part(first);
    }
    // pass 2 of a pair: the same job on its own rescaled query, its alignment where the caller
    // wants it
    second_jobs = first_jobs;
    for (PairJob& job : second_jobs) {
        job.query_off = rescaled_off[job.pair];
        job.align_off = pairs[job.pair].align_off;
    }
    const size_t n_jobs = first_jobs.size();
    DTW_HIP(ctx.path.reserve(std::max<size_t>(max_words * sizeof(Word), 8)));
    DTW_HIP(ctx.edges.reserve(std::max<size_t>(max_edges * sizeof(double), 8)));
    DTW_HIP(ctx.first_alignment.reserve(std::max<size_t>(max_first_alignment * sizeof(int32_t), 8)));
    DTW_HIP(ctx.rescaled.reserve(std::max<size_t>(rescaled_doubles * sizeof(double), 8)));
    DTW_HIP(ctx.jobs.reserve(std::max<size_t>(n_jobs * sizeof(PairJob), 8)));
    DTW_HIP(ctx.second_jobs.reserve(std::max<size_t>(n_jobs * sizeof(PairJob), 8)));
    DTW_HIP(ctx.distances.reserve(n * sizeof(double)));
    DTW_HIP(ctx.positions.reserve(n * 2 * sizeof(int32_t)));
    DTW_HIP(ctx.lengths.reserve(n * sizeof(int32_t)));
    DTW_HIP(ctx.slopes.reserve(n * sizeof(double)));
    DTW_HIP(ctx.bad_fit.reserve(n * sizeof(int32_t)));
    DTW_HIP(ctx.ref_lengths.reserve(n * sizeof(int32_t)));
    if (want_alignment)
        DTW_HIP(ctx.alignment.reserve(std::max<size_t>(alignment_ints * sizeof(int32_t), 8)));
    if (n_jobs) {
        DTW_HIP(hipMemcpyAsync(ctx.jobs.ptr, first_jobs.data(), n_jobs * sizeof(PairJob),
                               hipMemcpyHostToDevice, ctx.stream));
        DTW_HIP(hipMemcpyAsync(ctx.second_jobs.ptr, second_jobs.data(), n_jobs * sizeof(PairJob),
                               hipMemcpyHostToDevice, ctx.stream));
    }
    DTW_HIP(hipMemcpyAsync(ctx.ref_lengths.ptr, ref_lengths.data(), n * sizeof(int32_t),
                           hipMemcpyHostToDevice, ctx.stream));
    return DTW_OK;
}

// Queues, on ctx.stream and without a synchronise: pass 1, fit, pass 2 for every part, then the
// verdict.  ctx.refs and ctx.queries are filled by work queued before.  Leaves, per pair, on the
// device: distances, positions, lengths (of pass 2), slopes; the rescaled queries back to back in
// pair order in ctx.rescaled; the pass-2 alignments in ctx.alignment when wanted.
int queue_rescaled(Context& ctx, const ResidentPlan& plan) {
    const size_t n = plan.n_pairs;
    const bool want_alignment = plan.want_alignment;
    for (const Part& part : plan.parts) {
        launch_pass(ctx, part, (const PairJob*)ctx.jobs.ptr, (const double*)ctx.queries.ptr,
                    (int32_t*)ctx.first_alignment.ptr);
        hipLaunchKernelGGL(fit_kernel, dim3((unsigned)part.count), dim3(kLanes), 0, ctx.stream,
                           (const PairJob*)ctx.jobs.ptr + part.first,
                           (const PairJob*)ctx.second_jobs.ptr + part.first,
                           (const double*)ctx.refs.ptr, (const double*)ctx.queries.ptr,
                           (const int32_t*)ctx.first_alignment.ptr,
                           (const int32_t*)ctx.lengths.ptr, (double*)ctx.rescaled.ptr,
                           (double*)ctx.slopes.ptr, (int32_t*)ctx.bad_fit.ptr);
        launch_pass(ctx, part, (const PairJob*)ctx.second_jobs.ptr,
                    (const double*)ctx.rescaled.ptr,
                    want_alignment ? (int32_t*)ctx.alignment.ptr : nullptr);
        DTW_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(verdict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx.stream,
                       (int64_t)n, (const int32_t*)ctx.ref_lengths.ptr,
                       (const int32_t*)ctx.bad_fit.ptr, (double*)ctx.slopes.ptr,
                       (double*)ctx.distances.ptr, (int32_t*)ctx.positions.ptr);
    DTW_HIP(hipGetLastError());
    return DTW_OK;
}

int finish_timing(Context& ctx) {
    float ms = 0.f;
    DTW_HIP(hipEventElapsedTime(&ms, ctx.begin, ctx.end));
    ctx.last_ms = ms;
    return DTW_OK;
}

int run_rescaled(Context& ctx, const double* refs, const int64_t* ref_offsets,
                 const double* queries, const int64_t* query_offsets, int64_t n_pairs,
                 double* distances, int32_t* positions, double* slopes, double* rescaled,
                 int32_t* path_lengths, int32_t* alignment) {
    const int64_t n_ref = ref_offsets[n_pairs] - ref_offsets[0];
    const int64_t n_query = query_offsets[n_pairs] - query_offsets[0];
    const size_t align_first = (size_t)2 * (size_t)(ref_offsets[0] + query_offsets[0]);
    const size_t align_ints =
        (size_t)2 * (size_t)(ref_offsets[n_pairs] + query_offsets[n_pairs]) - align_first;
    DTW_HIP(ctx.refs.reserve((size_t)n_ref * sizeof(double)));
    DTW_HIP(ctx.queries.reserve((size_t)n_query * sizeof(double)));
    DTW_HIP(hipMemcpyAsync(ctx.refs.ptr, refs + ref_offsets[0], (size_t)n_ref * sizeof(double),
                           hipMemcpyHostToDevice, ctx.stream));
    DTW_HIP(hipMemcpyAsync(ctx.queries.ptr, queries + query_offsets[0],
                           (size_t)n_query * sizeof(double), hipMemcpyHostToDevice, ctx.stream));
    std::vector<ResidentPair> pairs((size_t)n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p) {
        ResidentPair& pair = pairs[(size_t)p];
        pair.ref_off = ref_offsets[p] - ref_offsets[0];
        pair.query_off = query_offsets[p] - query_offsets[0];
        pair.align_off = 2 * (ref_offsets[p] + query_offsets[p]) - (int64_t)align_first;
        pair.ref_len = (int32_t)(ref_offsets[p + 1] - ref_offsets[p]);
        pair.query_len = (int32_t)(query_offsets[p + 1] - query_offsets[p]);
    }
    ResidentPlan plan;
    int st = plan_rescaled(ctx, pairs, alignment != nullptr, align_ints, plan);
    if (st != DTW_OK) return st;
    DTW_HIP(hipEventRecord(ctx.begin, ctx.stream));
    st = queue_rescaled(ctx, plan);
    if (st != DTW_OK) return st;
    DTW_HIP(hipEventRecord(ctx.end, ctx.stream));
    DTW_HIP(hipMemcpyAsync(distances, ctx.distances.ptr, (size_t)n_pairs * sizeof(double),
                           hipMemcpyDeviceToHost, ctx.stream));
    DTW_HIP(hipMemcpyAsync(positions, ctx.positions.ptr, (size_t)n_pairs * 2 * sizeof(int32_t),
                           hipMemcpyDeviceToHost, ctx.stream));
    DTW_HIP(hipMemcpyAsync(slopes, ctx.slopes.ptr, (size_t)n_pairs * sizeof(double),
                           hipMemcpyDeviceToHost, ctx.stream));
    // every pair has a reference here, so the rescaled queries lie as the queries do
    if (rescaled)
        DTW_HIP(hipMemcpyAsync(rescaled + query_offsets[0], ctx.rescaled.ptr,
                               (size_t)n_query * sizeof(double), hipMemcpyDeviceToHost,
                               ctx.stream));
    if (path_lengths)
        DTW_HIP(hipMemcpyAsync(path_lengths, ctx.lengths.ptr, (size_t)n_pairs * sizeof(int32_t),
                               hipMemcpyDeviceToHost, ctx.stream));
    if (alignment)
        DTW_HIP(hipMemcpyAsync(alignment + align_first, ctx.alignment.ptr,
                               align_ints * sizeof(int32_t), hipMemcpyDeviceToHost, ctx.stream));
    DTW_HIP(hipStreamSynchronize(ctx.stream));
    return finish_timing(ctx);
}

struct LocateArguments {
    const int16_t* samples;
    const int64_t* region_offsets;
    const double* mean_std;
    int64_t n_reads;
    const double* queries;
    const int64_t* query_offsets;
    int64_t n_queries;
    const int64_t* jobs;
    int64_t n_jobs;
    const int64_t* group_offsets;
    int64_t n_groups;
    double threshold;
};

int run_locate(Context& ctx, const LocateArguments& a, double* distances, int32_t* positions,
               double* slopes, int32_t* hits) {
    const int64_t n_samples = a.region_offsets[a.n_reads] - a.region_offsets[0];
    const int64_t n_query = a.query_offsets[a.n_queries] - a.query_offsets[0];
    std::vector<int64_t> regions((size_t)a.n_reads + 1);
    for (int64_t r = 0; r <= a.n_reads; ++r)
        regions[(size_t)r] = a.region_offsets[r] - a.region_offsets[0];
    DTW_HIP(ctx.samples.reserve(std::max<size_t>((size_t)n_samples * sizeof(int16_t), 8)));
    DTW_HIP(ctx.refs.reserve(std::max<size_t>((size_t)n_samples * sizeof(double), 8)));
    DTW_HIP(ctx.queries.reserve((size_t)n_query * sizeof(double)));
    DTW_HIP(ctx.region_offsets.reserve(regions.size() * sizeof(int64_t)));
    DTW_HIP(ctx.mean_std.reserve((size_t)a.n_reads * 2 * sizeof(double)));
    DTW_HIP(ctx.group_offsets.reserve(((size_t)a.n_groups + 1) * sizeof(int64_t)));
    DTW_HIP(ctx.hits.reserve(std::max<size_t>((size_t)a.n_groups * sizeof(int32_t), 8)));
    if (n_samples)
        DTW_HIP(hipMemcpyAsync(ctx.samples.ptr, a.samples + a.region_offsets[0],
                               (size_t)n_samples * sizeof(int16_t), hipMemcpyHostToDevice,
                               ctx.stream));
    DTW_HIP(hipMemcpyAsync(ctx.queries.ptr, a.queries + a.query_offsets[0],
                           (size_t)n_query * sizeof(double), hipMemcpyHostToDevice, ctx.stream));
    DTW_HIP(hipMemcpyAsync(ctx.region_offsets.ptr, regions.data(),
                           regions.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx.stream));
    DTW_HIP(hipMemcpyAsync(ctx.mean_std.ptr, a.mean_std, (size_t)a.n_reads * 2 * sizeof(double),
                           hipMemcpyHostToDevice, ctx.stream));
    DTW_HIP(hipMemcpyAsync(ctx.group_offsets.ptr, a.group_offsets,
                           ((size_t)a.n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                           ctx.stream));
    // the windows overlap: every job points into the one normalised buffer, none is copied
    std::vector<ResidentPair> pairs((size_t)a.n_jobs);
    for (int64_t k = 0; k < a.n_jobs; ++k) {
        const int64_t read = a.jobs[4 * k], from = a.jobs[4 * k + 1], to = a.jobs[4 * k + 2];
        const int64_t query = a.jobs[4 * k + 3];
        ResidentPair& pair = pairs[(size_t)k];
        pair.ref_off = regions[(size_t)read] + from;
        pair.query_off = a.query_offsets[query] - a.query_offsets[0];
        pair.align_off = 0;
        pair.ref_len = (int32_t)(to - from);
        pair.query_len = (int32_t)(a.query_offsets[query + 1] - a.query_offsets[query]);
    }
    ResidentPlan plan;
    int st = plan_rescaled(ctx, pairs, false, 0, plan);
    if (st != DTW_OK) return st;
    DTW_HIP(hipEventRecord(ctx.begin, ctx.stream));
    hipLaunchKernelGGL(normalise_kernel, dim3((unsigned)a.n_reads), dim3(256), 0, ctx.stream,
                       (const int16_t*)ctx.samples.ptr, (const int64_t*)ctx.region_offsets.ptr,
                       (const double*)ctx.mean_std.ptr, (double*)ctx.refs.ptr);
    DTW_HIP(hipGetLastError());
    st = queue_rescaled(ctx, plan);
    if (st != DTW_OK) return st;
    if (a.n_groups)
        hipLaunchKernelGGL(select_kernel, dim3((unsigned)((a.n_groups + 255) / 256)), dim3(256),
                           0, ctx.stream, a.n_groups, (const int64_t*)ctx.group_offsets.ptr,
                           (const double*)ctx.distances.ptr, a.threshold,
                           (int32_t*)ctx.hits.ptr);
    DTW_HIP(hipGetLastError());
    DTW_HIP(hipEventRecord(ctx.end, ctx.stream));
    DTW_HIP(hipMemcpyAsync(distances, ctx.distances.ptr, (size_t)a.n_jobs * sizeof(double),
                           hipMemcpyDeviceToHost, ctx.stream));
    DTW_HIP(hipMemcpyAsync(positions, ctx.positions.ptr, (size_t)a.n_jobs * 2 * sizeof(int32_t),
                           hipMemcpyDeviceToHost, ctx.stream));
    DTW_HIP(hipMemcpyAsync(slopes, ctx.slopes.ptr, (size_t)a.n_jobs * sizeof(double),
                           hipMemcpyDeviceToHost, ctx.stream));
    if (a.n_groups)
        DTW_HIP(hipMemcpyAsync(hits, ctx.hits.ptr, (size_t)a.n_groups * sizeof(int32_t),
                               hipMemcpyDeviceToHost, ctx.stream));
    DTW_HIP(hipStreamSynchronize(ctx.stream));
    return finish_timing(ctx);
}

int bad_argument(const char* text) {
    g_error = text;
    return DTW_ERR_ARGUMENT;
}

// offsets[0 .. n]: not negative, ascending (equal neighbours allowed when `may_be_empty`), every
// stretch at most 2^30 long
bool offsets_fine(const int64_t* offsets, int64_t n, bool may_be_empty) {
    if (offsets[0] < 0) return false;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t length = offsets[k + 1] - offsets[k];
        if (length < (may_be_empty ? 0 : 1) || length > (1 << 30)) return false;
    }
    return true;
}

}  // namespace

extern "C" {

const char* dtw_version(void) { return "deepbinner_dtw 1 (gfx950)"; }

const char* dtw_status_string(int status) {
    switch (status) {
        case DTW_OK: return "ok";
        case DTW_ERR_ARGUMENT: return "invalid argument";
        case DTW_ERR_NO_DEVICE: return "no gfx950 device";
        case DTW_ERR_HIP: return "HIP error";
        default: return "unknown status";
    }
}

const char* dtw_last_error(void) { return g_error.c_str(); }

int dtw_semi_global_batch(const double* refs, const int64_t* ref_offsets, const double* queries,
                          const int64_t* query_offsets, int64_t n_pairs, double* distances,
                          int32_t* positions, int32_t* path_lengths, int32_t* alignment) {
    if (n_pairs < 0 || (n_pairs > 0 && (!refs || !ref_offsets || !queries || !query_offsets ||
                                        !distances || !positions || !path_lengths))) {
        g_error = "null pointer or negative pair count";
        return DTW_ERR_ARGUMENT;
    }
    if (n_pairs == 0) return DTW_OK;
    if (ref_offsets[0] < 0 || query_offsets[0] < 0) {
        g_error = "negative offset";
        return DTW_ERR_ARGUMENT;
    }
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t r = ref_offsets[p + 1] - ref_offsets[p];
        const int64_t q = query_offsets[p + 1] - query_offsets[p];
        if (r < 1 || q < 1 || r > (1 << 30) || q > (1 << 30)) {
            g_error = "every pair needs 1 .. 2^30 samples of reference and of query";
            return DTW_ERR_ARGUMENT;
        }
    }
    std::lock_guard<std::mutex> guard(g_ctx.lock);
    const int st = prepare(g_ctx);
    if (st != DTW_OK) return st;
    return run_batch(g_ctx, refs, ref_offsets, queries, query_offsets, n_pairs, distances,
                     positions, path_lengths, alignment);
}

double semi_global_dtw(const double* ref, const double* query, int ref_len, int query_len,
                       int* alignment, int* positions, int* path_length) {
    if (path_length) path_length[0] = 0;
    if (!positions || !path_length) return std::nan("");
    const int64_t ref_offsets[2] = {0, ref_len}, query_offsets[2] = {0, query_len};
    double distance = 0.0;
    int32_t n = 0;
    const int st = dtw_semi_global_batch(ref, ref_offsets, query, query_offsets, 1, &distance,
                                         positions, &n, alignment);
    if (st != DTW_OK) return std::nan("");
    path_length[0] = n;
    return distance;
}

int dtw_rescaled_batch(const double* refs, const int64_t* ref_offsets, const double* queries,
                       const int64_t* query_offsets, int64_t n_pairs, double* distances,
                       int32_t* positions, double* slopes, double* rescaled,
                       int32_t* path_lengths, int32_t* alignment) {
    if (n_pairs < 0 || (n_pairs > 0 && (!refs || !ref_offsets || !queries || !query_offsets ||
                                        !distances || !positions || !slopes)))
        return bad_argument("null pointer or negative pair count");
    if (alignment && !path_lengths)
        return bad_argument("an alignment is of no use without its path lengths");
    if (n_pairs == 0) return DTW_OK;
    if (n_pairs > INT32_MAX) return bad_argument("more than 2^31 - 1 pairs");
    if (!offsets_fine(ref_offsets, n_pairs, false) || !offsets_fine(query_offsets, n_pairs, false))
        return bad_argument("offsets ascending from 0 or more, please, and every pair with "
                            "1 .. 2^30 samples of reference and of query");
    std::lock_guard<std::mutex> guard(g_ctx.lock);
    const int st = prepare(g_ctx);
    if (st != DTW_OK) return st;
    return run_rescaled(g_ctx, refs, ref_offsets, queries, query_offsets, n_pairs, distances,
                        positions, slopes, rescaled, path_lengths, alignment);
}

int dtw_locate_batch(const int16_t* samples, const int64_t* region_offsets,
                     const double* mean_std, int64_t n_reads, const double* queries,
                     const int64_t* query_offsets, int64_t n_queries, const int64_t* jobs,
                     int64_t n_jobs, const int64_t* group_offsets, int64_t n_groups,
                     double threshold, double* distances, int32_t* positions, double* slopes,
                     int32_t* hits) {
    if (n_reads < 0 || n_queries < 0 || n_jobs < 0 || n_groups < 0)
        return bad_argument("negative count");
    if (!group_offsets || (n_groups > 0 && !hits)) return bad_argument("null pointer");
    if (group_offsets[0] != 0 || group_offsets[n_groups] != n_jobs)
        return bad_argument("the groups cover the jobs: group_offsets runs from 0 to n_jobs");
    for (int64_t g = 0; g < n_groups; ++g)
        if (group_offsets[g + 1] < group_offsets[g])
            return bad_argument("group offsets not ascending");
    if (n_jobs == 0) {
        for (int64_t g = 0; g < n_groups; ++g) hits[g] = -1;
        return DTW_OK;
    }
    if (!samples || !region_offsets || !mean_std || !queries || !query_offsets || !jobs ||
        !distances || !positions || !slopes)
        return bad_argument("null pointer");
    if (n_jobs > INT32_MAX || n_reads > INT32_MAX)
        return bad_argument("more than 2^31 - 1 jobs or reads");
    if (n_reads < 1 || n_queries < 1) return bad_argument("jobs without reads or without queries");
    if (!offsets_fine(region_offsets, n_reads, true))
        return bad_argument("region offsets ascending from 0 or more, please, and no region "
                            "longer than 2^30 samples");
    if (!offsets_fine(query_offsets, n_queries, false))
        return bad_argument("query offsets ascending from 0 or more, please, and every query "
                            "with 1 .. 2^30 samples");
    for (int64_t r = 0; r < n_reads; ++r) {
        const double mean = mean_std[2 * r], sd = mean_std[2 * r + 1];
        if (!(std::fabs(mean) <= DBL_MAX) || !(sd >= 0.0 && sd <= DBL_MAX))
            return bad_argument("a read's mean is not finite, or its std is not finite or "
                                "negative");
    }
    if (!(threshold == threshold)) return bad_argument("the threshold is not a number");
    for (int64_t k = 0; k < n_jobs; ++k) {
        const int64_t read = jobs[4 * k], from = jobs[4 * k + 1], to = jobs[4 * k + 2];
        const int64_t query = jobs[4 * k + 3];
        if (read < 0 || read >= n_reads) return bad_argument("a job's read is out of range");
        if (query < 0 || query >= n_queries) return bad_argument("a job's query is out of range");
        if (from < 0 || to < from || to > region_offsets[read + 1] - region_offsets[read])
            return bad_argument("a job's window is not inside its read's region");
    }
    std::lock_guard<std::mutex> guard(g_ctx.lock);
    const int st = prepare(g_ctx);
    if (st != DTW_OK) return st;
    const LocateArguments arguments{samples, region_offsets, mean_std, n_reads, queries,
                                    query_offsets, n_queries, jobs, n_jobs, group_offsets,
                                    n_groups, threshold};
    return run_locate(g_ctx, arguments, distances, positions, slopes, hits);
}

int dtw_last_kernel_time(double* milliseconds, int64_t* cells) {
    std::lock_guard<std::mutex> guard(g_ctx.lock);
    if (milliseconds) *milliseconds = g_ctx.last_ms;
    if (cells) *cells = g_ctx.last_cells;
    return DTW_OK;
}

}  // extern "C"
