// dbh_text.hip - training-data text parsed ON THE GPU (C ABI: the "training-data text" section of
// include/deepbinner_hip.h).  The grammar, the kinds and the walk over a line
// are dbh_text_core.h; this file is the wave that runs it, the three launches that find the lines,
// and the host entry that runs the same core with loops for lanes (dbh_text_parse_host).
//
// A block is a run of whole lines, its last byte a LF.  Four launches on one stream, none of which
// waits for another workgroup:
//   count_lf     a tile of 4,096 bytes per workgroup, 16 bytes per thread: the tile's LFs
//   scan_tiles   one workgroup: the exclusive prefix of the tile totals, and their sum = n_lines
//   line_starts  the tiles again: the byte behind the k-th LF is where line k + 1 starts (int64)
//   parse_lines  one wave per line (dbh_text_core.h, "the schedule"); the row goes straight to
//                memory - a step's values are neighbours in the row, so its stores fall into a few
//                lines of the cache that the L2 merges, and no LDS is held: 32 KB a wave for the
//                longest row would leave five waves to a CU where the loads want many
// The first line that is not kOk: an integer atomicMin over line indices (a minimum has no order
// to depend on).  Nothing here knows the launch geometry: a line's result is a function of its
// bytes and input_size alone, wherever the block was cut and however it is aligned.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <stddef.h>
#include <stdint.h>

#include "dbh_text_core.h"

namespace dbh_text_detail {

// the argument errors of both entries, before any work: dbh_status values
inline int check_arguments(const uint8_t* block, int64_t n_bytes, int input_size, int64_t max_lines,
                           const void* samples, const void* labels, const void* kinds,
                           const void* n_lines, const void* first_bad_line) {
    if (!block || !samples || !labels || !kinds || !n_lines || !first_bad_line) return 1;
    if (input_size < 1 || n_bytes < 0 || max_lines < 0) return 1;
    if (input_size > dbt::kMaxInput || n_bytes > dbt::kMaxBlock) return 5;
    if (n_bytes == 0 || block[n_bytes - 1] != '\n') return 1;
    return 0;
}

}  // namespace dbh_text_detail

extern "C" {
/* the GPU's parser run on the host: same core, steps and lanes as loops; needs no device */
__attribute__((visibility("default"))) int dbh_text_parse_host(
    const uint8_t* block, int64_t n_bytes, int input_size, int64_t max_lines, int16_t* samples,
    int32_t* labels, uint8_t* kinds, int64_t* n_lines, int64_t* first_bad_line) {
    const int st = dbh_text_detail::check_arguments(block, n_bytes, input_size, max_lines, samples,
                                                    labels, kinds, n_lines, first_bad_line);
    if (st != 0) return st;
    int64_t lines = 0;
    for (int64_t p = 0; p < n_bytes; ++p) lines += block[p] == '\n';
    *n_lines = lines;
    if (lines > max_lines) return 1;                       // DBH_ERR_INVALID_ARGUMENT, nothing written
    int64_t first_bad = -1, start = 0, line = 0;
    for (int64_t p = 0; p < n_bytes; ++p) {
        if (block[p] != '\n') continue;
        const int kind = dbt::model_line(block, n_bytes, start, p, input_size,
                                         samples + line * input_size, labels + line);
        kinds[line] = (uint8_t)kind;
        if (kind != dbt::kOk && first_bad < 0) first_bad = line;
        start = p + 1;
        line += 1;
    }
    *first_bad_line = first_bad;
    return 0;
}
}

#if defined(__HIPCC__)
#include <chrono>

#include "../../include/deepbinner_hip.h"
#include "dbh_host_layout.h"
#include "dbh_owned.h"
#include "dbh_status.h"
#include "dbh_wave.h"

namespace dbh_text_detail {

constexpr int kTile = 4096, kTileThreads = kTile / dbt::kPiece, kTileWaves = kTileThreads / 64;   // 256 threads
constexpr int kScanThreads = 1024;
constexpr int kParseThreads = 256, kParseWaves = kParseThreads / 64;
constexpr int kParseBlocks = 8192;
constexpr int32_t kNoBadLine = 0x7f7f7f7f;              // what hipMemsetAsync(.., 0x7f, 4) leaves

// the 16 bytes at `at` (a multiple of 16 below n_bytes): bit j set where byte j is a LF of the block
__device__ __forceinline__ uint32_t lf_mask(const uint8_t* __restrict__ block, int64_t at, int64_t n_bytes) {
    const uint4 v = *reinterpret_cast<const uint4*>(block + at);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const bool lf = ((w[j >> 2] >> ((j & 3) * 8)) & 0xffu) == '\n' && at + j < n_bytes;
        mask |= (lf ? 1u : 0u) << j;
    }
    return mask;
}

__global__ __launch_bounds__(kTileThreads) void count_lf(const uint8_t* __restrict__ block,
                                                          int64_t n_bytes, int32_t* __restrict__ tile_count) {
    const int64_t at = (int64_t)blockIdx.x * kTile + threadIdx.x * dbt::kPiece;
    const int count = at < n_bytes ? __popc(lf_mask(block, at, n_bytes)) : 0;
    __shared__ int wave_total[kTileWaves];
    int total;
    (void)dbh_wave::block_prefix<kTileWaves>(count, wave_total, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// one workgroup: tile_count [n_tiles] becomes its own exclusive prefix; *n_lines their sum
__global__ __launch_bounds__(kScanThreads) void scan_tiles(int32_t* __restrict__ tile_count, int n_tiles,
                                                           int32_t* __restrict__ n_lines) {
    __shared__ int part[kScanThreads];
    const int t = threadIdx.x;
    const int per = (n_tiles + kScanThreads - 1) / kScanThreads;
    const int first = t * per, last = min(first + per, n_tiles);
    int sum = 0;
    for (int i = first; i < last; ++i) sum += tile_count[i];
    const int incl = dbh_wave::block_scan_inclusive<int, kScanThreads>(sum, part);
    int running = incl - sum;
    for (int i = first; i < last; ++i) {
        const int c = tile_count[i];
        tile_count[i] = running;
        running += c;
    }
    if (t == kScanThreads - 1) *n_lines = incl;
}

// starts [max_lines + 1]: starts[k] = the first byte of line k, starts[n_lines] = n_bytes
__global__ __launch_bounds__(kTileThreads) void line_starts(const uint8_t* __restrict__ block,
                                                             int64_t n_bytes,
                                                             const int32_t* __restrict__ tile_before,
                                                             int64_t max_lines, int64_t* __restrict__ starts) {
    const int64_t at = (int64_t)blockIdx.x * kTile + threadIdx.x * dbt::kPiece;
    const uint32_t mask = at < n_bytes ? lf_mask(block, at, n_bytes) : 0u;
    __shared__ int wave_total[kTileWaves];
    int total;
    const int before = dbh_wave::block_prefix<kTileWaves>(__popc(mask), wave_total, &total);
    int64_t line = (int64_t)tile_before[blockIdx.x] + before;      // the line this piece begins in
    if (blockIdx.x == 0 && threadIdx.x == 0) starts[0] = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if ((mask >> j) & 1u) {
            line += 1;
            if (line <= max_lines) starts[line] = at + j + 1;
        }
    }
}

__global__ __launch_bounds__(kParseThreads) void parse_lines(
    const uint8_t* __restrict__ block, const int64_t* __restrict__ starts,
    const int32_t* __restrict__ n_lines_dev, int64_t max_lines, int32_t input_size,
    int16_t* __restrict__ samples, int32_t* __restrict__ labels, uint8_t* __restrict__ kinds,
    int32_t* first_bad) {
    const int lane = threadIdx.x & 63;
    const int64_t n_lines = min((int64_t)*n_lines_dev, max_lines);
    const int64_t waves = (int64_t)gridDim.x * kParseWaves;
    for (int64_t line = (int64_t)blockIdx.x * kParseWaves + (threadIdx.x >> 6); line < n_lines; line += waves) {
        const int64_t start = starts[line], lf = starts[line + 1] - 1;
        const dbt::Line l = dbt::line_head(block, start, lf);
        int16_t* row = samples + line * input_size;
        int flags = 0;
        int32_t carried = 0;
        if (l.head_ok) {
            const int32_t steps = (l.end + dbt::kStep - 1) / dbt::kStep;
            for (int32_t step = 0; step < steps; ++step) {
                const int32_t rel0 = step * dbt::kStep + lane * dbt::kPiece;
                uint4 cur = make_uint4(0u, 0u, 0u, 0u);
                if (rel0 < l.end) cur = *reinterpret_cast<const uint4*>(block + l.base + rel0);
                // the piece behind this one: the next lane's, or for lane 63 the next step's first
                uint4 next;
                next.x = (uint32_t)__shfl_down((int)cur.x, 1);
                next.y = (uint32_t)__shfl_down((int)cur.y, 1);
                next.z = (uint32_t)__shfl_down((int)cur.z, 1);
                next.w = (uint32_t)__shfl_down((int)cur.w, 1);
                if (lane == 63) {
                    next = make_uint4(0u, 0u, 0u, 0u);
                    if (rel0 + dbt::kPiece < l.end)
                        next = *reinterpret_cast<const uint4*>(block + l.base + rel0 + dbt::kPiece);
                }
                const uint32_t w[8] = {cur.x, cur.y, cur.z, cur.w, next.x, next.y, next.z, next.w};
                const int commas = dbt::piece_commas(w, rel0, l.tab, l.end);
                const int incl = dbh_wave::wave_scan_inclusive_shfl(commas);
                flags |= dbt::piece_values(w, rel0, l.tab, l.end, carried + incl - commas, input_size, row);
                carried += __shfl(incl, 63);
            }
        }
        const int all = (__ballot(flags & dbt::kFlagForm) != 0ull ? dbt::kFlagForm : 0) |
                        (__ballot(flags & dbt::kFlagRange) != 0ull ? dbt::kFlagRange : 0);
        const int kind = dbt::line_kind(l.head_ok, all, (int64_t)carried + 1, input_size);
        if (lane == 0) {
            kinds[line] = (uint8_t)kind;
            labels[line] = l.label;
            if (kind != dbt::kOk) atomicMin(first_bad, (int32_t)line);
        }
    }
}

thread_local double g_stage_ms[3] = {0.0, 0.0, 0.0};

}  // namespace dbh_text_detail

using namespace dbh_text_detail;

#define DBH_TEXT_HIP(call) DBH_HIP_AS("dbh_text_parse", call)

extern "C" {

int dbh_text_parse(const uint8_t* block, int64_t n_bytes, int input_size, int64_t max_lines,
                   int16_t* samples, int32_t* labels, uint8_t* kinds, int64_t* n_lines,
                   int64_t* first_bad_line) {
    const int st = check_arguments(block, n_bytes, input_size, max_lines, samples, labels, kinds,
                                   n_lines, first_bad_line);
    if (st != DBH_OK) return st;
    if (max_lines > n_bytes) max_lines = n_bytes;          // a line is a byte at least
    // every buffer, sized before the first launch
    const int n_tiles = (int)((n_bytes + kTile - 1) / kTile);
    const size_t text_bytes = ((size_t)n_bytes + 15) & ~(size_t)15;
    const size_t row_bytes = (size_t)input_size * sizeof(int16_t);
    uint8_t *text, *kinds_dev;
    int32_t *tiles, *counts, *labels_dev;
    int64_t* starts;
    int16_t* samples_dev;
    auto lay_out = [&](dbh_host::Carve& c) {
        text = c.take<uint8_t>(text_bytes);
        tiles = c.take<int32_t>((size_t)n_tiles);
        starts = c.take<int64_t>((size_t)max_lines + 1);
        counts = c.take<int32_t>(2);                       // n_lines, first_bad
        labels_dev = c.take<int32_t>((size_t)max_lines);
        kinds_dev = c.take<uint8_t>((size_t)max_lines);
        samples_dev = c.take<int16_t>((size_t)max_lines * (size_t)input_size);
        (void)c.take<char>(256);                           // (slack behind the rows)
    };
    dbh_owned::DeviceBlock dev;
    dbh_owned::Event ev[3];
    DBH_TEXT_HIP(dev.carve(lay_out));
    for (auto& e : ev) DBH_TEXT_HIP(hipEventCreate(&e.h));

    hipStream_t stream = 0;
    DBH_TEXT_HIP(hipEventRecord(ev[0], stream));
    DBH_TEXT_HIP(hipMemcpyAsync(text, block, (size_t)n_bytes, hipMemcpyHostToDevice, stream));
    DBH_TEXT_HIP(hipMemsetAsync(counts, 0x7f, 2 * sizeof(int32_t), stream));
    DBH_TEXT_HIP(hipEventRecord(ev[1], stream));
    hipLaunchKernelGGL(count_lf, dim3((unsigned)n_tiles), dim3(kTileThreads), 0, stream, text, n_bytes, tiles);
    DBH_TEXT_HIP(hipGetLastError());
    hipLaunchKernelGGL(scan_tiles, dim3(1), dim3(kScanThreads), 0, stream, tiles, n_tiles, counts);
    DBH_TEXT_HIP(hipGetLastError());
    hipLaunchKernelGGL(line_starts, dim3((unsigned)n_tiles), dim3(kTileThreads), 0, stream, text, n_bytes,
                       tiles, max_lines, starts);
    DBH_TEXT_HIP(hipGetLastError());
    if (max_lines > 0) {
        const int64_t want = (max_lines + kParseWaves - 1) / kParseWaves;
        const unsigned grid = (unsigned)(want < kParseBlocks ? want : kParseBlocks);
        hipLaunchKernelGGL(parse_lines, dim3(grid), dim3(kParseThreads), 0, stream, text, starts, counts,
                           max_lines, (int32_t)input_size, samples_dev, labels_dev, kinds_dev, counts + 1);
        DBH_TEXT_HIP(hipGetLastError());
    }
    DBH_TEXT_HIP(hipEventRecord(ev[2], stream));
    int32_t found[2] = {0, 0};
    DBH_TEXT_HIP(hipMemcpyAsync(found, counts, sizeof(found), hipMemcpyDeviceToHost, stream));
    DBH_TEXT_HIP(hipStreamSynchronize(stream));            // the one synchronisation

    *n_lines = found[0];
    if (found[0] > max_lines) return DBH_ERR_INVALID_ARGUMENT;        // nothing else is written
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)found[0];
    DBH_TEXT_HIP(hipMemcpy(samples, samples_dev, n * row_bytes, hipMemcpyDeviceToHost));
    DBH_TEXT_HIP(hipMemcpy(labels, labels_dev, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    DBH_TEXT_HIP(hipMemcpy(kinds, kinds_dev, n, hipMemcpyDeviceToHost));
    *first_bad_line = found[1] == kNoBadLine ? -1 : found[1];
    float upload = 0.f, kernels = 0.f;
    DBH_TEXT_HIP(hipEventElapsedTime(&upload, ev[0], ev[1]));
    DBH_TEXT_HIP(hipEventElapsedTime(&kernels, ev[1], ev[2]));
    g_stage_ms[0] = upload;
    g_stage_ms[1] = kernels;
    g_stage_ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DBH_OK;
}

int dbh_text_stage_ms(double* upload, double* kernels, double* download) {
    if (!upload || !kernels || !download) return DBH_ERR_INVALID_ARGUMENT;
    *upload = g_stage_ms[0];
    *kernels = g_stage_ms[1];
    *download = g_stage_ms[2];
    return DBH_OK;
}

}
#endif
