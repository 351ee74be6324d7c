// dbh_format.hip - int16 rows written as training-data text ON THE GPU (C ABI: the "training-data
// text, written" section of include/deepbinner_hip.h): the inverse of
// dbh_text.hip.  How wide a number is and which bytes it becomes: dbh_format_core.h; this file is
// the launches and the host entry that runs the same core with loops (dbh_text_format_host).
//
// Five launches on one stream, none of which waits for another workgroup:
//   line_bytes   one wave per line: the widths of its values, summed over the wave by shuffles, and
//                its label's; a label outside +-(10^9 - 1) marks the line
//   tile_bytes   a tile of 1,024 lines per workgroup, a line per thread: the tile's bytes
//   scan_tiles   one workgroup: the exclusive prefix of the tile totals (int64), and their sum =
//                the text's length; -1 where a line is marked
//   line_starts  the tiles again: a line starts at its tile's prefix plus the lines in front of it
//   write_lines  one wave per line, 64 values a step: each lane's value and the byte behind it go
//                where the prefix of the widths over the wave, carried from step to step, puts them.
//                Nothing is written where the length is -1 or above the capacity.
// No atomics; a line's bytes are a function of its label and row alone.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <stddef.h>
#include <stdint.h>

#include "dbh_format_core.h"

extern "C" {
__attribute__((visibility("default"))) int dbh_text_format_bound(int64_t n_lines, int input_size,
                                                                 int64_t* bytes) {
    if (!bytes || n_lines < 1 || input_size < 1) return 1;
    if (input_size > dbf::kMaxInput || n_lines > dbf::kMaxValues / input_size) return 5;
    *bytes = n_lines * dbf::line_bound(input_size);
    return 0;
}

/* the GPU's formatter run on the host: same core, lines and values as loops; needs no device */
__attribute__((visibility("default"))) int dbh_text_format_host(
    const int32_t* labels, const int16_t* samples, int64_t n_lines, int input_size, uint8_t* out,
    int64_t capacity, int64_t* n_bytes) {
    const int st = dbf::check_arguments(labels, samples, n_lines, input_size, out, capacity, n_bytes);
    if (st != 0) return st;
    int64_t need = 0;
    for (int64_t k = 0; k < n_lines; ++k) {
        if (!dbf::label_ok(labels[k])) return 1;
        need += dbf::model_line_bytes(labels[k], samples + k * input_size, input_size);
    }
    *n_bytes = need;
    if (need > capacity) return 1;                         // DBH_ERR_INVALID_ARGUMENT, nothing written
    int64_t at = 0;
    for (int64_t k = 0; k < n_lines; ++k) {
        const int16_t* row = samples + k * input_size;
        dbf::model_line(labels[k], row, input_size, out + at);
        at += dbf::model_line_bytes(labels[k], row, input_size);
    }
    return 0;
}
}

#if defined(__HIPCC__)
#include "../../include/deepbinner_hip.h"
#include "dbh_host_layout.h"
#include "dbh_owned.h"
#include "dbh_status.h"
#include "dbh_wave.h"

namespace dbh_format_detail {

constexpr int kLineThreads = 256, kLineWaves = kLineThreads / 64;
constexpr int kLineBlocks = 8192;
constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kLineThreads) void line_bytes(const int32_t* __restrict__ labels,
                                                           const int16_t* __restrict__ samples,
                                                           int64_t n_lines, int32_t input_size,
                                                           int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * kLineWaves;
    for (int64_t line = (int64_t)blockIdx.x * kLineWaves + (threadIdx.x >> 6); line < n_lines; line += waves) {
        const int16_t* row = samples + line * input_size;
        int32_t sum = 0;
        for (int32_t i = lane; i < input_size; i += 64) sum += dbf::value_width(row[i]) + 1;
        const int32_t all = dbh_wave::wave_scan_inclusive(sum);
        if (lane == 63) {
            const int32_t label = labels[line];
            counts[line] = dbf::label_ok(label) ? all + dbf::label_width(label) + 1 : dbf::kBadLabel;
        }
    }
}

// a tile of kScanThreads lines per workgroup, a line per thread: the tile's bytes, -1 where a
// count is kBadLabel
__global__ __launch_bounds__(kScanThreads) void tile_bytes(const int32_t* __restrict__ counts, int64_t n_lines,
                                                           int64_t* __restrict__ tiles) {
    __shared__ int64_t part[kScanThreads];
    __shared__ int any_bad;
    const int64_t line = (int64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const int32_t c = line < n_lines ? counts[line] : 0;
    if (threadIdx.x == 0) any_bad = 0;
    // (barriers in the scan: any_bad is 0 behind it)
    const int64_t incl = dbh_wave::block_scan_inclusive<int64_t, kScanThreads>(c < 0 ? 0 : c, part);
    if (c < 0) any_bad = 1;                                     // every writer stores the same value
    __syncthreads();
    if (threadIdx.x == kScanThreads - 1) tiles[blockIdx.x] = any_bad ? -1 : incl;
}

// one workgroup: tiles [n_tiles] becomes its own exclusive prefix; *n_bytes and starts[n_lines]
// their sum, *n_bytes -1 where a tile is marked
__global__ __launch_bounds__(kScanThreads) void scan_tiles(int64_t* __restrict__ tiles, int64_t n_tiles,
                                                           int64_t n_lines, int64_t* __restrict__ starts,
                                                           int64_t* __restrict__ n_bytes) {
    __shared__ int64_t part[kScanThreads];
    __shared__ int any_bad;
    const int t = threadIdx.x;
    const int64_t per = (n_tiles + kScanThreads - 1) / kScanThreads;
    const int64_t first = min(t * per, n_tiles), last = min(first + per, n_tiles);
    if (t == 0) any_bad = 0;
    int64_t sum = 0;
    bool bad = false;
    for (int64_t i = first; i < last; ++i) {
        const int64_t c = tiles[i];
        bad = bad || c < 0;
        sum += c < 0 ? 0 : c;
    }
    const int64_t incl = dbh_wave::block_scan_inclusive<int64_t, kScanThreads>(sum, part);
    if (bad) any_bad = 1;
    int64_t running = incl - sum;
    for (int64_t i = first; i < last; ++i) {
        const int64_t c = tiles[i];
        tiles[i] = running;
        running += c < 0 ? 0 : c;
    }
    __syncthreads();
    if (t == kScanThreads - 1) {
        starts[n_lines] = incl;
        *n_bytes = any_bad ? -1 : incl;
    }
}

// the tiles again: starts[k] = where line k begins
__global__ __launch_bounds__(kScanThreads) void line_starts(const int32_t* __restrict__ counts, int64_t n_lines,
                                                            const int64_t* __restrict__ tiles,
                                                            int64_t* __restrict__ starts) {
    __shared__ int64_t part[kScanThreads];
    const int64_t line = (int64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const int32_t c = line < n_lines ? counts[line] : 0;
    const int64_t v = c < 0 ? 0 : c;
    const int64_t incl = dbh_wave::block_scan_inclusive<int64_t, kScanThreads>(v, part);
    if (line < n_lines) starts[line] = tiles[blockIdx.x] + incl - v;
}

__global__ __launch_bounds__(kLineThreads) void write_lines(const int32_t* __restrict__ labels,
                                                            const int16_t* __restrict__ samples,
                                                            int64_t n_lines, int32_t input_size,
                                                            const int64_t* __restrict__ starts,
                                                            const int64_t* __restrict__ n_bytes,
                                                            int64_t capacity, uint8_t* __restrict__ out) {
    const int64_t total = *n_bytes;
    if (total < 0 || total > capacity) return;
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * kLineWaves;
    for (int64_t line = (int64_t)blockIdx.x * kLineWaves + (threadIdx.x >> 6); line < n_lines; line += waves) {
        const int16_t* row = samples + line * input_size;
        uint8_t* at = out + starts[line];
        const int32_t label = labels[line];
        const int label_bytes = dbf::label_width(label);
        if (lane == 0) {
            dbf::put_number(at, label, label_bytes, dbf::kLabelDigits);
            at[label_bytes] = '\t';
        }
        int32_t carried = label_bytes + 1;
        for (int32_t i0 = 0; i0 < input_size; i0 += 64) {
            const int32_t i = i0 + lane;
            const int32_t v = i < input_size ? row[i] : 0;
            const int32_t w = i < input_size ? dbf::value_width(v) + 1 : 0;
            const int32_t incl = dbh_wave::wave_scan_inclusive(w);
            if (i < input_size) {
                uint8_t* p = at + carried + incl - w;
                dbf::put_number(p, v, w - 1, dbf::kValueDigits);
                p[w - 1] = i + 1 < input_size ? ',' : '\n';
            }
            carried += __shfl(incl, 63);
        }
    }
}

// The workspace: the line lengths, the line starts (one more than lines), the tiles.  Over a null
// workspace it is sized (*bytes) and nothing is launched; over the caller's the same lines carve it.
hipError_t launch(const int32_t* labels, const int16_t* samples, int64_t n_lines, int input_size,
                  uint8_t* out, int64_t capacity, int64_t* n_bytes, void* workspace, hipStream_t stream,
                  size_t* bytes = nullptr) {
    const unsigned n_tiles = dbh_host::blocks_for(n_lines, kScanThreads);
    dbh_host::Carve c(workspace);
    int32_t* counts = c.take<int32_t>((size_t)n_lines);
    int64_t* starts = c.take<int64_t>((size_t)n_lines + 1);
    int64_t* tiles = c.take<int64_t>(n_tiles);
    if (bytes) *bytes = c.used;
    if (!workspace) return hipSuccess;
    const int64_t want = (n_lines + kLineWaves - 1) / kLineWaves;
    const unsigned grid = (unsigned)(want < kLineBlocks ? want : kLineBlocks);
    hipLaunchKernelGGL(line_bytes, dim3(grid), dim3(kLineThreads), 0, stream, labels, samples, n_lines,
                       (int32_t)input_size, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tile_bytes, dim3(n_tiles), dim3(kScanThreads), 0, stream, counts, n_lines, tiles);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scan_tiles, dim3(1), dim3(kScanThreads), 0, stream, tiles, (int64_t)n_tiles, n_lines,
                       starts, n_bytes);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(line_starts, dim3(n_tiles), dim3(kScanThreads), 0, stream, counts, n_lines, tiles, starts);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(write_lines, dim3(grid), dim3(kLineThreads), 0, stream, labels, samples, n_lines,
                       (int32_t)input_size, starts, n_bytes, capacity, out);
    return hipGetLastError();
}

inline size_t workspace_bytes(int64_t n_lines) {
    size_t bytes = 0;
    (void)launch(nullptr, nullptr, n_lines, 0, nullptr, 0, nullptr, nullptr, 0, &bytes);
    return bytes;
}

}  // namespace dbh_format_detail

using namespace dbh_format_detail;

#define DBH_FORMAT_HIP(call) DBH_HIP_AS("dbh_text_format", call)

extern "C" {

int dbh_text_format_workspace_bytes(int64_t n_lines, size_t* bytes) {
    if (!bytes || n_lines < 1) return DBH_ERR_INVALID_ARGUMENT;
    if (n_lines > dbf::kMaxValues) return DBH_ERR_UNSUPPORTED;
    *bytes = workspace_bytes(n_lines);
    return DBH_OK;
}

int dbh_text_format_dev(const int32_t* labels_dev, const int16_t* samples_dev, int64_t n_lines,
                        int input_size, uint8_t* out_dev, int64_t capacity, int64_t* n_bytes_dev,
                        void* workspace_dev, dbh_stream stream) {
    const int st = dbf::check_arguments(labels_dev, samples_dev, n_lines, input_size, out_dev, capacity,
                                        n_bytes_dev);
    if (st != DBH_OK) return st;
    if (!workspace_dev) return DBH_ERR_INVALID_ARGUMENT;
    DBH_FORMAT_HIP(launch(labels_dev, samples_dev, n_lines, input_size, out_dev, capacity, n_bytes_dev,
                          workspace_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_text_format(const int32_t* labels, const int16_t* samples, int64_t n_lines, int input_size,
                    uint8_t* out, int64_t capacity, int64_t* n_bytes) {
    const int st = dbf::check_arguments(labels, samples, n_lines, input_size, out, capacity, n_bytes);
    if (st != DBH_OK) return st;
    for (int64_t k = 0; k < n_lines; ++k)
        if (!dbf::label_ok(labels[k])) return DBH_ERR_INVALID_ARGUMENT;
    // every buffer, sized before the first launch; the text's takes the capacity or the bound,
    // whichever is smaller
    const int64_t bound = n_lines * dbf::line_bound(input_size);
    const size_t text_bytes = (size_t)(capacity < bound ? capacity : bound);
    const size_t label_bytes = (size_t)n_lines * sizeof(int32_t);
    const size_t sample_bytes = (size_t)n_lines * (size_t)input_size * sizeof(int16_t);
    int32_t* labels_dev;
    int16_t* samples_dev;
    int64_t* total_dev;
    char* work;
    uint8_t* text;
    auto lay_out = [&](dbh_host::Carve& c) {
        labels_dev = c.take<int32_t>((size_t)n_lines);
        samples_dev = c.take<int16_t>((size_t)n_lines * (size_t)input_size);
        total_dev = c.take<int64_t>(1);
        work = c.take<char>(workspace_bytes(n_lines));
        text = c.take<uint8_t>(text_bytes + 256);          // (slack behind the text)
    };
    dbh_owned::DeviceBlock dev;
    DBH_FORMAT_HIP(dev.carve(lay_out));
    hipStream_t stream = 0;
    DBH_FORMAT_HIP(hipMemcpyAsync(labels_dev, labels, label_bytes, hipMemcpyHostToDevice, stream));
    DBH_FORMAT_HIP(hipMemcpyAsync(samples_dev, samples, sample_bytes, hipMemcpyHostToDevice, stream));
    DBH_FORMAT_HIP(launch(labels_dev, samples_dev, n_lines, input_size, text, (int64_t)text_bytes,
                          total_dev, work, stream));
    int64_t total = 0;
    DBH_FORMAT_HIP(hipMemcpyAsync(&total, total_dev, sizeof(total), hipMemcpyDeviceToHost, stream));
    DBH_FORMAT_HIP(hipStreamSynchronize(stream));          // the one synchronisation
    if (total < 0) return DBH_ERR_INVALID_ARGUMENT;
    *n_bytes = total;
    if (total > capacity) return DBH_ERR_INVALID_ARGUMENT; // nothing written
    DBH_FORMAT_HIP(hipMemcpy(out, text, (size_t)total, hipMemcpyDeviceToHost));
    return DBH_OK;
}

}
#endif
