// dbh_zstd.hip - the zstd stage of ONT's VBZ filter ON THE GPU: streams of mode
// DBH_INFLATE_VBZ_ZSTD of dbh_inflate_dev (C ABI: the "compressed input" section of
// include/deepbinner_hip.h) - u32 LE original_size, then the zstd frame as the filter stored it -
// and of mode DBH_INFLATE_SVB16_ZSTD, the same for a row of a POD5 signal table.
// The decoder is dbh_zstd_core.h (what is decoded, what is refused, the schedule); this file is
// the wave that runs it and the host entry that runs the same code with loops for lanes.
//
// ONE WAVEFRONT PER FRAME, one frame per workgroup: the Huffman table and the three FSE tables
// (dbz::Ctx, 11.8 KB) in LDS, thirteen frames per CU.  The frame's content - the streamvbyte
// bytes - goes to the stream's own slots of the workspace (four bytes per byte of output, which
// the zlib kernels would fill with tokens: 4 * out_offset onwards, 4 * out_bytes of them), where
// dbh_vbz.hip's kernel, launched behind this one, reads it.  A frame whose content is larger than
// those slots is refused for space: none is whose out_bytes covers its original_size (n samples
// are at most 4.25 n + 1 streamvbyte bytes, the slots 8 n), a stream cut below 0.54 of its size
// may be.  No atomics, nothing shared between frames.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <stddef.h>
#include <stdint.h>

#include "dbh_zstd_core.h"

extern "C" {
/* the GPU's zstd decoder run on the host: same core, lanes as a loop (tests, tools) */
__attribute__((visibility("default"))) int dbh_zstd_decode_host(
    const uint8_t* frame, size_t frame_bytes, uint8_t* out, size_t out_capacity, size_t* produced,
    int32_t* status) {
    if (!frame || (!out && out_capacity) || !produced || !status) return 1;   // DBH_ERR_INVALID_ARGUMENT
    *status = dbz::decode_host(frame, frame_bytes, out, out_capacity, produced);
    if (*status != dbz::kOk) *produced = 0;
    return 0;
}
}

#if defined(__HIPCC__)
#include "../../include/deepbinner_hip.h"
#include "dbh_wave.h"

namespace dbh_zstd_detail {

struct WaveExec {
    int lane;
    __device__ __forceinline__ bool first() const { return lane == 0; }
    // what this wave's lanes stored, to LDS or to memory, is there for all of them (one wave:
    // its operations are issued in order; the waits and the fence are all it needs)
    __device__ __forceinline__ void settle() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    __device__ __forceinline__ void fill_tree(dbz::Ctx& c) const { dbz::fill_tree(c, lane, dbz::kLanes); }
    // forward, 1 KiB per step where there is that much; dst may lie below src and overlap it (a
    // step's loads are all done before its stores, and no step reads what one before it wrote)
    __device__ __forceinline__ void copy(uint8_t* dst, const uint8_t* src, size_t n) const {
        size_t k0 = 0;
        for (; k0 + 1024 <= n; k0 += 1024) {
            uint4 v;
            __builtin_memcpy(&v, src + k0 + 16 * lane, 16);
            __builtin_memcpy(dst + k0 + 16 * lane, &v, 16);
        }
        for (size_t k = k0 + lane; k < n; k += 64) {
            const uint8_t b = src[k];
            dst[k] = b;
        }
    }
    __device__ __forceinline__ void fill(uint8_t* dst, uint32_t b, size_t n) const {
        for (size_t k = lane; k < n; k += 64) dst[k] = (uint8_t)b;
    }
    // a match that overlaps its own output repeats the `offset` bytes before it: every byte is
    // read from those, which were there before the match began
    __device__ __forceinline__ void match(uint8_t* dst, size_t offset, size_t n) const {
        const uint8_t* src = dst - offset;
        if (offset >= n) {
            for (size_t k = lane; k < n; k += 64) {
                const uint8_t b = src[k];
                dst[k] = b;
            }
        } else {
            // (k mod offset kept up by additions: two divisions per match, none per byte)
            const uint32_t o = (uint32_t)offset, step = 64u % o;
            uint32_t at = (uint32_t)lane % o;
            for (uint32_t k = lane; k < (uint32_t)n; k += 64) {
                const uint8_t b = src[at];
                dst[k] = b;
                at += step;
                at = at >= o ? at - o : at;
            }
        }
    }
    // The block's 1 or 4 Huffman streams by 64 or 16 lanes each (dbh_zstd_core.h, "the schedule")
    __device__ __forceinline__ int literals(dbz::Ctx& c, const uint8_t* f, uint8_t* dst) const {
        using namespace dbz;
        const int four = c.lit_streams == 4;
        const int per = four ? 16 : 64;
        const int j = four ? lane >> 4 : 0, k = lane & (per - 1);
        uint32_t off = c.lit_off;
        for (int i = 0; i < j; ++i) off += c.stream_bytes[i];
        const uint8_t* src = f + off;
        const int32_t bits = back_start(src, c.stream_bytes[j]);
        if (__ballot(bits < 0) != 0ull) return kBadBitstream;
        const uint16_t* tab = c.huf;
        const int log = c.huf_log;
        int32_t start = piece_start(bits, k, per);
        const int32_t stop = piece_start(bits, k + 1, per);
        Piece r = huf_piece(tab, log, src, start, stop, nullptr);
        for (;;) {
            const int32_t prev_end = dbh_wave::from_lane_before(r.end);
            const int32_t want = k == 0 ? start : prev_end;
            const bool moved = want != start;
            if (__ballot(moved) == 0ull) break;
            if (moved) {
                start = want;
                r = huf_piece(tab, log, src, start, stop, nullptr);
            }
        }
        const uint32_t incl = dbh_wave::wave_scan_inclusive((uint32_t)r.count);
        const uint32_t base = (uint32_t)__shfl((int)(incl - (uint32_t)r.count), j * per);
        const uint32_t sum = (uint32_t)__shfl((int)incl, j * per + per - 1) - base;
        if (__ballot(r.bad || sum != stream_symbols(c, j)) != 0ull) return kBadBitstream;
        const uint32_t seg = (c.lit_size + 3) / 4;
        huf_piece(tab, log, src, start, stop, dst + (size_t)j * seg + (incl - (uint32_t)r.count - base));
        return kOk;
    }
};

__global__ __launch_bounds__(64) void zstd_decode_kernel(
    const uint8_t* __restrict__ comp, int64_t comp_total,
    const dbh_inflate_stream* __restrict__ streams, int n_streams, int64_t total_out,
    uint8_t* work, int32_t* __restrict__ status_out, char* produced0, int64_t produced_stride) {
    __shared__ __attribute__((aligned(16))) dbz::Ctx ctx;
    const int i = blockIdx.x;
    if (i >= n_streams) return;
    const dbh_inflate_stream s = streams[i];
    if (s.mode != DBH_INFLATE_VBZ_ZSTD && s.mode != DBH_INFLATE_SVB16_ZSTD) return;
    const int lane = threadIdx.x;
    int32_t st = 1;                                        // (refused, as dbh_vbz.hip's kRefused)
    size_t produced = 0;
    const bool region_ok = s.out_offset >= 0 && s.out_bytes >= 0 && s.out_offset <= total_out - s.out_bytes;
    const bool comp_ok = s.comp_offset >= 0 && s.comp_bytes >= 4 && s.comp_offset <= comp_total - s.comp_bytes;
    if (region_ok && comp_ok) {
        WaveExec x{lane};
        st = dbz::decode_frame(x, ctx, comp + s.comp_offset + 4, (size_t)(s.comp_bytes - 4),
                               work + 4 * s.out_offset, (size_t)(4 * s.out_bytes), &produced);
        x.settle();
    }
    if (lane == 0) {
        status_out[i] = st;
        *reinterpret_cast<int64_t*>(produced0 + (int64_t)i * produced_stride) = st == 0 ? (int64_t)produced : 0;
    }
}

}  // namespace dbh_zstd_detail

// (dbh_inflate.hip's dbh_inflate_dev launches it in front of dbh_vbz.hip's kernel; not part of
// the C ABI.)  produced0 + i * produced_stride: an int64 per stream for the frame's content size.
__attribute__((visibility("hidden"))) hipError_t dbh_zstd_launch(
    const uint8_t* comp_dev, int64_t comp_bytes, const dbh_inflate_stream* streams_dev,
    int n_streams, int64_t total_out_bytes, uint8_t* work_dev, int32_t* status_dev,
    char* produced0, int64_t produced_stride, hipStream_t stream) {
    hipLaunchKernelGGL(dbh_zstd_detail::zstd_decode_kernel, dim3((unsigned)n_streams), dim3(64), 0,
                       stream, comp_dev, comp_bytes, streams_dev, n_streams, total_out_bytes,
                       work_dev, status_dev, produced0, produced_stride);
    return hipGetLastError();
}
#endif
