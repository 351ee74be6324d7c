// dbh_host_layout.h — the host-side arithmetic of libdeepbinner_hip.so that touches no HIP call:
// regions of a buffer (align256, Carve), grid sizes, and the host units' (dbh_api*.hip) scan steps,
// staging layouts, inflate record order, staged copy and the pure checks of their arguments (do the
// offsets run forwards, a live chunk's flags).  No HIP include: oracle/api_host_test.cpp compiles it
// with g++.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/deepbinner_hip.h"

namespace dbh_host {
namespace {      // (internal linkage: nothing here is a symbol of the library)

// scan steps of a model (classify.py:330-331: windows every input_size / 2 samples), 0 when
// scan_size is not a positive multiple of that (check_input_size, classify.py:396-407)
inline int model_steps(int input_size, int scan_size) {
    const int half = input_size / 2;
    const int steps = scan_size / half;
    return (steps > 0 && steps * half == scan_size) ? steps : 0;
}

inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// workgroups of `threads` that cover n elements
inline unsigned blocks_for(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// One buffer cut into regions by ONE sequence of take() calls that runs twice: over a null base it
// sizes (every pointer null, `used` the bytes to allocate), over the buffer it carves, so the two
// cannot disagree.  Every region is a multiple of 256 bytes.  A new layout is laid out with this.
struct Carve {
    char* base;
    size_t used = 0;
    explicit Carve(void* p) : base((char*)p) {}
    template <typename T>
    T* take(size_t count) {
        T* p = base ? (T*)(base + used) : nullptr;
        used += align256(count * sizeof(T));
        return p;
    }
};

// What comes back per group of the host-buffer pipeline (host_groups) to classify_host, packed: each
// present model's probabilities, each present model's calls, the combined calls when both are there.
struct GroupOut {
    size_t probs[2], calls[2], final_calls, total;
    GroupOut(int64_t n_reads, int n_classes, bool has_start, bool has_end) {
        const size_t n = (size_t)n_reads, row = (size_t)n_classes * sizeof(float);
        probs[0] = 0;
        probs[1] = has_start ? n * row : 0;
        calls[0] = probs[1] + (has_end ? n * row : 0);
        calls[1] = calls[0] + (has_start ? n * sizeof(int32_t) : 0);
        final_calls = calls[1] + (has_end ? n * sizeof(int32_t) : 0);
        total = final_calls + (has_start && has_end ? n * sizeof(int32_t) : 0);
    }
};

// ... and to sweep_host: each present model's best, then its margin, n_reads x steps of each, carved
// from `base` (null: sizes only)
struct SweepOut {
    int32_t* best[2] = {nullptr, nullptr};
    double* margin[2] = {nullptr, nullptr};
    size_t total = 0;
    SweepOut(void* base, int64_t n_reads, int steps, bool has_start, bool has_end) {
        Carve carve(base);
        const bool has[2] = {has_start, has_end};
        for (int j = 0; j < 2; ++j) {
            if (!has[j]) continue;
            best[j] = carve.take<int32_t>((size_t)n_reads * steps);
            margin[j] = carve.take<double>((size_t)n_reads * steps);
        }
        total = carve.used;
    }
};

// The small buffer of dbh_classify_pair_deflated, the same on the host and on the device, every
// region a multiple of 256 bytes: [records | offsets] go in, [status | final calls | start calls |
// end calls] come out.
struct DeflatedSmall {
    size_t records = 0, offsets, status, final_calls, side_calls[2], in_bytes, out_bytes, total;
    DeflatedSmall(int64_t n_streams, int64_t n_reads) {
        const size_t calls_bytes = align256((size_t)n_reads * sizeof(int32_t));
        offsets = align256((size_t)n_streams * sizeof(dbh_inflate_stream));
        in_bytes = status = offsets + align256((size_t)(n_reads + 1) * sizeof(int64_t));
        final_calls = status + align256((size_t)n_streams * sizeof(int32_t));
        side_calls[0] = final_calls + calls_bytes;
        side_calls[1] = side_calls[0] + calls_bytes;
        total = side_calls[1] + calls_bytes;
        out_bytes = total - in_bytes;
    }
};

// The order the inflate records go over in: longest deflate stream first (a lane of the decoder
// takes streams off a counter in this order: what is long starts early, what is short fills the
// gaps), streams that need no decoding last, ties by index.  (A shuffled deflate stream is a
// deflate stream: DBH_INFLATE_ZLIB_SHUFFLE.)
inline void record_order(const dbh_inflate_stream* streams, int64_t n_streams,
                         std::vector<int32_t>& order) {
    order.resize((size_t)n_streams);
    for (int64_t i = 0; i < n_streams; ++i) order[(size_t)i] = (int32_t)i;
    auto key = [&](int32_t i) {
        const dbh_inflate_stream& s = streams[i];
        return s.mode == DBH_INFLATE_ZLIB || s.mode == DBH_INFLATE_ZLIB_SHUFFLE ? s.comp_bytes : (int64_t)-1;
    };
    std::sort(order.begin(), order.end(),
              [&](int32_t a, int32_t b) { return key(a) != key(b) ? key(a) > key(b) : a < b; });
}

// rel[0..n]: offsets from 0.  All n reads equally long: that length (then the forward kernel need
// not wait for the offsets), otherwise 0.
inline int64_t uniform_length(const int64_t* rel, int64_t n) {
    int64_t uniform = rel[1];
    for (int64_t i = 1; i <= n && uniform > 0; ++i)
        if (rel[i] != i * uniform) uniform = 0;
    return uniform;
}

// offsets[0 .. n_reads] of n_reads reads, wherever offsets[0] lies: does no read end before it
// starts?  *total: the samples from the first read's start to the last read's end (no read: 0, and
// the table is not looked at).
inline bool offsets_run_forwards(const int64_t* offsets, int64_t n_reads, int64_t* total = nullptr) {
    if (total) *total = n_reads > 0 ? offsets[n_reads] - offsets[0] : 0;
    for (int64_t i = 0; i < n_reads; ++i)
        if (offsets[i + 1] < offsets[i]) return false;
    return true;
}

// the flags of a live session's chunk: DBH_LIVE_BEGIN, DBH_LIVE_END, both or neither
inline bool live_chunk_flags_ok(uint32_t flags) {
    return (flags & ~(uint32_t)(DBH_LIVE_BEGIN | DBH_LIVE_END)) == 0;
}

// Pageable memory -> a pinned staging slot.  One thread moves ~10 GB/s; PCIe takes 50+.  Large
// copies are cut up between the calling thread (piece 0) and a few helpers: pieces of `share`
// bytes, a multiple of 4096, the last one shorter or empty.
struct CopySplit { int helpers; size_t share; };
inline CopySplit copy_split(size_t bytes) {
    constexpr size_t kPiece = 8u << 20;
    const int helpers = bytes >= 4 * kPiece ? 3 : (bytes >= 2 * kPiece ? 1 : 0);
    return {helpers, helpers ? ((bytes / (size_t)(helpers + 1)) + 4095) & ~(size_t)4095 : bytes};
}

inline void staged_copy(void* dst, const void* src, size_t bytes) {
    const CopySplit split = copy_split(bytes);
    std::vector<std::thread> team;
    for (int t = 1; t <= split.helpers; ++t) {
        const size_t lo = std::min(bytes, split.share * (size_t)t), hi = std::min(bytes, lo + split.share);
        if (hi > lo)
            team.emplace_back([=] { std::memcpy((char*)dst + lo, (const char*)src + lo, hi - lo); });
    }
    std::memcpy(dst, src, std::min(bytes, split.share));
    for (std::thread& t : team) t.join();
}

}  // namespace
}  // namespace dbh_host
