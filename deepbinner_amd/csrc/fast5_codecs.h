// fast5_codecs.h - what undoes a Signal chunk's filters: deflate (libdeflate or zlib), ONT's VBZ,
// HDF5's shuffle, and the per-thread state they work in.
#ifndef DEEPBINNER_FAST5_CODECS_H
#define DEEPBINNER_FAST5_CODECS_H

#include <dlfcn.h>
#include <zlib.h>

#include <cstdlib>

#include "dbh_zstd_core.h"
#include "fast5_bytes.h"

namespace {

// a compression filter this reader does not implement (ONT's VBZ, id 32020, is the one in the
// field): reported apart from damage, so that the caller can say what is the matter
struct UnsupportedFilter : FormatError {
    using FormatError::FormatError;
};

// libdeflate, when the system has it (looked up at run time: the image ships libdeflate.so.0 but
// no header): its whole-buffer inflate is 2-3 times as fast as zlib's streaming one, and inflating
// is most of what loading a read costs.  Same input (RFC 1950 streams, which is what the HDF5
// deflate filter writes), same output; anything it does not like - including an output that turns
// out larger than the chunk size promised - goes to zlib, which also decides what counts as
// corrupt.  DEEPBINNER_FAST5_INFLATE=zlib keeps it out.
struct LibDeflate {
    using Alloc = void* (*)();
    using Free = void (*)(void*);
    using Inflate = int (*)(void*, const void*, size_t, void*, size_t, size_t*);
    Alloc alloc = nullptr;
    Free release = nullptr;
    Inflate zlib_decompress = nullptr;
    LibDeflate() {
        void* lib = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!lib) return;
        alloc = reinterpret_cast<Alloc>(dlsym(lib, "libdeflate_alloc_decompressor"));
        release = reinterpret_cast<Free>(dlsym(lib, "libdeflate_free_decompressor"));
        zlib_decompress = reinterpret_cast<Inflate>(dlsym(lib, "libdeflate_zlib_decompress"));
        if (!alloc || !release || !zlib_decompress) alloc = nullptr;
    }
    bool usable() const {
        if (!alloc) return false;
        const char* choice = std::getenv("DEEPBINNER_FAST5_INFLATE");
        return !(choice && std::strcmp(choice, "zlib") == 0);
    }
};
const LibDeflate& libdeflate() {
    static const LibDeflate lib;
    return lib;
}

// libzstd, for ONT's VBZ filter (HDF5 filter 32020): looked up at run time like libdeflate - no
// header, no build dependency.  DEEPBINNER_ZSTD_LIB names another library (tests point it at
// nothing to see VBZ refused).  Where it cannot be loaded, a VBZ Signal with a zstd stage is
// refused (F5_ERR_FILTER), as it was before this reader knew VBZ.
struct LibZstd {
    using Decompress = size_t (*)(void*, size_t, const void*, size_t);
    using ContentSize = unsigned long long (*)(const void*, size_t);
    using IsError = unsigned (*)(size_t);
    Decompress decompress = nullptr;
    ContentSize content_size = nullptr;
    IsError is_error = nullptr;
    LibZstd() {
        const char* name = std::getenv("DEEPBINNER_ZSTD_LIB");
        void* lib = dlopen(name && name[0] ? name : "libzstd.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) return;
        decompress = reinterpret_cast<Decompress>(dlsym(lib, "ZSTD_decompress"));
        content_size = reinterpret_cast<ContentSize>(dlsym(lib, "ZSTD_getFrameContentSize"));
        is_error = reinterpret_cast<IsError>(dlsym(lib, "ZSTD_isError"));
        if (!decompress || !content_size || !is_error) decompress = nullptr;
    }
    bool usable() const { return decompress != nullptr; }
};
const LibZstd& libzstd() {
    static const LibZstd lib;
    return lib;
}

// ---- VBZ (filter 32020), version 0: the layout DESIGN.md section "VBZ" pins -------------------
//   u32 LE original_size | payload (a zstd frame if cd[3] != 0, else the streamvbyte bytes)
//   streamvbyte: ceil(n/4) control bytes (2 bits per value, low bits first), then the values in
//   code + 1 little-endian bytes each; value u -> zigzag -> delta, restarting at every chunk.
// Every self-check failure is a refused read (UnsupportedFilter -> F5_ERR_FILTER), never samples.
constexpr int kVbzFilter = 32020;

// cd[0] version 0, cd[1] 2-byte integers, cd[2] delta + zigzag on; cd[3] (absent = 0) zstd level
bool vbz_accepted(const std::vector<uint32_t>& cd) {
    return cd.size() >= 3 && cd[0] == 0 && cd[1] == 2 && cd[2] == 1;
}
bool vbz_zstd(const std::vector<uint32_t>& cd) { return cd.size() >= 4 && cd[3] != 0; }

// streamvbyte bytes -> n int16 samples; false if the data the control bytes call for do not end
// exactly at the end of the bytes
bool vbz_unpack(const uint8_t* p, size_t bytes, int64_t n, int16_t* out) {
    const size_t ctrl = (size_t)((n + 3) / 4);
    if (ctrl > bytes) return false;
    const uint8_t* d = p + ctrl;
    const uint8_t* const end = p + bytes;
    uint32_t prev = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int len = ((p[i >> 2] >> ((i & 3) * 2)) & 3) + 1;
        if (end - d < len) return false;
        uint32_t u = 0;
        for (int k = 0; k < len; ++k) u |= (uint32_t)d[k] << (8 * k);
        d += len;
        prev += (u >> 1) ^ (0u - (u & 1u));
        out[i] = (int16_t)(uint16_t)prev;
    }
    return d == end;
}

// The chunk's original_size after the self-checks (even, at most `cap` bytes)
uint32_t vbz_original_size(const uint8_t* src, size_t n, size_t cap) {
    if (n < 4) throw UnsupportedFilter("VBZ chunk shorter than its header");
    const uint32_t size = (uint32_t)src[0] | (uint32_t)src[1] << 8 | (uint32_t)src[2] << 16 |
                          (uint32_t)src[3] << 24;
    if ((size & 1) || size > cap) throw UnsupportedFilter("VBZ chunk of an impossible size");
    return size;
}

// The streamvbyte bytes a zstd-compressed VBZ chunk holds (its frame's content size), checked
// against what n values can occupy (n/4 control bytes + 1..4 bytes each)
uint64_t vbz_frame_size(const uint8_t* src, size_t n, uint32_t original_size) {
    const LibZstd& z = libzstd();
    if (!z.usable()) throw UnsupportedFilter("VBZ needs libzstd");
    const unsigned long long size = z.content_size(src + 4, n - 4);
    const uint64_t values = original_size / 2, ctrl = (values + 3) / 4;
    if (size >= (unsigned long long)-2 || size < ctrl + values || size > ctrl + 4 * values)
        throw UnsupportedFilter("VBZ chunk with a bad zstd frame");
    return (uint64_t)size;
}

// The same size from the frame's header alone (dbh_zstd_core.h, the GPU decoder's own parser):
// the route on which the GPU undoes the zstd stage and libzstd is not called.  A frame that
// decoder refuses by its header (no content size, a dictionary id, a checksum) refuses the read.
uint64_t vbz_frame_size_header(const uint8_t* src, size_t n, uint32_t original_size) {
    dbz::Frame fr;
    if (n < 4 || dbz::frame_header(src + 4, n - 4, &fr) != dbz::kOk)
        throw UnsupportedFilter("VBZ chunk with a bad zstd frame");
    const uint64_t values = original_size / 2, ctrl = (values + 3) / 4;
    if (fr.content < ctrl + values || fr.content > ctrl + 4 * values)
        throw UnsupportedFilter("VBZ chunk with a bad zstd frame");
    return fr.content;
}

// zstd stage undone: `dst` (frame_size bytes) <- the chunk's streamvbyte bytes
void vbz_unzstd(const uint8_t* src, size_t n, uint8_t* dst, uint64_t frame_size) {
    const LibZstd& z = libzstd();
    if (!z.usable()) throw UnsupportedFilter("VBZ needs libzstd");
    const size_t got = z.decompress(dst, (size_t)frame_size, src + 4, n - 4);
    if (z.is_error(got) || got != frame_size) throw UnsupportedFilter("VBZ chunk: zstd failed");
}

// one VBZ chunk as stored -> its int16 bytes (original_size of them; the caller zero-extends)
void vbz_decode(const uint8_t* src, size_t n, const std::vector<uint32_t>& cd, size_t cap,
                std::vector<uint8_t>* out, std::vector<uint8_t>* tmp) {
    const uint32_t size = vbz_original_size(src, n, cap);
    const uint8_t* packed = src + 4;
    size_t packed_bytes = n - 4;
    if (vbz_zstd(cd)) {
        const uint64_t frame = vbz_frame_size(src, n, size);
        tmp->resize((size_t)frame);
        vbz_unzstd(src, n, tmp->data(), frame);
        packed = tmp->data();
        packed_bytes = (size_t)frame;
    }
    out->resize(size);
    if (!vbz_unpack(packed, packed_bytes, size / 2, reinterpret_cast<int16_t*>(out->data())))
        throw UnsupportedFilter("VBZ chunk: data bytes do not match the control bytes");
}

// The chunk inflated last.  A read stored as ONE chunk (common) is asked for twice, once per end,
// and deflate cannot be entered in the middle.  One per thread: a Fast5 whose reads are resolved
// is read-only otherwise, so several threads can decode different reads of it at once.
// It also owns what decoding needs over and over - the second buffer of the filter pipeline and
// the inflate state - so that a thread working through thousands of reads does not allocate and
// free ~150 KB per read (in a fresh malloc arena that is a heap grow / trim per read, which
// serialises the threads on the address-space lock).
struct ChunkCache {
    std::vector<uint8_t> data, scratch;
    std::vector<uint8_t> vbz;           // a VBZ chunk's streamvbyte bytes (zstd stage undone)
    uint64_t addr = ~0ull, bytes = 0;
    uint64_t owner = 0;                 // the file the cached chunk came from, by Fast5's serial
                                        // number (chunk addresses repeat from file to file, and so
                                        // do the addresses of the Fast5 objects themselves)
    z_stream zs;
    bool zs_ready = false;
    void* fast_inflater = nullptr;      // libdeflate's, when there is one
    ChunkCache() { std::memset(&zs, 0, sizeof(zs)); }
    ~ChunkCache() {
        if (zs_ready) inflateEnd(&zs);
        if (fast_inflater) libdeflate().release(fast_inflater);
    }
    ChunkCache(const ChunkCache&) = delete;
    ChunkCache& operator=(const ChunkCache&) = delete;
};

// one zlib stream -> its bytes (libdeflate where the system has it, zlib otherwise)
inline void inflate_stream(const uint8_t* src, size_t src_len, size_t hint,
                           std::vector<uint8_t>* out, ChunkCache* cache) {
    const LibDeflate& fast = libdeflate();
    if (fast.usable()) {
        if (!cache->fast_inflater) cache->fast_inflater = fast.alloc();
        if (cache->fast_inflater) {
            out->resize(std::max<size_t>(hint, 64));
            size_t produced = 0;
            if (fast.zlib_decompress(cache->fast_inflater, src, src_len, out->data(),
                                     out->size(), &produced) == 0) {
                out->resize(produced);
                return;
            }
        }
    }
    z_stream& zs = cache->zs;
    if (cache->zs_ready) {
        if (inflateReset(&zs) != Z_OK) throw FormatError("zlib reset failed");
    } else {
        std::memset(&zs, 0, sizeof(zs));
        if (inflateInit(&zs) != Z_OK) throw FormatError("zlib init failed");
        cache->zs_ready = true;
    }
    out->resize(std::max<size_t>(hint, 64));
    zs.next_in = const_cast<Bytef*>(src);
    zs.avail_in = (uInt)src_len;
    size_t produced = 0;
    while (true) {
        zs.next_out = out->data() + produced;
        zs.avail_out = (uInt)(out->size() - produced);
        const int rc = inflate(&zs, Z_NO_FLUSH);
        produced = out->size() - zs.avail_out;
        if (rc == Z_STREAM_END) break;
        if (rc != Z_OK || (zs.avail_in == 0 && zs.avail_out != 0))
            throw FormatError("corrupt deflate stream");
        if (zs.avail_out == 0) {
            if (out->size() > (1u << 30))
                throw FormatError("chunk inflates to an implausible size");
            out->resize(out->size() * 2);
        }
    }
    out->resize(produced);
}

// HDF5's shuffle of `esize`-byte elements undone in place: the elements' first bytes, then their
// second ones, ... -> element by element (bytes beyond a whole number of elements stay)
inline void unshuffle(std::vector<uint8_t>* bytes, size_t esize, std::vector<uint8_t>* scratch) {
    const size_t n = bytes->size() / esize;
    scratch->assign(bytes->begin(), bytes->end());
    for (size_t e = 0; e < esize; ++e)
        for (size_t k = 0; k < n; ++k) (*scratch)[k * esize + e] = (*bytes)[e * n + k];
    bytes->swap(*scratch);
}

}  // namespace

#endif  // DEEPBINNER_FAST5_CODECS_H
