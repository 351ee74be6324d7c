// fast5_signal.h - the Signal dataset: its layouts, filter pipeline and chunk indexes, decoded
// (read_signal) or handed out piece by piece as stored (signal_pieces).
#ifndef DEEPBINNER_FAST5_SIGNAL_H
#define DEEPBINNER_FAST5_SIGNAL_H

#include <atomic>

#include "../../include/deepbinner_fast5.h"
#include "fast5_codecs.h"
#include "fast5_hdf5.h"

namespace {

struct Filter {
    int id;
    std::vector<uint32_t> cd;
};

struct SignalInfo {
    int64_t n = 0;             // samples
    int layout = -1;           // 0 compact, 1 contiguous, 2 chunked
    uint64_t addr = kUndef;    // contiguous data / chunk B-tree
    uint64_t compact_off = 0, compact_size = 0;
    int64_t chunk_elems = 0;
    // chunk index: 0 = version-1 B-tree (layout message up to version 3); layout version 4
    // (HDF5 1.10, libver latest): 1 = the single chunk itself, 2 = implicit (all chunks back to
    // back), 3 = fixed array, 4 = extensible array
    int index = 0;
    uint64_t single_bytes = 0;
    uint32_t single_mask = 0;
    bool unfiltered_edge = false;   // layout flag: a partial last chunk is stored unfiltered
    std::vector<Filter> filters;
};

// How the raw loaders (f5_load_batch_raw_ex, f5_stream_open_raw_ex) hand a Signal out, from their
// arguments (host_inflate_above, flags):
struct RawOptions {
    int64_t zlib_above = 0;     // deflate streams longer than this many bytes are the host's; 0: none
    int host_share = 0;         // ... or the longest ones holding this share (per cent) of the bytes
    bool vbz_zstd_gpu = false;  // F5_RAW_FLAG_VBZ_ZSTD_GPU: VBZ chunks with a zstd stage go out as stored
    bool shuffle_gpu = false;   // F5_RAW_FLAG_SHUFFLE_GPU: shuffled chunks go out as stored
};
// host_inflate_above > 0: a length in bytes; < 0: minus the host's share in per cent.  false: a flag
// this reader does not know.
bool raw_options(int64_t host_inflate_above, unsigned flags, RawOptions* o) {
    if (flags & ~(unsigned)(F5_RAW_FLAG_VBZ_ZSTD_GPU | F5_RAW_FLAG_SHUFFLE_GPU)) return false;
    o->zlib_above = host_inflate_above > 0 ? host_inflate_above : 0;
    o->host_share = host_inflate_above < 0 ? (int)std::min<int64_t>(100, -host_inflate_above) : 0;
    o->vbz_zstd_gpu = (flags & F5_RAW_FLAG_VBZ_ZSTD_GPU) != 0;
    o->shuffle_gpu = (flags & F5_RAW_FLAG_SHUFFLE_GPU) != 0;
    return true;
}

// An HDF5 file's int16 datasets of rank 1 - the Signals -, read from their object headers
class SignalFile : public Hdf5File {
  public:
    using Hdf5File::Hdf5File;

    // samples [first, first + count) of the Signal, decoded
    void read_signal(const SignalInfo& s, int64_t first, int64_t count, int16_t* out,
                     ChunkCache* cache = nullptr) {
        if (!cache) cache = &cache_;
        if (first < 0 || count < 0 || first + count > s.n) throw std::out_of_range("sample range");
        if (count == 0) return;
        if (s.layout == 0) {
            if ((uint64_t)(first + count) * 2 > s.compact_size) throw FormatError("compact data too short");
            need(s.compact_off, s.compact_size);
            std::memcpy(out, buf_ + s.compact_off + first * 2, (size_t)count * 2);
        } else if (s.layout == 1) {
            if (s.addr == kUndef) {
                std::memset(out, 0, (size_t)count * 2);
                return;
            }
            const uint64_t start = base_ + s.addr;
            need(start, (uint64_t)s.n * 2);
            std::memcpy(out, buf_ + start + first * 2, (size_t)count * 2);
        } else {
            std::memset(out, 0, (size_t)count * 2);
            if (s.addr == kUndef) return;
            if (s.chunk_elems <= 0) throw FormatError("bad chunk size");
            if (s.index == 0) {
                walk_chunks(s, s.addr, first, count, out, 0, cache);
                return;
            }
            for (int64_t k = first / s.chunk_elems; k * s.chunk_elems < first + count; ++k) {
                uint64_t addr = kUndef, nbytes = 0;
                uint32_t mask = 0;
                if (!indexed_chunk(s, (uint64_t)k, &addr, &nbytes, &mask)) continue;
                const bool partial = (k + 1) * s.chunk_elems > s.n;
                if (s.unfiltered_edge && partial) mask = ~0u;
                copy_from_chunk(s, k * s.chunk_elems, addr, nbytes, mask, first, count, out, cache);
            }
        }
    }

    // ---- the Signal as it is stored (for callers that inflate elsewhere: the GPU) ---------------
    // What a read's Signal consists of on disk, piece by piece, in sample order.  A piece covers
    // samples [first, first + count) of the read.
    struct RawPiece {
        int kind = 0;              // kZlib / kStored / kHostDecode / kZeros / kVbz
        uint64_t file_off = 0;     // where its bytes lie in the file (kZlib, kStored, kVbz)
        uint64_t nbytes = 0;       // how many
        int64_t first = 0, count = 0;
        uint64_t chunk_addr = 0, chunk_bytes = 0;      // kHostDecode: the chunk, for decode_chunk
        uint32_t mask = 0;
        int64_t comp_offset = 0, comp_bytes = 0;       // its place in a batch's byte buffer
        // kVbz: what the GPU is handed - the chunk with its zstd stage undone (u32 original_size,
        // streamvbyte bytes): vbz_bytes of them; vbz_zstd: the chunk has a zstd stage to undo
        uint64_t vbz_bytes = 0;
        bool vbz_zstd = false;
        // the chunk goes out as stored, zstd frame and all (F5_RAW_VBZ_ZSTD): the GPU undoes it
        bool vbz_gpu = false;
        // kZlib / kStored of a shuffled chunk the GPU unshuffles (F5_RAW_ZLIB_SHUFFLE,
        // F5_RAW_STORED_SHUFFLE): 4, the bytes of the u32 LE count * 2 that goes in front of the
        // piece's bytes in the batch's byte buffer; every other piece: 0 (a staged stream that
        // f5_load_batch_raw leaves to the host's share keeps it: inflated, then unshuffled)
        int prefix = 0;
    };
    enum { kZlib = 0, kStored = 1, kHostDecode = 2, kZeros = 3, kVbz = 4 };

    // o.zlib_above: deflate streams longer than this many bytes are left to the host (a lane of the
    // GPU decoder walks ONE stream: a stream ten times the usual length holds its wave ten times
    // as long, while a CPU core inflates it in a millisecond); <= 0: no limit.
    // o.vbz_zstd_gpu: VBZ chunks with a zstd stage are handed on as stored.
    // o.shuffle_gpu: whole chunks of shuffle (element size 2) + deflate, or of shuffle alone, with
    // or without fletcher32 behind, go out as stored, a prefix in front.
    // (o.host_share is the loaders' business: it is taken over a whole batch.)
    void signal_pieces(const SignalInfo& s, const RawOptions& o, std::vector<RawPiece>* out) const {
        out->clear();
        if (s.n <= 0) return;
        RawPiece p;
        p.first = 0;
        p.count = s.n;
        if (s.layout == 0) {
            if ((uint64_t)s.n * 2 > s.compact_size) throw FormatError("compact data too short");
            need(s.compact_off, s.compact_size);
            p.kind = kStored;
            p.file_off = s.compact_off;
            p.nbytes = (uint64_t)s.n * 2;
            out->push_back(p);
            return;
        }
        if (s.layout == 1) {
            if (s.addr == kUndef) {
                p.kind = kZeros;
            } else {
                p.kind = kStored;
                p.file_off = base_ + s.addr;
                p.nbytes = (uint64_t)s.n * 2;
                need(p.file_off, p.nbytes);
            }
            out->push_back(p);
            return;
        }
        if (s.chunk_elems <= 0) throw FormatError("bad chunk size");
        const int64_t n_chunks = (s.n + s.chunk_elems - 1) / s.chunk_elems;
        if (n_chunks > (1 << 24)) throw FormatError("implausible number of chunks");
        std::vector<RawPiece> by_chunk((size_t)n_chunks);
        for (int64_t k = 0; k < n_chunks; ++k) {
            RawPiece& q = by_chunk[(size_t)k];
            q.kind = kZeros;                       // a chunk that was never written reads as zeros
            q.first = k * s.chunk_elems;
            q.count = std::min<int64_t>(s.chunk_elems, s.n - q.first);
        }
        bool shuffle_i16 = false;                  // the pipeline's shuffle is one of 2-byte elements
        for (const Filter& f : s.filters)
            if (f.id == 2) shuffle_i16 = !f.cd.empty() && f.cd[0] == 2;
        auto found = [&](int64_t k, uint64_t addr, uint64_t nbytes, uint32_t mask) {
            if (k < 0 || k >= n_chunks) return;
            RawPiece& q = by_chunk[(size_t)k];
            const uint64_t start = file_off(addr);
            need(start, nbytes);
            q.chunk_addr = addr;
            q.chunk_bytes = nbytes;
            q.mask = mask;
            // the filters that were applied to THIS chunk, in the order they were applied
            int applied[8], n_applied = 0;
            bool known = true;
            for (size_t i = 0; i < s.filters.size(); ++i) {
                if (mask & (1u << i)) continue;
                if (n_applied == 8) known = false;
                else applied[n_applied++] = s.filters[i].id;
            }
            q.file_off = start;
            q.nbytes = nbytes;
            if (!known) {
                q.kind = kHostDecode;
            } else if (n_applied == 0) {
                q.kind = kStored;
            } else if (n_applied == 1 && applied[0] == 1) {
                q.kind = kZlib;
            } else if (n_applied == 2 && applied[0] == 1 && applied[1] == 3 && nbytes >= 4) {
                q.kind = kZlib;                    // deflate, then a checksum behind the stream
                q.nbytes = nbytes - 4;
            } else if (n_applied == 2 && applied[0] == 3 && applied[1] == 1) {
                q.kind = kZlib;                    // the checksum lies inside, behind the samples
            } else if (n_applied == 1 && applied[0] == 3 && nbytes >= 4) {
                q.kind = kStored;
                q.nbytes = nbytes - 4;
            } else if (n_applied == 1 && applied[0] == kVbzFilter) {
                // VBZ alone: the size of what the GPU gets needs the chunk's header (and the zstd
                // frame's); the self-checks on sizes run here, a failure refuses the read
                q.kind = kVbz;
                for (const Filter& f : s.filters)
                    if (f.id == kVbzFilter) q.vbz_zstd = vbz_zstd(f.cd);
                uint8_t head[32];
                const uint64_t h = std::min<uint64_t>(nbytes, sizeof(head));
                read_bytes(start, h, head);
                const uint32_t size = vbz_original_size(head, (size_t)h, (size_t)s.chunk_elems * 2);
                if (q.vbz_zstd && o.vbz_zstd_gpu) {
                    (void)vbz_frame_size_header(head, (size_t)h, size);     // (sized and checked)
                    q.vbz_zstd = false;                // nothing for the host to undo
                    q.vbz_gpu = true;
                    q.vbz_bytes = nbytes;
                } else {
                    q.vbz_bytes = q.vbz_zstd ? 4 + vbz_frame_size(head, (size_t)h, size) : nbytes;
                }
            } else if (o.shuffle_gpu && shuffle_i16 && q.count == s.chunk_elems && applied[0] == 2 &&
                       ((n_applied == 2 && applied[1] == 1) ||
                        (n_applied == 3 && applied[1] == 1 && applied[2] == 3 && nbytes >= 4))) {
                // shuffle + deflate of a chunk that is wanted WHOLE (of a partial one the wanted
                // high bytes lie behind more low bytes than the read has room for: the host's);
                // a checksum behind the stream stays unverified, as for plain deflate
                q.kind = kZlib;
                q.prefix = 4;
                q.nbytes = n_applied == 3 ? nbytes - 4 : nbytes;
            } else if (o.shuffle_gpu && shuffle_i16 && q.count == s.chunk_elems && applied[0] == 2 &&
                       (n_applied == 1 || (n_applied == 2 && applied[1] == 3 && nbytes >= 4)) &&
                       nbytes - (n_applied == 2 ? 4 : 0) == (uint64_t)q.count * 2) {
                q.kind = kStored;                  // shuffle alone: the two planes as they are
                q.prefix = 4;
                q.nbytes = (uint64_t)q.count * 2;
            } else {
                q.kind = kHostDecode;              // shuffle, or an order not seen in the field
            }
            if (q.kind == kZlib && o.zlib_above > 0 && (int64_t)q.nbytes > o.zlib_above) {
                q.kind = kHostDecode;
                q.prefix = 0;
            }
        };
        if (s.addr != kUndef) {
            if (s.index == 0) {
                collect_chunks(s, s.addr, 0, found);
            } else {
                for (int64_t k = 0; k < n_chunks; ++k) {
                    uint64_t addr = kUndef, nbytes = 0;
                    uint32_t mask = 0;
                    if (!indexed_chunk(s, (uint64_t)k, &addr, &nbytes, &mask)) continue;
                    if (s.unfiltered_edge && (k + 1) * s.chunk_elems > s.n) mask = ~0u;
                    found(k, addr, nbytes, mask);
                }
            }
        }
        *out = std::move(by_chunk);
    }

    // a piece the host decodes itself -> its samples' bytes at dst (count * 2 of them)
    void decode_piece(const SignalInfo& s, const RawPiece& p, uint8_t* dst, ChunkCache* cache) const {
        decode_chunk(s, p.chunk_addr, p.chunk_bytes, p.mask, cache);
        cache->owner = 0;                          // (not a chunk read_signal may reuse blindly)
        std::memcpy(dst, cache->data.data(), (size_t)p.count * 2);
    }

    // The one chunk a read's Signal is stored as, if it is ONE chunk of exactly the read's
    // samples compressed by the deflate filter alone: a one-read copy can carry it as it is.
    bool whole_deflated_chunk(const SignalInfo& s, uint64_t* off, uint64_t* nbytes) const {
        if (s.layout != 2 || s.n <= 0 || s.chunk_elems != s.n || s.filters.size() != 1 ||
            s.filters[0].id != 1)
            return false;
        std::vector<RawPiece> pieces;
        signal_pieces(s, RawOptions(), &pieces);
        if (pieces.size() != 1 || pieces[0].kind != kZlib || pieces[0].mask != 0 ||
            pieces[0].count != s.n)
            return false;
        *off = pieces[0].file_off;
        *nbytes = pieces[0].nbytes;
        return true;
    }

  protected:
    static uint64_t next_serial() {
        static std::atomic<uint64_t> last{0};
        return ++last;
    }
    const uint64_t serial_ = next_serial();            // never 0, never given twice (ChunkCache)
    ChunkCache cache_;                           // for callers that bring none (one thread)

    // ---- the Signal dataset ---------------------------------------------------------------------
    SignalInfo signal_info(uint64_t addr) const {
        const std::vector<Msg> msgs = object_header(addr);
        const Msg* dt = first_of(msgs, 0x0003);
        const Msg* ds = first_of(msgs, 0x0001);
        const Msg* lay = first_of(msgs, 0x0008);
        if (!dt || !ds || !lay) throw FormatError("Signal without datatype/dataspace/layout");
        const int cls = b(dt->off) & 0x0F;
        const uint64_t bits = u(dt->off + 1, 3);
        if (cls != 0 || u(dt->off + 4, 4) != 2 || (bits & 1) || !(bits & 0x08))
            throw FormatError("Signal is not a little-endian int16 dataset");
        const int ds_version = b(ds->off), rank = b(ds->off + 1);
        if ((ds_version != 1 && ds_version != 2) || rank != 1)
            throw FormatError("Signal is not one-dimensional");
        SignalInfo s;
        const uint64_t n = u(ds->off + (ds_version == 1 ? 8 : 4), kL);
        // deflate expands at most 1032-fold, so a signal cannot be much longer than that many
        // times the file (a damaged length would otherwise have the caller allocate terabytes)
        if (n > (1ull << 40) || n / 1100 > len_ + 4096)
            throw FormatError("implausible Signal length");
        s.n = (int64_t)n;

        const int version = b(lay->off);
        if (version == 1 || version == 2) {
            const int ndim = b(lay->off + 1), lcls = b(lay->off + 2);
            uint64_t p = lay->off + 8;
            if (lcls != 0) {
                s.addr = u(p, kO);
                p += kO;
            }
            const uint64_t dims = p;
            p += 4ull * ndim;
            if (lcls == 0) {
                s.layout = 0;
                s.compact_size = u(p, 4);
                s.compact_off = p + 4;
            } else if (lcls == 1) {
                s.layout = 1;
            } else {
                if (ndim != 2) throw FormatError("unexpected chunk rank");
                s.layout = 2;
                s.chunk_elems = (int64_t)u(dims, 4);
            }
        } else if (version == 3) {
            const int lcls = b(lay->off + 1);
            const uint64_t p = lay->off + 2;
            if (lcls == 0) {
                s.layout = 0;
                s.compact_size = u(p, 2);
                s.compact_off = p + 2;
            } else if (lcls == 1) {
                s.layout = 1;
                s.addr = u(p, kO);
            } else if (lcls == 2) {
                if (b(p) != 2) throw FormatError("unexpected chunk rank");
                s.layout = 2;
                s.addr = u(p + 1, kO);
                s.chunk_elems = (int64_t)u(p + 1 + kO, 4);
            } else {
                throw FormatError("unsupported data layout class");
            }
        } else if (version == 4) {
            const int lcls = b(lay->off + 1);
            uint64_t p = lay->off + 2;
            if (lcls == 0) {
                s.layout = 0;
                s.compact_size = u(p, 2);
                s.compact_off = p + 2;
            } else if (lcls == 1) {
                s.layout = 1;
                s.addr = u(p, kO);
            } else if (lcls == 2) {
                const int flags = b(p), ndim = b(p + 1), enc = b(p + 2);
                if (ndim != 2 || enc < 1 || enc > 8) throw FormatError("unexpected chunk rank");
                s.layout = 2;
                s.chunk_elems = (int64_t)u(p + 3, enc);
                s.unfiltered_edge = (flags & 1) != 0;
                p += 3 + 2ull * enc;
                s.index = b(p);
                p += 1;
                if (s.index == 1) {
                    s.single_bytes = (uint64_t)s.chunk_elems * 2;
                    if (flags & 2) {
                        s.single_bytes = u(p, kL);
                        s.single_mask = (uint32_t)u(p + kL, 4);
                        p += kL + 4;
                    }
                } else if (s.index == 2) {
                } else if (s.index == 3) {
                    p += 1;
                } else if (s.index == 4) {
                    p += 5;
                } else {
                    throw FormatError("unsupported chunk index type");
                }
                s.addr = u(p, kO);
            } else {
                throw FormatError("unsupported data layout class");
            }
        } else {
            throw FormatError("unsupported data layout version");
        }

        if (const Msg* fm = first_of(msgs, 0x000B)) {
            const int fversion = b(fm->off), nf = b(fm->off + 1);
            uint64_t p = fm->off + (fversion == 1 ? 8 : 2);
            for (int i = 0; i < nf; ++i) {
                Filter f;
                f.id = (int)u(p, 2);
                p += 2;
                uint64_t name_len = 0;
                if (fversion == 1 || f.id >= 256) {
                    name_len = u(p, 2);
                    p += 2;
                }
                p += 2;   // flags
                const uint64_t ncd = u(p, 2);
                p += 2;
                p += fversion == 1 ? pad8(name_len) : name_len;
                for (uint64_t k = 0; k < ncd; ++k) f.cd.push_back((uint32_t)u(p + 4 * k, 4));
                p += 4 * ncd;
                if (fversion == 1 && (ncd % 2) == 1) p += 4;
                if (f.id == kVbzFilter && s.layout == 2 &&
                    (!vbz_accepted(f.cd) || (vbz_zstd(f.cd) && !libzstd().usable())))
                    throw UnsupportedFilter("Signal uses a VBZ variant this reader does not decode");
                if (f.id != 1 && f.id != 2 && f.id != 3 && f.id != kVbzFilter && s.layout == 2)
                    throw UnsupportedFilter("Signal uses a filter other than deflate/shuffle/fletcher32/vbz");
                s.filters.push_back(f);
            }
        }
        return s;
    }

    // one stored chunk -> its elements (filters undone in reverse order, short chunks zero-extended)
    void decode_chunk(const SignalInfo& s, uint64_t addr, uint64_t nbytes, uint32_t mask,
                      ChunkCache* cache) const {
        std::vector<uint8_t>* raw = &cache->data;
        std::vector<uint8_t>& tmp = cache->scratch;
        const uint64_t start = file_off(addr);
        need(start, nbytes);
        raw->resize((size_t)nbytes);
        if (nbytes) read_bytes(start, nbytes, raw->data());
        for (int i = (int)s.filters.size() - 1; i >= 0; --i) {
            if (mask & (1u << i)) continue;
            const Filter& f = s.filters[(size_t)i];
            if (f.id == 1) {
                inflate_stream(raw->data(), raw->size(), (size_t)s.chunk_elems * 2 + 8, &tmp, cache);
                raw->swap(tmp);
            } else if (f.id == 2) {
                const size_t esize = f.cd.empty() ? 2 : f.cd[0];
                if (esize == 0) throw FormatError("bad shuffle parameter");
                unshuffle(raw, esize, &tmp);
            } else if (f.id == 3) {
                if (raw->size() < 4) throw FormatError("chunk shorter than its checksum");
                raw->resize(raw->size() - 4);
            } else if (f.id == kVbzFilter) {
                vbz_decode(raw->data(), raw->size(), f.cd, (size_t)s.chunk_elems * 2, &tmp,
                           &cache->vbz);
                raw->swap(tmp);
            } else {
                throw FormatError("unsupported filter");
            }
        }
        // some writers (MinKNOW) store a short final chunk; libhdf5 zero-extends it
        if (raw->size() < (size_t)s.chunk_elems * 2) raw->resize((size_t)s.chunk_elems * 2, 0);
    }

    // the part of [first, first + count) that the chunk starting at sample `lo` holds
    void copy_from_chunk(const SignalInfo& s, int64_t lo, uint64_t addr, uint64_t nbytes,
                         uint32_t mask, int64_t first, int64_t count, int16_t* out,
                         ChunkCache* cache) const {
        const int64_t hi = std::min<int64_t>(lo + s.chunk_elems, s.n);
        const int64_t a = std::max(lo, first), z = std::min(hi, first + count);
        if (a >= z) return;
        // the last chunk inflated stays around: a read stored as ONE chunk (common) is asked
        // for twice, once per end, and deflate cannot be entered in the middle
        if (cache->owner != serial_ || cache->addr != addr || cache->bytes != nbytes) {
            cache->addr = ~0ull;
            decode_chunk(s, addr, nbytes, mask, cache);
            cache->owner = serial_;
            cache->addr = addr;
            cache->bytes = nbytes;
        }
        std::memcpy(out + (a - first), cache->data.data() + (size_t)(a - lo) * 2, (size_t)(z - a) * 2);
    }

    // ---- chunk indexes of layout version 4 (hdf5_lite._fixed_array / _extensible_array) ----------
    // one record of a fixed / extensible array; false: the chunk was never written
    bool index_record(uint64_t p, bool filtered, int elmt_size, uint64_t chunk_bytes,
                      uint64_t* addr, uint64_t* nbytes, uint32_t* mask) const {
        *addr = u(p, kO);
        if (*addr == kUndef) return false;
        if (!filtered) {
            *nbytes = chunk_bytes;
            *mask = 0;
            return true;
        }
        const int size_len = elmt_size - kO - 4;
        if (size_len < 1 || size_len > 8) throw FormatError("bad chunk record size");
        *nbytes = u(p + kO, size_len);
        *mask = (uint32_t)u(p + kO + size_len, 4);
        return true;
    }

    static int log2_floor(uint64_t v) {
        int r = -1;
        while (v) {
            v >>= 1;
            ++r;
        }
        return r;
    }

    bool bit_set(uint64_t bitmap, uint64_t bit) const { return (b(bitmap + bit / 8) & (0x80u >> (bit % 8))) != 0; }

    bool indexed_chunk(const SignalInfo& s, uint64_t k, uint64_t* addr, uint64_t* nbytes,
                       uint32_t* mask) const {
        const uint64_t chunk_bytes = (uint64_t)s.chunk_elems * 2;
        if (s.index == 1) {
            if (k != 0) return false;
            *addr = s.addr;
            *nbytes = s.single_bytes;
            *mask = s.single_mask;
            return true;
        }
        if (s.index == 2) {
            *addr = s.addr + k * chunk_bytes;
            *nbytes = chunk_bytes;
            *mask = 0;
            return true;
        }
        const uint64_t p = file_off(s.addr);
        if (s.index == 3) {
            if (!sig(p, "FAHD") || b(p + 4) != 0) throw FormatError("bad fixed array header");
            const bool filtered = b(p + 5) == 1;
            const int elmt_size = b(p + 6), page_bits = b(p + 7);
            const uint64_t n = u(p + 8, kL);
            if (k >= n || page_bits > 40) return false;
            const uint64_t block = file_off(u(p + 8 + kL, kO));
            if (!sig(block, "FADB")) throw FormatError("bad fixed array data block");
            uint64_t q = block + 6 + kO;
            const uint64_t page = 1ull << page_bits;
            if (n > page) {            // paged: bitmap, checksum, then checksummed pages
                const uint64_t n_pages = (n + page - 1) / page;
                const uint64_t pg = k / page, within = k % page;
                if (!bit_set(q, pg)) return false;
                q += (n_pages + 7) / 8 + 4;
                return index_record(q + pg * (page * elmt_size + 4) + within * elmt_size, filtered,
                                    elmt_size, chunk_bytes, addr, nbytes, mask);
            }
            return index_record(q + k * elmt_size, filtered, elmt_size, chunk_bytes, addr, nbytes, mask);
        }
        // extensible array: the first records in the index block, then data blocks of doubling size,
        // the early ones addressed from the index block, the later ones through super blocks
        if (!sig(p, "EAHD") || b(p + 4) != 0) throw FormatError("bad extensible array header");
        const bool filtered = b(p + 5) == 1;
        const int elmt_size = b(p + 6), max_bits = b(p + 7), idx_elmts = b(p + 8),
                  dblk_min = b(p + 9), sblk_min_ptrs = b(p + 10), page_bits = b(p + 11);
        if (dblk_min < 1 || sblk_min_ptrs < 2 || max_bits > 64 || page_bits > 40 ||
            (dblk_min & (dblk_min - 1)) || (sblk_min_ptrs & (sblk_min_ptrs - 1)))
            throw FormatError("bad extensible array parameters");
        const uint64_t index_block = u(p + 12 + 6 * kL, kO);
        if (index_block == kUndef) return false;
        const uint64_t q = file_off(index_block);
        if (!sig(q, "EAIB")) throw FormatError("bad extensible array index block");
        const uint64_t elements = q + 6 + kO;
        if (k < (uint64_t)idx_elmts)
            return index_record(elements + k * elmt_size, filtered, elmt_size, chunk_bytes, addr,
                                nbytes, mask);
        const int off_size = (max_bits + 7) / 8;
        const int n_sblks = 1 + max_bits - log2_floor((uint64_t)dblk_min);
        const int iblock_sblks = 2 * log2_floor((uint64_t)sblk_min_ptrs);
        const uint64_t n_dblk_addrs = 2ull * (sblk_min_ptrs - 1);
        const uint64_t dblk_addrs = elements + (uint64_t)idx_elmts * elmt_size;
        const uint64_t sblk_addrs = dblk_addrs + n_dblk_addrs * kO;
        uint64_t rel = k - idx_elmts;
        const int s_idx = log2_floor(rel / dblk_min + 1);
        if (s_idx >= n_sblks || s_idx > 62) return false;
        // super block u: 2^(u/2) data blocks of 2^((u+1)/2) * dblk_min records
        uint64_t first_elmt = 0, first_dblk = 0;
        for (int v = 0; v < s_idx; ++v) {
            first_elmt += (1ull << (v / 2)) * ((1ull << ((v + 1) / 2)) * dblk_min);
            first_dblk += 1ull << (v / 2);
        }
        const uint64_t n_dblks = 1ull << (s_idx / 2);
        const uint64_t dblk_elmts = (1ull << ((s_idx + 1) / 2)) * dblk_min;
        rel -= first_elmt;
        const uint64_t d_idx = rel / dblk_elmts, within = rel % dblk_elmts;
        const uint64_t page = 1ull << page_bits;
        uint64_t block_addr;
        if (s_idx < iblock_sblks) {
            block_addr = u(dblk_addrs + (first_dblk + d_idx) * kO, kO);
        } else {
            const uint64_t super_addr = u(sblk_addrs + (uint64_t)(s_idx - iblock_sblks) * kO, kO);
            if (super_addr == kUndef) return false;
            const uint64_t sb = file_off(super_addr);
            if (!sig(sb, "EASB")) throw FormatError("bad extensible array super block");
            uint64_t t = sb + 6 + kO + off_size;
            if (dblk_elmts > page) {
                // "page initialised" bits: a whole number of bytes per data block is reserved,
                // but the bits are used as one run, `pages` per data block
                const uint64_t pages = dblk_elmts / page;
                if (!bit_set(t, d_idx * pages + within / page)) return false;
                t += n_dblks * ((pages + 7) / 8);
            }
            block_addr = u(t + d_idx * kO, kO);
        }
        if (block_addr == kUndef) return false;
        const uint64_t blk = file_off(block_addr);
        if (!sig(blk, "EADB")) throw FormatError("bad extensible array data block");
        uint64_t e = blk + 6 + kO + off_size;
        uint64_t at = within;
        if (dblk_elmts > page) {       // prefix checksum, then checksummed pages
            e += 4 + (within / page) * (page * elmt_size + 4);
            at = within % page;
        }
        return index_record(e + at * elmt_size, filtered, elmt_size, chunk_bytes, addr, nbytes, mask);
    }

    // chunk index: version-1 B-tree of raw-data chunks, rank 1 (hdf5_lite._walk_chunk_btree)
    void walk_chunks(const SignalInfo& s, uint64_t addr, int64_t first, int64_t count, int16_t* out,
                     int depth, ChunkCache* cache) const {
        if (depth > kMaxDepth) throw FormatError("chunk B-tree too deep");
        const uint64_t p = file_off(addr);
        if (!sig(p, "TREE")) throw FormatError("bad chunk B-tree signature");
        if (b(p + 4) != 1) throw FormatError("expected a raw-data chunk B-tree");
        const int level = b(p + 5);
        const uint64_t used = u(p + 6, 2);
        const uint64_t key_size = 8 + 8 * 2;
        const uint64_t q = p + 8 + 2 * kO;
        for (uint64_t i = 0; i < used; ++i) {
            const uint64_t k = q + i * (key_size + kO);
            const uint64_t nbytes = u(k, 4);
            const uint32_t mask = (uint32_t)u(k + 4, 4);
            const uint64_t offset = u(k + 8, 8);
            const uint64_t child = u(k + key_size, kO);
            if (level > 0) {
                // keys are the first chunk offsets of the children: skip subtrees wholly outside
                if (i + 1 < used) {
                    const uint64_t next = u(q + (i + 1) * (key_size + kO) + 8, 8);
                    if ((int64_t)next <= first) continue;
                }
                if ((int64_t)offset >= first + count) break;
                walk_chunks(s, child, first, count, out, depth + 1, cache);
                continue;
            }
            if (offset >= (uint64_t)s.n) continue;
            copy_from_chunk(s, (int64_t)offset, child, nbytes, mask, first, count, out, cache);
        }
    }

    // the same walk, reporting every chunk instead of copying from it
    template <class Found>
    void collect_chunks(const SignalInfo& s, uint64_t addr, int depth, const Found& found) const {
        if (depth > kMaxDepth) throw FormatError("chunk B-tree too deep");
        const uint64_t p = file_off(addr);
        if (!sig(p, "TREE")) throw FormatError("bad chunk B-tree signature");
        if (b(p + 4) != 1) throw FormatError("expected a raw-data chunk B-tree");
        const int level = b(p + 5);
        const uint64_t used = u(p + 6, 2);
        const uint64_t key_size = 8 + 8 * 2;
        const uint64_t q = p + 8 + 2 * kO;
        for (uint64_t i = 0; i < used; ++i) {
            const uint64_t k = q + i * (key_size + kO);
            const uint64_t nbytes = u(k, 4);
            const uint32_t mask = (uint32_t)u(k + 4, 4);
            const uint64_t offset = u(k + 8, 8);
            const uint64_t child = u(k + key_size, kO);
            if (level > 0) {
                collect_chunks(s, child, depth + 1, found);
                continue;
            }
            if (offset >= (uint64_t)s.n || offset % (uint64_t)s.chunk_elems) continue;
            found((int64_t)(offset / (uint64_t)s.chunk_elems), child, nbytes, mask);
        }
    }
};

}  // namespace

#endif  // DEEPBINNER_FAST5_SIGNAL_H
