// fast5_batch.h - a batch of reads and what the loaders share in filling one, packed or raw.
#ifndef DEEPBINNER_FAST5_BATCH_H
#define DEEPBINNER_FAST5_BATCH_H

#include <memory>

#include "fast5_file.h"
#include "fast5_pools.h"

struct f5_batch {
    SampleBuffer samples;
    std::vector<int64_t> offsets;
    std::vector<int32_t> status;
    std::vector<char> read_ids;
    // raw batches (f5_stream_open_raw): the Signal pieces as stored, for a decoder elsewhere
    SampleBuffer comp;                       // bytes (its count is in int16 units: see comp_bytes)
    int64_t comp_bytes = 0;
    std::vector<f5_raw_stream> streams;
};

// ---------------------------------------------------------------------------------------------
// What the loaders share.  Each of them (f5_load_batch, f5_load_batch_raw_ex, f5_load_reads, the
// packed and the raw f5_stream) deals the work out to its threads in its own way; what is done to
// a read, a range of reads or a batch is written here, once.
// ---------------------------------------------------------------------------------------------
namespace {

// Runs fn and maps what it throws to the ABI's status codes.
template <class Fn>
int guarded(Fn&& fn) {
    try {
        fn();
        return F5_OK;
    } catch (const UnsupportedFilter&) {
        return F5_ERR_FILTER;
    } catch (const ExistsError&) {
        return F5_ERR_EXISTS;
    } catch (const FormatError&) {
        return F5_ERR_FORMAT;
    } catch (const std::out_of_range&) {
        return F5_ERR_NO_READ;
    } catch (const std::bad_alloc&) {
        return F5_ERR_FORMAT;
    } catch (const std::exception&) {
        return F5_ERR_OPEN;
    }
}

void copy_read_id(const std::string& id, char* dst) {
    std::memset(dst, 0, F5_READ_ID_MAX);
    std::memcpy(dst, id.data(), std::min<size_t>(id.size(), F5_READ_ID_MAX - 1));
}

// a batch of n reads, none of them loaded yet
f5_batch* new_batch(int64_t n) {
    std::unique_ptr<f5_batch> batch(new f5_batch);
    batch->offsets.assign((size_t)n + 1, 0);
    batch->status.assign((size_t)n, F5_ERR_OPEN);
    batch->read_ids.assign((size_t)n * F5_READ_ID_MAX, 0);
    return batch.release();
}

// read i of the batch could not be loaded: no id, and why
void fail_read(f5_batch* batch, int64_t i, int rc) {
    std::memset(&batch->read_ids[(size_t)i * F5_READ_ID_MAX], 0, F5_READ_ID_MAX);
    batch->status[(size_t)i] = rc;
}

// File i of a batch of ONE-READ files (f5_load_batch, f5_load_batch_raw_ex), from the open to its
// status on one worker thread: read into the thread's buffer, parsed - a container is refused,
// F5_ERR_MULTI - and read0(file, read, cache) takes of its read what the batch wants.  false: the
// read failed (unreadable, or damaged where only inflating shows it) and is marked so.
template <class Read0>
bool load_one_read_file(const char* path, f5_batch* batch, int64_t i, Read0&& read0) {
    thread_local std::vector<uint8_t> file_bytes;
    thread_local ChunkCache cache;
    cache.addr = ~0ull;            // what it holds is another file's chunk
    bool multi = false;
    int rc = path ? F5_OK : F5_ERR_ARGUMENT;
    if (rc == F5_OK) rc = guarded([&] {
        Fast5 file(path, &file_bytes);
        file.parse();
        if (file.layout() == F5_LAYOUT_MULTI) {
            multi = true;
            return;
        }
        const ReadEntry& r = file.read(0);
        read0(file, r, &cache);
        copy_read_id(r.read_id, &batch->read_ids[(size_t)i * F5_READ_ID_MAX]);
    });
    if (multi) rc = F5_ERR_MULTI;
    if (rc != F5_OK) fail_read(batch, i, rc);
    else batch->status[(size_t)i] = F5_OK;
    return rc == F5_OK;
}

// ---- packed batches ---------------------------------------------------------------------------
// The head/tail rule: with keep > 0 a read longer than 2 * keep gives its first and its last `keep`
// samples only (windows are cut from those); how many samples a read of n gives
int64_t kept_length(int64_t n, int64_t keep) { return keep > 0 && n > 2 * keep ? 2 * keep : n; }

// ... and those samples, kept_length(s.n, keep) of them at dst: one whole read, or the two halves
void read_ends(Fast5& file, const SignalInfo& s, int64_t keep, int16_t* dst, ChunkCache* cache) {
    if (kept_length(s.n, keep) < s.n) {
        file.read_signal(s, 0, keep, dst, cache);
        file.read_signal(s, s.n - keep, keep, dst + keep, cache);
    } else {
        file.read_signal(s, 0, s.n, dst, cache);
    }
}

// The passes over reads first .. first + batch size of ONE file (f5_load_reads, f5_stream), each
// for places [a, b) of the batch.  Resolve: id, status and kept length of every read, each touched
// by one thread only; also(read, i) is what the caller needs of a resolved read besides.
template <class Also>
void resolve_reads(Fast5& file, int64_t first, int64_t keep, f5_batch* batch,
                   std::vector<int64_t>* lengths, int64_t a, int64_t b, Also&& also) {
    for (int64_t i = a; i < b; ++i)
        batch->status[(size_t)i] = guarded([&] {
            const ReadEntry& r = file.read(first + i);
            (*lengths)[(size_t)i] = kept_length(r.signal.n, keep);
            also(r, i);
            copy_read_id(r.read_id, &batch->read_ids[(size_t)i * F5_READ_ID_MAX]);
        });
}

// Between the passes: the offsets, a prefix sum that skips the reads that failed -> all samples
int64_t place_reads(f5_batch* batch, const std::vector<int64_t>& lengths) {
    const size_t n = batch->status.size();
    int64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        batch->offsets[i] = total;
        total += batch->status[i] == F5_OK ? lengths[i] : 0;
    }
    batch->offsets[n] = total;
    return total;
}

// Inflate into place: a read whose damage shows only now keeps its range, zero filled
void inflate_reads(Fast5& file, int64_t first, int64_t keep, f5_batch* batch,
                   const std::vector<int64_t>& lengths, int64_t a, int64_t b, ChunkCache* cache) {
    for (int64_t i = a; i < b; ++i) {
        if (batch->status[(size_t)i] != F5_OK) continue;
        int16_t* dst = batch->samples.data() + batch->offsets[(size_t)i];
        const int rc = guarded([&] { read_ends(file, file.read(first + i).signal, keep, dst, cache); });
        if (rc == F5_OK) continue;
        std::memset(dst, 0, (size_t)lengths[(size_t)i] * 2);
        fail_read(batch, i, rc);
    }
}

// ---- raw batches ------------------------------------------------------------------------------
// a raw stream's weight in the order of the records: the bytes of its deflate data (a shuffled
// deflate stream is one), 0 for everything else
int64_t deflate_weight(const f5_raw_stream& x) {
    return x.mode == F5_RAW_ZLIB || x.mode == F5_RAW_ZLIB_SHUFFLE ? x.comp_bytes : 0;
}
void put_u32le(uint8_t* dst, uint32_t v) {
    for (int k = 0; k < 4; ++k) dst[k] = (uint8_t)(v >> (8 * k));
}

// What a piece occupies in a raw batch's byte buffer: its stored bytes behind its prefix - of
// unfiltered data no more than is wanted -, a VBZ chunk with the host's stage undone, nothing for
// a chunk that was never written, and for a piece the host decodes (kHostDecode) its samples
int64_t raw_piece_bytes(const Fast5::RawPiece& p) {
    const int64_t wanted = p.count * 2;
    return p.kind == Fast5::kZlib     ? p.prefix + (int64_t)p.nbytes
           : p.kind == Fast5::kStored ? p.prefix + std::min<int64_t>((int64_t)p.nbytes, wanted)
           : p.kind == Fast5::kZeros  ? 0
           : p.kind == Fast5::kVbz    ? (int64_t)p.vbz_bytes
                                      : wanted;
}

// The pieces of read `read` get their places in the byte buffer, from byte *at on, and their
// records: where the bytes lie, where the samples go, how the decoder is to take them
void place_pieces(f5_batch* batch, int64_t read, std::vector<Fast5::RawPiece>* pieces, int64_t* at) {
    for (Fast5::RawPiece& p : *pieces) {
        p.comp_offset = *at;
        p.comp_bytes = raw_piece_bytes(p);
        *at += p.comp_bytes;
        f5_raw_stream rec;
        rec.comp_offset = p.comp_offset;
        rec.comp_bytes = p.comp_bytes;
        rec.out_offset = (batch->offsets[(size_t)read] + p.first) * 2;
        rec.out_bytes = p.count * 2;
        rec.mode = p.kind == Fast5::kZlib  ? (p.prefix ? F5_RAW_ZLIB_SHUFFLE : F5_RAW_ZLIB)
                   : p.kind == Fast5::kVbz ? (p.vbz_gpu ? F5_RAW_VBZ_ZSTD : F5_RAW_VBZ)
                   : p.kind == Fast5::kStored && p.prefix ? F5_RAW_STORED_SHUFFLE
                                                          : F5_RAW_STORED;
        rec.reserved = (int32_t)read;          // which read of the batch it belongs to
        batch->streams.push_back(rec);
    }
}

// All pieces placed, `at` bytes of them: the records go out longest deflate stream first, so that
// the lanes of a wave of the GPU decoder - which step together, one stream each - get streams of
// one length; the byte buffer is sized (in int16 units), 64 readable zero bytes behind the last
// stream, since the decoder fetches ahead of itself
void finish_raw_batch(f5_batch* batch, int64_t at) {
    std::stable_sort(batch->streams.begin(), batch->streams.end(),
                     [](const f5_raw_stream& x, const f5_raw_stream& y) {
                         return deflate_weight(x) > deflate_weight(y);
                     });
    batch->comp_bytes = at;
    batch->comp.resize((size_t)(at + 64 + 1) / 2);
    std::memset(reinterpret_cast<uint8_t*>(batch->comp.data()) + at, 0, 64);
}

// The host's zstd stage of a VBZ piece whose streamvbyte stage is the GPU's: the chunk as stored
// (p.nbytes of it) -> at dst its 4 header bytes and, behind them, the frame's content
void vbz_host_stage(const uint8_t* chunk, const Fast5::RawPiece& p, uint8_t* dst) {
    std::memcpy(dst, chunk, 4);
    vbz_unzstd(chunk, (size_t)p.nbytes, dst + 4, p.vbz_bytes - 4);
}

// One file of f5_load_batch_raw_ex between its passes
struct StagedRead {
    std::vector<Fast5::RawPiece> pieces;       // file_off = offset into `bytes` from here on
    std::string bytes;
    int64_t samples = 0;
};

// The host's share of a batch of ONE-READ files: the deflate streams of the whole batch one by
// one, longest first, until they hold `share` per cent of its compressed bytes.  Unlike the
// container's rule (Stream::take_host_share) it counts streams, not a length - of several
// streams of one length some may stay the GPU's - and knows no exception for long streams.  A
// shuffled stream keeps its prefix: pass 2 inflates the staged bytes and unshuffles them itself.
void take_host_share(std::vector<StagedRead>* staged, int share) {
    std::vector<std::pair<uint64_t, Fast5::RawPiece*>> streams;
    uint64_t total = 0;
    for (StagedRead& st : *staged)
        for (Fast5::RawPiece& p : st.pieces)
            if (p.kind == Fast5::kZlib) {
                streams.push_back({p.nbytes, &p});
                total += p.nbytes;
            }
    std::sort(streams.begin(), streams.end(),
              [](const auto& a, const auto& b) { return a.first > b.first; });
    uint64_t taken = 0;
    for (const auto& e : streams) {
        if (taken * 100 >= total * (uint64_t)share) break;
        e.second->kind = Fast5::kHostDecode;
        taken += e.first;
    }
}

}  // namespace

#endif  // DEEPBINNER_FAST5_BATCH_H
