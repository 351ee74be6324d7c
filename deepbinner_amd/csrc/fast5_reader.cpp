// libdeepbinner_fast5.so - native fast5 loader (C ABI: include/deepbinner_fast5.h).
//
// The reference reads fast5 files through h5py (deepbinner/load_fast5s.py:19,25-49); this is the
// slice of the HDF5 file format those files use, restated in C++ from the format specification
// exactly as deepbinner_amd/hdf5_lite.py restates it in Python (that module stays the readable
// description and the parity reference for this one: tests/test_fast5_native.py).
// Host-only: g++ -O2 -shared -fPIC fast5_reader.cpp -lz -ldl -pthread (libdeflate, if the system has
// it, and libzstd, for VBZ, are looked up at run time).
//
// One translation unit, in layers, each a header that includes only the ones before it:
//   fast5_bytes.h   a file as checked bytes (read whole or mapped, pread, preadv)
//   fast5_codecs.h  deflate, VBZ, shuffle; the per-thread ChunkCache
//   fast5_hdf5.h    superblock, object headers, groups, heaps, B-trees, attributes
//   fast5_signal.h  the Signal dataset: layouts, chunk indexes, decoded or piece by piece as stored
//   fast5_file.h    Fast5: the reads of a file, their ids, Signals and metadata
//   fast5_write.h   one-read files written (h5w) and placed without overwriting
//   fast5_pools.h   worker threads, sample buffers, the timing switch
//   fast5_batch.h   f5_batch and what the loaders share in filling one
//   fast5_stream.h  f5_stream
// and here the status codes' strings, the argument checks and the extern "C" functions.
#include "../../include/deepbinner_fast5.h"

#include "fast5_stream.h"
#include "fast5_write.h"

// The ABI's two handles: global names for what lives in this unit's anonymous namespace.  They
// are defined HERE, not in a header: a struct of external linkage with a member or a base from the
// anonymous namespace is what -Wsubobject-linkage warns about anywhere but in the main file.  So
// the stream's body is Stream (fast5_stream.h), f5_stream adds nothing to it, and Stream::open
// takes the handle's type to make one.  Stream has no virtual destructor: a stream is deleted
// through f5_stream* only (f5_stream_close).
struct f5_file {
    Fast5 impl;
    explicit f5_file(const char* path) : impl(path) {}
};
struct f5_stream : Stream {};

extern "C" {

const char* f5_version(void) { return "deepbinner_fast5 0.1"; }

int f5_vbz_decode(const uint8_t* chunk, int64_t chunk_bytes, const uint32_t* cd, int n_cd,
                  int64_t max_samples, int16_t* out, int64_t* n_samples) {
    if ((!chunk && chunk_bytes) || chunk_bytes < 0 || (!cd && n_cd) || n_cd < 0 || max_samples < 0 ||
        (!out && max_samples) || !n_samples)
        return F5_ERR_ARGUMENT;
    *n_samples = 0;
    const std::vector<uint32_t> values(cd, cd + n_cd);
    if (!vbz_accepted(values) || (vbz_zstd(values) && !libzstd().usable())) return F5_ERR_FILTER;
    std::vector<uint8_t> samples, tmp;
    const int rc = guarded([&] {
        vbz_decode(chunk, (size_t)chunk_bytes, values, (size_t)max_samples * 2, &samples, &tmp);
    });
    if (rc != F5_OK) return rc;
    if (!samples.empty()) std::memcpy(out, samples.data(), samples.size());
    *n_samples = (int64_t)samples.size() / 2;
    return F5_OK;
}

int f5_usable_cpus(void) { return usable_cpus(); }

const char* f5_status_string(int status) {
    switch (status) {
        case F5_OK: return "ok";
        case F5_ERR_OPEN: return "cannot open file";
        case F5_ERR_FORMAT: return "not a readable HDF5/fast5 file";
        case F5_ERR_NO_READ: return "no such read (or read without read_id / Signal)";
        case F5_ERR_MULTI: return "multi-read fast5 file";
        case F5_ERR_ARGUMENT: return "invalid argument";
        case F5_ERR_FILTER: return "Signal compressed with an unsupported filter (VBZ?)";
        case F5_ERR_EXISTS: return "a file of that name exists already (not overwritten)";
        default: return "unknown status";
    }
}

int f5_open(const char* path, f5_file** out) {
    if (!path || !out) return F5_ERR_ARGUMENT;
    *out = nullptr;
    f5_file* file = nullptr;
    const int rc = guarded([&] {
        file = new f5_file(path);
        file->impl.parse();
    });
    if (rc != F5_OK) {
        delete file;
        return rc;
    }
    *out = file;
    return F5_OK;
}

void f5_close(f5_file* file) { delete file; }

int f5_layout(f5_file* file, int* layout, int64_t* n_reads) {
    if (!file || !layout || !n_reads) return F5_ERR_ARGUMENT;
    *layout = file->impl.layout();
    *n_reads = file->impl.n_reads();
    return F5_OK;
}

int f5_read_info(f5_file* file, int64_t index, char read_id[F5_READ_ID_MAX], int64_t* n_samples) {
    if (!file || !read_id || !n_samples) return F5_ERR_ARGUMENT;
    return guarded([&] {
        const ReadEntry& r = file->impl.read(index);
        copy_read_id(r.read_id, read_id);
        *n_samples = r.signal.n;
    });
}

int f5_read_signal(f5_file* file, int64_t index, int64_t first, int64_t count, int16_t* out) {
    if (!file || (!out && count > 0)) return F5_ERR_ARGUMENT;
    return guarded([&] { file->impl.read_signal(file->impl.read(index).signal, first, count, out); });
}

int f5_load_batch(const char* const* paths, int64_t n_files, int64_t keep, int n_threads,
                  f5_batch** out) {
    if (!paths || !out || n_files < 0) return F5_ERR_ARGUMENT;
    *out = nullptr;
    f5_batch* batch = nullptr;
    try {
        batch = new_batch(n_files);
        // Pass 1, per file and entirely on one worker thread: read the file into the thread's
        // buffer, parse it, inflate what is asked for into a staging block of its own.  Pass 2,
        // after a prefix sum of the lengths: copy the staging blocks into the packed buffer.
        // (Keeping the parsed files from a first pass to a second one cost an mmap-sized
        // allocation per file; the extra copy of 13-26 KB per read is nothing beside it.)
        std::vector<std::unique_ptr<int16_t[]>> staged((size_t)n_files);
        std::vector<int64_t> lengths((size_t)n_files, 0);

        auto load_one = [&](int64_t i) {
            const bool ok = load_one_read_file(paths[i], batch, i, [&](Fast5& file, const ReadEntry& r,
                                                                      ChunkCache* cache) {
                const int64_t kept = kept_length(r.signal.n, keep);
                std::unique_ptr<int16_t[]> block(new int16_t[(size_t)std::max<int64_t>(kept, 1)]);
                read_ends(file, r.signal, keep, block.get(), cache);
                lengths[(size_t)i] = kept;
                staged[(size_t)i] = std::move(block);
            });
            if (!ok) lengths[(size_t)i] = 0;
        };
        auto pack_one = [&](int64_t i) {
            if (!staged[(size_t)i]) return;
            std::memcpy(batch->samples.data() + batch->offsets[(size_t)i], staged[(size_t)i].get(),
                        (size_t)lengths[(size_t)i] * 2);
            staged[(size_t)i].reset();
        };

        const int threads = team_size(n_threads, n_files);
        auto run_parallel = [&](const std::function<void(int64_t)>& fn) {
            worker_pool().run(threads, n_files, [&](int64_t i, int) { fn(i); });
        };

        run_parallel(load_one);
        batch->samples.resize((size_t)place_reads(batch, lengths));
        run_parallel(pack_one);
    } catch (const std::exception&) {
        delete batch;
        return F5_ERR_OPEN;
    }
    *out = batch;
    return F5_OK;
}

// One-read files with their Signals AS STORED (the one-read twin of f5_stream_open_raw's
// batches): pass 1, per file on one worker thread, reads and parses the file and stages its
// Signal pieces' bytes; then the host's share of the inflating is chosen over the whole batch;
// pass 2 copies - or, for the host's share, inflates - the staged bytes into the batch's byte
// buffer.
int f5_load_batch_raw(const char* const* paths, int64_t n_files, int n_threads,
                      int64_t host_inflate_above, f5_batch** out) {
    return f5_load_batch_raw_ex(paths, n_files, n_threads, host_inflate_above, 0u, out);
}

int f5_load_batch_raw_ex(const char* const* paths, int64_t n_files, int n_threads,
                         int64_t host_inflate_above, unsigned flags, f5_batch** out) {
    RawOptions options;
    if (!paths || !out || n_files < 0 || !raw_options(host_inflate_above, flags, &options))
        return F5_ERR_ARGUMENT;
    *out = nullptr;
    f5_batch* batch = nullptr;
    try {
        batch = new_batch(n_files);
        std::vector<StagedRead> staged((size_t)n_files);

        auto stage_one = [&](int64_t i) {
            StagedRead& st = staged[(size_t)i];
            const bool ok = load_one_read_file(paths[i], batch, i, [&](Fast5& file, const ReadEntry& r,
                                                                      ChunkCache* cache) {
                st.samples = r.signal.n;
                file.signal_pieces(r.signal, options, &st.pieces);
                for (Fast5::RawPiece& p : st.pieces) {
                    // what the piece will occupy is what is staged of it - except of a VBZ chunk
                    // (the stored chunk) and of a piece decoded here and now, stored from here on
                    const size_t at = st.bytes.size();
                    if (p.kind == Fast5::kHostDecode) {
                        st.bytes.resize(at + (size_t)p.count * 2);
                        file.decode_piece(r.signal, p, reinterpret_cast<uint8_t*>(&st.bytes[at]), cache);
                        p.kind = Fast5::kStored;
                        p.nbytes = (uint64_t)p.count * 2;
                    } else if (p.kind != Fast5::kZeros) {
                        const uint64_t take = p.kind == Fast5::kVbz ? p.nbytes
                                                                    : (uint64_t)(raw_piece_bytes(p) - p.prefix);
                        st.bytes.resize(at + (size_t)take);
                        file.read_bytes(p.file_off, take, reinterpret_cast<uint8_t*>(&st.bytes[at]));
                    }
                    p.file_off = at;
                }
            });
            if (!ok) st = StagedRead();
        };
        const int threads = team_size(n_threads, n_files);
        worker_pool().run(threads, n_files, [&](int64_t i, int) { stage_one(i); });

        // (kHostDecode from here on = "inflate the staged stream")
        if (options.host_share > 0) take_host_share(&staged, options.host_share);
        int64_t samples = 0, at = 0;
        size_t n_pieces = 0;
        for (int64_t i = 0; i < n_files; ++i) {
            batch->offsets[(size_t)i] = samples;
            samples += staged[(size_t)i].samples;
            n_pieces += staged[(size_t)i].pieces.size();
        }
        batch->offsets[(size_t)n_files] = samples;
        batch->streams.reserve(n_pieces);
        for (int64_t i = 0; i < n_files; ++i) place_pieces(batch, i, &staged[(size_t)i].pieces, &at);
        finish_raw_batch(batch, at);
        uint8_t* comp = reinterpret_cast<uint8_t*>(batch->comp.data());
        std::vector<int32_t> inflate_failed((size_t)n_files, 0);
        worker_pool().run(threads, n_files, [&](int64_t i, int) {
            thread_local ChunkCache cache;
            thread_local std::vector<uint8_t> tmp;
            const StagedRead& st = staged[(size_t)i];
            for (const Fast5::RawPiece& p : st.pieces) {
                const uint8_t* src = reinterpret_cast<const uint8_t*>(st.bytes.data()) + p.file_off;
                uint8_t* dst = comp + p.comp_offset;
                if (p.kind == Fast5::kVbz && p.vbz_zstd) {
                    // zstd on the host, the streamvbyte stage on the GPU
                    const int rc = guarded([&] { vbz_host_stage(src, p, dst); });
                    if (rc != F5_OK) {
                        std::memset(dst, 0, (size_t)p.comp_bytes);   // (the GPU refuses it too)
                        inflate_failed[(size_t)i] = rc;
                    }
                    continue;
                }
                if (p.kind != Fast5::kHostDecode) {
                    if (p.prefix) put_u32le(dst, (uint32_t)(p.count * 2));
                    std::memcpy(dst + p.prefix, src, (size_t)p.comp_bytes - (size_t)p.prefix);
                    continue;
                }
                const int rc = guarded([&] {
                    inflate_stream(src, (size_t)p.nbytes, (size_t)p.count * 2 + 8, &tmp, &cache);
                    if (p.prefix) {                    // a shuffled stream: its halves meet at count
                        if (tmp.size() != (size_t)p.count * 2)
                            throw FormatError("shuffled chunk of another size than its samples");
                        unshuffle(&tmp, 2, &cache.scratch);
                    }
                });
                const size_t have = rc == F5_OK ? std::min(tmp.size(), (size_t)p.count * 2) : 0;
                if (have) std::memcpy(dst, tmp.data(), have);
                std::memset(dst + have, 0, (size_t)p.count * 2 - have);
                if (rc != F5_OK) inflate_failed[(size_t)i] = rc;
            }
        });
        for (int64_t i = 0; i < n_files; ++i)
            if (inflate_failed[(size_t)i]) fail_read(batch, i, inflate_failed[(size_t)i]);
    } catch (const std::exception&) {
        delete batch;
        return F5_ERR_OPEN;
    }
    *out = batch;
    return F5_OK;
}

int f5_load_reads(const char* path, int64_t first, int64_t count, int64_t keep, int n_threads,
                  f5_batch** out) {
    if (!path || !out || first < 0) return F5_ERR_ARGUMENT;
    *out = nullptr;
    f5_batch* batch = nullptr;
    try {
        // ONE reader for all worker threads: the file is opened and its root group parsed once;
        // pass 1 resolves the reads (every read by exactly one thread, each touching only its
        // own entry), after which the reader is read-only and pass 2 needs per-thread state only
        // for the chunk inflated last.  Two passes like f5_load_batch: lengths, prefix sum,
        // inflate into place.
        PhaseClock clock(PhaseClock::env());      // open+parse, resolve, allocate, inflate
        clock.mark(0);
        std::unique_ptr<Fast5> shared;
        const int open_status = guarded([&] {
            shared.reset(new Fast5(path));
            shared->parse();
        });
        if (open_status != F5_OK) return open_status;
        if (count < 0) count = std::max<int64_t>(shared->n_reads() - first, 0);   // to the end
        if (first + count > shared->n_reads()) return F5_ERR_NO_READ;
        const int threads = team_size(n_threads, count);
        std::vector<ChunkCache> caches((size_t)threads);
        clock.mark(1);

        batch = new_batch(count);
        std::vector<int64_t> lengths((size_t)count, 0);
        worker_pool().run(threads, count, [&](int64_t i, int) {
            resolve_reads(*shared, first, keep, batch, &lengths, i, i + 1, [](const ReadEntry&, int64_t) {});
        });
        clock.mark(2);
        batch->samples.resize((size_t)place_reads(batch, lengths));
        clock.mark(3);
        worker_pool().run(threads, count, [&](int64_t i, int slot) {
            inflate_reads(*shared, first, keep, batch, lengths, i, i + 1, &caches[(size_t)slot]);
        });
        clock.mark(4);
        clock.report("allocate", "inflate", "f5_load_reads: %lld reads, %d threads", (long long)count,
                     threads);
    } catch (const std::exception&) {
        delete batch;
        return F5_ERR_OPEN;
    }
    *out = batch;
    return F5_OK;
}

int f5_write_single_reads(const char* container, int64_t n, const int64_t* read_index,
                          const char* const* out_paths, int n_threads, int32_t* status,
                          int64_t* bytes_written) {
    if (bytes_written) *bytes_written = 0;
    if (!container || n < 0 || (n > 0 && (!read_index || !out_paths || !status)))
        return F5_ERR_ARGUMENT;
    if (n == 0) return F5_OK;
    try {
        std::unique_ptr<Fast5> shared;
        const int open_status = guarded([&] {
            shared.reset(new Fast5(container));
            shared->parse();
        });
        if (open_status != F5_OK) return open_status;
        // pass 1: every wanted read of the container resolved by exactly one thread (a read asked
        // for twice must not be resolved by two at once); from then on the reader is read-only
        std::vector<int64_t> wanted(read_index, read_index + n);
        std::sort(wanted.begin(), wanted.end());
        wanted.erase(std::unique(wanted.begin(), wanted.end()), wanted.end());
        const int threads = team_size(n_threads, n);
        worker_pool().run(threads, (int64_t)wanted.size(), [&](int64_t k, int) {
            (void)guarded([&] { (void)shared->read(wanted[(size_t)k]); });
        });
        std::vector<ChunkCache> caches((size_t)threads);
        std::atomic<int64_t> written(0);
        worker_pool().run(threads, n, [&](int64_t i, int slot) {
            status[i] = guarded([&] {
                if (!out_paths[i]) throw std::out_of_range("no path");
                // (its read is resolved: the reader is read-only now)
                const std::string image =
                    single_read_image(*shared, read_index[i], true, &caches[(size_t)slot]);
                place_new_file(out_paths[i], image, i);
                written.fetch_add((int64_t)image.size());
            });
        });
        if (bytes_written) *bytes_written = written.load();
    } catch (const std::exception&) {
        return F5_ERR_OPEN;
    }
    return F5_OK;
}

/* the same file as bytes (tests: held against hdf5_write.single_read_fast5_bytes) */
int f5_single_read_image(const char* container, int64_t read_index, uint8_t* out, int64_t capacity,
                         int64_t* size) {
    if (!container || !size || capacity < 0 || (capacity > 0 && !out)) return F5_ERR_ARGUMENT;
    *size = 0;
    return guarded([&] {
        Fast5 file(container);
        file.parse();
        const std::string image = single_read_image(file, read_index, false);
        *size = (int64_t)image.size();
        if ((int64_t)image.size() <= capacity) std::memcpy(out, image.data(), image.size());
    });
}

int64_t f5_batch_size(const f5_batch* batch) { return batch ? (int64_t)batch->status.size() : 0; }
const int16_t* f5_batch_samples(const f5_batch* batch) { return batch ? batch->samples.data() : nullptr; }
const int64_t* f5_batch_offsets(const f5_batch* batch) { return batch ? batch->offsets.data() : nullptr; }
const int32_t* f5_batch_status(const f5_batch* batch) { return batch ? batch->status.data() : nullptr; }
const char* f5_batch_read_ids(const f5_batch* batch) { return batch ? batch->read_ids.data() : nullptr; }
void f5_batch_free(f5_batch* batch) { delete batch; }

int f5_set_sample_allocator(f5_alloc_fn alloc, f5_free_fn release, void* user) {
    if ((alloc == nullptr) != (release == nullptr)) return F5_ERR_ARGUMENT;
    sample_pool().set_allocator(alloc, release, user);
    return F5_OK;
}

void f5_release_idle_buffers(void) { sample_pool().flush(); }

int f5_stream_open(const char* const* paths, int64_t n_paths, int64_t keep, int n_threads,
                   int depth, f5_stream** out) {
    if (!out || n_paths < 0 || (n_paths > 0 && !paths)) return F5_ERR_ARGUMENT;
    *out = nullptr;
    return Stream::open(paths, n_paths, keep, false, RawOptions(), n_threads, depth, out);
}

int f5_stream_open_raw(const char* const* paths, int64_t n_paths, int n_threads, int depth,
                       int64_t host_inflate_above, f5_stream** out) {
    return f5_stream_open_raw_ex(paths, n_paths, n_threads, depth, host_inflate_above, 0u, out);
}

int f5_stream_open_raw_ex(const char* const* paths, int64_t n_paths, int n_threads, int depth,
                          int64_t host_inflate_above, unsigned flags, f5_stream** out) {
    RawOptions options;
    if (!raw_options(host_inflate_above, flags, &options)) return F5_ERR_ARGUMENT;
    if (!out || n_paths < 0 || (n_paths > 0 && !paths)) return F5_ERR_ARGUMENT;
    // A raw container is little work per read (no inflating) behind a serial start (one thread
    // opens and parses it: 5-6 ms of the ~30 ms of CPU a container of 4,000 reads costs): a window
    // of three starves a team of sixteen - 1.2 M reads/s where eight in flight give 1.7 M and
    // sixteen 1.9 M (profiles/r06_loader).  Default: half the team, between 3 and 8.
    if (depth <= 0) depth = std::max(3, std::min(8, thread_count(n_threads) / 2));
    return Stream::open(paths, n_paths, 0, true, options, n_threads, depth, out);
}

const uint8_t* f5_batch_comp(const f5_batch* batch) {
    return batch ? reinterpret_cast<const uint8_t*>(batch->comp.data()) : nullptr;
}
int64_t f5_batch_comp_bytes(const f5_batch* batch) { return batch ? batch->comp_bytes : 0; }
const f5_raw_stream* f5_batch_streams(const f5_batch* batch) {
    return batch && !batch->streams.empty() ? batch->streams.data() : nullptr;
}
int64_t f5_batch_n_streams(const f5_batch* batch) {
    return batch ? (int64_t)batch->streams.size() : 0;
}

int f5_stream_next(f5_stream* s, int64_t* index, int* container_status, f5_batch** batch) {
    if (!s || !index || !container_status || !batch) return F5_ERR_ARGUMENT;
    *batch = nullptr;
    std::unique_lock<std::mutex> lk(s->m);
    if (s->inflight.empty()) return F5_ERR_NO_READ;       // exhausted
    f5_stream::Container* front = s->inflight.front().get();
    s->done_cv.wait(lk, [&] { return front->phase == f5_stream::kDone; });
    std::unique_ptr<f5_stream::Container> c = std::move(s->inflight.front());
    s->inflight.pop_front();
    s->admit_locked();
    lk.unlock();
    s->work_cv.notify_all();
    *index = c->index;
    *container_status = c->status;
    if (c->status == F5_OK) {
        *batch = c->batch;
        c->batch = nullptr;
    }
    return F5_OK;
}

void f5_stream_close(f5_stream* s) { delete s; }

}  // extern "C"
