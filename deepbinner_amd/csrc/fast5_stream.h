// fast5_stream.h - multi-read containers in, batches out, several containers in flight.
#ifndef DEEPBINNER_FAST5_STREAM_H
#define DEEPBINNER_FAST5_STREAM_H

#include <pthread.h>

#include <climits>
#include <deque>

#include "fast5_batch.h"

namespace {

// ---------------------------------------------------------------------------------------------
// f5_stream: multi-read containers in, packed batches out, SEVERAL containers in flight.
// One f5_load_reads call per container leaves most of a many-core host idle most of the time:
// opening a 4,000-read container and walking its root group is 6-10 ms on ONE thread, the reads
// are resolved and inflated in two passes with a join after each, and the caller's own work per
// batch happens while nothing loads.  Here a team of threads works on a window of `depth`
// containers at once, always taking the oldest work there is: read ranges of a container that is
// being inflated, else ranges of one being resolved, else a container that still has to be opened -
// so that the next containers' serial parts run beside the current one's inflating, and the batches
// still come out in path order.
// ---------------------------------------------------------------------------------------------
struct Stream {
    enum Phase { kNew, kParsing, kResolve, kLayout, kInflate, kDone };
    struct Container {
        int64_t index = 0;
        std::string path;
        std::unique_ptr<Fast5> file;
        int status = F5_OK;                 // why the container could not be opened / laid out
        Phase phase = kNew;
        int64_t count = 0, next = 0, done = 0;
        f5_batch* batch = nullptr;
        std::vector<int64_t> lengths;
        std::vector<std::vector<Fast5::RawPiece>> pieces;      // raw mode: per read
        std::vector<int64_t> fetch_order;   // raw mode: the reads by where their Signal lies in the file
        PhaseClock clock{PhaseClock::env_once()};      // open+parse, resolve, layout, inflate or fetch
        ~Container() { delete batch; }
    };
    struct Task {
        Container* c = nullptr;
        Phase phase = kNew;
        int64_t a = 0, b = 0;
    };

    // (set by open(), before any worker starts)
    std::vector<std::string> paths;
    int64_t keep = 0;                // packed mode; 0 in raw mode
    int depth = 3;
    bool raw = false;                // hand out the Signal pieces as stored (f5_stream_open_raw)
    RawOptions options;              // ... in this way
    static constexpr int64_t kLongStreamBytes = 64 * 1024;
    std::mutex m;
    std::condition_variable work_cv, done_cv;
    std::deque<std::unique_ptr<Container>> inflight;      // in path order
    int64_t next_path = 0;
    bool stop = false;
    std::vector<std::thread> workers;

    static constexpr int64_t kInflateGrain = 8, kResolveGrain = 64, kFetchGrain = 256;

    // The one way to a stream, packed (raw = false: keep counts) or raw (options count): paths,
    // mode and options are in place before the team of n_threads starts.  depth <= 0: 3.
    // Handle: the ABI's f5_stream, which is this struct under a name of external linkage.
    template <class Handle>
    static int open(const char* const* paths, int64_t n_paths, int64_t keep, bool raw,
                    const RawOptions& options, int n_threads, int depth, Handle** out) {
        for (int64_t i = 0; i < n_paths; ++i)
            if (!paths[i]) return F5_ERR_ARGUMENT;
        Handle* s = nullptr;
        try {
            s = new Handle;
            s->paths.assign(paths, paths + n_paths);
            s->keep = keep;
            s->raw = raw;
            s->options = options;
            s->depth = depth > 0 ? std::min(depth, 64) : 3;
            {
                std::lock_guard<std::mutex> g(s->m);
                s->admit_locked();
            }
            const int threads = thread_count(n_threads);
            for (int t = 0; t < threads; ++t) s->workers.emplace_back([s] { s->worker(); });
        } catch (const std::exception&) {
            delete s;
            return F5_ERR_OPEN;
        }
        *out = s;
        return F5_OK;
    }

    ~Stream() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        work_cv.notify_all();
        for (std::thread& t : workers) t.join();
    }

    void admit_locked() {
        while ((int)inflight.size() < depth && next_path < (int64_t)paths.size()) {
            std::unique_ptr<Container> c(new Container);
            c->index = next_path;
            c->path = paths[(size_t)next_path++];
            inflight.push_back(std::move(c));
        }
    }

    bool pick_locked(Task* t) {
        for (auto& up : inflight) {
            Container* c = up.get();
            if ((c->phase == kInflate || c->phase == kResolve) && c->next < c->count) {
                const int64_t grain = c->phase != kInflate ? kResolveGrain : raw ? kFetchGrain : kInflateGrain;
                t->c = c;
                t->phase = c->phase;
                t->a = c->next;
                t->b = std::min(c->count, c->next + grain);
                c->next = t->b;
                return true;
            }
        }
        for (auto& up : inflight) {
            Container* c = up.get();
            if (c->phase == kNew) {
                c->phase = kParsing;
                t->c = c;
                t->phase = kParsing;
                return true;
            }
        }
        return false;
    }

    void parse(Container* c) {
        c->clock.mark(0);
        c->status = guarded([&] {
            c->file.reset(new Fast5(c->path.c_str()));
            c->file->parse();
        });
        if (c->status == F5_OK) {
            c->count = c->file->n_reads();
            try {
                c->batch = new_batch(c->count);
                c->lengths.assign((size_t)c->count, 0);
                if (raw) c->pieces.resize((size_t)c->count);
            } catch (const std::exception&) {
                c->status = F5_ERR_FORMAT;
            }
        }
        c->clock.mark(1);
    }

    void resolve(Container* c, int64_t a, int64_t b) {
        resolve_reads(*c->file, 0, keep, c->batch, &c->lengths, a, b, [&](const ReadEntry& r, int64_t i) {
            if (raw) c->file->signal_pieces(r.signal, options, &c->pieces[(size_t)i]);
        });
    }

    // The host's share of a CONTAINER's inflating: with options.host_share > 0 the longest deflate
    // streams holding that share (per cent) of the container's compressed bytes are left to the
    // host's threads - long streams are what a CPU core is good at (a stream is one lane's work on
    // the GPU however long it is) and what is left for the GPU is of even length.  Unlike the rule
    // for a batch of one-read files (take_host_share in fast5_batch.h) it takes EVERY stream at or above a
    // cut - the length of the last stream that still counted towards the share, all its equals
    // with it - and none at all from a container of long streams.  Such a piece loses its prefix:
    // the fetch pass decodes it from the file (Fast5::decode_piece), shuffle and all.
    void take_host_share(Container* c) {
        std::vector<int64_t> sizes;
        int64_t all = 0;
        for (int64_t i = 0; i < c->count; ++i)
            if (c->batch->status[(size_t)i] == F5_OK)
                for (const Fast5::RawPiece& p : c->pieces[(size_t)i])
                    if (p.kind == Fast5::kZlib) {
                        sizes.push_back((int64_t)p.nbytes);
                        all += (int64_t)p.nbytes;
                    }
        std::sort(sizes.begin(), sizes.end(), std::greater<int64_t>());
        int64_t cut = INT64_MAX, taken = 0;
        // ... of a container of ORDINARY reads.  Where the streams are long throughout
        // (mean above kLongStreamBytes: reads of ~50 k samples and more) the host keeps
        // none: a 200 KB stream is 0.6 ms of a core, and with a wavefront per stream the GPU
        // decodes such containers alone at 134 k reads/s where a fifth of the bytes on the
        // host's sixteen threads made it 54 k (profiles/r06_loader).
        const bool long_streams = !sizes.empty() && all / (int64_t)sizes.size() > kLongStreamBytes;
        for (int64_t v : sizes) {
            if (long_streams || taken * 100 >= all * options.host_share) break;
            taken += v;
            cut = v;
        }
        for (int64_t i = 0; i < c->count; ++i)
            if (c->batch->status[(size_t)i] == F5_OK)
                for (Fast5::RawPiece& p : c->pieces[(size_t)i])
                    if (p.kind == Fast5::kZlib && (int64_t)p.nbytes >= cut) {
                        p.kind = Fast5::kHostDecode;
                        p.prefix = 0;
                    }
    }

    void layout(Container* c) {
        c->clock.mark(2);
        struct MarkEnd {
            Container* c;
            ~MarkEnd() { c->clock.mark(3); }
        } mark_end{c};
        const int64_t total = place_reads(c->batch, c->lengths);
        try {
            if (!raw) {
                c->batch->samples.resize((size_t)total);
                return;
            }
            if (options.host_share > 0) take_host_share(c);
            // raw: every piece gets its place in the byte buffer and its record
            int64_t at = 0;
            size_t n_pieces = 0;
            for (int64_t i = 0; i < c->count; ++i)
                if (c->batch->status[(size_t)i] == F5_OK) n_pieces += c->pieces[(size_t)i].size();
            c->batch->streams.reserve(n_pieces);
            for (int64_t i = 0; i < c->count; ++i)
                if (c->batch->status[(size_t)i] == F5_OK) place_pieces(c->batch, i, &c->pieces[(size_t)i], &at);
            finish_raw_batch(c->batch, at);
            // the fetch pass walks the reads in FILE order (groups are listed by name - random
            // read ids - but written one after the other): neighbours in a task are neighbours in
            // the file, and Fast5::read_many reads them together
            c->fetch_order.resize((size_t)c->count);
            for (int64_t i = 0; i < c->count; ++i) c->fetch_order[(size_t)i] = i;
            {
                std::vector<uint64_t> where((size_t)c->count, ~0ull);
                for (int64_t i = 0; i < c->count; ++i)
                    if (c->batch->status[(size_t)i] == F5_OK)
                        for (const Fast5::RawPiece& p : c->pieces[(size_t)i])
                            if (p.kind == Fast5::kZlib || p.kind == Fast5::kStored ||
                                p.kind == Fast5::kVbz) {
                                where[(size_t)i] = p.file_off;
                                break;
                            }
                std::sort(c->fetch_order.begin(), c->fetch_order.end(),
                          [&](int64_t x, int64_t y) { return where[(size_t)x] < where[(size_t)y]; });
            }
        } catch (const std::exception&) {
            c->status = F5_ERR_FORMAT;
        }
    }

    // raw mode's pass 2: the pieces of the reads at places [a, b) of the container's fetch order
    // into the byte buffer - the stored ones together (Fast5::read_many), then what the host decodes
    void fetch(Container* c, int64_t a, int64_t b) {
        thread_local ChunkCache cache;
        thread_local std::vector<Fast5::IoItem> items;
        thread_local std::vector<char> failed;
        thread_local std::vector<uint8_t> vbz_chunk;
        uint8_t* comp = reinterpret_cast<uint8_t*>(c->batch->comp.data());
        auto fail = [&](int64_t i, int rc) {
            // what could not be fetched or decoded reads as nothing: a stored stream of no
            // bytes is zero-extended by the decoder; the read is marked
            for (f5_raw_stream& rec : c->batch->streams)
                if (rec.reserved == (int32_t)i) {
                    rec.mode = F5_RAW_STORED;
                    rec.comp_bytes = 0;
                }
            fail_read(c->batch, i, rc);
        };
        items.clear();
        for (int64_t k = a; k < b; ++k) {
            const int64_t i = c->fetch_order[(size_t)k];
            if (c->batch->status[(size_t)i] != F5_OK) continue;
            for (const Fast5::RawPiece& p : c->pieces[(size_t)i])
                if (p.kind == Fast5::kZlib || p.kind == Fast5::kStored ||
                    (p.kind == Fast5::kVbz && !p.vbz_zstd)) {
                    // (a shuffled piece: its size in front, the stored bytes behind it)
                    if (p.prefix) put_u32le(comp + p.comp_offset, (uint32_t)(p.count * 2));
                    items.push_back({p.file_off, (uint64_t)(p.comp_bytes - p.prefix),
                                     comp + p.comp_offset + p.prefix, i});
                }
        }
        const int rc_all = guarded([&] { c->file->read_many(items, &failed); });
        for (size_t k = 0; k < items.size(); ++k)
            if ((rc_all != F5_OK || failed[k]) && c->batch->status[(size_t)items[k].tag] == F5_OK)
                fail(items[k].tag, rc_all != F5_OK ? rc_all : F5_ERR_FORMAT);
        for (int64_t k = a; k < b; ++k) {
            const int64_t i = c->fetch_order[(size_t)k];
            if (c->batch->status[(size_t)i] != F5_OK) continue;
            const int rc = guarded([&] {
                const ReadEntry& r = c->file->read(i);
                for (const Fast5::RawPiece& p : c->pieces[(size_t)i])
                    if (p.kind == Fast5::kHostDecode) {
                        c->file->decode_piece(r.signal, p, comp + p.comp_offset, &cache);
                    } else if (p.kind == Fast5::kVbz && p.vbz_zstd) {
                        // zstd on the host, the streamvbyte stage on the GPU
                        vbz_chunk.resize((size_t)p.nbytes);
                        c->file->read_bytes(p.file_off, p.nbytes, vbz_chunk.data());
                        vbz_host_stage(vbz_chunk.data(), p, comp + p.comp_offset);
                    }
            });
            if (rc != F5_OK) fail(i, rc);
        }
    }

    void inflate(Container* c, int64_t a, int64_t b) {
        thread_local ChunkCache cache;
        inflate_reads(*c->file, 0, keep, c->batch, c->lengths, a, b, &cache);
    }

    void finish(Container* c) {      // no read of it is being worked on any more
        c->clock.mark(4);      // (a read that failed lost its id where it failed: fail_read)
        c->clock.report("layout", c->pieces.empty() ? "inflate" : "fetch",
                        "f5_stream: container %lld, %lld reads", (long long)c->index, (long long)c->count);
        c->file.reset();             // unmap and close now, not when the caller frees the batch
    }

    void worker() {
        // (a name an operator - and tools/gpu_inflate_split.py's CPU accounting - can tell from the
        // interpreter's and the GPU runtime's threads)
        pthread_setname_np(pthread_self(), "f5-stream");
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            Task t;
            while (!stop && !pick_locked(&t)) work_cv.wait(lk);
            if (stop) return;
            Container* c = t.c;
            lk.unlock();
            if (t.phase == kParsing) parse(c);
            else if (t.phase == kResolve) resolve(c, t.a, t.b);
            else if (raw) fetch(c, t.a, t.b);
            else inflate(c, t.a, t.b);
            lk.lock();
            if (t.phase == kParsing) {
                if (c->status != F5_OK) {
                    c->phase = kDone;
                    done_cv.notify_all();
                    continue;
                }
                c->next = c->done = 0;
                c->phase = c->count > 0 ? kResolve : kLayout;
                if (c->count > 0) {
                    work_cv.notify_all();
                    continue;
                }
            } else {
                c->done += t.b - t.a;
                if (c->done < c->count) continue;
                if (t.phase == kInflate) {
                    lk.unlock();
                    finish(c);
                    lk.lock();
                    c->phase = kDone;
                    done_cv.notify_all();
                    continue;
                }
                c->phase = kLayout;
            }
            // the last range of the resolve pass (or an empty container): sizes are known
            lk.unlock();
            layout(c);
            if (c->status == F5_OK && c->count == 0) finish(c);
            lk.lock();
            if (c->status != F5_OK || c->count == 0) {
                c->phase = kDone;
                done_cv.notify_all();
            } else {
                c->next = c->done = 0;
                c->phase = kInflate;
                work_cv.notify_all();
            }
        }
    }
};

}  // namespace

#endif  // DEEPBINNER_FAST5_STREAM_H
