// fast5_pools.h - what the loaders run on: the worker threads that outlive a call, and the
// recycled (pinned) buffers their batches lie in.
#ifndef DEEPBINNER_FAST5_POOLS_H
#define DEEPBINNER_FAST5_POOLS_H

#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/deepbinner_fast5.h"

// Worker threads that outlive the call: a batch of 256 one-read files is 3-4 ms of work, and
// starting and joining 32-64 threads twice per batch was a third of it.  One job at a time; a
// caller that finds the pool busy (several threads in f5_load_batch at once) starts threads of its
// own as before.  The calling thread always works too (slot 0).
class WorkerPool {
  public:
    using Job = std::function<void(int64_t item, int slot)>;

    ~WorkerPool() {
        if (getpid() != owner_) {      // a forked child: the threads exist in the parent only
            for (std::thread& t : workers_) t.detach();
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        wake_.notify_all();
        for (std::thread& t : workers_) t.join();
    }

    // items 0 .. count-1, each exactly once, on up to `threads` threads; slot < threads
    void run(int threads, int64_t count, const Job& job) {
        threads = (int)std::max<int64_t>(1, std::min<int64_t>(threads, count));
        if (threads == 1) {
            for (int64_t i = 0; i < count; ++i) job(i, 0);
            return;
        }
        std::unique_lock<std::mutex> owner(busy_, std::try_to_lock);
        if (!owner.owns_lock() || getpid() != owner_) {
            run_on_new_threads(threads, count, job);
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            while ((int)workers_.size() < threads - 1) {
                const int slot = (int)workers_.size() + 1;
                workers_.emplace_back([this, slot] { worker(slot); });
            }
            job_ = &job;
            count_ = count;
            next_.store(0);
            helpers_ = threads - 1;
            unfinished_ = threads - 1;
            ++generation_;
        }
        wake_.notify_all();
        drain(job, 0);
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return unfinished_ == 0; });
        job_ = nullptr;
    }

  private:
    void drain(const Job& job, int slot) {
        for (int64_t i = next_.fetch_add(1); i < count_; i = next_.fetch_add(1)) {
            try {
                job(i, slot);
            } catch (...) {    // jobs report through their own status fields; never unwind a worker
            }
        }
    }
    void worker(int slot) {
        uint64_t seen = 0;
        for (;;) {
            const Job* job = nullptr;
            {
                std::unique_lock<std::mutex> g(m_);
                wake_.wait(g, [&] { return stop_ || (generation_ != seen && slot <= helpers_); });
                if (stop_) return;
                seen = generation_;
                job = job_;
            }
            drain(*job, slot);
            {
                std::lock_guard<std::mutex> g(m_);
                --unfinished_;
            }
            done_.notify_one();
        }
    }
    static void run_on_new_threads(int threads, int64_t count, const Job& job) {
        std::atomic<int64_t> next(0);
        auto body = [&](int slot) {
            for (int64_t i = next.fetch_add(1); i < count; i = next.fetch_add(1)) job(i, slot);
        };
        std::vector<std::thread> extra;
        for (int t = 1; t < threads; ++t) extra.emplace_back(body, t);
        body(0);
        for (std::thread& t : extra) t.join();
    }

    const pid_t owner_ = getpid();
    std::mutex busy_, m_;
    std::condition_variable wake_, done_;
    std::vector<std::thread> workers_;
    const Job* job_ = nullptr;
    int64_t count_ = 0;
    std::atomic<int64_t> next_{0};
    int helpers_ = 0, unfinished_ = 0;
    uint64_t generation_ = 0;
    bool stop_ = false;
};

// How many hardware threads this process may really keep busy: the online CPUs, cut down to the
// scheduler's affinity mask and to the cgroup's CPU quota (cpu.max of cgroup v2, cfs_quota_us of
// v1).  A container that shows 256 CPUs with a quota of 16 runs a 128-thread team SLOWER than a
// 16-thread one - every thread beyond the quota only adds throttling stalls
// (profiles/r03_cpu_capacity.txt).
int usable_cpus() {
    static const int n = [] {
        int cpus = (int)std::thread::hardware_concurrency();
        if (cpus < 1) cpus = 1;
        cpu_set_t mask;
        if (sched_getaffinity(0, sizeof(mask), &mask) == 0) {
            const int allowed = CPU_COUNT(&mask);
            if (allowed > 0) cpus = std::min(cpus, allowed);
        }
        long long quota = -1, period = -1;
        if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char first[32] = {0};
            if (std::fscanf(f, "%31s %lld", first, &period) == 2 && std::strcmp(first, "max") != 0)
                quota = std::atoll(first);
            std::fclose(f);
        } else {
            if (FILE* q = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
                if (std::fscanf(q, "%lld", &quota) != 1) quota = -1;
                std::fclose(q);
            }
            if (FILE* p = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (std::fscanf(p, "%lld", &period) != 1) period = -1;
                std::fclose(p);
            }
        }
        if (quota > 0 && period > 0)
            cpus = std::min<long long>(cpus, std::max<long long>(1, (quota + period - 1) / period));
        return cpus;
    }();
    return n;
}

// n_threads as the ABI takes it: <= 0 = one per usable hardware thread, at most 64; an explicit
// count is honoured up to 256
int thread_count(int n_threads) {
    if (n_threads > 0) return std::min(n_threads, 256);
    return std::max(1, std::min(usable_cpus(), 64));
}
// ... and no more threads than there are items to work on
int team_size(int n_threads, int64_t items) {
    return (int)std::min<int64_t>(thread_count(n_threads), std::max<int64_t>(items, 1));
}

WorkerPool& worker_pool() {
    static WorkerPool pool;
    return pool;
}

// Packed samples of a batch.  Deliberately NOT value-initialised (a std::vector would zero 100+ MB
// on the calling thread before the workers start), and RECYCLED: a 4,000-read container's scanned
// ends are 106 MB, and a fresh allocation of that size is an mmap whose 26,000 pages are then
// faulted in by the worker threads one by one and unmapped again when the batch is freed.  Freed buffers wait in a pool (bounded: DEEPBINNER_FAST5_POOL_MB, default 2048)
// for the next batch that fits.  The memory comes from malloc or from an allocator the caller
// installs (f5_set_sample_allocator) - pinned host memory, so that the GPU's DMA engine reads the
// batch where the loader threads wrote it.
struct SampleAllocator {
    f5_alloc_fn alloc = nullptr;
    f5_free_fn release = nullptr;
    void* user = nullptr;
    uint64_t generation = 0;
};

class SamplePool {
  public:
    struct Block {
        void* ptr = nullptr;
        size_t bytes = 0;
        SampleAllocator from;
    };
    ~SamplePool() { flush(); }

    void set_allocator(f5_alloc_fn alloc, f5_free_fn release, void* user) {
        std::vector<Block> old;
        {
            std::lock_guard<std::mutex> g(m_);
            allocator_.alloc = alloc;
            allocator_.release = release;
            allocator_.user = user;
            ++allocator_.generation;
            old.swap(idle_);
            idle_bytes_ = 0;
        }
        for (Block& b : old) free_block(b);
    }

    Block take(size_t bytes) {
        if (bytes == 0) return Block();
        SampleAllocator from;
        {
            std::lock_guard<std::mutex> g(m_);
            // best fit among the idle blocks; one that is far too large stays for a larger batch
            size_t best = idle_.size();
            for (size_t i = 0; i < idle_.size(); ++i)
                if (idle_[i].bytes >= bytes && idle_[i].bytes / 4 <= bytes + (1u << 20) &&
                    (best == idle_.size() || idle_[i].bytes < idle_[best].bytes))
                    best = i;
            if (best != idle_.size()) {
                Block b = idle_[best];
                idle_.erase(idle_.begin() + (std::ptrdiff_t)best);     // (the front stays the oldest)
                idle_bytes_ -= b.bytes;
                return b;
            }
            from = allocator_;
        }
        // more than asked for: the next container is about, not exactly, as large - and a fresh
        // buffer costs its page faults (3-4 times the copy that fills it)
        Block b;
        b.bytes = (bytes + bytes / 4 + (1u << 20)) & ~(size_t)((1u << 20) - 1);
        b.from = from;
        b.ptr = from.alloc ? from.alloc(b.bytes, from.user) : std::malloc(b.bytes);
        if (!b.ptr) throw std::bad_alloc();
        return b;
    }

    void give(Block b) {
        if (!b.ptr) return;
        // The block just used is the size the caller needs NOW: it stays, and the blocks that
        // have waited longest go if the pool is over its limit (a pool full of another
        // workload's sizes would otherwise never serve a request nor take a block back - every
        // batch a fresh allocation and a free, and freeing pinned memory waits for the GPU).
        std::vector<Block> evicted;
        {
            std::lock_guard<std::mutex> g(m_);
            if (b.from.generation == allocator_.generation && b.bytes <= limit()) {
                idle_.push_back(b);
                idle_bytes_ += b.bytes;
                b = Block();
                size_t n = 0;
                while (idle_bytes_ > limit() && n + 1 < idle_.size()) {
                    idle_bytes_ -= idle_[n].bytes;
                    evicted.push_back(idle_[n++]);
                }
                idle_.erase(idle_.begin(), idle_.begin() + (std::ptrdiff_t)n);
            }
        }
        for (Block& old : evicted) free_block(old);
        free_block(b);
    }

    void flush() {
        std::vector<Block> old;
        {
            std::lock_guard<std::mutex> g(m_);
            old.swap(idle_);
            idle_bytes_ = 0;
        }
        for (Block& b : old) free_block(b);
    }

  private:
    static void free_block(Block& b) {
        if (!b.ptr) return;
        if (b.from.release) b.from.release(b.ptr, b.from.user);
        else if (!b.from.alloc) std::free(b.ptr);
        b.ptr = nullptr;
    }
    static size_t limit() {
        static const size_t bytes = [] {
            const char* mb = std::getenv("DEEPBINNER_FAST5_POOL_MB");
            const long v = mb ? std::atol(mb) : 2048;
            return (size_t)(v < 0 ? 0 : v) << 20;
        }();
        return bytes;
    }
    std::mutex m_;
    std::vector<Block> idle_;
    size_t idle_bytes_ = 0;
    SampleAllocator allocator_;
};

SamplePool& sample_pool() {
    static SamplePool* pool = new SamplePool;      // never destroyed: batches may outlive exit()
    return *pool;
}

struct SampleBuffer {
    SamplePool::Block block;
    size_t count = 0;
    SampleBuffer() = default;
    SampleBuffer(const SampleBuffer&) = delete;
    SampleBuffer& operator=(const SampleBuffer&) = delete;
    ~SampleBuffer() { sample_pool().give(block); }
    void resize(size_t n) {
        sample_pool().give(block);
        block = SamplePool::Block();
        block = sample_pool().take(n * sizeof(int16_t));
        count = n;
    }
    int16_t* data() const { return static_cast<int16_t*>(block.ptr); }
};

// DEEPBINNER_FAST5_TIMING: a load's four phases - open+parse, resolve, a third and a fourth - stamped
// at their five borders and written to stderr, one line per load.  f5_load_reads asks for the
// variable at every call (env), the stream once per process (env_once).
struct PhaseClock {
    static bool env() { return std::getenv("DEEPBINNER_FAST5_TIMING") != nullptr; }
    static bool env_once() {
        static const bool on = env();
        return on;
    }
    const bool on;
    std::chrono::steady_clock::time_point stamp[5];
    explicit PhaseClock(bool on) : on(on) {}
    void mark(int k) {
        if (on) stamp[k] = std::chrono::steady_clock::now();
    }
    // "<what>: open+parse .. ms, resolve .. ms, <third> .. ms, <fourth> .. ms"; what: as for printf
    __attribute__((format(printf, 4, 5)))
    void report(const char* third, const char* fourth, const char* what, ...) const {
        if (!on) return;
        auto ms = [&](int a) {
            return std::chrono::duration<double, std::milli>(stamp[a + 1] - stamp[a]).count();
        };
        char head[128];
        va_list args;
        va_start(args, what);
        std::vsnprintf(head, sizeof(head), what, args);
        va_end(args);
        std::fprintf(stderr, "%s: open+parse %.1f ms, resolve %.1f ms, %s %.1f ms, %s %.1f ms\n", head,
                     ms(0), ms(1), third, ms(2), fourth, ms(3));      // (one call: one whole line)
    }
};

#endif  // DEEPBINNER_FAST5_POOLS_H
