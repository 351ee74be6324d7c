// fast5_bytes.h - the fast5 loader's lowest layer: one file as bytes, every access checked
// against its length.
#ifndef DEEPBINNER_FAST5_BYTES_H
#define DEEPBINNER_FAST5_BYTES_H

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/uio.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace {

struct FormatError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// the writer found a file under the name it was to create (nothing is ever overwritten)
struct ExistsError : std::runtime_error {
    ExistsError() : std::runtime_error("file exists") {}
};

// bytes [off, off + n) of fd at dst, in as many pread calls as it takes; false: it could not be read
inline bool pread_all(int fd, uint8_t* dst, uint64_t n, uint64_t off) {
    uint64_t got = 0;
    while (got < n) {
        const ssize_t k = ::pread(fd, dst + got, (size_t)(n - got), (off_t)(off + got));
        if (k <= 0) return false;
        got += (uint64_t)k;
    }
    return true;
}

// One open file: read whole if it is small, mapped (and read with pread) if it is large
class FileBytes {
  public:
    // `reuse`: a buffer of the caller's (a worker thread's) that small files are read into
    // instead of one allocated per file - a few hundred KB per file is above malloc's mmap
    // threshold, i.e. an mmap + munmap per file, which many threads queue up on
    explicit FileBytes(const char* path, std::vector<uint8_t>* reuse = nullptr) {
        fd_ = ::open(path, O_RDONLY);
        if (fd_ < 0) throw std::runtime_error("cannot open file");
        struct stat st;
        if (fstat(fd_, &st) != 0 || st.st_size <= 0) {
            ::close(fd_);
            fd_ = -1;
            throw std::runtime_error("cannot stat file / file is empty");
        }
        len_ = (uint64_t)st.st_size;
        if (len_ <= kReadWhole) {
            // one-read files are a few hundred KB: read() them - with many loader threads every
            // mmap/munmap would queue on the process-wide address-space lock
            std::vector<uint8_t>& bytes = reuse ? *reuse : owned_;
            if (bytes.size() < len_) bytes.resize((size_t)len_);
            const bool whole = pread_all(fd_, bytes.data(), len_, 0);
            ::close(fd_);
            fd_ = -1;
            if (!whole) throw std::runtime_error("cannot read file");
            buf_ = bytes.data();
            return;
        }
        void* p = mmap(nullptr, len_, PROT_READ, MAP_PRIVATE, fd_, 0);
        if (p == MAP_FAILED) {
            ::close(fd_);
            fd_ = -1;
            throw std::runtime_error("cannot map file");
        }
        buf_ = static_cast<const uint8_t*>(p);
        mapped_ = true;
    }
    ~FileBytes() {
        if (mapped_) munmap(const_cast<uint8_t*>(buf_), len_);
        if (fd_ >= 0) ::close(fd_);
    }
    FileBytes(const FileBytes&) = delete;
    FileBytes& operator=(const FileBytes&) = delete;

    // bytes [off, off + n) of the file
    void read_bytes(uint64_t off, uint64_t n, uint8_t* dst) const {
        need(off, n);
        if (mapped_ && fd_ >= 0) {
            // large (multi-read) files: the payload comes through pread, not through the
            // mapping - page faults of many threads queue on the address-space lock
            if (!pread_all(fd_, dst, n, off)) throw FormatError("cannot read chunk");
        } else {
            std::memcpy(dst, buf_ + off, (size_t)n);
        }
    }

    // MANY byte ranges of the file at once (the stored Signal pieces of a stretch of a multi-read
    // container, f5_stream's raw batches): sorted by their place in the file, neighbours with small
    // gaps between them - the object headers and B-tree nodes between two reads' chunks - are read
    // by ONE preadv (the gaps go to a sink), up to kMaxIov ranges a call, where a pread per range
    // was a system call per read (half of the raw loader's time).  Ranges are checked against the
    // file's length first; failed[k] = 1 for every range that could not be read.
    struct IoItem {
        uint64_t off, n;
        uint8_t* dst;
        int64_t tag;                 // (the caller's: which read it belongs to)
    };
    void read_many(std::vector<IoItem>& items, std::vector<char>* failed) const {
        failed->assign(items.size(), 0);
        std::vector<size_t> order;
        order.reserve(items.size());
        for (size_t k = 0; k < items.size(); ++k) {
            const IoItem& it = items[k];
            if (it.off > len_ || it.n > len_ - it.off) (*failed)[k] = 1;
            else if (it.n > 0) order.push_back(k);
        }
        if (!(mapped_ && fd_ >= 0)) {
            for (size_t k : order) std::memcpy(items[k].dst, buf_ + items[k].off, (size_t)items[k].n);
            return;
        }
        std::sort(order.begin(), order.end(),
                  [&](size_t x, size_t y) { return items[x].off < items[y].off; });
        constexpr uint64_t kMaxGap = 32u << 10;
        constexpr size_t kMaxIov = 512;
        thread_local std::vector<uint8_t> sink(kMaxGap);
        thread_local std::vector<struct iovec> iov;
        auto one_by_one = [&](size_t a, size_t b) {
            for (size_t j = a; j < b; ++j) {
                const IoItem& it = items[order[j]];
                if (!pread_all(fd_, it.dst, it.n, it.off)) (*failed)[order[j]] = 1;
            }
        };
        size_t a = 0;
        while (a < order.size()) {
            iov.clear();
            size_t b = a;
            uint64_t pos = items[order[a]].off;
            while (b < order.size() && iov.size() + 2 <= kMaxIov) {
                const IoItem& it = items[order[b]];
                if (it.off < pos) break;                      // (overlapping ranges: on their own)
                const uint64_t gap = it.off - pos;
                if (b > a && gap > kMaxGap) break;
                if (gap > 0) iov.push_back({sink.data(), (size_t)gap});
                iov.push_back({it.dst, (size_t)it.n});
                pos = it.off + it.n;
                ++b;
            }
            if (b == a) {                                      // (an overlap at the run's start)
                one_by_one(a, a + 1);
                a += 1;
                continue;
            }
            const uint64_t total = pos - items[order[a]].off;
            const ssize_t k = b - a > 1 ? ::preadv(fd_, iov.data(), (int)iov.size(), (off_t)items[order[a]].off) : -1;
            if (k < 0 || (uint64_t)k != total) one_by_one(a, b);       // (short or failed: range by range)
            a = b;
        }
    }

  protected:
    static constexpr uint64_t kReadWhole = 8u << 20;   // files up to 8 MiB are read, larger mapped
    int fd_ = -1;
    bool mapped_ = false;
    std::vector<uint8_t> owned_;
    const uint8_t* buf_ = nullptr;
    uint64_t len_ = 0;

    // ---- checked access to the mapped file ---------------------------------------------------
    void need(uint64_t off, uint64_t n) const {
        if (off > len_ || n > len_ - off) throw FormatError("offset beyond end of file");
    }
    uint64_t u(uint64_t off, int size) const {
        need(off, (uint64_t)size);
        uint64_t v = 0;
        for (int i = size - 1; i >= 0; --i) v = (v << 8) | buf_[off + i];
        return v;
    }
    uint8_t b(uint64_t off) const {
        need(off, 1);
        return buf_[off];
    }
    bool sig(uint64_t off, const char* s4) const {
        need(off, 4);
        return std::memcmp(buf_ + off, s4, 4) == 0;
    }
};

}  // namespace

#endif  // DEEPBINNER_FAST5_BYTES_H
