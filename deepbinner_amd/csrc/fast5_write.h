// fast5_write.h - one-read fast5 files written: the image (h5w), and how it reaches its name
// without ever replacing a file.
#ifndef DEEPBINNER_FAST5_WRITE_H
#define DEEPBINNER_FAST5_WRITE_H

#include <linux/fs.h>
#include <sys/syscall.h>

#include <cerrno>
#include <cstdio>

#include "fast5_file.h"

namespace {

// errno values with which link() says "this filesystem has no hard links": ENOTSUP / EOPNOTSUPP /
// ENOSYS, and EPERM, which is what FAT / exFAT and several FUSE and SMB mounts answer.  (Not EACCES,
// EXDEV or EMLINK: those are errors of this call, not properties of the filesystem, and fall
// through to "cannot name file".)
static bool no_hard_links(int e) {
    return e == EPERM || e == ENOTSUP || e == EOPNOTSUPP || e == ENOSYS;
}
// DEEPBINNER_FAST5_NO_LINK=1 (tests): link() is not tried at all, as on such a filesystem
static bool links_forbidden() {
    static const bool forced = [] {
        const char* v = std::getenv("DEEPBINNER_FAST5_NO_LINK");
        return v && v[0] == '1';
    }();
    return forced;
}
// The image under a name that must not exist yet (O_EXCL; a symlink there is not followed); a
// failed write leaves nothing behind.
static void write_exclusive(const char* path, const std::string& image) {
    const int fd = ::open(path, O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0666);
    if (fd < 0) {
        if (errno == EEXIST) throw ExistsError();
        throw std::runtime_error("cannot create file");
    }
    size_t done = 0;
    while (done < image.size()) {
        const ssize_t k = ::write(fd, image.data() + done, image.size() - done);
        if (k <= 0) {
            ::close(fd);
            ::unlink(path);
            throw std::runtime_error("cannot write file");
        }
        done += (size_t)k;
    }
    if (::close(fd) != 0) {
        ::unlink(path);
        throw std::runtime_error("cannot close file");
    }
}

// The image under the name `path`, `i` the caller's number for it (it goes into the temporary name).
static void place_new_file(const char* path, const std::string& image, int64_t i) {
    // Never over a file that is there (the reference's move counts a clash and leaves
    // the earlier file alone, realtime.py:111-144), never through a symlink, and no
    // half-written file under the final name: the image goes to a fresh temporary
    // name in the same directory and is linked into place - link() fails if the name
    // exists, and is atomic.
    if (::access(path, F_OK) == 0) throw ExistsError();
    const std::string tmp = std::string(path) + ".part." +
                            std::to_string((long long)::getpid()) + "." +
                            std::to_string((long long)i);
    ::unlink(tmp.c_str());      // (a stale one of this very name: a killed run whose
                                // pid came round - the O_EXCL below would refuse it)
    write_exclusive(tmp.c_str(), image);
    int linked = -1, link_errno = EPERM;
    if (!links_forbidden()) {
        linked = ::link(tmp.c_str(), path);
        link_errno = errno;
    }
    if (linked != 0 && link_errno != EEXIST && no_hard_links(link_errno)) {
        // exFAT / FAT, many SMB and FUSE mounts (sequencing drives) have no link(): the
        // finished temporary file is RENAMED into place - nobody ever sees a partial
        // file under the final name, and a killed process leaves only the .part file -
        // without replacing (renameat2 RENAME_NOREPLACE); where the filesystem does not
        // know that flag, after a look at the name (rename is atomic there too; the
        // window between the look and the rename is the one thing link() had closed)
        int renamed = -1;
#ifdef RENAME_NOREPLACE
        renamed = (int)::syscall(SYS_renameat2, AT_FDCWD, tmp.c_str(), AT_FDCWD, path,
                                 RENAME_NOREPLACE);
        if (renamed != 0 && errno == EEXIST) {
            ::unlink(tmp.c_str());
            throw ExistsError();
        }
#endif
        if (renamed != 0) {
            struct stat st_there;
            if (::lstat(path, &st_there) == 0) {
                ::unlink(tmp.c_str());
                throw ExistsError();
            }
            if (::rename(tmp.c_str(), path) != 0) {
                ::unlink(tmp.c_str());
                throw std::runtime_error("cannot name file");
            }
        }
    } else {
        ::unlink(tmp.c_str());
        if (linked != 0) {
            if (link_errno == EEXIST) throw ExistsError();
            throw std::runtime_error("cannot name file");
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Writing one-read fast5 files: the layout of deepbinner_amd/hdf5_write.py (superblock version 0,
// version-1 object headers, groups as symbol tables, the Signal as one deflate-compressed chunk
// behind a version-1 B-tree, scalar attributes), byte for byte - that module is pinned to the
// real HDF5 library and to the reference's loader (tests/test_hdf5_write.py), and
// tests/test_fast5_writer.py holds this one to it.  Why twice: `deepbinner realtime` ends with
// every read of a multi-read container as a one-read file in its barcode's directory
// (reference realtime.py:111-150 after multi_to_single_fast5, :183-190); built in Python that is
// ~350 us per read under the interpreter lock plus a deflate of the signal - 2.5 k reads/s
// behind a GPU that classifies 170 k.  Here a read costs its attributes, one pread of its chunk
// AS STORED (nothing is inflated, nothing deflated again) and one write.
// ---------------------------------------------------------------------------------------------
namespace h5w {

constexpr uint64_t kUndefAddr = 0xFFFFFFFFFFFFFFFFull;
constexpr int kGroupLeafK = 4, kGroupInternalK = 16, kChunkK = 32;      // superblock v0 defaults

struct Bytes {
    std::string s;
    Bytes& u8(uint64_t v) { return put(v, 1); }
    Bytes& u16(uint64_t v) { return put(v, 2); }
    Bytes& u32(uint64_t v) { return put(v, 4); }
    Bytes& u64(uint64_t v) { return put(v, 8); }
    Bytes& zeros(size_t n) {
        s.append(n, '\0');
        return *this;
    }
    Bytes& raw(const std::string& b) {
        s += b;
        return *this;
    }
    Bytes& raw(const char* b, size_t n) {
        s.append(b, n);
        return *this;
    }
    Bytes& pad8() { return zeros((size_t)((8 - s.size() % 8) % 8)); }
    Bytes& put(uint64_t v, int n) {
        for (int i = 0; i < n; ++i) s.push_back((char)((v >> (8 * i)) & 0xFF));
        return *this;
    }
};
std::string padded8(const std::string& b) { return Bytes{b}.pad8().s; }

// the file as one growing byte string; every block starts 8-byte aligned
struct Image {
    std::string buf;
    uint64_t reserve(size_t size) {
        buf.append((8 - buf.size() % 8) % 8, '\0');
        const uint64_t addr = buf.size();
        buf.append(size, '\0');
        return addr;
    }
    uint64_t add(const std::string& data) {
        const uint64_t addr = reserve(data.size());
        std::memcpy(&buf[(size_t)addr], data.data(), data.size());
        return addr;
    }
};

std::string message(int type, const std::string& body, int flags = 0) {
    const std::string b = padded8(body);
    return Bytes().u16((uint64_t)type).u16(b.size()).u8((uint64_t)flags).zeros(3).raw(b).s;
}
std::string object_header(const std::vector<std::string>& messages) {
    std::string data;
    for (const std::string& m : messages) data += m;
    return Bytes().u8(1).u8(0).u16(messages.size()).u32(1).u32(data.size()).zeros(4).raw(data).s;
}
std::string string_datatype(size_t size) { return Bytes().u8(0x13).zeros(3).u32(size).s; }
std::string fixed_datatype(int size, bool is_signed) {
    return Bytes().u8(0x10).u8(is_signed ? 0x08 : 0).zeros(2).u32((uint64_t)size).u16(0)
        .u16((uint64_t)(8 * size)).s;
}
std::string float_datatype(int size) {
    if (size == 4)
        return Bytes().u8(0x11).u8(0x20).u8(0x1F).u8(0).u32(4).u16(0).u16(32).u8(23).u8(8).u8(0)
            .u8(23).u32(127).s;
    return Bytes().u8(0x11).u8(0x20).u8(0x3F).u8(0).u32(8).u16(0).u16(64).u8(52).u8(11).u8(0)
        .u8(52).u32(1023).s;
}
std::string scalar_dataspace() { return Bytes().u8(1).u8(0).u8(0).zeros(5).s; }
std::string simple_dataspace(uint64_t n) { return Bytes().u8(1).u8(1).u8(0).zeros(5).u64(n).s; }
std::string attribute(const std::string& name, const std::string& datatype,
                      const std::string& value) {
    const std::string name_z = name + std::string(1, '\0');
    const std::string space = scalar_dataspace();
    return message(0x000C, Bytes().u8(1).u8(0).u16(name_z.size()).u16(datatype.size())
                               .u16(space.size()).raw(padded8(name_z)).raw(padded8(datatype))
                               .raw(padded8(space)).raw(value).s);
}
std::string string_attribute(const std::string& name, const std::string& text) {
    const std::string raw = text + std::string(1, '\0');
    return attribute(name, string_datatype(raw.size()), raw);
}
std::string int_attribute(const std::string& name, uint64_t value, int size, bool is_signed) {
    return attribute(name, fixed_datatype(size, is_signed), Bytes().put(value, size).s);
}
std::string attribute_of(const std::string& name, const Fast5::Attr& a) {
    if (a.kind == 0) return string_attribute(name, a.bytes);
    if (a.kind == 1) return attribute(name, fixed_datatype(a.size, a.is_signed), a.bytes);
    return attribute(name, float_datatype(a.size), a.bytes);
}
std::vector<std::string> attributes_of(const Fast5::Attrs& values, const char* skip = nullptr) {
    std::vector<std::string> out;            // (a std::map walks its names in sorted order)
    for (const auto& kv : values)
        if (!skip || kv.first != skip) out.push_back(attribute_of(kv.first, kv.second));
    return out;
}

struct Node {
    uint64_t header = 0, btree = kUndefAddr, heap = kUndefAddr;
    bool is_group = true;
};

Node group(Image& image, const std::map<std::string, Node>& children,
           const std::vector<std::string>& attributes) {
    // local heap data: offset 0 is the empty string, then the names, each 8-byte aligned
    // (a std::map walks the names in byte order, which is what the symbol table wants)
    Bytes heap_data;
    heap_data.zeros(8);
    std::vector<uint64_t> offsets;
    for (const auto& kv : children) {
        offsets.push_back(heap_data.s.size());
        heap_data.raw(padded8(kv.first + std::string(1, '\0')));
    }
    const uint64_t heap_data_addr = image.add(heap_data.s);
    const uint64_t heap = image.add(
        Bytes().raw("HEAP", 4).u8(0).zeros(3).u64(heap_data.s.size()).u64(1).u64(heap_data_addr).s);
    Bytes snod;
    snod.raw("SNOD", 4).u8(1).u8(0).u16(children.size());
    size_t k = 0;
    for (const auto& kv : children) {
        const Node& c = kv.second;
        snod.u64(offsets[k++]).u64(c.header);
        if (c.is_group)
            snod.u32(1).u32(0).u64(c.btree).u64(c.heap);
        else
            snod.u32(0).u32(0).zeros(16);
    }
    snod.zeros(40 * (2 * kGroupLeafK - children.size()));
    const uint64_t snod_addr = image.add(snod.s);
    // B-tree v1, group node (type 0), leaf level, one child: keys are heap offsets of names
    Bytes node;
    node.raw("TREE", 4).u8(0).u8(0).u16(1).u64(kUndefAddr).u64(kUndefAddr);
    node.u64(0).u64(snod_addr).u64(offsets.back());
    node.zeros(24 + 16 * kGroupInternalK * 2 + 8 - node.s.size());
    Node g;
    g.btree = image.add(node.s);
    g.heap = heap;
    std::vector<std::string> messages = {message(0x0011, Bytes().u64(g.btree).u64(heap).s)};
    messages.insert(messages.end(), attributes.begin(), attributes.end());
    g.header = image.add(object_header(messages));
    return g;
}

// a group without links that only carries attributes (channel_id, tracking_id, ...)
Node attribute_group(Image& image, const std::vector<std::string>& attributes) {
    const uint64_t heap_data_addr = image.add(std::string(8, '\0'));
    Node g;
    g.heap = image.add(Bytes().raw("HEAP", 4).u8(0).zeros(3).u64(8).u64(1).u64(heap_data_addr).s);
    Bytes node;
    node.raw("TREE", 4).u8(0).u8(0).u16(0).u64(kUndefAddr).u64(kUndefAddr);
    node.zeros(24 + 16 * kGroupInternalK * 2 + 8 - node.s.size());
    g.btree = image.add(node.s);
    std::vector<std::string> messages = {message(0x0011, Bytes().u64(g.btree).u64(g.heap).s)};
    messages.insert(messages.end(), attributes.begin(), attributes.end());
    g.header = image.add(object_header(messages));
    return g;
}

// int16[n] as one deflate-compressed chunk (`packed`: its zlib stream) behind a chunk B-tree
Node dataset_int16(Image& image, uint64_t n, const std::string& packed) {
    std::vector<std::string> messages = {
        message(0x0001, simple_dataspace(n)),
        message(0x0003, fixed_datatype(2, true), 1),                   // constant message
        message(0x0005, Bytes().u8(2).u8(2).u8(0).u8(0).s)};           // fill value: never written
    if (n > 0) {
        const uint64_t chunk = image.add(packed);
        const size_t key_size = 8 + 8 * 2;
        Bytes node;
        node.raw("TREE", 4).u8(1).u8(0).u16(1).u64(kUndefAddr).u64(kUndefAddr);
        node.u32(packed.size()).u32(0).u64(0).u64(0).u64(chunk);
        node.u32(0).u32(0).u64(n).u64(0);
        node.zeros(24 + 2 * kChunkK * 8 + (2 * kChunkK + 1) * key_size - node.s.size());
        const uint64_t btree = image.add(node.s);
        messages.push_back(message(
            0x000B, Bytes().u8(1).u8(1).zeros(6).u16(1).u16(0).u16(0).u16(1).u32(1).u32(0).s));
        messages.push_back(message(0x0008, Bytes().u8(3).u8(2).u8(2).u64(btree).u32(n).u32(2).s));
    } else {
        messages.push_back(message(0x0008, Bytes().u8(3).u8(1).u64(kUndefAddr).u64(0).s));
    }
    Node d;
    d.is_group = false;
    d.header = image.add(object_header(messages));
    return d;
}

// The bytes of a one-read fast5 file: /read_<id>/{Raw/Signal, channel_id, tracking_id,
// context_tags} with the attributes of `meta` (hdf5_write.single_read_fast5_bytes).
std::string single_read_file(const std::string& read_id, uint64_t n_samples,
                             const std::string& packed, const Fast5::ReadMeta& meta) {
    Image image;
    const uint64_t superblock = image.reserve(96);
    const Node signal = dataset_int16(image, n_samples, packed);
    std::vector<std::string> raw_attributes = {string_attribute("read_id", read_id)};
    if (meta.raw.find("duration") == meta.raw.end())
        raw_attributes.push_back(int_attribute("duration", n_samples, 4, false));
    for (const std::string& a : attributes_of(meta.raw, "read_id")) raw_attributes.push_back(a);
    std::map<std::string, Node> children;
    children["Raw"] = group(image, {{"Signal", signal}}, raw_attributes);
    for (int k = 0; k < 3; ++k)
        if (meta.has[k])
            children[Fast5::meta_group_name(k)] =
                attribute_group(image, attributes_of(meta.group[k]));
    const Node read = group(image, children, attributes_of(meta.read));
    const Node root = group(image, {{"read_" + read_id, read}},
                            {string_attribute("file_version", "2.0")});
    image.buf.append((8 - image.buf.size() % 8) % 8, '\0');
    const uint64_t end = image.buf.size();
    const std::string head =
        Bytes().raw("\x89HDF\r\n\x1a\n", 8).zeros(5).u8(8).u8(8).u8(0).u16(kGroupLeafK)
            .u16(kGroupInternalK).u32(0).u64(0).u64(kUndefAddr).u64(end).u64(kUndefAddr)
            .u64(0).u64(root.header).u32(1).u32(0).u64(root.btree).u64(root.heap).s;
    std::memcpy(&image.buf[(size_t)superblock], head.data(), head.size());
    return std::move(image.buf);
}

}  // namespace h5w

// The one-read copy of read `index` of a container, as the bytes of its file.  without_meta_if_need_be:
// a read whose attributes cannot be read is copied without them (the writer), not refused.
std::string single_read_image(Fast5& file, int64_t index, bool without_meta_if_need_be,
                              ChunkCache* cache = nullptr) {
    const ReadEntry& r = file.read(index);
    Fast5::ReadMeta meta;
    try {
        file.read_metadata(index, &meta);
    } catch (const std::exception&) {
        if (!without_meta_if_need_be) throw;
        meta = Fast5::ReadMeta();      // the signal and the read id are what binning
    }                                  // cannot do without; the rest is left behind
    const int64_t samples = r.signal.n;
    std::string packed;
    uint64_t off = 0, nbytes = 0;
    if (samples > 0 && file.whole_deflated_chunk(r.signal, &off, &nbytes)) {
        packed.resize((size_t)nbytes);
        file.read_bytes(off, nbytes, reinterpret_cast<uint8_t*>(&packed[0]));
    } else if (samples > 0) {
        // stored some other way (contiguous, several chunks, more filters): decoded and
        // deflated again, level 1 like hdf5_write.py
        std::vector<int16_t> raw((size_t)samples);
        file.read_signal(r.signal, 0, samples, raw.data(), cache);
        uLongf bound = compressBound((uLong)samples * 2);
        packed.resize((size_t)bound);
        if (compress2(reinterpret_cast<Bytef*>(&packed[0]), &bound,
                      reinterpret_cast<const Bytef*>(raw.data()), (uLong)samples * 2,
                      1) != Z_OK)
            throw FormatError("deflate failed");
        packed.resize((size_t)bound);
    }
    return h5w::single_read_file(r.read_id, (uint64_t)samples, packed, meta);
}

}  // namespace

#endif  // DEEPBINNER_FAST5_WRITE_H
