// fast5_hdf5.h - the HDF5 structures a fast5 file is made of: superblock, object headers, groups,
// fractal heap, version-2 B-tree, global heap, attributes.  Nothing here knows what a read or a
// Signal is.
#ifndef DEEPBINNER_FAST5_HDF5_H
#define DEEPBINNER_FAST5_HDF5_H

#include <map>
#include <string>
#include <utility>

#include "fast5_bytes.h"

namespace {

constexpr uint64_t kUndef = ~0ull;
constexpr int kO = 8, kL = 8;          // only 8-byte offsets / lengths are supported
constexpr int kMaxDepth = 32;          // B-tree / indirect-block recursion guard

struct Msg {
    uint32_t type;
    uint64_t off;
    uint32_t size;
};

inline uint64_t pad8(uint64_t n) { return (n + 7) & ~7ull; }

inline int bit_length(uint64_t v) {
    int n = 0;
    while (v) {
        ++n;
        v >>= 1;
    }
    return n;
}

// The file's bytes read as HDF5: addresses, object headers and the links and attributes in them
class Hdf5File : public FileBytes {
  public:
    using FileBytes::FileBytes;

  protected:
    uint64_t base_ = 0, root_addr_ = 0;          // (parse_superblock sets them)

    // an address as the file states it -> its offset in the file
    uint64_t file_off(uint64_t addr) const {
        if (addr > len_ || base_ > len_ - addr) throw FormatError("address beyond end of file");
        return base_ + addr;
    }

    // ---- superblock (hdf5_lite._parse_superblock) ---------------------------------------------
    void parse_superblock() {
        static const uint8_t kSig[8] = {0x89, 'H', 'D', 'F', '\r', '\n', 0x1a, '\n'};
        uint64_t off = 0;
        while (true) {
            if (off + 8 > len_) throw FormatError("HDF5 signature not found");
            if (std::memcmp(buf_ + off, kSig, 8) == 0) break;
            off = off == 0 ? 512 : off * 2;
        }
        const int version = b(off + 8);
        int O, L;
        if (version == 0 || version == 1) {
            O = b(off + 13);
            L = b(off + 14);
            if (O != kO || L != kL) throw FormatError("only 8-byte offsets/lengths are supported");
            uint64_t p = off + 24 + (version == 1 ? 4 : 0);
            base_ = u(p, kO);
            p += 4 * kO;
            root_addr_ = u(p + kO, kO);
        } else if (version == 2 || version == 3) {
            O = b(off + 9);
            L = b(off + 10);
            if (O != kO || L != kL) throw FormatError("only 8-byte offsets/lengths are supported");
            base_ = u(off + 12, kO);
            root_addr_ = u(off + 12 + 3 * kO, kO);
        } else {
            throw FormatError("unsupported superblock version");
        }
        if (base_ == 0 && off) base_ = off;
    }

    // ---- object headers (hdf5_lite._read_object_header) ---------------------------------------
    std::vector<Msg> object_header(uint64_t addr) const {
        const uint64_t start = file_off(addr);
        need(start, 16);
        std::vector<Msg> messages;
        std::vector<std::pair<uint64_t, uint64_t>> blocks;
        if (sig(start, "OHDR")) {
            if (b(start + 4) != 2) throw FormatError("unsupported object header version");
            const int flags = b(start + 5);
            uint64_t p = start + 6;
            if (flags & 0x20) p += 16;
            if (flags & 0x10) p += 4;
            const int csize = 1 << (flags & 3);
            const uint64_t chunk0 = u(p, csize);
            p += csize;
            const bool track_order = flags & 0x04;
            blocks.emplace_back(p, chunk0);
            for (size_t i = 0; i < blocks.size(); ++i) {
                if (blocks.size() > 4096) throw FormatError("too many header continuation blocks");
                uint64_t bp = blocks[i].first;
                const uint64_t end = bp + blocks[i].second;
                need(bp, blocks[i].second);
                while (bp + 4 <= end) {
                    const uint32_t mtype = b(bp);
                    const uint32_t msize = (uint32_t)u(bp + 1, 2);
                    bp += 4 + (track_order ? 2 : 0);
                    if (mtype == 0x10) {
                        const uint64_t caddr = u(bp, kO), clen = u(bp + kO, kL);
                        if (clen < 8) throw FormatError("bad continuation block");
                        blocks.emplace_back(file_off(caddr) + 4, clen - 8);
                    } else if (mtype != 0) {
                        messages.push_back(Msg{mtype, bp, msize});
                    }
                    bp += msize;
                }
            }
            return messages;
        }
        if (b(start) != 1) throw FormatError("unsupported object header version");
        const uint64_t nmsgs = u(start + 2, 2);
        const uint64_t hsize = u(start + 8, 4);
        blocks.emplace_back(start + 16, hsize);
        uint64_t seen = 0;
        for (size_t i = 0; i < blocks.size() && seen < nmsgs; ++i) {
            uint64_t bp = blocks[i].first;
            const uint64_t end = bp + blocks[i].second;
            need(bp, blocks[i].second);
            while (bp + 8 <= end && seen < nmsgs) {
                const uint32_t mtype = (uint32_t)u(bp, 2);
                const uint32_t msize = (uint32_t)u(bp + 2, 2);
                bp += 8;
                ++seen;
                if (mtype == 0x0010) {
                    const uint64_t caddr = u(bp, kO), clen = u(bp + kO, kL);
                    blocks.emplace_back(file_off(caddr), clen);
                } else if (mtype != 0) {
                    messages.push_back(Msg{mtype, bp, msize});
                }
                bp += msize;
            }
        }
        return messages;
    }

    static const Msg* first_of(const std::vector<Msg>& msgs, uint32_t type) {
        for (const Msg& m : msgs)
            if (m.type == type) return &m;
        return nullptr;
    }

    // ---- groups (hdf5_lite.Group._load_links) --------------------------------------------------
    std::string cstring(uint64_t off) const {
        need(off, 1);
        const void* end = std::memchr(buf_ + off, 0, (size_t)(len_ - off));
        if (!end) throw FormatError("unterminated string");
        return std::string(reinterpret_cast<const char*>(buf_ + off),
                           (size_t)(static_cast<const uint8_t*>(end) - (buf_ + off)));
    }

    void walk_group_btree(uint64_t addr, uint64_t heap_data, std::map<std::string, uint64_t>* links,
                          int depth) const {
        if (depth > kMaxDepth) throw FormatError("group B-tree too deep");
        const uint64_t p = file_off(addr);
        if (!sig(p, "TREE")) throw FormatError("bad group B-tree signature");
        const int level = b(p + 5);
        const uint64_t used = u(p + 6, 2);
        const uint64_t q = p + 8 + 2 * kO;
        for (uint64_t i = 0; i < used; ++i) {
            const uint64_t child = u(q + kL + i * (kL + kO), kO);
            if (level > 0) {
                walk_group_btree(child, heap_data, links, depth + 1);
            } else {
                const uint64_t s = file_off(child);
                if (!sig(s, "SNOD")) throw FormatError("bad symbol table node signature");
                const uint64_t nsym = u(s + 6, 2);
                uint64_t e = s + 8;
                for (uint64_t k = 0; k < nsym; ++k) {
                    const uint64_t name_off = u(e, kO), ohdr = u(e + kO, kO);
                    (*links)[cstring(heap_data + name_off)] = ohdr;
                    e += 2 * kO + 24;
                }
            }
        }
    }

    // link message -> (name, object header address); false for soft/external links
    bool parse_link(uint64_t off, std::string* name, uint64_t* addr) const {
        if (b(off) != 1) throw FormatError("bad link message version");
        const int flags = b(off + 1);
        uint64_t p = off + 2;
        int ltype = 0;
        if (flags & 0x08) ltype = b(p++);
        if (flags & 0x04) p += 8;
        if (flags & 0x10) p += 1;
        const int lsize = 1 << (flags & 3);
        const uint64_t nlen = u(p, lsize);
        p += lsize;
        need(p, nlen);
        name->assign(reinterpret_cast<const char*>(buf_ + p), (size_t)nlen);
        p += nlen;
        if (ltype != 0) return false;
        *addr = u(p, kO);
        return true;
    }

    std::map<std::string, uint64_t> group_links(const std::vector<Msg>& msgs) const {
        std::map<std::string, uint64_t> links;
        if (const Msg* stab = first_of(msgs, 0x0011)) {
            const uint64_t btree = u(stab->off, kO), heap = u(stab->off + kO, kO);
            const uint64_t hp = file_off(heap);
            if (!sig(hp, "HEAP")) throw FormatError("bad local heap signature");
            const uint64_t heap_data = file_off(u(hp + 8 + 2 * kL, kO));
            walk_group_btree(btree, heap_data, &links, 0);
        }
        for (const Msg& m : msgs) {
            if (m.type != 0x0006) continue;
            std::string name;
            uint64_t addr;
            if (parse_link(m.off, &name, &addr)) links[name] = addr;
        }
        if (const Msg* linfo = first_of(msgs, 0x0002)) {
            const int flags = b(linfo->off + 1);
            const uint64_t p = linfo->off + 2 + ((flags & 1) ? 8 : 0);
            const uint64_t heap_addr = u(p, kO), index_addr = u(p + kO, kO);
            if (heap_addr != kUndef && index_addr != kUndef) {
                for (uint64_t obj_off : dense_objects(heap_addr, index_addr)) {
                    std::string name;
                    uint64_t addr;
                    if (parse_link(obj_off, &name, &addr)) links[name] = addr;
                }
            }
        }
        return links;
    }

    // ---- fractal heap + v2 B-tree (dense link / attribute storage) ----------------------------
    struct FractalHeap {
        uint64_t id_len = 0, max_managed = 0, width = 0, start_size = 0, max_direct = 0;
        uint64_t root_addr = kUndef, cur_rows = 0;
        int off_bytes = 0, max_direct_rows = 2;
    };

    FractalHeap fractal_heap(uint64_t addr) const {
        FractalHeap h;
        const uint64_t p = file_off(addr);
        if (!sig(p, "FRHP")) throw FormatError("bad fractal heap signature");
        h.id_len = u(p + 5, 2);
        if (u(p + 7, 2)) throw FormatError("filtered fractal heaps are not supported");
        h.max_managed = u(p + 10, 4);
        const uint64_t q = p + 14 + kL + kO + kL + kO + 8 * kL;
        h.width = u(q, 2);
        h.start_size = u(q + 2, kL);
        h.max_direct = u(q + 2 + kL, kL);
        const uint64_t max_heap_bits = u(q + 2 + 2 * kL, 2);
        h.root_addr = u(q + 6 + 2 * kL, kO);
        h.cur_rows = u(q + 6 + 2 * kL + kO, 2);
        h.off_bytes = (int)((max_heap_bits + 7) / 8);
        if (h.width == 0 || h.start_size == 0 || h.off_bytes > 8) throw FormatError("bad fractal heap");
        uint64_t size = h.start_size;
        while (size < h.max_direct && h.max_direct_rows < 64) {
            size <<= 1;
            ++h.max_direct_rows;
        }
        return h;
    }

    uint64_t heap_locate(const FractalHeap& h, uint64_t offset) const {
        if (h.root_addr == kUndef) throw FormatError("empty fractal heap");
        if (h.cur_rows == 0) return file_off(h.root_addr) + offset;
        uint64_t iaddr = h.root_addr, rel = offset;
        for (int depth = 0; depth < kMaxDepth; ++depth) {
            const uint64_t blk = file_off(iaddr);
            if (!sig(blk, "FHIB")) throw FormatError("bad fractal heap indirect block signature");
            const uint64_t first = h.width * h.start_size;
            const int row = rel < first ? 0 : bit_length(rel / first);
            if (row > 62) throw FormatError("bad fractal heap offset");
            const uint64_t row_start = row == 0 ? 0 : (h.width * h.start_size) << (row - 1);
            const uint64_t bsize = row == 0 ? h.start_size : h.start_size << (row - 1);
            const uint64_t col = (rel - row_start) / bsize;
            const uint64_t entry = blk + 5 + kO + h.off_bytes + ((uint64_t)row * h.width + col) * kO;
            const uint64_t child = u(entry, kO);
            if (child == kUndef) throw FormatError("heap object in an unallocated block");
            rel -= row_start + col * bsize;
            if (row < h.max_direct_rows) return file_off(child) + rel;
            iaddr = child;
        }
        throw FormatError("fractal heap too deep");
    }

    static int enc_size(uint64_t limit) { return (bit_length(std::max<uint64_t>(limit, 1)) - 1) / 8 + 1; }

    void btree2_walk(uint64_t naddr, uint64_t nrec, int d, uint64_t rec_size, int nrec_size,
                     const std::vector<int>& cum_size, std::vector<uint64_t>* records,
                     int depth) const {
        if (depth > kMaxDepth) throw FormatError("v2 B-tree too deep");
        const uint64_t blk = file_off(naddr);
        if (d == 0) {
            if (!sig(blk, "BTLF")) throw FormatError("bad v2 B-tree leaf signature");
            for (uint64_t i = 0; i < nrec; ++i) {
                need(blk + 6 + i * rec_size, rec_size);
                records->push_back(blk + 6 + i * rec_size);
            }
            return;
        }
        if (!sig(blk, "BTIN")) throw FormatError("bad v2 B-tree internal node signature");
        const uint64_t recs = blk + 6;
        const uint64_t ptrs = recs + nrec * rec_size;
        const uint64_t ptr = kO + nrec_size + (d > 1 ? cum_size[(size_t)d - 1] : 0);
        for (uint64_t i = 0; i <= nrec; ++i) {
            const uint64_t e = ptrs + i * ptr;
            const uint64_t child = u(e, kO);
            const uint64_t child_nrec = u(e + kO, nrec_size);
            btree2_walk(child, child_nrec, d - 1, rec_size, nrec_size, cum_size, records, depth + 1);
            if (i < nrec) {
                need(recs + i * rec_size, rec_size);
                records->push_back(recs + i * rec_size);
            }
        }
    }

    // file offsets of the raw records of a version-2 B-tree, in key order
    std::vector<uint64_t> btree2_records(uint64_t addr, uint64_t* rec_size_out, int* type_out) const {
        std::vector<uint64_t> records;
        const uint64_t p = file_off(addr);
        if (!sig(p, "BTHD")) throw FormatError("bad v2 B-tree signature");
        *type_out = b(p + 5);
        const uint64_t node_size = u(p + 6, 4);
        const uint64_t rec_size = u(p + 10, 2);
        const int depth = (int)u(p + 12, 2);
        const uint64_t root = u(p + 16, kO);
        const uint64_t root_nrec = u(p + 16 + kO, 2);
        *rec_size_out = rec_size;
        if (root == kUndef || root_nrec == 0) return records;
        if (rec_size == 0 || node_size < 16 || depth > kMaxDepth) throw FormatError("bad v2 B-tree header");
        std::vector<uint64_t> cum_max;
        std::vector<int> cum_size;
        const uint64_t max0 = (node_size - 10) / rec_size;
        cum_max.push_back(max0);
        const int nrec_size = enc_size(max0);
        cum_size.push_back(enc_size(max0));
        for (int d = 1; d <= depth; ++d) {
            const uint64_t ptr = kO + nrec_size + (d > 1 ? cum_size[(size_t)d - 1] : 0);
            const uint64_t m = (node_size - (10 + ptr)) / (rec_size + ptr);
            cum_max.push_back((m + 1) * cum_max[(size_t)d - 1] + m);
            cum_size.push_back(enc_size(cum_max[(size_t)d]));
        }
        btree2_walk(root, root_nrec, depth, rec_size, nrec_size, cum_size, &records, 0);
        return records;
    }

    // file offsets of the messages held in dense (fractal heap + v2 B-tree) storage
    std::vector<uint64_t> dense_objects(uint64_t heap_addr, uint64_t index_addr) const {
        const FractalHeap heap = fractal_heap(heap_addr);
        uint64_t rec_size = 0;
        int btype = 0;
        std::vector<uint64_t> out;
        for (uint64_t rec : btree2_records(index_addr, &rec_size, &btype)) {
            // type 5 (link name) record: hash(4) + heap id; type 8 (attribute name): heap id first
            const uint64_t id = btype == 5 ? rec + 4 : rec;
            if ((btype == 5 ? 4 : 0) + heap.id_len > rec_size) throw FormatError("bad dense record");
            if (((b(id) >> 4) & 3) != 0) throw FormatError("only managed fractal-heap objects are supported");
            out.push_back(heap_locate(heap, u(id + 1, heap.off_bytes)));
        }
        return out;
    }

    // ---- attributes: only string values are needed (read_id) -----------------------------------
    std::string global_heap_object(uint64_t coll_addr, uint64_t index) const {
        const uint64_t p = file_off(coll_addr);
        if (!sig(p, "GCOL")) throw FormatError("bad global heap signature");
        const uint64_t size = u(p + 8, kL);
        uint64_t o = p + 8 + kL;
        const uint64_t end = p + size;
        while (o + 8 + kL <= end) {
            const uint64_t idx = u(o, 2);
            const uint64_t osize = u(o + 8, kL);
            if (idx == 0) break;
            if (idx == index) {
                need(o + 8 + kL, osize);
                return std::string(reinterpret_cast<const char*>(buf_ + o + 8 + kL), (size_t)osize);
            }
            o += 8 + kL + pad8(osize);
        }
        throw FormatError("global heap object not found");
    }

    // attribute message at `off`: its name; if it is a scalar string, its value
    bool parse_string_attribute(uint64_t off, std::string* name, std::string* value) const {
        const int version = b(off);
        const uint64_t nsz = u(off + 2, 2), tsz = u(off + 4, 2), ssz = u(off + 6, 2);
        uint64_t p = off + 8;
        if (version == 3)
            p += 1;
        else if (version != 1 && version != 2)
            throw FormatError("unsupported attribute version");
        const bool padded = version == 1;
        need(p, nsz);
        name->assign(reinterpret_cast<const char*>(buf_ + p), (size_t)nsz);
        name->resize(std::strlen(name->c_str()));
        p += padded ? pad8(nsz) : nsz;
        const uint64_t dt_off = p;
        p += padded ? pad8(tsz) : tsz;
        const uint64_t ds_off = p;
        p += padded ? pad8(ssz) : ssz;
        // dataspace: scalar or a single element
        const int ds_version = b(ds_off), rank = b(ds_off + 1);
        if (ds_version != 1 && ds_version != 2) return false;
        uint64_t count = 1;
        const uint64_t dims = ds_off + (ds_version == 1 ? 8 : 4);
        for (int i = 0; i < rank; ++i) count *= u(dims + (uint64_t)i * kL, kL);
        if (count != 1) return false;
        const int cls = b(dt_off) & 0x0F;
        const uint64_t bits = u(dt_off + 1, 3);
        const uint64_t size = u(dt_off + 4, 4);
        if (cls == 3) {            // fixed-length string, NUL padding stripped like h5py does
            need(p, size);
            value->assign(reinterpret_cast<const char*>(buf_ + p), (size_t)size);
            value->resize(std::strlen(value->c_str()));
            return true;
        }
        if (cls == 9 && (bits & 0x0F) == 1) {   // variable-length string in the global heap
            const uint64_t coll = u(p + 4, kO), idx = u(p + 4 + kO, 4);
            *value = coll ? global_heap_object(coll, idx) : std::string();
            return true;
        }
        return false;
    }

    bool find_string_attribute(const std::vector<Msg>& msgs, const char* wanted,
                               std::string* value) const {
        std::string name, v;
        for (const Msg& m : msgs) {
            if (m.type == 0x000C) {
                if (parse_string_attribute(m.off, &name, &v) && name == wanted) {
                    *value = v;
                    return true;
                }
            } else if (m.type == 0x0015) {   // dense attribute storage
                const int flags = b(m.off + 1);
                const uint64_t p = m.off + 2 + ((flags & 1) ? 2 : 0);
                const uint64_t heap_addr = u(p, kO), index_addr = u(p + kO, kO);
                if (heap_addr == kUndef || index_addr == kUndef) continue;
                for (uint64_t obj_off : dense_objects(heap_addr, index_addr))
                    if (parse_string_attribute(obj_off, &name, &v) && name == wanted) {
                        *value = v;
                        return true;
                    }
            }
        }
        return false;
    }

    // ---- every scalar attribute of an object, as a one-read copy of the read carries it --------
    // (what deepbinner_amd/hdf5_write.py's attribute_from_value keeps of what hdf5_lite reads:
    // strings, integers of 1/2/4/8 bytes, floats of 4/8 bytes; arrays, enums, references and
    // anything else are left behind)
  public:
    struct Attr {
        int kind = 0;              // 0 string, 1 integer, 2 float
        int size = 0;              // bytes of an integer / a float
        bool is_signed = false;
        std::string bytes;         // the text without its NUL / the value, little-endian
    };
    typedef std::map<std::string, Attr> Attrs;

    bool parse_attribute(uint64_t off, std::string* name, Attr* a) const {
        const int version = b(off);
        const uint64_t nsz = u(off + 2, 2), tsz = u(off + 4, 2), ssz = u(off + 6, 2);
        uint64_t p = off + 8;
        if (version == 3)
            p += 1;
        else if (version != 1 && version != 2)
            throw FormatError("unsupported attribute version");
        const bool padded = version == 1;
        need(p, nsz);
        name->assign(reinterpret_cast<const char*>(buf_ + p), (size_t)nsz);
        name->resize(std::strlen(name->c_str()));
        p += padded ? pad8(nsz) : nsz;
        const uint64_t dt_off = p;
        p += padded ? pad8(tsz) : tsz;
        const uint64_t ds_off = p;
        p += padded ? pad8(ssz) : ssz;
        const int ds_version = b(ds_off), rank = b(ds_off + 1);
        if ((ds_version != 1 && ds_version != 2) || rank != 0) return false;     // scalars only
        const int cls = b(dt_off) & 0x0F;
        const uint64_t bits = u(dt_off + 1, 3);
        const uint64_t size = u(dt_off + 4, 4);
        const bool big_endian = (bits & 1) != 0;
        a->bytes.clear();
        if (cls == 0 || cls == 1) {
            if (cls == 0 && size != 1 && size != 2 && size != 4 && size != 8) return false;
            if (cls == 1 && size != 4 && size != 8) return false;
            need(p, size);
            a->kind = cls == 0 ? 1 : 2;
            a->size = (int)size;
            a->is_signed = cls == 0 && (bits & 0x08) != 0;
            a->bytes.assign(reinterpret_cast<const char*>(buf_ + p), (size_t)size);
            if (big_endian) std::reverse(a->bytes.begin(), a->bytes.end());
            return true;
        }
        if (cls == 3) {            // fixed-length string, NUL padding stripped like h5py does
            need(p, size);
            a->kind = 0;
            a->bytes.assign(reinterpret_cast<const char*>(buf_ + p), (size_t)size);
            a->bytes.resize(std::strlen(a->bytes.c_str()));
            return true;
        }
        if (cls == 9 && (bits & 0x0F) == 1) {   // variable-length string in the global heap
            need(p, 8 + kO);
            const uint64_t coll = u(p + 4, kO), idx = u(p + 4 + kO, 4);
            a->kind = 0;
            a->bytes = coll ? global_heap_object(coll, idx) : std::string();
            return true;
        }
        return false;
    }

    Attrs attributes(uint64_t header_addr) const {
        Attrs found;
        std::string name;
        Attr a;
        auto take = [&](uint64_t off) {
            try {
                if (parse_attribute(off, &name, &a)) found[name] = a;
                else found.erase(name);
            } catch (const std::exception&) {      // one unreadable attribute is one left behind
            }
        };
        for (const Msg& m : object_header(header_addr)) {
            if (m.type == 0x000C) {
                take(m.off);
            } else if (m.type == 0x0015) {   // dense attribute storage
                const int flags = b(m.off + 1);
                const uint64_t p = m.off + 2 + ((flags & 1) ? 2 : 0);
                const uint64_t heap_addr = u(p, kO), index_addr = u(p + kO, kO);
                if (heap_addr == kUndef || index_addr == kUndef) continue;
                for (uint64_t obj_off : dense_objects(heap_addr, index_addr)) take(obj_off);
            }
        }
        return found;
    }
};

}  // namespace

#endif  // DEEPBINNER_FAST5_HDF5_H
