// loader_host_test - every loader of include/deepbinner_fast5.h over the fast5 files named on the
// command line, one line of digests per call (tests/test_fast5_native.py holds the lines for
// tests/golden/fast5 to tests/golden/loader_digests.txt).  A plain program: the loader is compiled
// into it, so that it also runs under -fsanitize=address,undefined with nothing preloaded.
//
//   loader_host_test FILE.fast5 ...        (taken in the order of their base names)
//
// The grid: f5_load_batch (keep 0, 100, 6656), f5_load_reads (the same, whole and a proper
// sub-range), f5_stream_open (keep 0, 6656), f5_load_batch_raw_ex and f5_stream_open_raw_ex
// (host_inflate_above 0, 1, 20000, -50 x flags 0..3), each with 1 and with 4 threads.  A line is
// the call, its arguments and the 64-bit FNV-1a digests of what came back.  No result depends on
// the thread count: the program fails if the lines for 1 and 4 threads differ.  A stream is one
// call and one line: its digests run over its containers in the order they come out.  Every raw
// batch is also decoded here, on the host, and held to the packed loaders' samples.
// Exit status: 0, or 1 with the differences on stderr.
#include "../deepbinner_amd/csrc/fast5_reader.cpp"

#include <cinttypes>
#include <cstdarg>

namespace loader_test {

int n_errors = 0;

uint64_t fnv1a(const void* data, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    for (size_t k = 0; k < n; ++k) h = (h ^ p[k]) * 0x100000001b3ull;
    return h;
}

std::string base_name(const std::string& path) {
    const size_t slash = path.rfind('/');
    return slash == std::string::npos ? path : path.substr(slash + 1);
}

std::string format(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
std::string format(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

// what a packed batch holds, copied out of it
struct Packed {
    std::vector<int64_t> offsets;
    std::vector<int32_t> status;
    std::vector<int16_t> samples;
};

Packed copy_packed(const f5_batch* b) {
    Packed p;
    const int64_t n = f5_batch_size(b);
    p.offsets.assign(f5_batch_offsets(b), f5_batch_offsets(b) + n + 1);
    p.status.assign(f5_batch_status(b), f5_batch_status(b) + n);
    if (p.offsets[(size_t)n] > 0)
        p.samples.assign(f5_batch_samples(b), f5_batch_samples(b) + p.offsets[(size_t)n]);
    return p;
}

// The digests of one call's line: of one batch, or of all the batches of a stream in the order
// they came out (each digest runs on from batch to batch).
struct Digests {
    static constexpr uint64_t kStart = 0xcbf29ce484222325ull;
    int64_t n = 0, streams = 0, comp_bytes = 0;
    uint64_t ids = kStart, offsets = kStart, status = kStart, data = kStart;

    void add_head(const f5_batch* b) {
        const int64_t k = f5_batch_size(b);
        n += k;
        ids = fnv1a(f5_batch_read_ids(b), (size_t)k * F5_READ_ID_MAX, ids);
        offsets = fnv1a(f5_batch_offsets(b), (size_t)(k + 1) * 8, offsets);
        status = fnv1a(f5_batch_status(b), (size_t)k * 4, status);
    }
    void add_packed(const f5_batch* b) {
        add_head(b);
        data = fnv1a(f5_batch_samples(b), (size_t)f5_batch_offsets(b)[f5_batch_size(b)] * 2, data);
    }
    // comp[0 : comp_bytes + 64] together with the records.  Bytes of the buffer that no record
    // claims (the place of a piece whose read failed while it was fetched: its records are
    // emptied, what lies there is whatever the recycled buffer held) count as zeros.
    void add_raw(const f5_batch* b) {
        add_head(b);
        const int64_t bytes = f5_batch_comp_bytes(b), k = f5_batch_n_streams(b);
        const f5_raw_stream* recs = f5_batch_streams(b);
        std::vector<uint8_t> comp((size_t)bytes + 64, 0);
        for (int64_t j = 0; j < k; ++j)
            if (recs[j].comp_bytes > 0)
                std::memcpy(&comp[(size_t)recs[j].comp_offset], f5_batch_comp(b) + recs[j].comp_offset,
                            (size_t)recs[j].comp_bytes);
        if (f5_batch_comp(b)) std::memcpy(&comp[(size_t)bytes], f5_batch_comp(b) + bytes, 64);
        streams += k;
        comp_bytes += bytes;
        data = fnv1a(recs, (size_t)k * sizeof(f5_raw_stream), fnv1a(comp.data(), comp.size(), data));
    }
    std::string text(bool raw) const {
        std::string t = format("n=%" PRId64 " ids=%016" PRIx64 " offsets=%016" PRIx64 " status=%016" PRIx64, n,
                               ids, offsets, status);
        if (!raw) return t + format(" samples=%016" PRIx64, data);
        return t + format(" streams=%" PRId64 " comp_bytes=%" PRId64 " comp+records=%016" PRIx64, streams,
                          comp_bytes, data);
    }
};

std::string packed_digests(const f5_batch* b) {
    Digests d;
    d.add_packed(b);
    return d.text(false);
}
std::string raw_digests(const f5_batch* b) {
    Digests d;
    d.add_raw(b);
    return d.text(true);
}

// `n` bytes of a zlib stream inflated (fewer if the stream ends before); false if zlib refuses it
bool inflate_some(const uint8_t* src, size_t src_bytes, uint8_t* dst, size_t n, size_t* got) {
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (inflateInit(&zs) != Z_OK) return false;
    zs.next_in = const_cast<uint8_t*>(src);
    zs.avail_in = (uInt)src_bytes;
    zs.next_out = dst;
    zs.avail_out = (uInt)n;
    const int rc = n ? inflate(&zs, Z_FINISH) : Z_STREAM_END;
    *got = n - zs.avail_out;
    inflateEnd(&zs);
    return rc == Z_STREAM_END || ((rc == Z_OK || rc == Z_BUF_ERROR) && *got == n);
}

void unshuffle(std::vector<uint8_t>* bytes) {
    const size_t n = bytes->size() / 2;
    std::vector<uint8_t> out(bytes->size());
    for (size_t k = 0; k < n; ++k) {
        out[2 * k] = (*bytes)[k];
        out[2 * k + 1] = (*bytes)[n + k];
    }
    bytes->swap(out);
}

// One record decoded on the host: stored pieces copied, zlib pieces through zlib, shuffle undone,
// VBZ through f5_vbz_decode; short output is zero-extended.  false: the piece does not decode.
bool decode_record(const uint8_t* comp, const f5_raw_stream& r, uint8_t* out) {
    const uint8_t* src = comp + r.comp_offset;
    const size_t want = (size_t)r.out_bytes;
    std::memset(out, 0, want);
    size_t got = 0;
    if (r.mode == F5_RAW_STORED) {
        std::memcpy(out, src, std::min((size_t)r.comp_bytes, want));
        return true;
    }
    if (r.mode == F5_RAW_ZLIB) return inflate_some(src, (size_t)r.comp_bytes, out, want, &got);
    if (r.mode == F5_RAW_ZLIB_SHUFFLE || r.mode == F5_RAW_STORED_SHUFFLE) {
        if (r.comp_bytes < 4) return false;
        const size_t n = (size_t)src[0] | (size_t)src[1] << 8 | (size_t)src[2] << 16 | (size_t)src[3] << 24;
        std::vector<uint8_t> planes(n, 0);
        if (r.mode == F5_RAW_STORED_SHUFFLE) {
            if ((size_t)r.comp_bytes - 4 != n) return false;
            std::memcpy(planes.data(), src + 4, n);
        } else if (!inflate_some(src + 4, (size_t)r.comp_bytes - 4, planes.data(), n, &got) || got != n) {
            return false;
        }
        unshuffle(&planes);
        std::memcpy(out, planes.data(), std::min(n, want));
        return true;
    }
    if (r.mode == F5_RAW_VBZ || r.mode == F5_RAW_VBZ_ZSTD) {
        if (r.comp_bytes < 4) return false;
        const uint32_t cd[4] = {0, 2, 1, r.mode == F5_RAW_VBZ_ZSTD ? 1u : 0u};
        const int64_t cap = ((int64_t)src[0] | (int64_t)src[1] << 8 | (int64_t)src[2] << 16 |
                             (int64_t)src[3] << 24) / 2;
        std::vector<int16_t> samples((size_t)cap + 1);
        int64_t n = 0;
        if (f5_vbz_decode(src, r.comp_bytes, cd, 4, cap, samples.data(), &n) != F5_OK) return false;
        std::memcpy(out, samples.data(), std::min((size_t)n * 2, want));
        return true;
    }
    return false;
}

// a raw batch decoded and held to the packed loader's batch of the same reads
void check_raw(const std::string& call, const f5_batch* b, const Packed& ref) {
    const int64_t n = f5_batch_size(b);
    if (n != (int64_t)ref.status.size()) {
        std::fprintf(stderr, "%s: %" PRId64 " reads, the packed loader has %zu\n", call.c_str(), n,
                     ref.status.size());
        ++n_errors;
        return;
    }
    const int64_t* offsets = f5_batch_offsets(b);
    std::vector<uint8_t> out((size_t)offsets[n] * 2 + 2, 0);
    std::vector<char> bad((size_t)n, 0);
    const f5_raw_stream* recs = f5_batch_streams(b);
    for (int64_t k = 0; k < f5_batch_n_streams(b); ++k) {
        const f5_raw_stream& r = recs[k];
        const int64_t i = r.reserved;
        if (i < 0 || i >= n || r.comp_offset < 0 || r.comp_bytes < 0 ||
            r.comp_offset + r.comp_bytes > f5_batch_comp_bytes(b) || r.out_offset < offsets[i] * 2 ||
            r.out_bytes < 0 || r.out_offset + r.out_bytes > offsets[i + 1] * 2) {
            std::fprintf(stderr, "%s: record %" PRId64 " out of bounds\n", call.c_str(), k);
            ++n_errors;
            return;
        }
        if (!decode_record(f5_batch_comp(b), r, &out[(size_t)r.out_offset])) bad[(size_t)i] = 1;
    }
    for (int64_t i = 0; i < n; ++i) {
        if (f5_batch_status(b)[i] != F5_OK || ref.status[(size_t)i] != F5_OK) continue;
        const int64_t len = offsets[i + 1] - offsets[i];
        const int64_t ref_len = ref.offsets[(size_t)i + 1] - ref.offsets[(size_t)i];
        if (bad[(size_t)i] || len != ref_len ||
            (len && std::memcmp(&out[(size_t)offsets[i] * 2], &ref.samples[(size_t)ref.offsets[(size_t)i]],
                                (size_t)len * 2) != 0)) {
            std::fprintf(stderr, "%s: read %" PRId64 " decodes to other samples than the packed loader's%s\n",
                         call.c_str(), i, bad[(size_t)i] ? " (a piece does not decode)" : "");
            ++n_errors;
        }
    }
}

// all containers of a stream: one line for the call, their statuses in path order in it
void drain(f5_stream* s, const std::string& call, const std::vector<std::string>& paths, bool raw,
           const std::vector<Packed>* refs, std::vector<std::string>* lines) {
    Digests d;
    std::string statuses;
    for (;;) {
        int64_t index = -1;
        int status = -1;
        f5_batch* b = nullptr;
        if (f5_stream_next(s, &index, &status, &b) != F5_OK) break;
        statuses += format("%d", status);
        if (!b) continue;
        if (raw) d.add_raw(b);
        else d.add_packed(b);
        if (raw && refs)
            check_raw(call + " container " + base_name(paths[(size_t)index]), b, (*refs)[(size_t)index]);
        f5_batch_free(b);
    }
    f5_stream_close(s);
    lines->push_back(call + " containers=" + statuses + " " + d.text(raw));
}

std::vector<std::string> run_grid(const std::vector<std::string>& paths, int threads,
                                  const Packed* batch_ref, const std::vector<Packed>* read_refs) {
    std::vector<std::string> lines;
    std::vector<const char*> c_paths;
    for (const std::string& p : paths) c_paths.push_back(p.c_str());
    const int64_t n = (int64_t)paths.size();
    const int64_t keeps[] = {0, 100, 6656};

    for (int64_t keep : keeps) {
        f5_batch* b = nullptr;
        const int rc = f5_load_batch(c_paths.data(), n, keep, threads, &b);
        lines.push_back(format("f5_load_batch keep=%" PRId64 " rc=%d ", keep, rc) + (b ? packed_digests(b) : ""));
        f5_batch_free(b);
    }
    for (const std::string& path : paths) {
        int64_t n_reads = 0;
        for (int64_t keep : keeps)
            for (int sub = 0; sub < 2; ++sub) {
                // the proper sub-range: without the first read, and without the last where there are three
                const int64_t first = sub, count = sub ? std::max<int64_t>(n_reads - 2, 1) : -1;
                if (sub && n_reads < 2) continue;
                f5_batch* b = nullptr;
                const int rc = f5_load_reads(path.c_str(), first, count, keep, threads, &b);
                if (b && !sub) n_reads = f5_batch_size(b);
                lines.push_back(format("f5_load_reads %s first=%" PRId64 " count=%" PRId64 " keep=%" PRId64 " rc=%d ",
                                       base_name(path).c_str(), first, count, keep, rc) +
                                (b ? packed_digests(b) : ""));
                f5_batch_free(b);
            }
    }
    for (int64_t keep : {(int64_t)0, (int64_t)6656}) {
        f5_stream* s = nullptr;
        const std::string call = format("f5_stream_open keep=%" PRId64, keep);
        const int rc = f5_stream_open(c_paths.data(), n, keep, threads, 0, &s);
        if (rc != F5_OK) lines.push_back(call + format(" rc=%d", rc));
        else drain(s, call, paths, false, nullptr, &lines);
    }
    for (int64_t above : {(int64_t)0, (int64_t)1, (int64_t)20000, (int64_t)-50})
        for (unsigned flags = 0; flags < 4; ++flags) {
            f5_batch* b = nullptr;
            std::string call = format("f5_load_batch_raw_ex host_inflate_above=%" PRId64 " flags=%u", above, flags);
            int rc = f5_load_batch_raw_ex(c_paths.data(), n, threads, above, flags, &b);
            lines.push_back(call + format(" rc=%d ", rc) + (b ? raw_digests(b) : ""));
            if (b && batch_ref) check_raw(call, b, *batch_ref);
            f5_batch_free(b);
            f5_stream* s = nullptr;
            call = format("f5_stream_open_raw_ex host_inflate_above=%" PRId64 " flags=%u", above, flags);
            rc = f5_stream_open_raw_ex(c_paths.data(), n, threads, 0, above, flags, &s);
            if (rc != F5_OK) lines.push_back(call + format(" rc=%d", rc));
            else drain(s, call, paths, true, read_refs, &lines);
        }
    return lines;
}

}  // namespace loader_test

int main(int argc, char** argv) {
    using namespace loader_test;
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s FILE.fast5 ...\n", argv[0]);
        return 2;
    }
    std::vector<std::string> paths(argv + 1, argv + argc);
    std::sort(paths.begin(), paths.end(), [](const std::string& a, const std::string& b) {
        return std::make_pair(base_name(a), a) < std::make_pair(base_name(b), b);
    });
    std::vector<const char*> c_paths;
    for (const std::string& p : paths) c_paths.push_back(p.c_str());

    // what the raw batches have to decode to: the packed loaders' whole reads
    Packed batch_ref;
    std::vector<Packed> read_refs(paths.size());
    f5_batch* b = nullptr;
    if (f5_load_batch(c_paths.data(), (int64_t)paths.size(), 0, 1, &b) == F5_OK) batch_ref = copy_packed(b);
    f5_batch_free(b);
    for (size_t k = 0; k < paths.size(); ++k) {
        b = nullptr;
        if (f5_load_reads(c_paths[k], 0, -1, 0, 1, &b) == F5_OK) read_refs[k] = copy_packed(b);
        f5_batch_free(b);
    }

    const std::vector<std::string> one = run_grid(paths, 1, &batch_ref, &read_refs);
    const std::vector<std::string> four = run_grid(paths, 4, &batch_ref, &read_refs);
    for (const std::string& line : one) std::printf("threads=1 %s\n", line.c_str());
    for (const std::string& line : four) std::printf("threads=4 %s\n", line.c_str());
    if (one.size() != four.size()) {
        std::fprintf(stderr, "%zu lines with 1 thread, %zu with 4\n", one.size(), four.size());
        ++n_errors;
    }
    for (size_t k = 0; k < std::min(one.size(), four.size()); ++k)
        if (one[k] != four[k]) {
            std::fprintf(stderr, "1 and 4 threads differ:\n  %s\n  %s\n", one[k].c_str(), four[k].c_str());
            ++n_errors;
        }
    if (n_errors) std::fprintf(stderr, "loader_host_test: %d differences\n", n_errors);
    return n_errors ? 1 : 0;
}
