// TEST INFRASTRUCTURE (oracle/): the host-side arithmetic of libdeepbinner_hip.so's API layer
// (deepbinner_amd/csrc/dbh_host_layout.h, dbh_network.h and dbh_pack.h, the very headers the library
// is compiled from) as a program
// of its own, so that tests/test_api_host.py can hold it to account on the build box, without a
// GPU - and so that it can run under AddressSanitizer (oracle/Makefile: api_host_test_asan).  Not
// part of the product; nothing in deepbinner_amd/ calls it.
//   api_host_test [RECORDS]      RECORDS: a file of dbh_inflate_stream records
// One line per check, "ok ..." or "FAIL ..."; "model_steps INPUT SCAN = STEPS", "offsets_forwards
// CASE = ok TOTAL | bad" and "chunk_flags FLAGS = ok | bad" (what the pure checks of the host units'
// arguments answer) and, with RECORDS, "order I J K ..." for the caller to compare.  Exit status 1 if
// a check failed.
//   api_host_test --network [BLOB CLASSES]...      BLOB: a canonical weight blob (fp32) of CLASSES
// The network table of dbh_network.h ("conv", "bn", "bn_eps", "param_count", "blob",
// "stage_lengths", "same_pad_left") and, per BLOB, "packed persistent|general NAME CLASSES FLOATS
// DIGEST": the 64-bit FNV-1a digest of each image dbh_pack.h makes of it - for the caller to compare.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../deepbinner_amd/csrc/dbh_host_layout.h"
#include "../deepbinner_amd/csrc/dbh_pack.h"

static int g_failed = 0;

static void report(bool ok, const char* what, long a = 0, long b = 0, long c = 0) {
    std::printf("%s %s %ld %ld %ld\n", ok ? "ok" : "FAIL", what, a, b, c);
    if (!ok) ++g_failed;
}

// regions (offset, bytes) in the order they are meant to lie in: each starts where the one before
// ended (so none overlap and the total is the sum), on a multiple of `align`
static bool tiles(const std::vector<std::pair<size_t, size_t>>& regions, size_t total, size_t align) {
    size_t at = 0;
    for (const auto& r : regions) {
        if (r.first != at || r.first % align != 0) return false;
        at += r.second;
    }
    return at == total;
}

static void check_layouts() {
    using dbh_host::align256;
    // the small buffer of the deflated path: zero streams, one read, odd counts, a container's worth
    const long cases[][2] = {{0, 1}, {1, 1}, {3, 1}, {0, 5}, {7, 40}, {64, 64}, {4001, 4000}};
    for (const auto& c : cases) {
        const long n_streams = c[0], n_reads = c[1];
        const dbh_host::DeflatedSmall s(n_streams, n_reads);
        const size_t calls = align256((size_t)n_reads * 4);
        const bool ok = tiles({{s.records, align256((size_t)n_streams * sizeof(dbh_inflate_stream))},
                               {s.offsets, align256((size_t)(n_reads + 1) * 8)},
                               {s.status, align256((size_t)n_streams * 4)},
                               {s.final_calls, calls},
                               {s.side_calls[0], calls},
                               {s.side_calls[1], calls}},
                              s.total, 256) &&
                        s.in_bytes == s.status && s.in_bytes + s.out_bytes == s.total;
        report(ok, "layout deflated", n_streams, n_reads);
    }
    // a group's results on the host path: the start model alone, the end model alone, both
    for (int has = 1; has <= 3; ++has)
        for (long n_reads : {1L, 37L})
            for (int n_classes : {2, 13}) {
                const bool start = has & 1, end = has & 2;
                const dbh_host::GroupOut g(n_reads, n_classes, start, end);
                const size_t probs = (size_t)n_reads * n_classes * 4, calls = (size_t)n_reads * 4;
                const bool ok = tiles({{g.probs[0], start ? probs : 0},
                                       {g.probs[1], end ? probs : 0},
                                       {g.calls[0], start ? calls : 0},
                                       {g.calls[1], end ? calls : 0},
                                       {g.final_calls, start && end ? calls : 0}},
                                      g.total, 4);
                report(ok, "layout group", has, n_reads, n_classes);
            }
    // a group's results of the sweep, a Carve: the sizing pass (null base: null pointers) ends at the
    // same `used` as the carving pass; a present side's best then its margin, start before end, tile
    // the buffer on multiples of 256 bytes; an absent side has null pointers and takes no bytes; and
    // the buffer, allocated with exactly `total` bytes, takes a write to every region's two ends
    for (int has = 1; has <= 3; ++has)
        for (long n_reads : {0L, 1L, 300L})
            for (int steps : {1, 24}) {
                const bool present[2] = {(has & 1) != 0, (has & 2) != 0};
                const dbh_host::SweepOut sized(nullptr, n_reads, steps, present[0], present[1]);
                std::vector<char> buffer(sized.total ? sized.total : 1);      // (data() is never null)
                const dbh_host::SweepOut s(buffer.data(), n_reads, steps, present[0], present[1]);
                const size_t cells = (size_t)n_reads * steps;
                bool ok = sized.total == s.total && s.total % 256 == 0;
                std::vector<std::pair<size_t, size_t>> regions;
                for (int j = 0; j < 2; ++j) {
                    ok = ok && !sized.best[j] && !sized.margin[j];
                    if (!present[j]) {
                        ok = ok && !s.best[j] && !s.margin[j];
                        continue;
                    }
                    ok = ok && s.best[j] && s.margin[j];
                    regions.push_back({(size_t)((char*)s.best[j] - buffer.data()), align256(cells * 4)});
                    regions.push_back({(size_t)((char*)s.margin[j] - buffer.data()), align256(cells * 8)});
                    if (cells) {
                        s.best[j][0] = s.best[j][cells - 1] = j;
                        s.margin[j][0] = s.margin[j][cells - 1] = 0.5;
                    }
                }
                ok = ok && tiles(regions, s.total, 256) &&
                     s.total == (size_t)(present[0] + present[1]) * (align256(cells * 4) + align256(cells * 8));
                report(ok, "layout sweep", has, n_reads, steps);
            }
}

// Carve: one sequence of take() calls, over a null base (the sizing pass) and over a buffer (the
// carving pass).  Both end at the same `used`; the sizing pass hands out null pointers only; every
// carved pointer lies a multiple of 256 bytes behind the base, where the one before it ended; no
// elements take no bytes; and the buffer, allocated with exactly `used` bytes, takes a write to
// every region's first and last byte (the sanitizer build is what holds that to account).
static void check_carve() {
    const size_t counts[] = {0, 1, 63, 64, 65, 1000, 4097};     // elements per take, three types each
    auto run = [&](void* base, std::vector<char*>& got, std::vector<size_t>& bytes) {
        dbh_host::Carve c(base);
        for (size_t n : counts) {
            got.push_back((char*)c.take<char>(n));
            bytes.push_back(n);
            got.push_back((char*)c.take<int32_t>(n));
            bytes.push_back(n * 4);
            got.push_back((char*)c.take<double>(n));
            bytes.push_back(n * 8);
        }
        return c.used;
    };
    std::vector<char*> sized, carved;
    std::vector<size_t> bytes, bytes_again;
    const size_t need = run(nullptr, sized, bytes);
    std::vector<char> buffer(need);
    const size_t used = run(buffer.data(), carved, bytes_again);
    report(need == used && need % 256 == 0, "carve used", (long)need, (long)used);
    bool all_null = true, aligned = true, in_order = true;
    size_t at = 0;
    for (size_t k = 0; k < carved.size(); ++k) {
        all_null = all_null && sized[k] == nullptr;
        const size_t offset = (size_t)(carved[k] - buffer.data());
        aligned = aligned && offset % 256 == 0;
        in_order = in_order && offset == at;
        at += dbh_host::align256(bytes[k]);
        if (bytes[k]) carved[k][0] = carved[k][bytes[k] - 1] = (char)k;
    }
    report(all_null, "carve null_base");
    report(aligned, "carve aligned");
    report(in_order && at == used, "carve in_order", (long)at);
    dbh_host::Carve none(buffer.data());
    report(none.take<char>(0) == buffer.data() && none.used == 0 && none.take<double>(0) == (double*)buffer.data() &&
               none.used == 0,
           "carve take_nothing");
    report(dbh_host::blocks_for(0, 256) == 0 && dbh_host::blocks_for(1, 256) == 1 &&
               dbh_host::blocks_for(256, 256) == 1 && dbh_host::blocks_for(257, 256) == 2 &&
               dbh_host::blocks_for((1LL << 40) + 1, 1024) == (1u << 30) + 1,
           "blocks_for");
}

// destination byte-equal to the source, the guard bytes on both sides untouched; and the pieces
// the copy is cut into cover the buffer once
static void check_staged_copy() {
    const size_t MiB = 1u << 20, kGuard = 64;
    for (size_t bytes : {(size_t)0, (size_t)1, 16 * MiB - 1, 16 * MiB, 32 * MiB, 32 * MiB + 4097}) {
        std::vector<unsigned char> src(bytes + 1), dst(bytes + 2 * kGuard, 0xEE);
        uint32_t x = 0x9E3779B9u ^ (uint32_t)bytes;
        for (size_t i = 0; i < bytes; ++i) {
            x = x * 1664525u + 1013904223u;
            src[i] = (unsigned char)(x >> 24);
        }
        dbh_host::staged_copy(dst.data() + kGuard, src.data(), bytes);
        bool ok = std::memcmp(dst.data() + kGuard, src.data(), bytes) == 0;
        for (size_t i = 0; i < kGuard; ++i) ok = ok && dst[i] == 0xEE && dst[kGuard + bytes + i] == 0xEE;
        const dbh_host::CopySplit split = dbh_host::copy_split(bytes);
        ok = ok && (split.helpers == 0 ? split.share == bytes
                                       : split.share % 4096 == 0 && split.share * (size_t)(split.helpers + 1) >= bytes &&
                                             split.share * (size_t)split.helpers < bytes);
        report(ok, "staged_copy", (long)bytes, split.helpers);
    }
}

static void check_uniform_length() {
    const int64_t same[] = {0, 512, 1024, 1536}, ragged[] = {0, 512, 1024, 1537}, empty[] = {0, 0, 0};
    report(dbh_host::uniform_length(same, 3) == 512 && dbh_host::uniform_length(same, 1) == 512 &&
               dbh_host::uniform_length(ragged, 3) == 0 && dbh_host::uniform_length(ragged, 2) == 512 &&
               dbh_host::uniform_length(empty, 2) == 0,
           "uniform_length");
}

// what the host units' pure argument checks answer, a line each for the caller to compare: do the
// offsets run forwards (and the samples they span), is a live chunk's flag word BEGIN, END, both or
// neither
static void print_argument_checks() {
    struct Table { const char* name; std::vector<int64_t> offsets; };
    const Table tables[] = {
        {"empty", {}},                                   // no read: the table is not looked at
        {"one_read_no_samples", {5, 5}},
        {"forwards", {0, 3, 3, 10}},
        {"backward_first", {4, 3, 8, 10}},
        {"backward_middle", {0, 6, 5, 10}},
        {"backward_last", {0, 3, 8, 7}},
        {"first_not_zero", {100, 103, 110}},
    };
    for (const Table& t : tables) {
        const int64_t n_reads = t.offsets.empty() ? 0 : (int64_t)t.offsets.size() - 1;
        int64_t total = -1;
        const bool ok = dbh_host::offsets_run_forwards(t.offsets.empty() ? nullptr : t.offsets.data(),
                                                       n_reads, &total);
        if (ok) std::printf("offsets_forwards %s = ok %lld\n", t.name, (long long)total);
        else std::printf("offsets_forwards %s = bad\n", t.name);
    }
    // each flag bit beside one bit outside the mask, and the words a session takes
    for (uint32_t flags : {0u, (uint32_t)DBH_LIVE_BEGIN, (uint32_t)DBH_LIVE_END,
                           (uint32_t)(DBH_LIVE_BEGIN | DBH_LIVE_END), 4u, DBH_LIVE_BEGIN | 4u,
                           DBH_LIVE_END | 4u, DBH_LIVE_BEGIN | DBH_LIVE_END | 0x80000000u})
        std::printf("chunk_flags %u = %s\n", flags, dbh_host::live_chunk_flags_ok(flags) ? "ok" : "bad");
}

// the network as dbh_network.h has it, for the caller to hold to model_format.py and the oracle
static void print_network() {
    namespace net = dbh_net;
    for (int i = 0; i < net::kNumConvs; ++i) {
        const net::Conv& c = net::kConvs[i];
        std::printf("conv %d %d %d %d %d in %d out %d\n", i + 1, c.k, c.cin, c.cout, c.stride, c.in, c.out);
    }
    for (int j = 0; j < net::kNumBn; ++j) std::printf("bn %d %d\n", j + 1, net::kBnChannels[j]);
    std::printf("bn_eps %.17g\n", net::kBnEps);
    for (int n_classes : {2, 13, 32, 33, 256})
        std::printf("param_count %d %lld\n", n_classes, (long long)net::param_count(n_classes));
    for (int n_classes : {2, 256}) {
        std::printf("blob %d", n_classes);      // kernel and bias of conv 1..20, then BN 1..7
        for (int i = 0; i < net::kNumConvs; ++i)
            std::printf(" %zu %zu", net::blob_kernel(i, n_classes), net::blob_bias(i, n_classes));
        for (int j = 0; j < net::kNumBn; ++j) std::printf(" %zu", net::blob_bn(j, n_classes));
        std::printf("\n");
    }
    for (int L : {96, 98, 200, 1024, 16382, 16384}) {
        int len[8];
        net::stage_lengths(L, len);
        std::printf("stage_lengths");
        for (int v : len) std::printf(" %d", v);
        std::printf("\n");
    }
    // every (k, stride) of the table, output length as SAME gives it
    for (int i = 0; i < net::kNumConvs; ++i)
        for (int lin : {1, 2, 3, 6, 7}) {
            const int k = net::kConvs[i].k, stride = net::kConvs[i].stride;
            const int lout = (lin + stride - 1) / stride;
            std::printf("same_pad_left %d %d %d %d = %d\n", k, stride, lin, lout,
                        net::same_pad_left(k, stride, lin, lout));
        }
}

// 64-bit FNV-1a, as oracle/loader_host_test.cpp has it
static uint64_t fnv1a(const void* data, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    for (size_t k = 0; k < n; ++k) h = (h ^ p[k]) * 0x100000001b3ull;
    return h;
}

// both packed images of a canonical blob (a file of little-endian fp32), a line each
static bool print_packed(const char* path, int n_classes) {
    if (n_classes < 2 || n_classes > 256) return false;
    std::vector<float> blob((size_t)dbh_net::param_count(n_classes));
    FILE* in = std::fopen(path, "rb");
    if (!in) return false;
    const size_t got = std::fread(blob.data(), sizeof(float), blob.size(), in);
    const bool whole = got == blob.size() && std::fgetc(in) == EOF;     // the blob and nothing else
    std::fclose(in);
    if (!whole) return false;
    const char* slash = std::strrchr(path, '/');
    const char* name = slash ? slash + 1 : path;
    if (n_classes <= dbh::kMaxClasses) {
        std::vector<float> packed;
        dbh_pack::pack_persistent(blob.data(), n_classes, packed);
        std::printf("packed persistent %s %d %zu %016" PRIx64 "\n", name, n_classes, packed.size(),
                    fnv1a(packed.data(), packed.size() * sizeof(float)));
    }
    dbh_pack::GeneralOffsets g;
    const std::vector<float> packed = dbh_pack::pack_general(blob.data(), n_classes, &g);
    uint64_t offsets = fnv1a(g.w_off, sizeof(g.w_off));
    offsets = fnv1a(g.b_off, sizeof(g.b_off), offsets);
    offsets = fnv1a(g.sc_off, sizeof(g.sc_off), offsets);
    offsets = fnv1a(g.sh_off, sizeof(g.sh_off), offsets);
    std::printf("packed general %s %d %zu %016" PRIx64 " offsets %016" PRIx64 "\n", name, n_classes,
                packed.size(), fnv1a(packed.data(), packed.size() * sizeof(float)), offsets);
    return true;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--network") == 0) {
        print_network();
        for (int a = 2; a + 1 < argc; a += 2)
            if (!print_packed(argv[a], std::atoi(argv[a + 1]))) return 2;
        return 0;
    }
    check_layouts();
    check_carve();
    check_staged_copy();
    check_uniform_length();
    print_argument_checks();
    for (int input : {96, 1024, 2048})
        for (int scan : {0, 48, 96, 512, 1000, 1024, 1536, 2048, 6144, 6145, 6192})
            std::printf("model_steps %d %d = %d\n", input, scan, dbh_host::model_steps(input, scan));
    if (argc > 1) {
        FILE* in = std::fopen(argv[1], "rb");
        if (!in) return 2;
        std::vector<dbh_inflate_stream> records;
        dbh_inflate_stream r;
        while (std::fread(&r, sizeof(r), 1, in) == 1) records.push_back(r);
        std::fclose(in);
        std::vector<int32_t> order;
        dbh_host::record_order(records.data(), (int64_t)records.size(), order);
        std::printf("order");
        for (int32_t i : order) std::printf(" %d", i);
        std::printf("\n");
    }
    return g_failed ? 1 : 0;
}
