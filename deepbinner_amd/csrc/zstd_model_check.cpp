// zstd_model_check.cpp - the CPU model of the GPU's zstd decoder (dbz::decode_host, dbh_zstd_core.h)
// on the frames of tests/zstd_written.py, each in a heap block of exactly its size + 64 (the
// padding a caller owes the decoder) and decoded into a heap block of exactly the capacity given,
// so that AddressSanitizer and UBSan see any byte read or written outside them.  `make zstd_check`
// writes the frames (python tests/zstd_written.py --dump FILE: [u32 frame bytes][u32 capacity]
// [frame] records), builds this and runs it; it needs no device.  A status and a hash of the bytes
// per record go to stdout.
#include "dbh_zstd_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: zstd_model_check FILE\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::vector<uint8_t> all;
    uint8_t buf[1 << 16];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
    std::fclose(f);
    long records = 0, accepted = 0;
    size_t at = 0;
    while (at < all.size()) {
        if (all.size() - at < 8) {
            std::fprintf(stderr, "a record's head is cut short at byte %zu\n", at);
            return 2;
        }
        const uint32_t frame_bytes = dbz::le32(all.data() + at), capacity = dbz::le32(all.data() + at + 4);
        at += 8;
        if (all.size() - at < frame_bytes) {
            std::fprintf(stderr, "record %ld is cut short\n", records);
            return 2;
        }
        uint8_t* frame = (uint8_t*)std::malloc((size_t)frame_bytes + 64);
        uint8_t* out = (uint8_t*)std::malloc(capacity ? capacity : 1);
        std::memcpy(frame, all.data() + at, frame_bytes);
        std::memset(frame + frame_bytes, 0, 64);
        at += frame_bytes;
        size_t produced = 0;
        const int status = dbz::decode_host(frame, frame_bytes, out, capacity, &produced);
        uint64_t hash = 0xcbf29ce484222325ull;              // FNV-1a of what was produced
        if (status == dbz::kOk)
            for (size_t k = 0; k < produced; ++k) hash = (hash ^ out[k]) * 0x100000001b3ull;
        std::printf("%ld\t%d\t%zu\t%016llx\n", records, status, status == dbz::kOk ? produced : (size_t)0,
                    (unsigned long long)hash);
        accepted += status == dbz::kOk;
        ++records;
        std::free(frame);
        std::free(out);
    }
    std::fprintf(stderr, "zstd_model_check: %ld records, %ld accepted: clean\n", records, accepted);
    return records ? 0 : 2;
}
