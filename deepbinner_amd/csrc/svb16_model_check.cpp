// svb16_model_check.cpp - the rules of POD5's 16-bit streamvbyte code (dbh_svb16_core.h: the lines
// the GPU's wave and dbh_svb16_decode_host compile) under AddressSanitizer + UBSan, as a program of
// its own (make svb16_asan): decode_host over every length 0 .. 2,100 with random key patterns,
// with all values one byte and all values two bytes, every stream and every output a heap block of
// exactly its size, so that an access one byte outside is caught, against a plain loop written
// here - one value at a time; every stream once more cut by one byte and once more extended by one
// byte, both of which must be refused with zeros.  No device, no Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dbh_svb16_core.h"

namespace {

int failures = 0;

template <typename T>
T* exactly(size_t count) {          // a heap block of exactly count elements (one of size 0: 1 byte)
    T* p = (T*)std::malloc(count ? count * sizeof(T) : 1);
    if (!p) std::abort();
    return p;
}

unsigned long long state = 0x9E3779B97F4A7C15ull;
unsigned long long draw() {         // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return state * 0x2545F4914F6CDD1Dull;
}

// the code said again, one value at a time: samples -> stream
std::vector<uint8_t> encode_plain(const std::vector<int16_t>& samples) {
    const size_t n = samples.size();
    std::vector<uint8_t> keys((n + 7) / 8, 0), data;
    uint16_t before = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint16_t now = (uint16_t)samples[i];
        const uint16_t delta = (uint16_t)(now - before);
        before = now;
        const uint16_t v = (uint16_t)((uint16_t)(delta << 1) ^ (uint16_t)(0 - (delta >> 15)));
        data.push_back((uint8_t)(v & 0xFF));
        if (v > 0xFF) {
            keys[i >> 3] |= (uint8_t)(1u << (i & 7));
            data.push_back((uint8_t)(v >> 8));
        }
    }
    keys.insert(keys.end(), data.begin(), data.end());
    return keys;
}

// ... and stream -> samples; false where the data do not end with the stream
bool decode_plain(const std::vector<uint8_t>& stream, size_t n, std::vector<int16_t>& out) {
    const size_t keys = (n + 7) / 8;
    out.assign(n, 0);
    if (keys > stream.size()) return false;
    size_t at = keys;
    uint16_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool two = (stream[i >> 3] >> (i & 7)) & 1;
        if (at + (two ? 2 : 1) > stream.size()) return false;
        uint16_t v = stream[at];
        if (two) v = (uint16_t)(v | (stream[at + 1] << 8));
        at += two ? 2 : 1;
        sum = (uint16_t)(sum + (uint16_t)((v >> 1) ^ (uint16_t)(0 - (v & 1))));
        out[i] = (int16_t)sum;
    }
    return at == stream.size();
}

// one stream through decode_host from heap blocks of exactly its sizes, against decode_plain
void check(const std::vector<uint8_t>& stream, size_t n, const char* what) {
    std::vector<int16_t> want;
    const bool ok = decode_plain(stream, n, want);
    if (!ok) want.assign(n, 0);
    uint8_t* in = exactly<uint8_t>(stream.size());
    if (!stream.empty()) std::memcpy(in, stream.data(), stream.size());
    int16_t* out = exactly<int16_t>(n);
    for (size_t k = 0; k < n; ++k) out[k] = 0x5A5A;
    const int status = dbh_svb16::decode_host(in, (int64_t)stream.size(), (int64_t)n, out);
    bool same = status == (ok ? 0 : dbh_svb16::kRefused);
    for (size_t k = 0; same && k < n; ++k) same = out[k] == want[k];
    if (!same) {
        ++failures;
        std::fprintf(stderr, "svb16 %s: n = %zu, %zu bytes, status %d, plain loop %s\n", what, n,
                     stream.size(), status, ok ? "accepts" : "refuses");
    }
    std::free(in);
    std::free(out);
}

void family(const std::vector<int16_t>& samples, const char* what) {
    const size_t n = samples.size();
    std::vector<uint8_t> stream = encode_plain(samples);
    std::vector<int16_t> back;
    if (!decode_plain(stream, n, back) || back != samples) {
        ++failures;
        std::fprintf(stderr, "svb16 %s: the plain loops disagree at n = %zu\n", what, n);
    }
    check(stream, n, what);
    if (!stream.empty()) {          // every truncation by one byte ...
        std::vector<uint8_t> cut(stream.begin(), stream.end() - 1);
        check(cut, n, "cut by one byte");
    }
    std::vector<uint8_t> more = stream;     // ... and every extension by one
    more.push_back((uint8_t)draw());
    check(more, n, "extended by one byte");
}

}  // namespace

int main() {
    long long streams = 0;
    for (size_t n = 0; n <= 2100; ++n) {
        std::vector<int16_t> random(n), small(n), large(n);
        uint16_t r = 0, s = 0, l = 0;
        const unsigned density = (unsigned)(draw() % 9);      // how many of eight values take two bytes
        for (size_t i = 0; i < n; ++i) {
            const bool two = (draw() & 7) < density;
            const uint16_t step = two ? (uint16_t)(128 + draw() % 32640) : (uint16_t)(draw() % 128);
            r = (uint16_t)(r + ((draw() & 1) ? step : (uint16_t)(0 - step)));
            random[i] = (int16_t)r;
            s = (uint16_t)(s + ((draw() & 1) ? (uint16_t)(draw() % 128) : (uint16_t)(0 - (draw() % 129))));
            small[i] = (int16_t)s;      // |delta| <= 127 or -128: one byte each
            l = (uint16_t)(l + ((draw() & 1) ? (uint16_t)(128 + draw() % 32640) : (uint16_t)(0 - (129 + draw() % 32640))));
            large[i] = (int16_t)l;      // two bytes each, -32,768 and 32,767 among the deltas
        }
        family(random, "random keys");
        family(small, "all one byte");
        family(large, "all two bytes");
        streams += 9;
    }
    // the deltas at the edges of 16 bits, and back
    family({-32768, 32767, -32768, 0, 32767, 0, -1, 1}, "wrapping deltas");
    // unused bits of the last key byte are not looked at
    {
        std::vector<int16_t> three = {1, -300, 7};
        std::vector<uint8_t> stream = encode_plain(three);
        stream[0] |= 0xF8;
        check(stream, 3, "unused key bits");
    }
    if (failures) {
        std::fprintf(stderr, "svb16_model_check: %d failures\n", failures);
        return 1;
    }
    std::printf("svb16_model_check: %lld streams, lengths 0 .. 2100, no failure\n", streams);
    return 0;
}
