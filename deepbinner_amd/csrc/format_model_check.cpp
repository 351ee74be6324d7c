// format_model_check.cpp - the CPU models of the random-signal generator and of the training-data
// text formatter (dbh_random_signals_host, dbh_text_format_host: dbh_random.hip and dbh_format.hip
// compiled as plain C++ with their core headers) in heap blocks of exactly the sizes the entries are
// told, so that AddressSanitizer and UBSan see any byte read or written outside them.
// `make format_asan` builds and runs it; it needs no device and no Python.  Every text is also held
// to snprintf and read back by the parser's model (dbh_text_parse_host).
#include "dbh_format.hip"
#include "dbh_random.hip"
#include "dbh_text.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

long g_texts = 0, g_signals = 0;

std::string plain_text(const std::vector<int32_t>& labels, const std::vector<int16_t>& samples, int size) {
    std::string text;
    char number[16];
    for (size_t k = 0; k < labels.size(); ++k) {
        std::snprintf(number, sizeof(number), "%d", labels[k]);
        text += number;
        for (int i = 0; i < size; ++i) {
            std::snprintf(number, sizeof(number), "%c%d", i ? ',' : '\t', (int)samples[k * size + i]);
            text += number;
        }
        text += '\n';
    }
    return text;
}

// labels and samples in blocks of their own size; the text at its exact length, then one byte short
bool check_text(const std::vector<int32_t>& labels_in, const std::vector<int16_t>& samples_in, int size) {
    const int64_t n = (int64_t)labels_in.size();
    const std::string want = plain_text(labels_in, samples_in, size);
    const int64_t need = (int64_t)want.size();
    int32_t* labels = (int32_t*)std::malloc(labels_in.size() * sizeof(int32_t));
    int16_t* samples = (int16_t*)std::malloc(samples_in.size() * sizeof(int16_t));
    std::memcpy(labels, labels_in.data(), labels_in.size() * sizeof(int32_t));
    std::memcpy(samples, samples_in.data(), samples_in.size() * sizeof(int16_t));
    bool ok = true;
    int64_t bound = 0;
    ok = ok && dbh_text_format_bound(n, size, &bound) == 0 && need <= bound;
    for (int short_by = 0; short_by <= 1 && ok; ++short_by) {
        const int64_t capacity = need - short_by;
        uint8_t* out = (uint8_t*)std::malloc((size_t)capacity + 1);      // (+ 1: capacity may be 0)
        std::memset(out, 0xa5, (size_t)capacity + 1);
        int64_t n_bytes = -7;
        const int st = dbh_text_format_host(labels, samples, n, size, out, capacity, &n_bytes);
        ok = ok && n_bytes == need && out[capacity] == 0xa5;
        if (short_by) {
            ok = ok && st == 1;
            for (int64_t p = 0; p < capacity; ++p) ok = ok && out[p] == 0xa5;
        } else {
            ok = ok && st == 0 && std::memcmp(out, want.data(), (size_t)need) == 0;
            // and back through the parser's model
            std::vector<int16_t> back((size_t)n * size);
            std::vector<int32_t> back_labels((size_t)n);
            std::vector<uint8_t> kinds((size_t)n);
            int64_t lines = 0, first_bad = 0;
            ok = ok && dbh_text_parse_host(out, need, size, n, back.data(), back_labels.data(), kinds.data(),
                                           &lines, &first_bad) == 0;
            ok = ok && lines == n && first_bad == -1 && back == samples_in && back_labels == labels_in;
        }
        std::free(out);
    }
    std::free(labels);
    std::free(samples);
    g_texts += 1;
    if (!ok) std::fprintf(stderr, "format_model_check: a text of %ld lines of %d values failed\n", (long)n, size);
    return ok;
}

bool check_signals(uint64_t seed, int64_t first, int64_t n, int size, int* kinds_seen) {
    int16_t* out = (int16_t*)std::malloc((size_t)n * size * sizeof(int16_t));
    bool ok = dbh_random_signals_host(seed, first, n, size, out) == 0;
    std::vector<int32_t> labels((size_t)n, 0);
    std::vector<int16_t> samples(out, out + n * size);
    for (int64_t k = 0; k < n; ++k)
        kinds_seen[dbr::signal_of((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(first + k)).kind] += 1;
    std::free(out);
    g_signals += n;
    return ok && check_text(labels, samples, size);
}

}  // namespace

int main() {
    bool ok = true;
    const int16_t extremes[] = {0, -1, 9, -9, 10, -10, 99, -99, 100, -100, 999, 1000, -1000, 9999, 10000,
                                -10000, 32767, -32767, -32768};
    const int32_t labels[] = {0, 7, 10, 255, -1, 999999999, -999999999, 100000000};
    const int n_extremes = (int)(sizeof(extremes) / sizeof(extremes[0]));
    for (int size : {1, 2, 63, 64, 65, 1024}) {
        std::vector<int32_t> l(labels, labels + 8);
        std::vector<int16_t> s((size_t)8 * size);
        for (size_t p = 0; p < s.size(); ++p) s[p] = extremes[(p * 7 + p / size) % n_extremes];
        for (int i = 0; i < size; ++i) s[i] = -32768;                     // the widest line
        ok = ok && check_text(l, s, size);
        ok = ok && check_text({l[5]}, std::vector<int16_t>(s.begin(), s.begin() + size), size);
    }
    // long rows: 100,003 values (no multiple of the wave's 64) and 2^20, the longest the entries take
    for (int size : {100003, 1 << 20}) {
        std::vector<int32_t> l = {labels[5], labels[4]};
        std::vector<int16_t> s((size_t)2 * size);
        for (size_t p = 0; p < s.size(); ++p) s[p] = extremes[(p * 7 + p / size) % n_extremes];
        ok = ok && check_text(l, s, size);
    }
    // a label outside +-(10^9 - 1) is refused
    {
        int32_t bad[2] = {0, 1000000000};
        int16_t v[2] = {1, 2};
        uint8_t out[64];
        int64_t n_bytes = 0;
        ok = ok && dbh_text_format_host(bad, v, 2, 1, out, 64, &n_bytes) == 1;
        bad[1] = -1000000000;
        ok = ok && dbh_text_format_host(bad, v, 2, 1, out, 64, &n_bytes) == 1;
    }
    // every kind of signal, at L = 1, around one segment (96, 102), and over many segments
    // (131,072 values: more than the 256 segments of 500 that the kernel draws at a time; 2^20: the
    // longest row - of these, 8 signals from 0 on and the 4 last ones)
    for (int size : {1, 96, 102, 1024, 16384, 131072, 1 << 20}) {
        int kinds[4] = {0, 0, 0, 0};
        const int64_t n = size > 16384 ? 8 : (size > 1024 ? 24 : 64), at_end = size > 16384 ? 4 : 8;
        ok = ok && check_signals(5 + (uint64_t)size, 0, n, size, kinds);
        ok = ok && check_signals(0xfeedfacecafef00dull, ((int64_t)1 << 32) - at_end, at_end, size, kinds);
        for (int k = 0; k < 4; ++k) ok = ok && kinds[k] > 0;
        if (!ok) std::fprintf(stderr, "format_model_check: signals of %d values failed\n", size);
    }
    std::printf("format_model_check: %ld texts, %ld signals: %s\n", g_texts, g_signals, ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
