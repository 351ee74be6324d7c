// text_model_check.cpp - the CPU model of the training-data text parser (dbh_text_parse_host:
// dbh_text.hip compiled as plain C++, dbh_text_core.h) on malformed lines and on every truncation
// of every line, in heap blocks of exactly the sizes the entry is told, so that AddressSanitizer
// and UBSan see any byte read or written outside them.  `make text_asan` builds and runs it; it
// needs no device and no Python.  Each result is also held to a plain byte-by-byte parser below.
#include "dbh_text.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

// the grammar of dbh_text_core.h, one byte at a time: kind, and label and values where kOk
int plain_kind(const std::string& line_in, int input_size, int32_t* label, std::vector<int>* values) {
    std::string line = line_in;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    size_t p = 0;
    const auto digit = [&](size_t q) { return q < line.size() && line[q] >= '0' && line[q] <= '9'; };
    bool negative = p < line.size() && line[p] == '-';
    if (negative) ++p;
    const size_t first = p;
    while (digit(p)) ++p;
    const size_t n = p - first;
    if (n < 1 || n > 9 || (line[first] == '0' && (n > 1 || negative))) return dbt::kForm;
    if (p >= line.size() || line[p] != '\t') return dbt::kForm;
    *label = (int32_t)std::strtol(line.substr(0, p).c_str(), nullptr, 10);
    ++p;
    values->clear();
    bool range = false;
    for (;;) {
        const bool minus = p < line.size() && line[p] == '-';
        if (p < line.size() && (line[p] == '+' || line[p] == '-')) ++p;
        const size_t from = p;
        while (digit(p)) ++p;
        if (p - from < 1 || p - from > 7) return dbt::kForm;
        const long v = std::strtol(line.substr(from, p - from).c_str(), nullptr, 10) * (minus ? -1 : 1);
        range = range || v < -32768 || v > 32767;
        values->push_back((int)v);
        if (p == line.size()) break;
        if (line[p] != ',') return dbt::kForm;
        ++p;
    }
    if ((int)values->size() != input_size) return dbt::kCount;
    return range ? dbt::kRange : dbt::kOk;
}

long g_blocks = 0, g_lines = 0;

// the lines as one block, `shift` bytes of a line in front; false (and a message) on a mismatch
bool check_block(const std::vector<std::string>& lines_in, int shift, int input_size) {
    std::vector<std::string> lines;
    if (shift) lines.push_back(std::string((size_t)shift - 1, '#'));
    lines.insert(lines.end(), lines_in.begin(), lines_in.end());
    std::string text;
    for (const auto& l : lines) text += l + "\n";
    const int64_t n_bytes = (int64_t)text.size(), max_lines = (int64_t)lines.size();
    uint8_t* block = (uint8_t*)std::malloc((size_t)n_bytes);
    int16_t* samples = (int16_t*)std::malloc((size_t)max_lines * input_size * sizeof(int16_t));
    int32_t* labels = (int32_t*)std::malloc((size_t)max_lines * sizeof(int32_t));
    uint8_t* kinds = (uint8_t*)std::malloc((size_t)max_lines);
    std::memcpy(block, text.data(), (size_t)n_bytes);
    int64_t n_lines = -1, first_bad = -2;
    bool ok = dbh_text_parse_host(block, n_bytes, input_size, max_lines, samples, labels, kinds,
                                  &n_lines, &first_bad) == 0 && n_lines == max_lines;
    int64_t want_bad = -1;
    for (int64_t k = 0; ok && k < n_lines; ++k) {
        int32_t label = 0;
        std::vector<int> values;
        const int kind = plain_kind(lines[(size_t)k], input_size, &label, &values);
        ok = kinds[k] == kind;
        if (kind != dbt::kOk && want_bad < 0) want_bad = k;
        if (ok && kind == dbt::kOk) {
            ok = labels[k] == label;
            for (int i = 0; ok && i < input_size; ++i) ok = samples[k * input_size + i] == values[(size_t)i];
        }
        if (!ok) std::printf("line %lld of a block differs: '%s' (input_size %d, shift %d)\n", (long long)k,
                             lines[(size_t)k].c_str(), input_size, shift);
    }
    if (ok && first_bad != want_bad) {
        ok = false;
        std::printf("first_bad_line %lld, expected %lld\n", (long long)first_bad, (long long)want_bad);
    }
    // one line fewer than the block holds: refused, and nothing written past the arrays
    if (ok && max_lines > 1) {
        ok = dbh_text_parse_host(block, n_bytes, input_size, max_lines - 1, samples, labels, kinds,
                                 &n_lines, &first_bad) == 1 && n_lines == max_lines;
    }
    std::free(block);
    std::free(samples);
    std::free(labels);
    std::free(kinds);
    g_blocks += 1;
    g_lines += max_lines;
    return ok;
}

}  // namespace

int main() {
    std::vector<std::string> corpus = {
        "3\t1,2", "3\t-32768,+32767", "0\t0000012,-0000001", "-12\t5,6\r", "999999999\t1,2",
        "", "\r", "x", "1", "1\t", "\t", "\t5,6", "1\t5", "1\t5,6,7", "1\t,6", "1\t5,", "1\t5,,6",
        "1\t\t5,6", "1\t5\t6", "1 5,6", "1\t5,6\r\r", "1\t5\r,6", "01\t5,6", "+1\t5,6", "-0\t5,6",
        "-\t5,6", "1234567890\t5,6", "2147483648\t5,6", "00\t5,6", "1\t12345678,6", "1\t00000123,6",
        "1\t--5,6", "1\t+-5,6", "1\t+,6", "1\t5,-", "1\t32768,6", "1\t-32769,6", "1\t9999999,-9999999",
        "1\t99999", "1\t99999,5,5", "1\t5 ,6", " 1\t5,6", "1_0\t5,6", "1\t1_0,6", "1\t5;6", "1\t5.0,6",
        std::string("1\t5,\0" "6", 6), "1\t5,\xc3\x95", "1\t5,6\xff", std::string("\0", 1), "1,2\t5,6",
        "7\t" + std::string(7, '1') + "," + std::string(7, '2'),
    };
    {   // lines around the 1,024-byte step and longer than two steps
        std::string many = "5\t-32768";
        for (int i = 1; i < 300; ++i) many += ",-32768";
        corpus.push_back(many);
        std::string wide = "5\t1";
        for (int i = 1; i < 96; ++i) wide += "," + std::to_string((i * 7919) % 65536 - 32768);
        corpus.push_back(wide);
    }
    bool ok = true;
    for (int input_size : {1, 2, 3, 96, 300}) {
        for (int shift = 0; ok && shift < 16; ++shift) ok = check_block(corpus, shift, input_size);
        for (size_t k = 0; ok && k < corpus.size(); ++k) {
            const std::string& line = corpus[k];
            if (line.size() > 700 && input_size != 300) continue;
            // every truncation, alone and in front of the whole line, at three alignments
            for (size_t cut = 0; ok && cut <= line.size(); ++cut)
                for (int shift : {0, 7, 15})
                    ok = check_block({line.substr(0, cut), line}, shift, input_size);
        }
    }
    {   // one line of 2^20 values, the most a line may hold: thousands of steps, at two alignments
        std::string longest = "-999999999\t0";
        for (int i = 1; i < (1 << 20); ++i) longest += "," + std::to_string((int)((i * 7919LL) % 65536) - 32768);
        for (int shift : {0, 15}) ok = ok && check_block({longest}, shift, 1 << 20);
    }
    std::printf("text_model_check: %ld blocks, %ld lines: %s\n", g_blocks, g_lines, ok ? "clean" : "FAILED");
    return ok ? 0 : 1;
}
