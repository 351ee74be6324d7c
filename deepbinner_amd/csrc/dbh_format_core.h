// dbh_format_core.h - int16 rows to training-data text, the inverse of dbh_text_core.h: labels [n]
// and samples [n][L] become the bytes ``label TAB v1,...,vL LF`` per line, which is what Python's
// '{}\t{}\n'.format(label, ','.join(map(str, row))) gives and what section 22's strict grammar
// takes.  How wide a number is and which bytes it becomes, for the GPU's wave (dbh_format.hip) and
// the CPU model (dbh_text_format_host, same file).  C ABI: the "training-data text, written"
// section of include/deepbinner_hip.h; DESIGN.md section 23.
//
// A value takes 1 to 6 bytes (a '-' and up to five digits) and the byte behind it: a comma, or
// the line's LF behind the last.  A label is '0', or up to nine digits with an optional '-'.  So a
// line holds at most 12 + 7 * L bytes (line_bound).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DBF_FN __host__ __device__ __forceinline__
#else
#define DBF_FN inline
#endif
#if defined(__clang__)
#define DBF_UNROLL _Pragma("unroll")
#else
#define DBF_UNROLL
#endif

namespace dbf {

constexpr int kMaxInput = 1 << 20;
constexpr int64_t kMaxValues = (int64_t)1 << 30;
constexpr int32_t kMaxLabel = 999999999;
constexpr int kValueDigits = 5, kLabelDigits = 9;
constexpr int32_t kBadLabel = -1;                        // a line's byte count where its label is refused

DBF_FN int64_t line_bound(int64_t input_size) { return 12 + 7 * input_size; }
DBF_FN bool label_ok(int32_t label) { return label >= -kMaxLabel && label <= kMaxLabel; }

// bytes of a value without what follows it
DBF_FN int value_width(int32_t v) {
    const int32_t a = v < 0 ? -v : v;
    return (v < 0 ? 1 : 0) + 1 + (a >= 10 ? 1 : 0) + (a >= 100 ? 1 : 0) + (a >= 1000 ? 1 : 0) +
           (a >= 10000 ? 1 : 0);
}

// bytes of a label that label_ok took
DBF_FN int label_width(int32_t label) {
    const int32_t a = label < 0 ? -label : label;
    int w = (label < 0 ? 1 : 0) + 1;
    int32_t limit = 10;
    DBF_UNROLL
    for (int k = 1; k < kLabelDigits; ++k) {
        w += a >= limit ? 1 : 0;
        limit *= 10;
    }
    return w;
}

// the number's `width` bytes at `at`, at most `digits` of them digits
DBF_FN void put_number(uint8_t* at, int32_t v, int width, int digits) {
    int32_t a = v < 0 ? -v : v;
    if (v < 0) at[0] = '-';
    for (int k = 0; k < digits; ++k) {
        const int place = width - 1 - k;
        if (place >= (v < 0 ? 1 : 0)) at[place] = (uint8_t)('0' + a % 10);
        a /= 10;
    }
}

// the argument errors of every entry, before any work: dbh_status values
inline int check_arguments(const void* labels, const void* samples, int64_t n_lines, int input_size,
                           const void* out, int64_t capacity, const void* n_bytes) {
    if (!labels || !samples || !out || !n_bytes) return 1;
    if (n_lines < 1 || input_size < 1 || capacity < 0) return 1;
    if (input_size > kMaxInput || n_lines > kMaxValues / input_size) return 5;
    return 0;
}

// ---- the CPU model ----------------------------------------------------------------------------------
inline int64_t model_line_bytes(int32_t label, const int16_t* row, int32_t input_size) {
    int64_t n = label_width(label) + 1;
    for (int32_t i = 0; i < input_size; ++i) n += value_width(row[i]) + 1;
    return n;
}

// the line at `at`, which holds model_line_bytes() bytes
inline void model_line(int32_t label, const int16_t* row, int32_t input_size, uint8_t* at) {
    int w = label_width(label);
    put_number(at, label, w, kLabelDigits);
    at[w] = '\t';
    at += w + 1;
    for (int32_t i = 0; i < input_size; ++i) {
        w = value_width(row[i]);
        put_number(at, row[i], w, kValueDigits);
        at[w] = i + 1 < input_size ? ',' : '\n';
        at += w + 1;
    }
}

}  // namespace dbf
