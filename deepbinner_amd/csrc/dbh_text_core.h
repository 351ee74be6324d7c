// dbh_text_core.h - training-data text (``label<TAB>v1,v2,...`` per line) to int16 rows: what a
// line must look like, what it is called when it does not, and the schedule both the GPU's wave
// (dbh_text.hip) and the CPU model (dbh_text_parse_host, same file) run it by.  C ABI: the
// "training-data text" section of include/deepbinner_hip.h; DESIGN.md section 22.
//
// The strict line, as bytes (anything Python's own parser would take beyond it is the host's):
//     line  := label TAB value ( ',' value )* [CR] LF
//     label := '0' | ['-'] [1-9] [0-9]{0,8}
//     value := ['+' | '-'] [0-9]{1,7}
// kinds, the first that applies: kForm (outside the grammar), kCount (values != input_size),
// kRange (a value outside int16), else kOk.
//
// THE SCHEDULE.  A line is walked from the 16-byte boundary at or below its first byte (`base`) in
// steps of 1,024 bytes, 64 pieces of 16 bytes, one piece per lane.  The label (at most 10 bytes and
// the TAB) is read from the line's head by itself.  Behind the TAB every value hangs on the
// SEPARATOR IN FRONT OF IT - the TAB or a comma - and belongs to the piece that separator lies in:
// that piece parses sign, digits and the byte that ends the value (a comma, or the line's end) from
// its own bytes and the next piece's, 9 bytes at most, so a value never needs more than the
// following piece, be that the next lane's or the next step's first.  Each value proves the byte
// behind it to be the next separator or the end, so the chain TAB, value, comma, value, ... covers
// every byte up to the line's end or breaks as kForm; a separator needs no look at the byte in
// front of it.  A value's place in the row is the number of commas up to and including its
// separator: a count within the piece, a prefix count over the pieces of the step, a carry from
// step to step.  Every loop is bounded by the line's length, fixed before the walk begins.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DBT_FN __host__ __device__ __forceinline__
#else
#define DBT_FN inline
#endif
#if defined(__clang__)
#define DBT_UNROLL _Pragma("unroll")
#else
#define DBT_UNROLL
#endif

namespace dbt {

constexpr int kOk = 0, kForm = 1, kCount = 2, kRange = 3;
constexpr int kLanes = 64, kPiece = 16, kStep = kLanes * kPiece;
constexpr int kLabelBytes = 10;                         // '-' and nine digits
constexpr int kValueBytes = 8;                          // a sign and seven digits
constexpr int kMaxInput = 1 << 20;
constexpr int64_t kMaxBlock = (int64_t)1 << 30;
constexpr uint32_t kEnd = 0x0a;                         // stands for every byte at or past the end
constexpr int kFlagForm = 1, kFlagRange = 2;

// a line's frame: positions are relative to `base`, the 16-byte boundary at or below its start
struct Line {
    int64_t base;
    int32_t begin, end;       // first byte; one past the last (the LF's place, or the CR's in CR LF)
    int32_t tab;              // the TAB's place
    int32_t label;
    bool head_ok;             // the label is strict and a TAB follows it
};

// `start`: the line's first byte, `lf`: its LF (start <= lf); reads [start, lf) only
DBT_FN Line line_head(const uint8_t* block, int64_t start, int64_t lf) {
    Line l;
    l.base = start & ~(int64_t)(kPiece - 1);
    l.begin = (int32_t)(start - l.base);
    int64_t end = lf;
    if (end > start && block[end - 1] == '\r') end -= 1;
    l.end = (int32_t)(end - l.base);
    const int32_t len = l.end - l.begin;
    // 0 nothing yet, 1 behind '-', 2 in digits, 3 the TAB found, 4 refused
    int state = 0, digits = 0;
    bool negative = false, zero = false;
    int32_t value = 0;
    l.tab = 0;
    for (int k = 0; k <= kLabelBytes; ++k) {
        const uint32_t c = k < len ? block[start + k] : kEnd;
        const uint32_t d = c - '0';
        if (state >= 3) {
        } else if (c == '\t') {
            l.tab = l.begin + k;
            state = state == 2 ? 3 : 4;
        } else if (c == '-' && state == 0) {
            negative = true;
            state = 1;
        } else if (d < 10u && !zero && digits < kLabelBytes - 1 && !(d == 0 && state == 1)) {
            zero = d == 0 && state == 0;                 // '0' stands alone: no '01', no '-0'
            value = value * 10 + (int32_t)d;
            digits += 1;
            state = 2;
        } else {
            state = 4;
        }
    }
    l.head_ok = state == 3;
    l.label = l.head_ok ? (negative ? -value : value) : 0;
    return l;
}

// byte `o` (0..31) of a piece and the piece behind it, as eight little-endian words
DBT_FN uint32_t byte_at(const uint32_t (&w)[8], int o) { return (w[o >> 2] >> ((o & 3) * 8)) & 0xffu; }

// the commas of the piece at `rel0` that separate values: behind the TAB, in front of the end
DBT_FN int piece_commas(const uint32_t (&w)[8], int32_t rel0, int32_t tab, int32_t end) {
    int n = 0;
    DBT_UNROLL
    for (int j = 0; j < kPiece; ++j) {
        const int32_t rel = rel0 + j;
        n += (rel > tab && rel < end && byte_at(w, j) == ',') ? 1 : 0;
    }
    return n;
}

// The values whose separators lie in the piece at `rel0`; `before`: the commas in front of it.
// A value in range whose place is inside the row is stored; returns kFlagForm | kFlagRange.
DBT_FN int piece_values(const uint32_t (&w)[8], int32_t rel0, int32_t tab, int32_t end, int32_t before,
                        int32_t input_size, int16_t* row) {
    int flags = 0;
    int32_t place = before;
    DBT_UNROLL
    for (int j = 0; j < kPiece; ++j) {
        const int32_t rel = rel0 + j;
        const bool comma = rel > tab && rel < end && byte_at(w, j) == ',';
        place += comma ? 1 : 0;
        if (comma || rel == tab) {
            bool negative = false, done = false, bad = false;
            int32_t value = 0;
            int digits = 0;
            DBT_UNROLL
            for (int k = 0; k <= kValueBytes; ++k) {
                const uint32_t c = rel + 1 + k >= end ? kEnd : byte_at(w, j + 1 + k);
                const uint32_t d = c - '0';
                if (done) {
                } else if (k == 0 && (c == '+' || c == '-')) {
                    negative = c == '-';
                } else if (d < 10u && digits < kValueBytes - 1) {
                    value = value * 10 + (int32_t)d;
                    digits += 1;
                } else {
                    done = true;
                    bad = !((c == ',' || c == kEnd) && digits >= 1);
                }
            }
            value = negative ? -value : value;
            if (bad || !done) flags |= kFlagForm;
            else if (value < -32768 || value > 32767) flags |= kFlagRange;
            else if (place < input_size) row[place] = (int16_t)value;
        }
    }
    return flags;
}

DBT_FN int line_kind(bool head_ok, int flags, int64_t values, int32_t input_size) {
    if (!head_ok || (flags & kFlagForm)) return kForm;
    if (values != input_size) return kCount;
    return (flags & kFlagRange) ? kRange : kOk;
}

// ---- the CPU model: the same walk with loops for steps and lanes ---------------------------------
// the 16 bytes at block + at as four words; what lies outside [0, n_bytes) reads as zero
inline void model_piece(const uint8_t* block, int64_t n_bytes, int64_t at, uint32_t* w4) {
    for (int q = 0; q < 4; ++q) {
        uint32_t v = 0;
        for (int b = 0; b < 4; ++b) {
            const int64_t p = at + 4 * q + b;
            if (p >= 0 && p < n_bytes) v |= (uint32_t)block[p] << (8 * b);
        }
        w4[q] = v;
    }
}

// one line [start, lf) of the block into row (input_size values) and *label; returns its kind
inline int model_line(const uint8_t* block, int64_t n_bytes, int64_t start, int64_t lf,
                      int32_t input_size, int16_t* row, int32_t* label) {
    const Line l = line_head(block, start, lf);
    *label = l.label;
    int flags = 0;
    int64_t carried = 0;
    if (l.head_ok) {
        const int32_t steps = (l.end + kStep - 1) / kStep;
        for (int32_t step = 0; step < steps; ++step) {
            uint32_t w[kLanes][8];
            int32_t commas[kLanes];
            for (int lane = 0; lane < kLanes; ++lane) {
                const int32_t rel0 = step * kStep + lane * kPiece;
                for (int half = 0; half < 2; ++half) {
                    const int32_t r = rel0 + half * kPiece;
                    if (r < l.end) model_piece(block, n_bytes, l.base + r, w[lane] + 4 * half);
                    else w[lane][4 * half] = w[lane][4 * half + 1] = w[lane][4 * half + 2] = w[lane][4 * half + 3] = 0;
                }
                commas[lane] = piece_commas(w[lane], rel0, l.tab, l.end);
            }
            for (int lane = 0; lane < kLanes; ++lane) {
                flags |= piece_values(w[lane], step * kStep + lane * kPiece, l.tab, l.end,
                                      (int32_t)carried, input_size, row);
                carried += commas[lane];
            }
        }
    }
    return line_kind(l.head_ok, flags, carried + 1, input_size);
}

}  // namespace dbt
