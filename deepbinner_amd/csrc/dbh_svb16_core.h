// dbh_svb16_core.h - the rules of POD5's 16-bit streamvbyte code ("svb16", the content of a
// `minknow.vbz` value once its zstd frame is undone), as the integers and
// comparisons that the GPU's wave (dbh_vbz.hip: svb16_stream), the host entry
// dbh_svb16_decode_host (the same file) and the stand-alone check (svb16_model_check.cpp, make
// svb16_asan) all compile from these lines.  A stream of n values is
//   ceil(n/8) key bytes | data bytes
// bit i & 7 of key byte i >> 3 (low bit first) says whether value i takes one byte (0) or two,
// little-endian (1); v -> (v >> 1) ^ (0 - (v & 1)) in 16 bits; sample i is the sum of the decoded
// values 0..i modulo 2^16, read as int16.  The data end exactly where the stream does; the unused
// bits of the last key byte are not looked at.
//
// The schedule: 64 lanes x 16 values (two key bytes) per step.  A lane's data are 16 + popcount of
// its 16 key bits long; a prefix sum over the lanes places them; the lane fetches its <= 32 bytes as
// four groups of four values (each group at most 8 bytes, its start known from the key bits alone,
// so the four fetches go out together) and takes the values off each group's 64-bit word by
// shifts.  Sums are kept in 32 bits and cut to 16 at the store: 2^16 divides 2^32.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DBH_SVB16_HD __host__ __device__ inline
#else
#define DBH_SVB16_HD inline
#endif

namespace dbh_svb16 {

constexpr int kRefused = 1;            // status of a stream that fails a self-check
constexpr int kLanes = 64;
constexpr int kPerLane = 16;           // values per lane and step: two key bytes
constexpr int kStep = kLanes * kPerLane;
constexpr int kGroups = 4;             // fetches per lane and step
constexpr int kGroupValues = kPerLane / kGroups;
constexpr int kGroupBytes = 8;         // what a group's fetch takes: its values need 4 .. 8 of them
// bytes a device fetch may take beyond the stream's last byte (a group that holds one 1-byte value)
constexpr int kReadBeyond = kGroupBytes - 1;

DBH_SVB16_HD int popcount16(uint32_t v) { return __builtin_popcount(v & 0xFFFFu); }

// the 4-byte prefix of a stream record: the size of the decoded samples in bytes
DBH_SVB16_HD bool prefix_ok(uint32_t original_size) { return (original_size & 1u) == 0u; }

// n values in `payload` bytes: where the keys end and how long the data are; false if the key bytes
// alone do not fit (whether the data fit is known once the keys have been walked)
DBH_SVB16_HD bool shape(int64_t n, int64_t payload, int64_t* key_bytes, int64_t* data_bytes) {
    if (n < 0 || payload < 0) return false;
    const int64_t keys = n / 8 + ((n & 7) ? 1 : 0);
    if (keys > payload) return false;
    *key_bytes = keys;
    *data_bytes = payload - keys;
    return true;
}

// how many of the 16 values at `base` there are
DBH_SVB16_HD int lane_valid(int64_t n, int64_t base) {
    const int64_t left = n - base;
    return left <= 0 ? 0 : left >= kPerLane ? kPerLane : (int)left;
}
// how many of the lane's two key bytes are read at all
DBH_SVB16_HD int lane_key_bytes(int valid) { return valid > 8 ? 2 : valid > 0 ? 1 : 0; }
// the lane's key bits: those of values beyond n are not looked at
DBH_SVB16_HD uint32_t lane_keys(uint32_t two_key_bytes, int valid) {
    return two_key_bytes & ((1u << valid) - 1u) & 0xFFFFu;
}
// the lane's data bytes
DBH_SVB16_HD uint32_t lane_span(uint32_t keys, int valid) {
    return (uint32_t)valid + (uint32_t)popcount16(keys);
}
// where group g's bytes begin within the lane's data
DBH_SVB16_HD uint32_t group_start(uint32_t keys, int g) {
    return (uint32_t)(kGroupValues * g) + (uint32_t)popcount16(keys & ((1u << (kGroupValues * g)) - 1u));
}
// whether group g holds a value at all (a fetch is made for such groups only)
DBH_SVB16_HD bool group_used(int valid, int g) { return kGroupValues * g < valid; }

DBH_SVB16_HD uint32_t unzigzag(uint32_t v) { return (v >> 1) ^ (0u - (v & 1u)); }

// The lane's values from its groups' words (grp[g]: the 8 bytes at group_start(keys, g), little-
// endian; what lies behind the group's own bytes is not looked at): run[k] = the sum of the decoded
// values 0..k of the lane (0 from `valid` on: the sum stays), returned: run[15].  Modulo 2^32.
DBH_SVB16_HD uint32_t lane_decode(uint32_t keys, int valid, const uint64_t grp[kGroups],
                                  uint32_t run[kPerLane]) {
    uint32_t sum = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int g = 0; g < kGroups; ++g) {
        uint64_t cur = grp[g];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < kGroupValues; ++j) {
            const int k = kGroupValues * g + j;
            const uint32_t two = (keys >> k) & 1u;
            const uint32_t v = (uint32_t)cur & (two ? 0xFFFFu : 0xFFu);
            cur >>= two ? 16 : 8;
            sum += k < valid ? unzigzag(v) : 0u;
            run[k] = sum;
        }
    }
    return sum;
}

// ---- the wave's schedule with loops for lanes: dbh_svb16_decode_host and the check ---------------
// `stream`: exactly stream_bytes readable bytes, `out`: exactly n samples.  Every byte read lies
// inside the stream (a group's fetch is byte by byte here, up to the stream's end).  Returns 0, or
// kRefused with out all zeros.
inline int decode_host(const uint8_t* stream, int64_t stream_bytes, int64_t n, int16_t* out) {
    int64_t key_bytes = 0, data_len = 0;
    bool bad = !shape(n, stream_bytes, &key_bytes, &data_len);
    const uint8_t* const kbase = stream;
    const uint8_t* const dbase = bad ? stream : stream + key_bytes;
    int64_t doff = 0;
    uint32_t carry = 0;
    for (int64_t v0 = 0; !bad && v0 < n; v0 += kStep) {
        uint32_t span[kLanes], keys[kLanes];
        int valid[kLanes];
        for (int lane = 0; lane < kLanes; ++lane) {
            const int64_t base = v0 + (int64_t)lane * kPerLane;
            valid[lane] = lane_valid(n, base);
            uint32_t kb = 0;
            for (int b = 0; b < lane_key_bytes(valid[lane]); ++b)
                kb |= (uint32_t)kbase[base / 8 + b] << (8 * b);
            keys[lane] = lane_keys(kb, valid[lane]);
            span[lane] = lane_span(keys[lane], valid[lane]);
        }
        uint32_t incl = 0, prefix = carry;
        bool any_overrun = false;
        for (int lane = 0; lane < kLanes; ++lane) {
            const int64_t base = v0 + (int64_t)lane * kPerLane;
            const int64_t my = doff + (int64_t)incl;
            incl += span[lane];
            const bool overrun = my + (int64_t)span[lane] > data_len;
            any_overrun = any_overrun || overrun;
            uint64_t grp[kGroups] = {0, 0, 0, 0};
            for (int g = 0; g < kGroups; ++g) {
                if (!group_used(valid[lane], g) || overrun) continue;
                const int64_t at = my + (int64_t)group_start(keys[lane], g);
                for (int b = 0; b < kGroupBytes && at + b < data_len; ++b)
                    grp[g] |= (uint64_t)dbase[at + b] << (8 * b);
            }
            uint32_t run[kPerLane];
            const uint32_t sum = lane_decode(keys[lane], valid[lane], grp, run);
            if (!any_overrun)
                for (int k = 0; k < valid[lane]; ++k) out[base + k] = (int16_t)(uint16_t)(prefix + run[k]);
            prefix += sum;
        }
        carry = prefix;
        doff += (int64_t)incl;
        if (any_overrun) bad = true;               // data that would run past the stream's end
    }
    if (!bad && doff != data_len) bad = true;      // data that end before the stream does
    if (bad)
        for (int64_t k = 0; k < n; ++k) out[k] = 0;
    return bad ? kRefused : 0;
}

}  // namespace dbh_svb16
