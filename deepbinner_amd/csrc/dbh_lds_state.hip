// dbh_lds_state.hip - test support: put a known word into every CU's LDS, and ask what a CU's LDS
// holds (C ABI: the "LDS state" section of include/deepbinner_hip.h).  LDS is
// not cleared between workgroups: a kernel that reads a word of its arena before it has written it
// computes with what the workgroup before left there.  tests/test_gpu_lds_state.py runs every kernel
// with a __shared__ arena behind a fill and holds its output to the run behind a fill of zeros.
//
// lds_state<true>   fill: 512 threads and all 160 KiB as dynamic LDS, so one workgroup sits on a CU;
//                   every word of the arena is stored (plain 16-byte vector stores), then the
//                   workgroup keeps its CU for a counted wait, so that the dispatcher has to hand
//                   the grid's next workgroups to the CUs that had none yet.
// lds_state<false>  survey: the same shape, stores nothing to LDS, counts the words that equal
//                   the pattern.
// Either way every wave leaves one record {CU + 1, words} in pinned host memory by a plain store: no
// atomics, no LDS for the sums (a wave adds up through lane exchanges), no copy kernel between a
// fill and what runs behind it.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "../../include/deepbinner_hip.h"
#include "dbh_status.h"

namespace dbh_lds_detail {

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kArenaBytes = 160 * 1024;
constexpr int kArenaVectors = kArenaBytes / 16;             // 10,240 uint4 = 20 per thread
constexpr int kDefaultMultiple = 4, kDefaultHoldUs = 50;    // (profiles/lds_state/survey.txt)
constexpr int kMaxMultiple = 64, kMaxHoldUs = 10000;
static_assert(kArenaVectors % kThreads == 0, "every thread takes the same share of the arena");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Record {
    uint32_t cu_plus_1;     // __smid() + 1: XCC, shader engine and CU of the wave; 0 = never written
    uint32_t words;
};

template <bool FILL>
__global__ __launch_bounds__(kThreads) void lds_state(uint32_t pattern, long long hold_ticks,
                                                      int max_polls, Record* __restrict__ out) {
    extern __shared__ u32x4 arena[];
    // (volatile: nothing reads the fill, nothing wrote the survey; LDS address space: ds_write_b128
    // and ds_read_b128, where a generic pointer would give flat instructions)
    volatile __attribute__((address_space(3))) u32x4* words =
        (volatile __attribute__((address_space(3))) u32x4*)arena;
    const int tid = threadIdx.x;
    uint32_t n = 0;
    for (int i = tid; i < kArenaVectors; i += kThreads) {
        if (FILL) {
            words[i] = u32x4{pattern, pattern, pattern, pattern};
            n += 4;
        } else {
            const u32x4 v = words[i];
            n += (v.x == pattern) + (v.y == pattern) + (v.z == pattern) + (v.w == pattern);
        }
    }
    __syncthreads();
    // the counted wait: at most max_polls looks at the 100 MHz clock, a short sleep between two
    const long long t0 = wall_clock64();
    for (int i = 0; i < max_polls && wall_clock64() - t0 < hold_ticks; ++i) __builtin_amdgcn_s_sleep(8);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off);
    if ((tid & 63) == 0) {
        Record r;
        r.cu_plus_1 = __smid() + 1;
        r.words = n;
        out[blockIdx.x * kWaves + (tid >> 6)] = r;
    }
}

// the device of a call, for its length
struct OnDevice {
    int before = -1;
    hipError_t enter(int device) {
        hipError_t e = hipGetDevice(&before);
        if (e != hipSuccess) before = -1;
        return e == hipSuccess ? hipSetDevice(device) : e;
    }
    ~OnDevice() { if (before >= 0) (void)hipSetDevice(before); }
};

struct PinnedRecords {
    Record* ptr = nullptr;
    ~PinnedRecords() { if (ptr) (void)hipHostFree(ptr); }
};

// One launch on the null stream and a device synchronise; per CU slot the words its workgroups
// counted and how many words they looked at.
template <bool FILL>
int run(int device, uint32_t pattern, int grid_multiple, int hold_us, int64_t* counted,
        int64_t* looked_at, int* cus_seen, int* cus_total) {
    if (grid_multiple == 0) grid_multiple = kDefaultMultiple;
    if (hold_us < 0) hold_us = kDefaultHoldUs;
    if (grid_multiple < 1 || grid_multiple > kMaxMultiple || hold_us > kMaxHoldUs || !cus_seen)
        return DBH_ERR_INVALID_ARGUMENT;
    OnDevice on;
    DBH_HIP(on.enter(device));
    int cus = 0, clock_khz = 0;
    DBH_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    DBH_HIP(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, device));
    DBH_HIP(hipFuncSetAttribute((const void*)lds_state<FILL>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, kArenaBytes));
    const unsigned grid = (unsigned)(cus * grid_multiple);
    const size_t n_records = (size_t)grid * kWaves;
    PinnedRecords records;
    DBH_HIP(hipHostMalloc((void**)&records.ptr, n_records * sizeof(Record), hipHostMallocDefault));
    memset(records.ptr, 0, n_records * sizeof(Record));
    const long long ticks = (long long)hold_us * clock_khz / 1000;
    // (a poll is a sleep of some 0.25 us and a clock read: never more than ~4 polls per microsecond)
    const int max_polls = hold_us * 16 + 16;
    hipLaunchKernelGGL(lds_state<FILL>, dim3(grid), dim3(kThreads), kArenaBytes, 0, pattern, ticks,
                       max_polls, records.ptr);
    DBH_HIP(hipGetLastError());
    DBH_HIP(hipDeviceSynchronize());
    int64_t sum[DBH_LDS_CU_SLOTS] = {}, seen_words[DBH_LDS_CU_SLOTS] = {};
    int seen = 0;
    for (size_t i = 0; i < n_records; ++i) {
        const Record r = records.ptr[i];
        if (r.cu_plus_1 == 0 || r.cu_plus_1 > DBH_LDS_CU_SLOTS) continue;
        if (seen_words[r.cu_plus_1 - 1] == 0) ++seen;
        sum[r.cu_plus_1 - 1] += r.words;
        seen_words[r.cu_plus_1 - 1] += kArenaBytes / 4 / kWaves;
    }
    if (counted) memcpy(counted, sum, sizeof sum);
    if (looked_at) memcpy(looked_at, seen_words, sizeof seen_words);
    *cus_seen = seen;
    if (cus_total) *cus_total = cus;
    return DBH_OK;
}

}  // namespace dbh_lds_detail

extern "C" {

int dbh_lds_fill(int device, uint32_t pattern, int grid_multiple, int hold_us, int* cus_seen,
                 int* cus_total) {
    return dbh_lds_detail::run<true>(device, pattern, grid_multiple, hold_us, nullptr, nullptr,
                                     cus_seen, cus_total);
}

int dbh_lds_survey(int device, uint32_t pattern, int grid_multiple, int hold_us, int64_t* matching,
                   int64_t* looked_at, int* cus_seen, int* cus_total) {
    if (!matching || !looked_at) return DBH_ERR_INVALID_ARGUMENT;
    return dbh_lds_detail::run<false>(device, pattern, grid_multiple, hold_us, matching, looked_at,
                                      cus_seen, cus_total);
}

}
