// dbh_api.hip — host side of libdeepbinner_hip.so: the C ABI declared in
// include/deepbinner_hip.h.  Uploads the weights dbh_pack.h packs into the kernel's fragment order,
// owns the device buffers and prepares the launches.  Host code only: the forward kernel and the
// small seam kernels (stand-alone normalise, merge, combine_calls) are built, and launched, in
// dbh_kernels.hip; this file calls its launch functions (dbh_kernels.h).  The sweep's fold and tally
// kernels likewise: dbh_sweep.hip behind dbh_sweep.h; the scan's front and event kernels:
// dbh_scan.hip behind dbh_scan.h; the live sessions' kernels: dbh_live.hip behind dbh_live.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <mutex>
#include <vector>

#include "../../include/deepbinner_hip.h"
#include "dbh_general.h"
#include "dbh_host_layout.h"
#include "dbh_kernels.h"
#include "dbh_layout.h"
#include "dbh_live.h"
#include "dbh_locate.h"
#include "dbh_occlude.h"
#include "dbh_owned.h"
#include "dbh_pack.h"
#include "dbh_scan.h"
#include "dbh_status.h"
#include "dbh_early_core.h"
#include "dbh_sweep.h"

namespace {
thread_local std::string g_last_error;
}  // namespace

// (every unit that reports through dbh_last_error() comes here: dbh_status.h)
int dbh_hip::hip_fail(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? DBH_ERR_OUT_OF_MEMORY : DBH_ERR_HIP;
}

namespace {

using dbh_hip::hip_fail;

#define DBH_TRY(call)                                         \
    do {                                                      \
        const int st_ = (call);                               \
        if (st_ != DBH_OK) return st_;                        \
    } while (0)

using dbh_host::align256;
using dbh_owned::DeviceBlock;
using dbh_owned::PinnedBlock;

// Where a forward launch parks its conv17 outputs until the batched tail runs (dbh_forward.hip):
// a 256-byte header whose first word is the counter the launch's workgroups take their windows
// off (zero between launches, so zeroed only when the block is new, on the stream that launches
// next), then kWgScratchFloats floats per workgroup.  One per stream a model launches on: launches
// on one stream follow each other, launches on two may overlap.
struct TailScratch {
    DeviceBlock block;
    hipError_t reserve(int64_t workgroups, hipStream_t stream) {
        bool fresh = false;
        const hipError_t e =
            block.reserve(256 + (size_t)workgroups * dbh::kWgScratchFloats * sizeof(float), &fresh);
        return e == hipSuccess && fresh ? hipMemsetAsync(block.get(), 0, 256, stream) : e;
    }
    int* counter() const { return block.as<int>(); }
    float* scratch() const { return block.as<float>(256); }
};

// live timing of the forward kernel (dbh_forward_timing_*): state here, logic in dbh_probes.h
struct TimingBrackets {
    int every = 0;               // 0 = off, n = open an event bracket at every n-th forward launch
    int span = 1;                // consecutive launches one bracket covers (<= every)
    hipEvent_t open_stop = nullptr;   // stop event of the bracket being filled
    int64_t open_windows = 0, launch_counter = 0, timed_launches = 0, timed_windows = 0;
    std::vector<std::pair<dbh_owned::Event, dbh_owned::Event>> events;
    size_t events_used = 0;
    hipError_t begin(hipStream_t stream, int64_t windows);
    hipError_t end(hipStream_t stream);
    void reset();
};

struct HostSlot {
    dbh_owned::Stream stream;
    PinnedBlock h_in, h_out;
    DeviceBlock d_in, d_out, d_work;
    TailScratch tail;
};

struct DeflatedQueue {
    dbh_owned::Stream stream;
    dbh_owned::Event inflated, classified;      // hand-over to the forward stream
    PinnedBlock h_small;                        // records, offsets, results
    PinnedBlock h_comp;                         // staging for pageable input
    DeviceBlock d_comp, d_small, d_samples, d_tokens, d_out, d_work;
    TailScratch tail;
    std::vector<int32_t> order;                 // the records as they were sent
};

}  // namespace

struct dbh_model {
    int n_classes = 0;
    int input_size = dbh::kWindow;
    int kind = DBH_MODEL_KIND_PERSISTENT;   // DBH_MODEL_KIND_GENERAL: dbh_general.hip runs it
    dbh_gen::Net gen;                       // ... with these weights (dbh_gen::destroy frees them)
    int device = 0;
    int cus = 256;               // workgroups of a persistent forward launch (one per CU)
    int cus_total = 256;         // ... before dbh_model_reserve_cus took some away
    bool windows_by_counter = true;        // DEEPBINNER_STATIC_WINDOWS=1: fixed shares (A/B)
    bool launch_per_batch = false;   // DEEPBINNER_LAUNCH_PER_BATCH=1: one launch per batch (A/B)
    bool forward_lean = true;        // DEEPBINNER_FORWARD_BUILD=full: production launches on the full kernel (A/B)
    // The end of a persistent launch: with fewer than chunk4_rounds x grid windows not yet handed
    // out a workgroup asks for groups of 2 instead of 4, below chunk2_rounds x grid for single
    // windows (DEEPBINNER_CHUNK4_ROUNDS / DEEPBINNER_CHUNK2_ROUNDS: A/B)
    // (measured on configs[1] one launch per step, 10,000 windows: 8 / 3: 5.44 M reads/s, 4 / 2: 5.75 M,
    // 2 / 1: 5.74 M, 0 / 0 - always four - 5.74 M: a small group pays the whole stage D-E-F chain for
    // one or two windows, so they are kept to the launch's very end)
    int chunk4_rounds = 2, chunk2_rounds = 1;
    DeviceBlock packed;
    DeviceBlock in, work, out;   // workspace of the host-pointer entry points, grown on demand
    // per stream the callers of the *_dev entry points bring (the null stream among them): the
    // forward kernel's scratch, and the general path's activations for dbh_predict(_dev)
    std::map<hipStream_t, TailScratch> tails;
    std::map<hipStream_t, DeviceBlock> gen_scratch;
    DeviceBlock clock;                                     // dbh_forward_clock_enable
    bool clock_probe = false;  unsigned clock_grid = 0;
    bool phase_probe = false;      // dbh_forward_phases_enable
    TimingBrackets timing;
    // staging slots of the host-buffer entry points (host_groups: overlapped H2D / kernels / D2H)
    static constexpr int kSlots = 3;
    static constexpr int64_t kDefaultGroup = 32768;
    int64_t host_group_windows = kDefaultGroup;     // dbh_model_set_host_group
    bool host_zero_copy = true;      // DEEPBINNER_HOST_ZERO_COPY=0: copy host samples to HBM first
    HostSlot slot[kSlots];
    // buffers of dbh_classify_pair_deflated (the start model's, or the only model's, are used)
    DeflatedQueue deflated;
    int64_t hint_len = 0, hint_cap = 0;   // dbh_model_set_read_length_hint
    ~dbh_model() { dbh_gen::destroy(&gen); }
};

namespace {

// "every read is len_hint samples long": offsets[0] belongs to read number read0 of the sample
// buffer, which holds at least hint_cap samples (see dbh_model_set_read_length_hint)
struct ReadHints { int64_t read0 = 0, len_hint = 0, hint_cap = 0; };

struct FusedInput {          // seam-b2 mode of the forward kernel (all null/zero = seam b1)
    const int16_t* samples = nullptr;
    const int64_t* offsets = nullptr;
    int steps = 1;
    int side = 0;
    double score_diff = 0.0;
    int32_t* calls = nullptr;
    ReadHints hints;
    // where this launch parks its conv17 outputs (null = the model's own, by stream)
    TailScratch* tail = nullptr;
};

int launch_forward(dbh_model* m, const float* x_dev, int64_t n, float* probs_dev,
                   int debug_stage, float* debug_dev, hipStream_t stream,
                   const FusedInput& in = FusedInput()) {
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;   // (introspection)
    if (n == 0) return DBH_OK;
    const bool timed = m->timing.every > 0 && (debug_stage < 0 || debug_stage >= 100);
    TailScratch* tail = in.tail ? in.tail : &m->tails[stream];
    // grid.x limit is 2^31-1 blocks; chunk anyway to keep launches bounded
    const int64_t kChunk = (int64_t)(1 << 20) * in.steps;   // whole reads per launch
    for (int64_t off = 0; off < n; off += kChunk) {
        const int64_t cnt = (n - off < kChunk) ? (n - off) : kChunk;
        if (timed) DBH_HIP(m->timing.begin(stream, cnt));
        // production launches are persistent: at most one workgroup per CU, each walking its
        // share of the windows; the debug modes keep one workgroup per window
        // (a workgroup takes its windows in groups of dbh::kGroup: dbh_forward.hip)
        const bool one_per_group = debug_stage >= 0;
        const int64_t groups = (cnt + dbh::kGroup - 1) / dbh::kGroup;
        const unsigned grid = (unsigned)(one_per_group || groups < m->cus ? groups : m->cus);
        // (a no-op for a tail the deflated path sized before it took the forward stream's lock)
        DBH_HIP(tail->reserve(grid, stream));
        dbh::ForwardArgs a;
        a.packed = m->packed.as<float>();
        a.x = x_dev ? x_dev + off * dbh::kWindow : nullptr;
        a.probs = probs_dev ? probs_dev + off * m->n_classes : nullptr;
        a.debug_out = debug_dev ? debug_dev + off * dbh::kStageFloats[debug_stage < 0 || debug_stage > 7 ? 0 : debug_stage]
                                : nullptr;
        a.samples = in.samples;
        a.offsets = in.offsets ? (const long long*)(in.offsets + off / in.steps) : nullptr;
        a.calls = in.calls ? (int*)(in.calls + off / in.steps) : nullptr;
        a.tail_scratch = tail->scratch();
        // production launches hand their windows out by counter; the debug modes (which may stop
        // half-way, and index their output by window) keep fixed shares
        a.win_counter = (debug_stage < 0 && m->windows_by_counter) ? tail->counter() : nullptr;
        a.clock_out = nullptr;
        if (m->clock_probe && debug_stage < 0) {
            DBH_HIP(m->clock.reserve((size_t)grid * (4 + dbh::kPhaseMarks * dbh::kPhaseGroups) * sizeof(int64_t)));
            a.clock_out = m->clock.as<long long>();
            m->clock_grid = grid;
        }
        a.score_diff = in.score_diff;
        a.read0 = (long long)(in.hints.read0 + off / in.steps);
        a.len_hint = (long long)in.hints.len_hint;
        a.hint_cap = (long long)in.hints.hint_cap;
        a.n_windows = (long long)cnt;
        a.n_classes = m->n_classes;
        a.debug_stage = debug_stage;
        a.steps = in.steps;
        a.side = in.side;
        a.phases = m->phase_probe ? 1 : 0;
        a.chunk4_min_left = m->chunk4_rounds * (int)grid;
        a.chunk2_min_left = m->chunk2_rounds * (int)grid;
        // production launches run the lean build of the kernel (dbh_lean.hip); the debug stages,
        // the 100 + k timing stops and the timeline stay on the full one.  (The lean build keeps
        // the phase stamps - compiling them out as well measured +0.3 %, inside the runs' spread -
        // so phase_cycles_per_group is still measured on the kernel that ships.)
        const bool lean = m->forward_lean && debug_stage < 0;
        DBH_HIP(lean ? dbh_kernels::launch_forward_lean(a, grid, stream)
                     : dbh_kernels::launch_forward(a, grid, stream));
        if (timed) DBH_HIP(m->timing.end(stream));
    }
    return DBH_OK;
}

// the general path's workspace (its share of dbh_classify_workspace_bytes and of
// dbh_sweep_workspace_bytes): per-window probabilities, then, at general_act_offset, the
// activations of one chunk.  Sizing and window_probs_dev place them by the one function.
size_t general_act_offset(const dbh_model* m, int64_t windows) {
    return align256((size_t)windows * m->n_classes * sizeof(float));
}
size_t general_workspace(const dbh_model* m, int64_t n_reads, int steps) {
    const int64_t windows = n_reads * steps;
    return general_act_offset(m, windows) + dbh_gen::activation_bytes(m->gen, windows);
}

// The window pass of either model kind: the probabilities of every window of n_reads reads,
// [n_reads * steps, C], to the front of the workspace.  A general model runs layer by layer with its
// activations behind them; a persistent model's forward kernel slices and normalises its own windows
// and, given no calls pointer, leaves per-window probabilities at one scan step too.  (score_diff
// only travels with the launch: nothing is called here.)
int window_probs_dev(dbh_model* m, const int16_t* samples_dev, const int64_t* offsets_dev,
                     int64_t n_reads, int steps, int side, double score_diff, const ReadHints& hints,
                     TailScratch* tail, void* workspace_dev, hipStream_t stream) {
    if (!workspace_dev) return DBH_ERR_INVALID_ARGUMENT;
    const int64_t windows = n_reads * steps;
    float* wprobs = (float*)workspace_dev;
    if (m->kind == DBH_MODEL_KIND_GENERAL) {
        DBH_HIP(dbh_gen::forward(m->gen, nullptr, samples_dev, offsets_dev, steps, side, windows, wprobs,
                                 nullptr, (char*)workspace_dev + general_act_offset(m, windows), stream));
        return DBH_OK;
    }
    const FusedInput in{samples_dev, offsets_dev, steps, side, score_diff, nullptr, hints, tail};
    return launch_forward(m, nullptr, windows, wprobs, -1, nullptr, stream, in);
}

// dbh_predict(_dev) and dbh_evidence_dev on a general model: activations in a per-stream buffer of
// the model (evidence_dev null: the probabilities alone)
int general_predict(dbh_model* m, const float* x_dev, int64_t n, float* probs_dev,
                    hipStream_t stream, float* evidence_dev = nullptr) {
    if (n == 0) return DBH_OK;
    DeviceBlock& act = m->gen_scratch[stream];
    DBH_HIP(act.reserve(dbh_gen::activation_bytes(m->gen, n)));
    DBH_HIP(dbh_gen::forward(m->gen, x_dev, nullptr, nullptr, 1, 0, n, probs_dev, evidence_dev,
                             act.get(), stream));
    return DBH_OK;
}

}  // namespace

extern "C" {

const char* dbh_version(void) { return "deepbinner_hip 0.1 (gfx950)"; }

const char* dbh_status_string(int status) {
    switch (status) {
        case DBH_OK: return "ok";
        case DBH_ERR_INVALID_ARGUMENT: return "invalid argument";
        case DBH_ERR_NO_DEVICE: return "no HIP device available";
        case DBH_ERR_HIP: return "HIP runtime error";
        case DBH_ERR_BAD_WEIGHTS: return "weight blob does not match the Deepbinner architecture";
        case DBH_ERR_UNSUPPORTED: return "unsupported model geometry";
        case DBH_ERR_OUT_OF_MEMORY: return "out of device memory";
        case DBH_ERR_COMM: return "multi-device exchange failed";
        default: return "unknown status";
    }
}

const char* dbh_last_error(void) { return g_last_error.c_str(); }

int dbh_device_count(int* count) {
    if (!count) return DBH_ERR_INVALID_ARGUMENT;
    int n = 0;
    // A host thread that waits for the GPU sleeps instead of spinning: the hosts this runs on
    // have few cores per GPU (profiles/r03_cpu_capacity.txt) and the loader wants them.  Must be
    // said before the runtime creates its context; DEEPBINNER_SPIN_WAIT=1 keeps the default.
    static const bool once = [] {
        const char* spin = std::getenv("DEEPBINNER_SPIN_WAIT");
        if (!(spin && spin[0] == '1')) {
            int devices = 0;
            if (hipGetDeviceCount(&devices) == hipSuccess)
                for (int d = 0; d < devices; ++d)
                    if (hipSetDevice(d) == hipSuccess)
                        (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
            if (devices > 0) (void)hipSetDevice(0);
            (void)hipGetLastError();
        }
        return true;
    }();
    (void)once;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        hip_fail(e, "hipGetDeviceCount");
        return DBH_ERR_NO_DEVICE;
    }
    *count = n;
    return n > 0 ? DBH_OK : DBH_ERR_NO_DEVICE;
}

int dbh_set_device(int ordinal) {
    DBH_HIP(hipSetDevice(ordinal));
    return DBH_OK;
}

int dbh_get_device(int* ordinal) {
    if (!ordinal) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipGetDevice(ordinal));
    return DBH_OK;
}

int dbh_device_name(int ordinal, char* buf, int buf_len) {
    if (!buf || buf_len <= 0) return DBH_ERR_INVALID_ARGUMENT;
    hipDeviceProp_t prop;
    DBH_HIP(hipGetDeviceProperties(&prop, ordinal));
    std::snprintf(buf, (size_t)buf_len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName,
                  prop.multiProcessorCount);
    return DBH_OK;
}

int dbh_device_synchronize(void) {
    DBH_HIP(hipDeviceSynchronize());
    return DBH_OK;
}

int dbh_malloc(void** dev_ptr, size_t bytes) {
    if (!dev_ptr) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipMalloc(dev_ptr, bytes ? bytes : 1));
    return DBH_OK;
}
int dbh_free(void* dev_ptr) {
    if (dev_ptr) DBH_HIP(hipFree(dev_ptr));
    return DBH_OK;
}
int dbh_malloc_host(void** host_ptr, size_t bytes) {
    if (!host_ptr) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipHostMalloc(host_ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return DBH_OK;
}
int dbh_free_host(void* host_ptr) {
    if (host_ptr) DBH_HIP(hipHostFree(host_ptr));
    return DBH_OK;
}
int dbh_host_device_pointer(void* host_ptr, void** dev_ptr) {
    if (!host_ptr || !dev_ptr) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipHostGetDevicePointer(dev_ptr, host_ptr, 0));
    return DBH_OK;
}
int dbh_memcpy_h2d(void* dst, const void* src, size_t bytes, dbh_stream stream) {
    DBH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return DBH_OK;
}
int dbh_memcpy_d2h(void* dst, const void* src, size_t bytes, dbh_stream stream) {
    DBH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return DBH_OK;
}
int dbh_memcpy_d2d(void* dst, const void* src, size_t bytes, dbh_stream stream) {
    DBH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DBH_OK;
}
int dbh_stream_create(dbh_stream* stream) {
    if (!stream) return DBH_ERR_INVALID_ARGUMENT;
    hipStream_t s;
    DBH_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (dbh_stream)s;
    return DBH_OK;
}
int dbh_stream_destroy(dbh_stream stream) {
    DBH_HIP(hipStreamDestroy((hipStream_t)stream));
    return DBH_OK;
}
int dbh_stream_synchronize(dbh_stream stream) {
    DBH_HIP(hipStreamSynchronize((hipStream_t)stream));
    return DBH_OK;
}
int dbh_event_create(dbh_event* event) {
    if (!event) return DBH_ERR_INVALID_ARGUMENT;
    hipEvent_t e;
    DBH_HIP(hipEventCreate(&e));
    *event = (dbh_event)e;
    return DBH_OK;
}
int dbh_event_destroy(dbh_event event) {
    DBH_HIP(hipEventDestroy((hipEvent_t)event));
    return DBH_OK;
}
int dbh_event_record(dbh_event event, dbh_stream stream) {
    DBH_HIP(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return DBH_OK;
}
int dbh_event_synchronize(dbh_event event) {
    DBH_HIP(hipEventSynchronize((hipEvent_t)event));
    return DBH_OK;
}
int dbh_stream_wait_event(dbh_stream stream, dbh_event event) {
    DBH_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
    return DBH_OK;
}
int dbh_event_elapsed_ms(dbh_event start, dbh_event stop, float* ms) {
    if (!ms) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return DBH_OK;
}

int dbh_model_create(const float* weights, int64_t n_floats, int n_classes, int input_size,
                     dbh_model** model) {
    if (!weights || !model) return DBH_ERR_INVALID_ARGUMENT;
    *model = nullptr;
    if (input_size != dbh::kWindow || n_classes < 2 || n_classes > dbh::kMaxClasses)
        return DBH_ERR_UNSUPPORTED;
    if (n_floats != dbh_net::param_count(n_classes)) return DBH_ERR_BAD_WEIGHTS;
    int count = 0;
    DBH_TRY(dbh_device_count(&count));
    std::vector<float> packed;
    dbh_pack::pack_persistent(weights, n_classes, packed);
    std::unique_ptr<dbh_model> m(new (std::nothrow) dbh_model());
    if (!m) return DBH_ERR_OUT_OF_MEMORY;
    m->n_classes = n_classes;
    hipError_t e = hipGetDevice(&m->device);
    if (e == hipSuccess) {
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device);
        if (e == hipSuccess && cus > 0) m->cus = cus;
        // DEEPBINNER_GRID_CAP=n: at most n workgroups per launch (tests: long shares of windows
        // per workgroup - prefetch across windows, full and partial tail batches - out of a few
        // hundred windows)
        if (const char* cap = std::getenv("DEEPBINNER_GRID_CAP")) {
            const int c = std::atoi(cap);
            if (c > 0 && c < m->cus) m->cus = c;
        }
        m->cus_total = m->cus;
    }
    const char* knob = std::getenv("DEEPBINNER_LAUNCH_PER_BATCH");
    m->launch_per_batch = knob && knob[0] == '1';
    const char* zc = std::getenv("DEEPBINNER_HOST_ZERO_COPY");
    m->host_zero_copy = !(zc && zc[0] == '0');
    const char* sw = std::getenv("DEEPBINNER_STATIC_WINDOWS");
    m->windows_by_counter = !(sw && sw[0] == '1');
    const char* fb = std::getenv("DEEPBINNER_FORWARD_BUILD");
    m->forward_lean = !(fb && std::strcmp(fb, "full") == 0);
    if (const char* c4 = std::getenv("DEEPBINNER_CHUNK4_ROUNDS")) m->chunk4_rounds = std::atoi(c4);
    if (const char* c2 = std::getenv("DEEPBINNER_CHUNK2_ROUNDS")) m->chunk2_rounds = std::atoi(c2);
    if (e == hipSuccess) e = m->packed.reserve(packed.size() * sizeof(float));
    if (e == hipSuccess)
        e = hipMemcpy(m->packed.get(), packed.data(), packed.size() * sizeof(float),
                      hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "dbh_model_create");      // (m frees what it holds)
    *model = m.release();
    return DBH_OK;
}

int dbh_model_create_ex(const float* weights, int64_t n_floats, int n_classes, int input_size,
                        unsigned flags, dbh_model** model) {
    if (!weights || !model || flags > DBH_MODEL_GENERAL) return DBH_ERR_INVALID_ARGUMENT;
    *model = nullptr;
    if (!dbh_gen::geometry_ok(input_size, n_classes)) return DBH_ERR_UNSUPPORTED;
    if (n_floats != dbh_net::param_count(n_classes)) return DBH_ERR_BAD_WEIGHTS;
    if (flags == DBH_MODEL_AUTO && input_size == dbh::kWindow && n_classes <= dbh::kMaxClasses)
        return dbh_model_create(weights, n_floats, n_classes, input_size, model);
    int count = 0;
    DBH_TRY(dbh_device_count(&count));
    std::unique_ptr<dbh_model> m(new (std::nothrow) dbh_model());
    if (!m) return DBH_ERR_OUT_OF_MEMORY;
    m->n_classes = n_classes;
    m->input_size = input_size;
    m->kind = DBH_MODEL_KIND_GENERAL;
    hipError_t e = hipGetDevice(&m->device);
    if (e == hipSuccess) e = dbh_gen::create(weights, n_classes, input_size, &m->gen);
    if (e != hipSuccess) return hip_fail(e, "dbh_model_create_ex");
    *model = m.release();
    return DBH_OK;
}

int dbh_model_kind(const dbh_model* m, int* kind) {
    if (!m || !kind) return DBH_ERR_INVALID_ARGUMENT;
    *kind = m->kind;
    return DBH_OK;
}

int dbh_model_destroy(dbh_model* m) {
    delete m;      // (every buffer, stream and event is a member that frees itself: dbh_owned.h)
    return DBH_OK;
}

int dbh_model_input_size(const dbh_model* m, int* input_size) {
    if (!m || !input_size) return DBH_ERR_INVALID_ARGUMENT;
    *input_size = m->input_size;
    return DBH_OK;
}
int dbh_model_output_size(const dbh_model* m, int* n_classes) {
    if (!m || !n_classes) return DBH_ERR_INVALID_ARGUMENT;
    *n_classes = m->n_classes;
    return DBH_OK;
}

int dbh_predict_dev(dbh_model* m, const float* x_dev, int64_t n, float* probs_dev,
                    dbh_stream stream) {
    if (!m || n < 0 || (n > 0 && (!x_dev || !probs_dev))) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind == DBH_MODEL_KIND_GENERAL)
        return general_predict(m, x_dev, n, probs_dev, (hipStream_t)stream);
    return launch_forward(m, x_dev, n, probs_dev, -1, nullptr, (hipStream_t)stream);
}

int dbh_predict(dbh_model* m, const float* x_host, int64_t n, float* probs_host) {
    if (!m || n < 0 || (n > 0 && (!x_host || !probs_host))) return DBH_ERR_INVALID_ARGUMENT;
    if (n == 0) return DBH_OK;
    DBH_HIP(hipSetDevice(m->device));      // (see dbh_classify_i16)
    // bounded staging: 65,536 windows of 1,024 samples (256 MiB of fp32 input) per round trip
    const int64_t L = m->input_size;
    const int64_t kChunk = 65536 * dbh::kWindow / L;
    const int64_t cap = n < kChunk ? n : kChunk;
    DBH_HIP(m->in.reserve((size_t)(cap * L) * sizeof(float)));
    DBH_HIP(m->out.reserve((size_t)cap * m->n_classes * sizeof(float)));
    for (int64_t off = 0; off < n; off += kChunk) {
        const int64_t cnt = (n - off < kChunk) ? (n - off) : kChunk;
        DBH_HIP(hipMemcpyAsync(m->in.get(), x_host + off * L, (size_t)(cnt * L) * sizeof(float),
                               hipMemcpyHostToDevice, 0));
        DBH_TRY(m->kind == DBH_MODEL_KIND_GENERAL
                    ? general_predict(m, m->in.as<float>(), cnt, m->out.as<float>(), 0)
                    : launch_forward(m, m->in.as<float>(), cnt, m->out.as<float>(), -1, nullptr, 0));
        DBH_HIP(hipMemcpyAsync(probs_host + off * m->n_classes, m->out.get(),
                               (size_t)cnt * m->n_classes * sizeof(float), hipMemcpyDeviceToHost, 0));
        DBH_HIP(hipStreamSynchronize(0));
    }
    return DBH_OK;
}

int dbh_normalise_windows_dev(const int16_t* samples_dev, const int64_t* offsets_dev,
                              int64_t n_reads, int side, int scan_size, float* windows_dev,
                              dbh_stream stream) {
    const int steps = dbh_host::model_steps(dbh::kWindow, scan_size);
    if (n_reads < 0 || steps <= 0 ||
        (side != DBH_SIDE_START && side != DBH_SIDE_END))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!samples_dev || !offsets_dev || !windows_dev) return DBH_ERR_INVALID_ARGUMENT;
    const int64_t kChunkReads = (1 << 24) / steps;
    for (int64_t r0 = 0; r0 < n_reads; r0 += kChunkReads) {
        const int64_t cnt = (n_reads - r0 < kChunkReads) ? (n_reads - r0) : kChunkReads;
        DBH_HIP(dbh_kernels::launch_normalise(samples_dev, (const long long*)(offsets_dev + r0), steps,
                                              side, windows_dev + r0 * steps * dbh::kWindow,
                                              (unsigned)(cnt * steps), (hipStream_t)stream));
    }
    return DBH_OK;
}

int dbh_merge_calls_dev(const float* window_probs_dev, int64_t n_reads, int steps, int n_classes,
                        double score_diff, float* probs_dev, int32_t* calls_dev,
                        dbh_stream stream) {
    if (n_reads < 0 || steps <= 0 || n_classes < 2 || n_classes > dbh::kMaxClasses)
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!window_probs_dev || !probs_dev || !calls_dev) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(dbh_kernels::launch_merge(window_probs_dev, (long long)n_reads, steps, n_classes,
                                      score_diff, probs_dev, (int*)calls_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_combine_calls_dev(const int32_t* start_calls_dev, const int32_t* end_calls_dev,
                          int64_t n_reads, int mode, int32_t* out_dev, dbh_stream stream) {
    if (n_reads < 0 || mode < DBH_REQUIRE_EITHER || mode > DBH_REQUIRE_BOTH)
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!start_calls_dev || !end_calls_dev || !out_dev) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(dbh_kernels::launch_combine(start_calls_dev, end_calls_dev, (long long)n_reads, mode,
                                        out_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_classify_workspace_bytes(const dbh_model* m, int64_t n_reads, int scan_size,
                                 size_t* bytes) {
    if (!m || !bytes || n_reads < 0) return DBH_ERR_INVALID_ARGUMENT;
    const int steps = dbh_host::model_steps(m->input_size, scan_size);
    if (steps <= 0) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind == DBH_MODEL_KIND_GENERAL) {
        *bytes = general_workspace(m, n_reads, steps);
        return DBH_OK;
    }
    // the per-window probabilities the merge kernel reads; one scan step needs nothing (the
    // forward kernel finishes the read itself), and the windows themselves never leave LDS
    const size_t windows = (size_t)n_reads * steps;
    *bytes = steps == 1 ? 0 : windows * m->n_classes * sizeof(float) + 256;
    return DBH_OK;
}

}  // extern "C"

namespace {
int classify_i16_dev(dbh_model* m, const int16_t* samples_dev, const int64_t* offsets_dev,
                     int64_t n_reads, int side, int scan_size, double score_diff,
                     float* probs_dev, int32_t* calls_dev, void* workspace_dev, dbh_stream stream,
                     const ReadHints& hints, TailScratch* tail = nullptr) {
    if (!m || n_reads < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    const int steps = dbh_host::model_steps(m->input_size, scan_size);
    if (steps <= 0 || (side != DBH_SIDE_START && side != DBH_SIDE_END) || !samples_dev ||
        !offsets_dev || !probs_dev || !calls_dev)
        return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind == DBH_MODEL_KIND_PERSISTENT && steps == 1) {
        // one window per read: slice + normalise + CNN + renormalise + call in ONE launch
        const FusedInput in{samples_dev, offsets_dev, steps, side, score_diff, calls_dev, hints, tail};
        return launch_forward(m, nullptr, n_reads, probs_dev, -1, nullptr, (hipStream_t)stream, in);
    }
    // a general model (any steps, C <= 256), or several scan steps per read: every window's
    // probabilities to the workspace, then the model's merge kernel finishes each read
    DBH_TRY(window_probs_dev(m, samples_dev, offsets_dev, n_reads, steps, side, score_diff, hints, tail,
                             workspace_dev, (hipStream_t)stream));
    const float* wprobs = (const float*)workspace_dev;
    if (m->kind == DBH_MODEL_KIND_GENERAL) {
        DBH_HIP(dbh_gen::merge(wprobs, n_reads, steps, m->n_classes, score_diff, probs_dev,
                               calls_dev, (hipStream_t)stream));
        return DBH_OK;
    }
    return dbh_merge_calls_dev(wprobs, n_reads, steps, m->n_classes, score_diff, probs_dev,
                               calls_dev, stream);
}

// A pair of models (start, end; either may be null) on the same reads: they must sit on one
// device, agree on the class count and take the scan size
int check_pair(dbh_model* const models[2], int scan_size) {
    if (models[0] && models[1] && (models[0]->device != models[1]->device ||
                                   models[0]->n_classes != models[1]->n_classes))
        return DBH_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < 2; ++j)
        if (models[j] && dbh_host::model_steps(models[j]->input_size, scan_size) <= 0)
            return DBH_ERR_INVALID_ARGUMENT;
    return DBH_OK;
}

// one workspace serves both, their kernels follow each other on one stream (after check_pair, for
// n_reads >= 0, dbh_classify_workspace_bytes has nothing left to refuse)
size_t pair_workspace_bytes(dbh_model* const models[2], int64_t n_reads, int scan_size) {
    size_t bytes = 0, mine = 0;
    for (int j = 0; j < 2; ++j)
        if (models[j] && dbh_classify_workspace_bytes(models[j], n_reads, scan_size, &mine) == DBH_OK)
            bytes = std::max(bytes, mine);
    return bytes;
}

// Each model of the pair over the same samples - probabilities to probs_dev[j], calls to
// calls_dev[j] - then, when both are there, combine_calls of the two to final_dev.
int classify_pair_dev(dbh_model* const models[2], const int sides[2], const int16_t* samples_dev,
                      const int64_t* offsets_dev, int64_t n_reads, int scan_size, double score_diff,
                      float* const probs_dev[2], int32_t* const calls_dev[2], int combine_mode,
                      int32_t* final_dev, void* workspace_dev, hipStream_t stream,
                      const ReadHints& hints, TailScratch* tail) {
    for (int j = 0; j < 2; ++j) {
        if (!models[j]) continue;
        DBH_TRY(classify_i16_dev(models[j], samples_dev, offsets_dev, n_reads, sides[j], scan_size,
                                 score_diff, probs_dev[j], calls_dev[j], workspace_dev,
                                 (dbh_stream)stream, hints, tail));
    }
    if (!(models[0] && models[1])) return DBH_OK;
    return dbh_combine_calls_dev(calls_dev[0], calls_dev[1], n_reads, combine_mode, final_dev,
                                 (dbh_stream)stream);
}

// Is [p, p + bytes) host memory the GPU's DMA engine can read in place (hipHostMalloc /
// hipHostRegister: what dbh_malloc_host and dbh_host_alloc hand out)?
bool is_pinned(const void* p, size_t bytes) {
    if (!p || bytes == 0) return false;
    hipPointerAttribute_t a0, a1;
    if (hipPointerGetAttributes(&a0, p) != hipSuccess ||
        hipPointerGetAttributes(&a1, (const char*)p + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();      // "not a registered pointer" is an answer, not a failure
        return false;
    }
    return a0.type == hipMemoryTypeHost && a1.type == hipMemoryTypeHost;
}

using dbh_host::staged_copy;

// One call of the host-buffer pipeline (host_groups): what its tenants differ in.
struct GroupJob {
    int steps = 1;                                    // windows per read: sets the group size
    std::function<size_t(int64_t cnt)> out_bytes;     // a group's results (sl.d_out, sl.h_out)
    std::function<size_t(int64_t cnt)> work_bytes;    // ... and its workspace (sl.d_work)
    // the device work of a group of cnt reads, on sl.stream, results to sl.d_out -> status
    std::function<int(HostSlot& sl, const int16_t* d_samples, const int64_t* d_offsets, int64_t cnt,
                      const ReadHints& hints)> launch;
    // reads r0 .. r0 + cnt - 1 are back: h_out is what their group left at sl.d_out
    std::function<void(int64_t r0, int64_t cnt, const char* h_out)> collect;
};

// The host-buffer pipeline behind dbh_classify_i16, dbh_classify_pair_i16 and dbh_sweep_pair_i16.
// Reads travel in groups of at most ~32k windows per model through the kSlots staging slots of m,
// each with its own stream: while the GPU works on group g, group g+1 is uploaded (straight from
// the caller's buffer when that is pinned, through a pinned staging copy otherwise) and the results
// of group g-1 come back.  What a group launches reads the SAME uploaded samples, kernel after
// kernel on the group's stream.  The slots keep what they have grown to from call to call, whichever
// tenant's layout they held last.  For n_reads > 0 and offsets_host not null.
int host_groups(dbh_model* m, const GroupJob& job, const int16_t* samples_host,
                const int64_t* offsets_host, int64_t n_reads) {
    // the current device is a per-thread setting: a caller on another thread than the one that
    // created the model gets the model's device
    DBH_HIP(hipSetDevice(m->device));
    const int64_t total_samples = offsets_host[n_reads] - offsets_host[0];
    if (total_samples < 0 || (total_samples > 0 && !samples_host)) return DBH_ERR_INVALID_ARGUMENT;
    const bool pinned = total_samples > 0 &&
                        is_pinned(samples_host + offsets_host[0], (size_t)total_samples * 2);
    const int64_t group = std::max<int64_t>(
        1, (m->kind == DBH_MODEL_KIND_GENERAL ? dbh_model::kDefaultGroup : m->host_group_windows) / job.steps);
    constexpr int kSlots = dbh_model::kSlots;
    struct Pending { int64_t r0 = 0, cnt = 0; bool live = false; } pending[kSlots];
    auto drain = [&](int k) -> int {
        HostSlot& sl = m->slot[k];
        if (!pending[k].live) return DBH_OK;
        DBH_HIP(hipStreamSynchronize(sl.stream));
        job.collect(pending[k].r0, pending[k].cnt, sl.h_out.as<char>());
        pending[k].live = false;
        return DBH_OK;
    };
    // an error in the middle of the loop must not leave another slot's copies in flight: its
    // pinned buffers belong to the next call
    auto fail = [&](int status) -> int {
        for (auto& sl : m->slot)
            if (sl.stream) (void)hipStreamSynchronize(sl.stream);
        return status;
    };
    int64_t g = 0;
    for (int64_t r0 = 0; r0 < n_reads; r0 += group, ++g) {
        const int k = (int)(g % kSlots);
        HostSlot& sl = m->slot[k];
        int st = drain(k);
        if (st != DBH_OK) return fail(st);
        hipError_t e = hipSuccess;
        if (!sl.stream) e = hipStreamCreateWithFlags(&sl.stream.h, hipStreamNonBlocking);
        if (e != hipSuccess) return fail(hip_fail(e, "hipStreamCreateWithFlags"));
        const int64_t cnt = (n_reads - r0 < group) ? (n_reads - r0) : group;
        const int64_t s0 = offsets_host[r0], s1 = offsets_host[r0 + cnt];
        if (s1 < s0) return fail(DBH_ERR_INVALID_ARGUMENT);
        const size_t raw_bytes = (size_t)(s1 - s0) * sizeof(int16_t);
        const size_t sample_bytes = align256(raw_bytes);
        const size_t off_bytes = (size_t)(cnt + 1) * sizeof(int64_t);
        const size_t out_bytes = job.out_bytes(cnt), work = job.work_bytes(cnt);
        // host side: the relative offsets always, the samples only when they have to be staged
        e = sl.h_in.reserve(off_bytes + (pinned ? 0 : sample_bytes));
        if (e == hipSuccess) e = sl.h_out.reserve(out_bytes);
        if (e == hipSuccess) e = sl.d_in.reserve(sample_bytes + off_bytes);
        if (e == hipSuccess) e = sl.d_out.reserve(out_bytes);
        if (e == hipSuccess && work) e = sl.d_work.reserve(work);
        if (e != hipSuccess) return fail(hip_fail(e, "growing a staging slot"));

        int64_t* rel = sl.h_in.as<int64_t>();
        for (int64_t i = 0; i <= cnt; ++i) rel[i] = offsets_host[r0 + i] - s0;
        const void* src = samples_host + s0;
        if (raw_bytes && !pinned) {
            staged_copy(sl.h_in.as<char>(off_bytes), src, raw_bytes);
            src = sl.h_in.as<char>(off_bytes);
        }
        // The samples reach the kernel either by a copy into HBM first, or not at all: the
        // forward kernel asks for a window's 2 KB ~25,000 cycles before it needs them, which
        // hides a PCIe round trip as well as an HBM one - so it can read pinned host memory in
        // place.  (A copy between two launches cannot overlap them here: the persistent kernel
        // fills every CU's registers and LDS, and the copy of the next group only starts when
        // it has drained - 1.2 ms of idle GPU per 6 ms group, profiles/r03_host_path_trace.txt.)
        const int16_t* d_samples = sl.d_in.as<int16_t>();
        const int64_t* d_offsets = sl.d_in.as<int64_t>(sample_bytes);
        if (raw_bytes && m->host_zero_copy) {
            void* mapped = nullptr;
            e = hipHostGetDevicePointer(&mapped, const_cast<void*>(src), 0);
            d_samples = (const int16_t*)mapped;
        } else if (raw_bytes) {
            e = hipMemcpyAsync(sl.d_in.get(), src, raw_bytes, hipMemcpyHostToDevice, sl.stream);
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync((void*)d_offsets, rel, off_bytes, hipMemcpyHostToDevice, sl.stream);
        if (e != hipSuccess) return fail(hip_fail(e, "hipMemcpyAsync H2D"));
        // (all reads of the group equally long?  then the kernel need not wait for the offsets)
        st = job.launch(sl, d_samples, d_offsets, cnt,
                        ReadHints{0, dbh_host::uniform_length(rel, cnt), s1 - s0});
        if (st != DBH_OK) return fail(st);
        e = hipMemcpyAsync(sl.h_out.get(), sl.d_out.get(), out_bytes, hipMemcpyDeviceToHost, sl.stream);
        if (e != hipSuccess) return fail(hip_fail(e, "hipMemcpyAsync D2H"));
        pending[k].r0 = r0;
        pending[k].cnt = cnt;
        pending[k].live = true;
    }
    for (int i = 0; i < kSlots; ++i) {       // oldest first
        const int st = drain((int)((g + i) % kSlots));
        if (st != DBH_OK) return fail(st);
    }
    return DBH_OK;
}

struct HostJob {
    dbh_model* model[2] = {nullptr, nullptr};      // start model, end model (either may be null)
    int side[2] = {DBH_SIDE_START, DBH_SIDE_END};
    float* probs_host[2] = {nullptr, nullptr};     // per model: n_reads x C, or null
    int32_t* calls_host[2] = {nullptr, nullptr};   // per model: n_reads, or null
    int32_t* final_host = nullptr;                 // combine_calls of the two, or null
    int combine_mode = DBH_REQUIRE_EITHER;
};

// dbh_classify_i16 and dbh_classify_pair_i16 through host_groups: per group both models' kernels,
// the merge kernels and the combine kernel, a GroupOut coming back
int classify_host(const HostJob& job, const int16_t* samples_host, const int64_t* offsets_host,
                  int64_t n_reads, int scan_size, double score_diff) {
    dbh_model* m = job.model[0] ? job.model[0] : job.model[1];      // owns the slots
    if (!m || n_reads < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    const bool both = job.model[0] && job.model[1];
    if (!offsets_host || check_pair(job.model, scan_size) != DBH_OK || (job.final_host && !both))
        return DBH_ERR_INVALID_ARGUMENT;
    const int C = m->n_classes;
    auto layout = [&](int64_t cnt) { return dbh_host::GroupOut(cnt, C, job.model[0], job.model[1]); };
    GroupJob groups;
    for (dbh_model* mj : job.model)      // the larger of the models' (they may differ in input size)
        if (mj) groups.steps = std::max(groups.steps, dbh_host::model_steps(mj->input_size, scan_size));
    groups.out_bytes = [&](int64_t cnt) { return layout(cnt).total; };
    groups.work_bytes = [&](int64_t cnt) { return pair_workspace_bytes(job.model, cnt, scan_size); };
    groups.launch = [&](HostSlot& sl, const int16_t* d_samples, const int64_t* d_offsets, int64_t cnt,
                        const ReadHints& hints) {
        const dbh_host::GroupOut out = layout(cnt);
        float* const d_probs[2] = {sl.d_out.as<float>(out.probs[0]), sl.d_out.as<float>(out.probs[1])};
        int32_t* const d_calls[2] = {sl.d_out.as<int32_t>(out.calls[0]), sl.d_out.as<int32_t>(out.calls[1])};
        return classify_pair_dev(job.model, job.side, d_samples, d_offsets, cnt, scan_size, score_diff,
                                 d_probs, d_calls, job.combine_mode, sl.d_out.as<int32_t>(out.final_calls),
                                 sl.d_work.get(), sl.stream, hints, &sl.tail);
    };
    groups.collect = [&](int64_t r0, int64_t cnt, const char* h) {
        const dbh_host::GroupOut at = layout(cnt);
        for (int j = 0; j < 2; ++j) {
            if (job.model[j] && job.probs_host[j])
                std::memcpy(job.probs_host[j] + r0 * C, h + at.probs[j], (size_t)cnt * C * sizeof(float));
            if (job.model[j] && job.calls_host[j])
                std::memcpy(job.calls_host[j] + r0, h + at.calls[j], (size_t)cnt * sizeof(int32_t));
        }
        if (both && job.final_host)
            std::memcpy(job.final_host + r0, h + at.final_calls, (size_t)cnt * sizeof(int32_t));
    };
    return host_groups(m, groups, samples_host, offsets_host, n_reads);
}

}  // namespace

extern "C" {

int dbh_model_set_read_length_hint(dbh_model* m, int64_t read_length, int64_t capacity_samples) {
    if (!m || read_length < 0 || capacity_samples < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_OK;       // (nothing to tune)
    m->hint_len = read_length;
    m->hint_cap = read_length > 0 ? capacity_samples : 0;
    return DBH_OK;
}

int dbh_classify_i16_dev(dbh_model* m, const int16_t* samples_dev, const int64_t* offsets_dev,
                         int64_t n_reads, int side, int scan_size, double score_diff,
                         float* probs_dev, int32_t* calls_dev, void* workspace_dev,
                         dbh_stream stream) {
    if (!m) return DBH_ERR_INVALID_ARGUMENT;
    return classify_i16_dev(m, samples_dev, offsets_dev, n_reads, side, scan_size, score_diff,
                            probs_dev, calls_dev, workspace_dev, stream,
                            ReadHints{0, m->hint_len, m->hint_cap});
}

int dbh_classify_i16_batched_dev(dbh_model* m, const int16_t* samples_dev,
                                 const int64_t* offsets_dev, int64_t n_reads, int batch_size,
                                 int side, int scan_size, double score_diff, float* probs_dev,
                                 int32_t* calls_dev, dbh_stream stream) {
    if (!m || n_reads < 0 || batch_size <= 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    // The reference walks its reads batch by batch because model.predict does (classify.py:130,
    // 361); a read's result does not depend on its batch.  Here the forward kernel is
    // persistent - one workgroup per CU walking windows in read order - so the batches flow
    // through ONE launch without a boundary between them (DEEPBINNER_LAUNCH_PER_BATCH=1 brings
    // the launch per batch back, for comparison).  Reads with several scan steps go in chunks
    // whose per-window probabilities fit a bounded workspace, one merge launch per chunk.
    const int steps = dbh_host::model_steps(m->input_size, scan_size);
    if (steps <= 0) return DBH_ERR_INVALID_ARGUMENT;
    // (a general model goes 65,536 windows at a time: its workspace holds them all, C up to 256)
    const int64_t chunk = m->kind == DBH_MODEL_KIND_GENERAL
                              ? std::max<int64_t>(1, 65536 / steps)
                              : m->launch_per_batch ? (int64_t)batch_size
                                                    : (steps == 1 ? n_reads : ((int64_t)1 << 20) / steps);
    size_t work = 0;
    DBH_TRY(dbh_classify_workspace_bytes(m, chunk < n_reads ? chunk : n_reads, scan_size, &work));
    if (work) DBH_HIP(m->work.reserve(work));
    // in-order on the caller's stream, so the workspace can be reused chunk after chunk
    for (int64_t r0 = 0; r0 < n_reads; r0 += chunk) {
        const int64_t cnt = (n_reads - r0 < chunk) ? (n_reads - r0) : chunk;
        DBH_TRY(classify_i16_dev(m, samples_dev, offsets_dev + r0, cnt, side, scan_size, score_diff,
                                 probs_dev + r0 * m->n_classes, calls_dev + r0, m->work.get(), stream,
                                 ReadHints{r0, m->hint_len, m->hint_cap}));
    }
    return DBH_OK;
}

int dbh_classify_i16(dbh_model* m, const int16_t* samples_host, const int64_t* offsets_host,
                     int64_t n_reads, int side, int scan_size, double score_diff,
                     float* probs_host, int32_t* calls_host) {
    if (!m || n_reads < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!offsets_host || !probs_host || !calls_host ||
        (side != DBH_SIDE_START && side != DBH_SIDE_END))
        return DBH_ERR_INVALID_ARGUMENT;
    const HostJob job{{m, nullptr}, {side, DBH_SIDE_END}, {probs_host, nullptr}, {calls_host, nullptr}};
    return classify_host(job, samples_host, offsets_host, n_reads, scan_size, score_diff);
}

int dbh_classify_pair_i16(dbh_model* start_model, dbh_model* end_model,
                          const int16_t* samples_host, const int64_t* offsets_host,
                          int64_t n_reads, int scan_size, double score_diff, int combine_mode,
                          int32_t* calls_host, int32_t* start_calls_host, int32_t* end_calls_host,
                          float* start_probs_host, float* end_probs_host) {
    if ((!start_model && !end_model) || n_reads < 0 || combine_mode < DBH_REQUIRE_EITHER ||
        combine_mode > DBH_REQUIRE_BOTH)
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!offsets_host || !calls_host) return DBH_ERR_INVALID_ARGUMENT;
    HostJob job{{start_model, end_model}, {DBH_SIDE_START, DBH_SIDE_END},
                {start_probs_host, end_probs_host}, {start_calls_host, end_calls_host}, nullptr,
                combine_mode};
    if (start_model && end_model) job.final_host = calls_host;
    else if (start_model && !start_calls_host) job.calls_host[0] = calls_host;
    else if (end_model && !end_calls_host) job.calls_host[1] = calls_host;
    const int st = classify_host(job, samples_host, offsets_host, n_reads, scan_size, score_diff);
    // one model and the caller wanted its calls twice (final + per side)
    if (st == DBH_OK && !(start_model && end_model)) {
        int32_t* side_calls = start_model ? start_calls_host : end_calls_host;
        if (side_calls && side_calls != calls_host)
            std::memcpy(calls_host, side_calls, (size_t)n_reads * sizeof(int32_t));
    }
    return st;
}

// ---- sweep: every scan size and every threshold from one window pass (dbh_sweep.hip) -------------
int dbh_sweep_windows_dev(const dbh_model* m, const float* window_probs_dev, int64_t n_reads,
                          int steps, int32_t* best_dev, double* margin_dev, dbh_stream stream) {
    if (!m || n_reads < 0 || steps < 1) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!window_probs_dev || !best_dev || !margin_dev) return DBH_ERR_INVALID_ARGUMENT;
    // the form whose sums run in the order of the model's own merge
    DBH_HIP(m->kind == DBH_MODEL_KIND_GENERAL
                ? dbh_sweep::fold256(window_probs_dev, n_reads, steps, m->n_classes, best_dev,
                                     margin_dev, (hipStream_t)stream)
                : dbh_sweep::fold32(window_probs_dev, n_reads, steps, m->n_classes, best_dev,
                                    margin_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_sweep_workspace_bytes(const dbh_model* m, int64_t n_reads, int max_scan_size,
                              size_t* bytes) {
    if (!m || !bytes || n_reads < 0) return DBH_ERR_INVALID_ARGUMENT;
    const int steps = dbh_host::model_steps(m->input_size, max_scan_size);
    if (steps <= 0) return DBH_ERR_INVALID_ARGUMENT;
    // every window's probabilities, one scan step included: the fold reads them all
    *bytes = m->kind == DBH_MODEL_KIND_GENERAL
                 ? general_workspace(m, n_reads, steps)
                 : (size_t)n_reads * steps * m->n_classes * sizeof(float) + 256;
    return DBH_OK;
}

}  // extern "C"

namespace {
// the model's own window pass at max_scan_size, then the fold where classify_i16_dev has the merge
int sweep_i16_dev(dbh_model* m, const int16_t* samples_dev, const int64_t* offsets_dev,
                  int64_t n_reads, int side, int max_scan_size, int32_t* best_dev,
                  double* margin_dev, void* workspace_dev, dbh_stream stream,
                  const ReadHints& hints, TailScratch* tail = nullptr) {
    if (!m || n_reads < 0) return DBH_ERR_INVALID_ARGUMENT;
    const int steps = dbh_host::model_steps(m->input_size, max_scan_size);
    if (steps <= 0 || (side != DBH_SIDE_START && side != DBH_SIDE_END))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!samples_dev || !offsets_dev || !best_dev || !margin_dev || !workspace_dev)
        return DBH_ERR_INVALID_ARGUMENT;
    // (at one scan step too, where classify takes the fused one-launch finish)
    DBH_TRY(window_probs_dev(m, samples_dev, offsets_dev, n_reads, steps, side, 0.0, hints, tail,
                             workspace_dev, (hipStream_t)stream));
    return dbh_sweep_windows_dev(m, (const float*)workspace_dev, n_reads, steps, best_dev, margin_dev,
                                 stream);
}

// A pair for a sweep: one device, one class count and - one fold serves both sides' prefixes -
// one input size, which max_scan_size must fit.  -> steps, or 0
int sweep_pair_steps(dbh_model* const models[2], int max_scan_size) {
    const dbh_model* m = models[0] ? models[0] : models[1];
    if (!m) return 0;
    if (models[0] && models[1] && (models[0]->device != models[1]->device ||
                                   models[0]->n_classes != models[1]->n_classes ||
                                   models[0]->input_size != models[1]->input_size))
        return 0;
    return dbh_host::model_steps(m->input_size, max_scan_size);
}

// dbh_sweep_pair_i16 through host_groups: per group each model's window pass and fold, a SweepOut -
// (best, margin) of every prefix - coming back
int sweep_host(dbh_model* const models[2], const int16_t* samples_host, const int64_t* offsets_host,
               int64_t n_reads, int max_scan_size, int32_t* const best_host[2],
               double* const margin_host[2]) {
    dbh_model* m = models[0] ? models[0] : models[1];      // owns the slots
    const int steps = sweep_pair_steps(models, max_scan_size);
    if (!m || n_reads < 0 || steps <= 0) return DBH_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < 2; ++j)
        if (models[j] && n_reads > 0 && (!best_host[j] || !margin_host[j])) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!offsets_host) return DBH_ERR_INVALID_ARGUMENT;
    const int64_t total_samples = offsets_host[n_reads] - offsets_host[0];
    if (total_samples < 0 || (total_samples > 0 && !samples_host)) return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_reads; ++i)
        if (offsets_host[i + 1] < offsets_host[i]) return DBH_ERR_INVALID_ARGUMENT;
    auto layout = [&](const void* base, int64_t cnt) {
        return dbh_host::SweepOut(const_cast<void*>(base), cnt, steps, models[0], models[1]);
    };
    GroupJob groups;
    groups.steps = steps;
    groups.out_bytes = [&](int64_t cnt) { return layout(nullptr, cnt).total; };
    groups.work_bytes = [&](int64_t cnt) {
        size_t work = 0, mine = 0;
        for (int j = 0; j < 2; ++j)
            if (models[j] && dbh_sweep_workspace_bytes(models[j], cnt, max_scan_size, &mine) == DBH_OK)
                work = std::max(work, mine);
        return work;
    };
    groups.launch = [&](HostSlot& sl, const int16_t* d_samples, const int64_t* d_offsets, int64_t cnt,
                        const ReadHints& hints) {
        const dbh_host::SweepOut d = layout(sl.d_out.get(), cnt);
        for (int j = 0; j < 2; ++j) {
            if (!models[j]) continue;
            DBH_TRY(sweep_i16_dev(models[j], d_samples, d_offsets, cnt, j == 0 ? DBH_SIDE_START : DBH_SIDE_END,
                                  max_scan_size, d.best[j], d.margin[j], sl.d_work.get(),
                                  (dbh_stream)sl.stream.h, hints, &sl.tail));
        }
        return (int)DBH_OK;
    };
    groups.collect = [&](int64_t r0, int64_t cnt, const char* h_out) {
        const dbh_host::SweepOut h = layout(h_out, cnt);
        for (int j = 0; j < 2; ++j) {
            if (!models[j]) continue;
            std::memcpy(best_host[j] + r0 * steps, h.best[j], (size_t)cnt * steps * sizeof(int32_t));
            std::memcpy(margin_host[j] + r0 * steps, h.margin[j], (size_t)cnt * steps * sizeof(double));
        }
    };
    return host_groups(m, groups, samples_host, offsets_host, n_reads);
}

// the arguments of both tally entries (device or host pointers alike)
bool tally_arguments_ok(const void* start_best, const void* start_margin, const void* end_best,
                        const void* end_margin, int64_t n_reads, int steps, int n_classes,
                        const void* thresholds, int n_thresholds, const void* counts) {
    const bool start = start_best && start_margin, end = end_best && end_margin;
    if ((start_best != nullptr) != (start_margin != nullptr) ||
        (end_best != nullptr) != (end_margin != nullptr))
        return false;
    return (start || end) && n_reads >= 0 && steps >= 1 && n_classes >= 2 &&
           n_classes <= dbh_sweep::kMaxClasses && n_thresholds >= 1 && thresholds && counts;
}

}  // namespace

extern "C" {

int dbh_sweep_i16_dev(dbh_model* m, const int16_t* samples_dev, const int64_t* offsets_dev,
                      int64_t n_reads, int side, int max_scan_size, int32_t* best_dev,
                      double* margin_dev, void* workspace_dev, dbh_stream stream) {
    if (!m) return DBH_ERR_INVALID_ARGUMENT;
    return sweep_i16_dev(m, samples_dev, offsets_dev, n_reads, side, max_scan_size, best_dev,
                         margin_dev, workspace_dev, stream, ReadHints{0, m->hint_len, m->hint_cap});
}

int dbh_sweep_pair_i16(dbh_model* start_model, dbh_model* end_model, const int16_t* samples_host,
                       const int64_t* offsets_host, int64_t n_reads, int max_scan_size,
                       int32_t* start_best_host, double* start_margin_host,
                       int32_t* end_best_host, double* end_margin_host) {
    dbh_model* const models[2] = {start_model, end_model};
    int32_t* const best[2] = {start_best_host, end_best_host};
    double* const margin[2] = {start_margin_host, end_margin_host};
    return sweep_host(models, samples_host, offsets_host, n_reads, max_scan_size, best, margin);
}

int dbh_sweep_tally_dev(const int32_t* start_best_dev, const double* start_margin_dev,
                        const int32_t* end_best_dev, const double* end_margin_dev,
                        const int32_t* labels_dev, int64_t n_reads, int steps, int n_classes,
                        const double* thresholds_dev, int n_thresholds, int64_t* counts_dev,
                        dbh_stream stream) {
    if (!tally_arguments_ok(start_best_dev, start_margin_dev, end_best_dev, end_margin_dev, n_reads,
                            steps, n_classes, thresholds_dev, n_thresholds, counts_dev))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    DBH_HIP(dbh_sweep::tally(start_best_dev, start_margin_dev, end_best_dev, end_margin_dev,
                             labels_dev, n_reads, steps, n_classes, thresholds_dev, n_thresholds,
                             (unsigned long long*)counts_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_sweep_tally(const int32_t* start_best_host, const double* start_margin_host,
                    const int32_t* end_best_host, const double* end_margin_host,
                    const int32_t* labels_host, int64_t n_reads, int steps, int n_classes,
                    const double* thresholds_host, int n_thresholds, int64_t* counts_host) {
    if (!tally_arguments_ok(start_best_host, start_margin_host, end_best_host, end_margin_host,
                            n_reads, steps, n_classes, thresholds_host, n_thresholds, counts_host))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    const bool start = start_best_host != nullptr, end = end_best_host != nullptr;
    const size_t per_side = (size_t)n_reads * steps;
    const size_t cells = (size_t)steps * n_thresholds * (start && end ? 3 : 1) * (n_classes + 3);
    // one block on the calling thread's device, freed on return
    DeviceBlock block;
    int32_t *d_best[2] = {nullptr, nullptr}, *d_labels = nullptr;
    double *d_margin[2] = {nullptr, nullptr}, *d_thresholds = nullptr;
    int64_t* d_counts = nullptr;
    DBH_HIP(block.carve([&](dbh_host::Carve& c) {
        d_best[0] = c.take<int32_t>(start ? per_side : 0);
        d_margin[0] = c.take<double>(start ? per_side : 0);
        d_best[1] = c.take<int32_t>(end ? per_side : 0);
        d_margin[1] = c.take<double>(end ? per_side : 0);
        d_labels = c.take<int32_t>(labels_host ? (size_t)n_reads : 0);
        d_thresholds = c.take<double>((size_t)n_thresholds);
        d_counts = c.take<int64_t>(cells);
    }));
    const int32_t* const h_best[2] = {start_best_host, end_best_host};
    const double* const h_margin[2] = {start_margin_host, end_margin_host};
    for (int j = 0; j < 2; ++j) {
        if (!h_best[j]) continue;
        DBH_HIP(hipMemcpy(d_best[j], h_best[j], per_side * sizeof(int32_t), hipMemcpyHostToDevice));
        DBH_HIP(hipMemcpy(d_margin[j], h_margin[j], per_side * sizeof(double), hipMemcpyHostToDevice));
    }
    if (labels_host)
        DBH_HIP(hipMemcpy(d_labels, labels_host, (size_t)n_reads * sizeof(int32_t), hipMemcpyHostToDevice));
    DBH_HIP(hipMemcpy(d_thresholds, thresholds_host, (size_t)n_thresholds * sizeof(double), hipMemcpyHostToDevice));
    DBH_HIP(hipMemset(d_counts, 0, cells * sizeof(int64_t)));
    DBH_HIP(dbh_sweep::tally(start ? d_best[0] : nullptr, start ? d_margin[0] : nullptr,
                             end ? d_best[1] : nullptr, end ? d_margin[1] : nullptr,
                             labels_host ? d_labels : nullptr, n_reads, steps, n_classes,
                             d_thresholds, n_thresholds, (unsigned long long*)d_counts, 0));
    std::vector<int64_t> got(cells);
    DBH_HIP(hipMemcpy(got.data(), d_counts, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cells; ++i) counts_host[i] += got[i];
    return DBH_OK;
}

// ---- the early tally: the live decision of every min_windows and threshold (dbh_early_core.h) ----
}  // extern "C"

namespace {
// the arguments of the three early entries (device or host pointers alike) -> P, or 0 if refused
int early_pushes_ok(const void* start_best, const void* start_margin, const void* end_best,
                    const void* end_margin, const void* lengths, int64_t n_reads, int steps,
                    int n_classes, int input_size, int64_t chunk_samples, const void* thresholds,
                    int n_thresholds, const void* calls, const void* early, const void* windows,
                    const void* pushes) {
    if (!start_best || !start_margin || (end_best != nullptr) != (end_margin != nullptr) ||
        !thresholds || !calls || !early || !windows || (lengths != nullptr) != (pushes != nullptr))
        return 0;
    if (!dbh_early::shape_ok(n_reads, steps, n_classes, input_size, chunk_samples, n_thresholds))
        return 0;
    return (int)dbh_early::pushes_bound(input_size, (long long)steps * (input_size / 2),
                                        chunk_samples);
}
}  // namespace

extern "C" {

int dbh_sweep_early_pushes(int input_size, int scan_size, int64_t chunk_samples, int* pushes) {
    if (!pushes || input_size < 2 || input_size % 2 != 0 || chunk_samples < 1 ||
        dbh_host::model_steps(input_size, scan_size) <= 0)
        return DBH_ERR_INVALID_ARGUMENT;
    const long long p = dbh_early::pushes_bound(input_size, scan_size, chunk_samples);
    if (p > dbh_early::kMaxPushes) return DBH_ERR_INVALID_ARGUMENT;
    *pushes = (int)p;
    return DBH_OK;
}

int dbh_sweep_early_tally_dev(const int32_t* start_best_dev, const double* start_margin_dev,
                              const int32_t* end_best_dev, const double* end_margin_dev,
                              const int32_t* labels_dev, const int64_t* lengths_dev,
                              int64_t n_reads, int steps, int n_classes, int input_size,
                              int64_t chunk_samples, const double* thresholds_dev,
                              int n_thresholds, int64_t* calls_dev, int64_t* early_dev,
                              int64_t* windows_dev, int64_t* pushes_dev, dbh_stream stream) {
    const int P = early_pushes_ok(start_best_dev, start_margin_dev, end_best_dev, end_margin_dev,
                                  lengths_dev, n_reads, steps, n_classes, input_size, chunk_samples,
                                  thresholds_dev, n_thresholds, calls_dev, early_dev, windows_dev,
                                  pushes_dev);
    if (P < 1) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    DBH_HIP(dbh_sweep::early_tally(
        start_best_dev, start_margin_dev, end_best_dev, end_margin_dev, labels_dev, lengths_dev,
        n_reads, steps, n_classes, input_size, chunk_samples, thresholds_dev, n_thresholds, P,
        (unsigned long long*)calls_dev, (unsigned long long*)early_dev,
        (unsigned long long*)windows_dev, (unsigned long long*)pushes_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_sweep_early_host(const int32_t* start_best_host, const double* start_margin_host,
                         const int32_t* end_best_host, const double* end_margin_host,
                         const int32_t* labels_host, const int64_t* lengths_host, int64_t n_reads,
                         int steps, int n_classes, int input_size, int64_t chunk_samples,
                         const double* thresholds_host, int n_thresholds, int64_t* calls_host,
                         int64_t* early_host, int64_t* windows_host, int64_t* pushes_host) {
    if (early_pushes_ok(start_best_host, start_margin_host, end_best_host, end_margin_host,
                        lengths_host, n_reads, steps, n_classes, input_size, chunk_samples,
                        thresholds_host, n_thresholds, calls_host, early_host, windows_host,
                        pushes_host) < 1)
        return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; lengths_host && i < n_reads; ++i)
        if (lengths_host[i] < 0) return DBH_ERR_INVALID_ARGUMENT;
    dbh_early::tally_host(start_best_host, start_margin_host, end_best_host, end_margin_host,
                          labels_host, lengths_host, n_reads, steps, n_classes, input_size,
                          chunk_samples, thresholds_host, n_thresholds, calls_host, early_host,
                          windows_host, pushes_host);
    return DBH_OK;
}

int dbh_sweep_early_tally(const int32_t* start_best_host, const double* start_margin_host,
                          const int32_t* end_best_host, const double* end_margin_host,
                          const int32_t* labels_host, const int64_t* lengths_host, int64_t n_reads,
                          int steps, int n_classes, int input_size, int64_t chunk_samples,
                          const double* thresholds_host, int n_thresholds, int64_t* calls_host,
                          int64_t* early_host, int64_t* windows_host, int64_t* pushes_host) {
    const int P = early_pushes_ok(start_best_host, start_margin_host, end_best_host,
                                  end_margin_host, lengths_host, n_reads, steps, n_classes,
                                  input_size, chunk_samples, thresholds_host, n_thresholds,
                                  calls_host, early_host, windows_host, pushes_host);
    if (P < 1) return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; lengths_host && i < n_reads; ++i)
        if (lengths_host[i] < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    const bool end = end_best_host != nullptr;
    const size_t per_side = (size_t)n_reads * steps, cells = (size_t)steps * n_thresholds;
    // the four arrays in one run of int64: calls, early, windows, pushes
    const size_t n_out[4] = {cells * (end ? 3 : 1) * (n_classes + 3), cells * dbh_early::kColumns,
                             cells * steps, lengths_host ? cells * P : 0};
    const size_t n_all = n_out[0] + n_out[1] + n_out[2] + n_out[3];
    // one block on the calling thread's device, freed on return
    DeviceBlock block;
    int32_t *d_best[2] = {nullptr, nullptr}, *d_labels = nullptr;
    double *d_margin[2] = {nullptr, nullptr}, *d_thresholds = nullptr;
    int64_t *d_lengths = nullptr, *d_out = nullptr;
    DBH_HIP(block.carve([&](dbh_host::Carve& c) {
        d_best[0] = c.take<int32_t>(per_side);
        d_margin[0] = c.take<double>(per_side);
        d_best[1] = c.take<int32_t>(end ? per_side : 0);
        d_margin[1] = c.take<double>(end ? per_side : 0);
        d_labels = c.take<int32_t>(labels_host ? (size_t)n_reads : 0);
        d_lengths = c.take<int64_t>(lengths_host ? (size_t)n_reads : 0);
        d_thresholds = c.take<double>((size_t)n_thresholds);
        d_out = c.take<int64_t>(n_all);
    }));
    const int32_t* const h_best[2] = {start_best_host, end_best_host};
    const double* const h_margin[2] = {start_margin_host, end_margin_host};
    for (int j = 0; j < 2; ++j) {
        if (!h_best[j]) continue;
        DBH_HIP(hipMemcpy(d_best[j], h_best[j], per_side * sizeof(int32_t), hipMemcpyHostToDevice));
        DBH_HIP(hipMemcpy(d_margin[j], h_margin[j], per_side * sizeof(double), hipMemcpyHostToDevice));
    }
    if (labels_host)
        DBH_HIP(hipMemcpy(d_labels, labels_host, (size_t)n_reads * sizeof(int32_t), hipMemcpyHostToDevice));
    if (lengths_host)
        DBH_HIP(hipMemcpy(d_lengths, lengths_host, (size_t)n_reads * sizeof(int64_t), hipMemcpyHostToDevice));
    DBH_HIP(hipMemcpy(d_thresholds, thresholds_host, (size_t)n_thresholds * sizeof(double), hipMemcpyHostToDevice));
    DBH_HIP(hipMemset(d_out, 0, n_all * sizeof(int64_t)));
    int64_t* const d_early = d_out + n_out[0];
    int64_t* const d_windows = d_early + n_out[1];
    DBH_HIP(dbh_sweep::early_tally(
        d_best[0], d_margin[0], end ? d_best[1] : nullptr, end ? d_margin[1] : nullptr,
        labels_host ? d_labels : nullptr, lengths_host ? d_lengths : nullptr, n_reads, steps,
        n_classes, input_size, chunk_samples, d_thresholds, n_thresholds, P,
        (unsigned long long*)d_out, (unsigned long long*)d_early, (unsigned long long*)d_windows,
        lengths_host ? (unsigned long long*)(d_windows + n_out[2]) : nullptr, 0));
    std::vector<int64_t> got(n_all);
    DBH_HIP(hipMemcpy(got.data(), d_out, n_all * sizeof(int64_t), hipMemcpyDeviceToHost));
    int64_t* const out[4] = {calls_host, early_host, windows_host, pushes_host};
    size_t at = 0;
    for (int a = 0; a < 4; ++a)
        for (size_t i = 0; i < n_out[a]; ++i) out[a][i] += got[at++];
    return DBH_OK;
}

// ---- scan: every window of every read, and the events of the track (dbh_scan.hip) ---------------
}  // extern "C"

namespace {
bool scan_input_size_ok(int input_size) {
    return input_size % 2 == 0 && input_size >= 96 && input_size <= dbh_gen::kMaxInput;
}
}  // namespace

extern "C" {

int dbh_scan_window_count(int input_size, int64_t n_samples, int64_t* count) {
    if (!count || n_samples < 0 || !scan_input_size_ok(input_size)) return DBH_ERR_INVALID_ARGUMENT;
    *count = dbh_scan::window_count(n_samples, input_size);
    return DBH_OK;
}

int dbh_scan_window_offsets_dev(const int64_t* offsets_dev, int64_t n_reads, int input_size,
                                int64_t* window_offsets_dev, dbh_stream stream) {
    if (n_reads < 0 || !scan_input_size_ok(input_size) || !window_offsets_dev ||
        (n_reads > 0 && !offsets_dev))
        return DBH_ERR_INVALID_ARGUMENT;
    // (no read: the one entry, zero, by the same kernel)
    DBH_HIP(dbh_scan::window_offsets(offsets_dev, n_reads, input_size, window_offsets_dev,
                                     (hipStream_t)stream));
    return DBH_OK;
}

int dbh_scan_windows_dev(const int16_t* samples_dev, const int64_t* offsets_dev,
                         const int64_t* window_offsets_dev, int64_t n_reads, int input_size,
                         int side, int64_t first_window, int64_t n_windows, float* x_dev,
                         dbh_stream stream) {
    if (n_reads < 0 || first_window < 0 || n_windows < 0 || !scan_input_size_ok(input_size) ||
        (side != DBH_SIDE_START && side != DBH_SIDE_END))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0 || n_windows == 0) return DBH_OK;
    // (samples_dev may be null when every read is empty: no window then reads a sample)
    if (!offsets_dev || !window_offsets_dev || !x_dev) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(dbh_scan::windows(samples_dev, offsets_dev, window_offsets_dev, n_reads, input_size,
                              side, first_window, n_windows, x_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_scan_events_dev(const int32_t* best_dev, const double* margin_dev,
                        const int64_t* window_offsets_dev, int64_t n_reads, double threshold,
                        int min_windows, int skip_windows, dbh_scan_event* events_dev,
                        int64_t max_events, int32_t* per_read_interior_dev, int64_t* n_events_dev,
                        dbh_stream stream) {
    if (n_reads < 0 || min_windows < 1 || skip_windows < 0 || max_events < 0 || !n_events_dev ||
        !(threshold == threshold) || (max_events > 0 && !events_dev))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads > 0 && (!best_dev || !margin_dev || !window_offsets_dev))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) {
        DBH_HIP(hipMemsetAsync(n_events_dev, 0, sizeof(int64_t), (hipStream_t)stream));
        return DBH_OK;
    }
    DeviceBlock work;                       // the per-read counts and their prefix, freed on return
    DBH_HIP(work.reserve(dbh_scan::events_workspace_bytes(n_reads)));
    DBH_HIP(dbh_scan::events(best_dev, margin_dev, window_offsets_dev, n_reads, threshold,
                             min_windows, skip_windows, events_dev, max_events,
                             per_read_interior_dev, n_events_dev, work.get(), (hipStream_t)stream));
    DBH_HIP(hipStreamSynchronize((hipStream_t)stream));
    return DBH_OK;
}

int dbh_scan_i16(dbh_model* m, const int16_t* samples_host, const int64_t* offsets_host,
                 int64_t n_reads, int side, double threshold, int min_windows, int skip_windows,
                 int32_t* best_host, double* margin_host, dbh_scan_event* events_host,
                 int64_t max_events, int64_t* n_events, int64_t* n_interior) {
    if (!m || n_reads < 0 || (side != DBH_SIDE_START && side != DBH_SIDE_END) || min_windows < 1 ||
        skip_windows < 0 || max_events < 0 || !(threshold == threshold) || !n_events ||
        !n_interior || (max_events > 0 && !events_host) || !scan_input_size_ok(m->input_size))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads > 0 && !offsets_host) return DBH_ERR_INVALID_ARGUMENT;
    const int L = m->input_size, C = m->n_classes;
    int64_t total_windows = 0;
    for (int64_t i = 0; i < n_reads; ++i) {
        const int64_t n = offsets_host[i + 1] - offsets_host[i];
        if (n < 0) return DBH_ERR_INVALID_ARGUMENT;
        const int64_t w = dbh_scan::window_count(n, L);
        if (w > INT32_MAX) return DBH_ERR_INVALID_ARGUMENT;      // (an event's window is an int32)
        total_windows += w;
    }
    const int64_t total_samples = n_reads > 0 ? offsets_host[n_reads] - offsets_host[0] : 0;
    if (total_samples > 0 && !samples_host) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) {
        *n_events = *n_interior = 0;
        return DBH_OK;
    }
    DBH_HIP(hipSetDevice(m->device));      // (see dbh_classify_i16)
    // chunks of windows: 256 MiB of fp32 input at the most, and a persistent model's host group
    int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)L * (int64_t)sizeof(float)));
    if (m->kind == DBH_MODEL_KIND_PERSISTENT) chunk = std::min(chunk, std::max<int64_t>(1, m->host_group_windows));
    chunk = std::min(chunk, total_windows);
    // one block for the call, freed on return
    DeviceBlock block;
    int16_t* d_samples = nullptr;
    int64_t *d_offsets = nullptr, *d_window_offsets = nullptr, *d_n_events = nullptr;
    int32_t *d_best = nullptr, *d_interior = nullptr;
    double* d_margin = nullptr;
    float *d_x = nullptr, *d_probs = nullptr;
    dbh_scan_event* d_events = nullptr;
    char* d_work = nullptr;
    DBH_HIP(block.carve([&](dbh_host::Carve& c) {
        d_samples = c.take<int16_t>((size_t)total_samples);
        d_offsets = c.take<int64_t>((size_t)n_reads + 1);
        d_window_offsets = c.take<int64_t>((size_t)n_reads + 1);
        d_best = c.take<int32_t>((size_t)total_windows);
        d_margin = c.take<double>((size_t)total_windows);
        d_x = c.take<float>((size_t)chunk * L);
        d_probs = c.take<float>((size_t)chunk * C);
        d_events = c.take<dbh_scan_event>((size_t)max_events);
        d_interior = c.take<int32_t>((size_t)n_reads);
        d_n_events = c.take<int64_t>(1);
        d_work = c.take<char>(dbh_scan::events_workspace_bytes(n_reads));
    }));
    std::vector<int64_t> rel((size_t)n_reads + 1);
    for (int64_t i = 0; i <= n_reads; ++i) rel[(size_t)i] = offsets_host[i] - offsets_host[0];
    if (total_samples > 0)
        DBH_HIP(hipMemcpyAsync(d_samples, samples_host + offsets_host[0],
                               (size_t)total_samples * sizeof(int16_t), hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(d_offsets, rel.data(), rel.size() * sizeof(int64_t),
                           hipMemcpyHostToDevice, 0));
    DBH_HIP(dbh_scan::window_offsets(d_offsets, n_reads, L, d_window_offsets, 0));
    for (int64_t w0 = 0; w0 < total_windows; w0 += chunk) {
        const int64_t cnt = std::min(chunk, total_windows - w0);
        DBH_HIP(dbh_scan::windows(d_samples, d_offsets, d_window_offsets, n_reads, L, side, w0, cnt,
                                  d_x, 0));
        DBH_TRY(dbh_predict_dev(m, d_x, cnt, d_probs, nullptr));
        DBH_TRY(dbh_sweep_windows_dev(m, d_probs, cnt, 1, d_best + w0, d_margin + w0, nullptr));
    }
    DBH_HIP(dbh_scan::events(d_best, d_margin, d_window_offsets, n_reads, threshold, min_windows,
                             skip_windows, d_events, max_events, d_interior, d_n_events, d_work, 0));
    std::vector<int32_t> interior((size_t)n_reads);
    int64_t found = 0;
    DBH_HIP(hipMemcpyAsync(interior.data(), d_interior, interior.size() * sizeof(int32_t),
                           hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipMemcpyAsync(&found, d_n_events, sizeof(int64_t), hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipStreamSynchronize(0));
    const int64_t written = std::min(found, max_events);
    if (written > 0)
        DBH_HIP(hipMemcpy(events_host, d_events, (size_t)written * sizeof(dbh_scan_event),
                          hipMemcpyDeviceToHost));
    if (best_host)
        DBH_HIP(hipMemcpy(best_host, d_best, (size_t)total_windows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (margin_host)
        DBH_HIP(hipMemcpy(margin_host, d_margin, (size_t)total_windows * sizeof(double), hipMemcpyDeviceToHost));
    int64_t inside = 0;
    for (int32_t v : interior) inside += v;
    *n_events = found;
    *n_interior = inside;
    return DBH_OK;
}

// ---- locate: where in the signal a call comes from (dbh_locate.hip) ------------------------------
}  // extern "C"

namespace {
// the arguments dbh_locate_dev and dbh_locate_host share: a geometry the general path takes, the
// cells that geometry has, steps whose flat cell index fits an int
bool locate_shape_ok(int64_t n_reads, int steps, int cells, int n_classes, int input_size, int side) {
    if (n_reads < 0 || steps < 1 || !dbh_gen::geometry_ok(input_size, n_classes) ||
        (side != DBH_SIDE_START && side != DBH_SIDE_END))
        return false;
    int len[8];
    dbh_net::stage_lengths(input_size, len);
    return cells == len[7] && (int64_t)steps * cells <= (int64_t)1 << 24;
}

// reads per group of dbh_locate_i16: the windows of a group fit one chunk of the layer chain, so
// that evidence plus activations stay inside the general path's budget.  DEEPBINNER_LOCATE_GROUP=n:
// at most n reads (tests: groups of a few reads out of a few dozen)
int64_t locate_group_reads(const dbh_model* m, int steps) {
    int64_t reads = std::max<int64_t>(1, m->gen.chunk / steps);
    if (const char* cap = std::getenv("DEEPBINNER_LOCATE_GROUP")) {
        const long long c = std::atoll(cap);
        if (c > 0 && c < reads) reads = c;
    }
    return reads;
}

// the device workspace of one group of `reads` reads, laid out once for sizing and for use
struct LocateGroup {
    float *wprobs = nullptr, *evidence = nullptr;
    char* act = nullptr;
    void lay_out(dbh_host::Carve& c, const dbh_model* m, int64_t reads, int steps) {
        const size_t windows = (size_t)reads * steps;
        wprobs = c.take<float>(windows * m->n_classes);
        evidence = c.take<float>(windows * m->gen.len[7] * m->n_classes);
        act = c.take<char>(dbh_gen::activation_bytes(m->gen, (int64_t)windows));
    }
};
}  // namespace

extern "C" {

int dbh_evidence_floats(const dbh_model* m, int64_t* per_window) {
    if (!m || !per_window) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_GENERAL) return DBH_ERR_UNSUPPORTED;
    *per_window = (int64_t)m->gen.len[7] * m->n_classes;
    return DBH_OK;
}

int dbh_evidence_dev(dbh_model* m, const float* x_dev, int64_t n_windows, float* probs_dev,
                     float* evidence_dev, dbh_stream stream) {
    if (!m || n_windows < 0 || (n_windows > 0 && (!x_dev || !probs_dev || !evidence_dev)))
        return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_GENERAL) return DBH_ERR_UNSUPPORTED;
    return general_predict(m, x_dev, n_windows, probs_dev, (hipStream_t)stream, evidence_dev);
}

int dbh_locate_dev(const float* evidence_dev, const int32_t* calls_dev, const int64_t* offsets_dev,
                   int64_t n_reads, int steps, int cells, int n_classes, int input_size, int side,
                   dbh_location* locations_dev, dbh_stream stream) {
    if (!locate_shape_ok(n_reads, steps, cells, n_classes, input_size, side))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!evidence_dev || !calls_dev || !offsets_dev || !locations_dev) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(dbh_locate::locate(evidence_dev, calls_dev, offsets_dev, n_reads, steps, cells, n_classes,
                               input_size, side, locations_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_locate_host(const float* evidence_host, const int32_t* calls_host,
                    const int64_t* offsets_host, int64_t n_reads, int steps, int cells,
                    int n_classes, int input_size, int side, dbh_location* locations_host) {
    if (!locate_shape_ok(n_reads, steps, cells, n_classes, input_size, side))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!evidence_host || !calls_host || !offsets_host || !locations_host)
        return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_reads; ++i)
        if (offsets_host[i + 1] < offsets_host[i]) return DBH_ERR_INVALID_ARGUMENT;
    dbh_locate::locate_host(evidence_host, calls_host, offsets_host, n_reads, steps, cells, n_classes,
                            input_size, side, locations_host);
    return DBH_OK;
}

int dbh_locate_workspace_bytes(const dbh_model* m, int64_t n_reads, int scan_size, size_t* bytes) {
    if (!m || !bytes || n_reads < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_GENERAL) return DBH_ERR_UNSUPPORTED;
    const int steps = dbh_host::model_steps(m->input_size, scan_size);
    if (steps <= 0) return DBH_ERR_INVALID_ARGUMENT;
    dbh_host::Carve sizing(nullptr);
    LocateGroup().lay_out(sizing, m, std::min(n_reads, locate_group_reads(m, steps)), steps);
    *bytes = sizing.used;
    return DBH_OK;
}

int dbh_locate_i16(dbh_model* m, const int16_t* samples_host, const int64_t* offsets_host,
                   int64_t n_reads, int side, int scan_size, double score_diff, float* probs_host,
                   int32_t* calls_host, dbh_location* locations_host) {
    if (!m || n_reads < 0 || (side != DBH_SIDE_START && side != DBH_SIDE_END))
        return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_GENERAL) return DBH_ERR_UNSUPPORTED;
    const int steps = dbh_host::model_steps(m->input_size, scan_size);
    if (steps <= 0 || !(score_diff == score_diff)) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!offsets_host || !probs_host || !calls_host || !locations_host)
        return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_reads; ++i)
        if (offsets_host[i + 1] < offsets_host[i]) return DBH_ERR_INVALID_ARGUMENT;
    const int64_t total_samples = offsets_host[n_reads] - offsets_host[0];
    if (total_samples > 0 && !samples_host) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipSetDevice(m->device));      // (see dbh_classify_i16)
    const int C = m->n_classes, cells = m->gen.len[7];
    const int64_t group = std::min(n_reads, locate_group_reads(m, steps));
    // one block for the call, freed on return: the reads, the results of every read, then one
    // group's workspace.  The groups follow each other on one stream, which is what lets them share
    // that workspace; nothing is waited for until the results are copied back.
    DeviceBlock block;
    int16_t* d_samples = nullptr;
    int64_t* d_offsets = nullptr;
    float* d_probs = nullptr;
    int32_t* d_calls = nullptr;
    dbh_location* d_locations = nullptr;
    LocateGroup g;
    DBH_HIP(block.carve([&](dbh_host::Carve& c) {
        d_samples = c.take<int16_t>((size_t)std::max<int64_t>(total_samples, 1));
        d_offsets = c.take<int64_t>((size_t)n_reads + 1);
        d_probs = c.take<float>((size_t)n_reads * C);
        d_calls = c.take<int32_t>((size_t)n_reads);
        d_locations = c.take<dbh_location>((size_t)n_reads);
        g.lay_out(c, m, group, steps);
    }));
    std::vector<int64_t> rel((size_t)n_reads + 1);
    for (int64_t i = 0; i <= n_reads; ++i) rel[(size_t)i] = offsets_host[i] - offsets_host[0];
    if (total_samples > 0)
        DBH_HIP(hipMemcpyAsync(d_samples, samples_host + offsets_host[0],
                               (size_t)total_samples * sizeof(int16_t), hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(d_offsets, rel.data(), rel.size() * sizeof(int64_t),
                           hipMemcpyHostToDevice, 0));
    for (int64_t r0 = 0; r0 < n_reads; r0 += group) {
        const int64_t cnt = std::min(group, n_reads - r0);
        // slice + forward with evidence, merge and call, then the rule: a read's results come from
        // its own windows alone, so the grouping does not show in them
        DBH_HIP(dbh_gen::forward(m->gen, nullptr, d_samples, d_offsets + r0, steps, side, cnt * steps,
                                 g.wprobs, g.evidence, g.act, 0));
        DBH_HIP(dbh_gen::merge(g.wprobs, cnt, steps, C, score_diff, d_probs + r0 * C, d_calls + r0,
                               0));
        DBH_HIP(dbh_locate::locate(g.evidence, d_calls + r0, d_offsets + r0, cnt, steps, cells, C,
                                   m->input_size, side, d_locations + r0, 0));
    }
    DBH_HIP(hipMemcpyAsync(probs_host, d_probs, (size_t)n_reads * C * sizeof(float),
                           hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipMemcpyAsync(calls_host, d_calls, (size_t)n_reads * sizeof(int32_t),
                           hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipMemcpyAsync(locations_host, d_locations, (size_t)n_reads * sizeof(dbh_location),
                           hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipStreamSynchronize(0));
    return DBH_OK;
}

// ---- occlude: blank the located span and call the read again (dbh_occlude.hip) -------------------
}  // extern "C"

namespace {
// the arguments the plan and window entries share
bool occlude_shape_ok(int64_t n_reads, int steps, int input_size, int side) {
    return n_reads >= 0 && steps >= 1 && scan_input_size_ok(input_size) &&
           (int64_t)steps * input_size <= (int64_t)1 << 30 &&
           (side == DBH_SIDE_START || side == DBH_SIDE_END);
}

bool offsets_run_forwards(const int64_t* offsets, int64_t n_reads) {
    for (int64_t i = 0; i < n_reads; ++i)
        if (offsets[i + 1] < offsets[i]) return false;
    return true;
}

// what a group of dbh_locate_occluded_i16 holds beside locate's: its windows as sliced, the three
// variants' windows, their merged probabilities and calls, the plans.  The four passes go through
// LocateGroup's workspace one after another.
struct OccludeGroup {
    float *x = nullptr, *variants[3] = {nullptr, nullptr, nullptr}, *vprobs = nullptr;
    int32_t* vcalls = nullptr;
    dbh_occlude_plan* plans = nullptr;
    void lay_out(dbh_host::Carve& c, const dbh_model* m, int64_t reads, int steps) {
        const size_t floats = (size_t)reads * steps * m->input_size;
        x = c.take<float>(floats);
        for (float*& v : variants) v = c.take<float>(floats);
        vprobs = c.take<float>((size_t)3 * reads * m->n_classes);
        vcalls = c.take<int32_t>((size_t)3 * reads);
        plans = c.take<dbh_occlude_plan>((size_t)reads);
    }
};
}  // namespace

extern "C" {

int dbh_occlude_plan_dev(const dbh_location* locations_dev, const int64_t* offsets_dev,
                         int64_t n_reads, int steps, int input_size, int side,
                         dbh_occlude_plan* plans_dev, dbh_occlusion* occlusions_dev,
                         dbh_stream stream) {
    if (!occlude_shape_ok(n_reads, steps, input_size, side)) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!locations_dev || !offsets_dev || !plans_dev || !occlusions_dev)
        return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(dbh_occlude::plan(locations_dev, offsets_dev, n_reads, steps, input_size, side,
                              plans_dev, occlusions_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_occlude_plan_host(const dbh_location* locations_host, const int64_t* offsets_host,
                          int64_t n_reads, int steps, int input_size, int side,
                          dbh_occlude_plan* plans_host, dbh_occlusion* occlusions_host) {
    if (!occlude_shape_ok(n_reads, steps, input_size, side)) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!locations_host || !offsets_host || !plans_host || !occlusions_host ||
        !offsets_run_forwards(offsets_host, n_reads))
        return DBH_ERR_INVALID_ARGUMENT;
    dbh_occlude::plan_host(locations_host, offsets_host, n_reads, steps, input_size, side,
                           plans_host, occlusions_host);
    return DBH_OK;
}

int dbh_occlude_windows_dev(const float* x_dev, const int64_t* offsets_dev,
                            const dbh_occlude_plan* plans_dev, int64_t n_reads, int steps,
                            int input_size, int side, float* variants_dev, dbh_stream stream) {
    if (!occlude_shape_ok(n_reads, steps, input_size, side)) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!x_dev || !offsets_dev || !plans_dev || !variants_dev) return DBH_ERR_INVALID_ARGUMENT;
    const size_t floats = (size_t)n_reads * steps * input_size;
    float* const out[3] = {variants_dev, variants_dev + floats, variants_dev + 2 * floats};
    DBH_HIP(dbh_occlude::windows(x_dev, offsets_dev, plans_dev, n_reads, steps, input_size, side,
                                 out, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_occlude_windows_host(const float* x_host, const int64_t* offsets_host,
                             const dbh_occlude_plan* plans_host, int64_t n_reads, int steps,
                             int input_size, int side, float* variants_host) {
    if (!occlude_shape_ok(n_reads, steps, input_size, side)) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!x_host || !offsets_host || !plans_host || !variants_host ||
        !offsets_run_forwards(offsets_host, n_reads))
        return DBH_ERR_INVALID_ARGUMENT;
    const size_t floats = (size_t)n_reads * steps * input_size;
    float* const out[3] = {variants_host, variants_host + floats, variants_host + 2 * floats};
    dbh_occlude::windows_host(x_host, offsets_host, plans_host, n_reads, steps, input_size, side,
                              out);
    return DBH_OK;
}

int dbh_locate_occluded_workspace_bytes(const dbh_model* m, int64_t n_reads, int scan_size,
                                        size_t* bytes) {
    if (!m || !bytes || n_reads < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_GENERAL) return DBH_ERR_UNSUPPORTED;
    const int steps = dbh_host::model_steps(m->input_size, scan_size);
    if (steps <= 0 || !occlude_shape_ok(n_reads, steps, m->input_size, DBH_SIDE_START))
        return DBH_ERR_INVALID_ARGUMENT;
    const int64_t group = std::min(n_reads, locate_group_reads(m, steps));
    dbh_host::Carve sizing(nullptr);
    LocateGroup().lay_out(sizing, m, group, steps);
    OccludeGroup().lay_out(sizing, m, group, steps);
    *bytes = sizing.used;
    return DBH_OK;
}

int dbh_locate_occluded_i16(dbh_model* m, const int16_t* samples_host, const int64_t* offsets_host,
                            int64_t n_reads, int side, int scan_size, double score_diff,
                            float* probs_host, int32_t* calls_host, dbh_location* locations_host,
                            dbh_occlusion* occlusions_host) {
    if (!m || n_reads < 0 || (side != DBH_SIDE_START && side != DBH_SIDE_END))
        return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_GENERAL) return DBH_ERR_UNSUPPORTED;
    const int steps = dbh_host::model_steps(m->input_size, scan_size);
    if (steps <= 0 || !(score_diff == score_diff) ||
        !occlude_shape_ok(n_reads, steps, m->input_size, side))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!offsets_host || !probs_host || !calls_host || !locations_host || !occlusions_host ||
        !offsets_run_forwards(offsets_host, n_reads))
        return DBH_ERR_INVALID_ARGUMENT;
    const int64_t total_samples = offsets_host[n_reads] - offsets_host[0];
    if (total_samples > 0 && !samples_host) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipSetDevice(m->device));      // (see dbh_classify_i16)
    const int C = m->n_classes, cells = m->gen.len[7], L = m->input_size;
    const int64_t group = std::min(n_reads, locate_group_reads(m, steps));
    // dbh_locate_i16's block and stream order, with the occlusions beside the other results and the
    // group's windows beside its workspace
    DeviceBlock block;
    int16_t* d_samples = nullptr;
    int64_t* d_offsets = nullptr;
    float* d_probs = nullptr;
    int32_t* d_calls = nullptr;
    dbh_location* d_locations = nullptr;
    dbh_occlusion* d_occlusions = nullptr;
    LocateGroup g;
    OccludeGroup o;
    DBH_HIP(block.carve([&](dbh_host::Carve& c) {
        d_samples = c.take<int16_t>((size_t)std::max<int64_t>(total_samples, 1));
        d_offsets = c.take<int64_t>((size_t)n_reads + 1);
        d_probs = c.take<float>((size_t)n_reads * C);
        d_calls = c.take<int32_t>((size_t)n_reads);
        d_locations = c.take<dbh_location>((size_t)n_reads);
        d_occlusions = c.take<dbh_occlusion>((size_t)n_reads);
        g.lay_out(c, m, group, steps);
        o.lay_out(c, m, group, steps);
    }));
    std::vector<int64_t> rel((size_t)n_reads + 1);
    for (int64_t i = 0; i <= n_reads; ++i) rel[(size_t)i] = offsets_host[i] - offsets_host[0];
    if (total_samples > 0)
        DBH_HIP(hipMemcpyAsync(d_samples, samples_host + offsets_host[0],
                               (size_t)total_samples * sizeof(int16_t), hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(d_offsets, rel.data(), rel.size() * sizeof(int64_t),
                           hipMemcpyHostToDevice, 0));
    for (int64_t r0 = 0; r0 < n_reads; r0 += group) {
        const int64_t cnt = std::min(group, n_reads - r0);
        // the group's windows, sliced and normalised once; the unblanked pass on them (the front
        // takes a window given as fp32 as the value it would have sliced), merge, call and locate
        DBH_HIP(dbh_occlude::slice(d_samples, d_offsets + r0, cnt, steps, L, side, o.x, 0));
        DBH_HIP(dbh_gen::forward(m->gen, o.x, nullptr, nullptr, steps, side, cnt * steps, g.wprobs,
                                 g.evidence, g.act, 0));
        DBH_HIP(dbh_gen::merge(g.wprobs, cnt, steps, C, score_diff, d_probs + r0 * C, d_calls + r0,
                               0));
        DBH_HIP(dbh_locate::locate(g.evidence, d_calls + r0, d_offsets + r0, cnt, steps, cells, C,
                                   L, side, d_locations + r0, 0));
        // the plan, the three variants' windows, and one pass each through the same workspace
        DBH_HIP(dbh_occlude::plan(d_locations + r0, d_offsets + r0, cnt, steps, L, side, o.plans,
                                  d_occlusions + r0, 0));
        DBH_HIP(dbh_occlude::windows(o.x, d_offsets + r0, o.plans, cnt, steps, L, side, o.variants,
                                     0));
        for (int v = 0; v < 3; ++v) {
            DBH_HIP(dbh_gen::forward(m->gen, o.variants[v], nullptr, nullptr, steps, side,
                                     cnt * steps, g.wprobs, nullptr, g.act, 0));
            DBH_HIP(dbh_gen::merge(g.wprobs, cnt, steps, C, score_diff,
                                   o.vprobs + (size_t)v * group * C, o.vcalls + (size_t)v * group,
                                   0));
        }
        DBH_HIP(dbh_occlude::gather(o.plans, d_probs + r0 * C, o.vprobs, o.vcalls, cnt, group, C,
                                    d_occlusions + r0, 0));
    }
    DBH_HIP(hipMemcpyAsync(probs_host, d_probs, (size_t)n_reads * C * sizeof(float),
                           hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipMemcpyAsync(calls_host, d_calls, (size_t)n_reads * sizeof(int32_t),
                           hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipMemcpyAsync(locations_host, d_locations, (size_t)n_reads * sizeof(dbh_location),
                           hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipMemcpyAsync(occlusions_host, d_occlusions, (size_t)n_reads * sizeof(dbh_occlusion),
                           hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipStreamSynchronize(0));
    return DBH_OK;
}

// ---- live: each read's barcode called while its signal arrives (dbh_live.hip) --------------------
}  // extern "C"

// A session: the channels' state on the device, and on the host a mirror of every channel's record
// and gate.  The mirror runs dbh_live_core.h's append over the arguments of a push - the lines the
// append kernel runs over the device's copy - so the host knows how many windows the push makes
// ready without reading the device back, and a push needs no synchronise between its kernels.  What
// only the device can know (a decision, and with it the stop under STOP_ON_DECISION) comes back in
// the results at the push's one synchronise and is put into the mirror there.  Destroy a session
// before its model.
struct dbh_live_session {
    dbh_model* model = nullptr;
    int n_channels = 0;
    dbh_live::Shape shape{};
    int64_t round_windows = 0;
    dbh_owned::Stream stream;
    DeviceBlock state_block, push_block, in_block;
    PinnedBlock h_in, h_out;
    dbh_live::State st{};
    dbh_live::Chunk* d_chunks = nullptr;
    int32_t *d_first = nullptr, *d_count = nullptr;
    int64_t* d_win_offsets = nullptr;
    float *d_x = nullptr, *d_probs = nullptr;
    dbh_live_result* d_results = nullptr;
    dbh_live_end_result* d_end_results = nullptr;
    std::vector<dbh_live_result> rec;          // the mirror
    std::vector<dbh_live::Gate> gate;
    std::vector<int64_t> seen;                 // the push that last named the channel
    int64_t pushes = 0;
    // a pair session (dbh_live_create_pair; pair.ring null: start only): the end model, the rings
    // and the end fold's state, its forward rounds, and per channel whether the end track stands
    dbh_model* end_model = nullptr;
    dbh_live::Pair pair{};
    int64_t end_round_windows = 0;
    std::vector<char> end_done;
    // a yield policy (dbh_live_set_policy; pol.weight null: none): on the device the weights, the
    // two yields, every channel's action and a push's action records
    DeviceBlock policy_block;
    dbh_live::PolicyArgs pol{};
};

namespace {
bool live_fold_general(const dbh_model* m) { return m->kind == DBH_MODEL_KIND_GENERAL; }

// a forward round: what the caller said, else 64 MiB of fp32 input; never more than all windows
int64_t live_round_windows(int64_t all, int L, int64_t max_round_windows) {
    const int64_t by_default = std::max<int64_t>(1, ((int64_t)64 << 20) / ((int64_t)L * 4));
    return std::min(all, max_round_windows > 0 ? max_round_windows : by_default);
}

// dbh_live_create (end null) and dbh_live_create_pair
int live_create(dbh_model* m, dbh_model* end, int n_channels, int scan_size, double score_diff,
                int min_windows, uint32_t flags, int combine_mode, int64_t max_round_windows,
                dbh_live_session** session) {
    const dbh_live::Shape shape =
        dbh_live::shape_of(m->input_size, scan_size, score_diff, min_windows, flags);
    if (!dbh_live::shape_ok(shape, scan_size)) return DBH_ERR_INVALID_ARGUMENT;
    dbh_live::Shape end_shape{};
    if (end) {
        end_shape = dbh_live::shape_of(end->input_size, scan_size, score_diff, 1, 0);
        if (!dbh_live::shape_ok(end_shape, scan_size)) return DBH_ERR_INVALID_ARGUMENT;
    }
    DBH_HIP(hipSetDevice(m->device));
    std::unique_ptr<dbh_live_session> s(new (std::nothrow) dbh_live_session);
    if (!s) return DBH_ERR_OUT_OF_MEMORY;
    s->model = m;
    s->end_model = end;
    s->n_channels = n_channels;
    s->shape = shape;
    const int L = shape.L, C = m->n_classes, steps = shape.steps;
    s->round_windows = live_round_windows((int64_t)n_channels * steps, L, max_round_windows);
    const int Le = end_shape.L, steps_e = end_shape.steps;
    if (end)
        s->end_round_windows =
            live_round_windows((int64_t)n_channels * steps_e, Le, max_round_windows);
    DBH_HIP(hipStreamCreateWithFlags(&s->stream.h, hipStreamNonBlocking));
    const size_t n = (size_t)n_channels;
    s->st.stride = (shape.cap + 7) & ~(long long)7;
    s->st.n_classes = C;
    dbh_live::Pair& pair = s->pair;
    pair.shape = end_shape;
    pair.stride = (end_shape.cap + 7) & ~(long long)7;
    pair.combine_mode = combine_mode;
    pair.end.n_classes = C;
    DBH_HIP(s->state_block.carve([&](dbh_host::Carve& c) {
        s->st.samples = c.take<int16_t>(n * (size_t)s->st.stride);
        s->st.rec = c.take<dbh_live_result>(n);
        s->st.gate = c.take<dbh_live::Gate>(n);
        s->st.merged = c.take<float>(n * C);
        s->st.best = c.take<int32_t>(n * steps);
        s->st.margin = c.take<double>(n * steps);
        if (end) {
            pair.ring = c.take<int16_t>(n * (size_t)pair.stride);
            pair.end.rec = c.take<dbh_live_result>(n);
            pair.end.merged = c.take<float>(n * C);
            pair.end.best = c.take<int32_t>(n * steps_e);
            pair.end.margin = c.take<double>(n * steps_e);
        }
    }));
    // one x and one probs serve both sides' rounds, which run one after the other
    const size_t x_floats = std::max((size_t)s->round_windows * L, (size_t)s->end_round_windows * Le);
    const size_t p_floats = (size_t)std::max(s->round_windows, s->end_round_windows) * C;
    DBH_HIP(s->push_block.carve([&](dbh_host::Carve& c) {
        s->d_first = c.take<int32_t>(n);
        s->d_count = c.take<int32_t>(n);
        s->d_win_offsets = c.take<int64_t>(n + 1);
        s->d_results = c.take<dbh_live_result>(n);
        if (end) s->d_end_results = c.take<dbh_live_end_result>(n);
        s->d_x = c.take<float>(x_floats);
        s->d_probs = c.take<float>(p_floats);
    }));
    DBH_HIP(s->h_out.reserve(n * (sizeof(dbh_live_result) + sizeof(dbh_live_end_result))));
    s->rec.assign(n, dbh_live::fresh_record());
    s->gate.assign(n, dbh_live::Gate{0, 0});
    s->seen.assign(n, -1);
    s->end_done.assign(n, 0);
    DBH_HIP(hipMemcpyAsync(s->st.rec, s->rec.data(), n * sizeof(dbh_live_result),
                           hipMemcpyHostToDevice, s->stream));
    DBH_HIP(hipMemsetAsync(s->st.gate, 0, n * sizeof(dbh_live::Gate), s->stream));
    if (end)
        DBH_HIP(hipMemcpyAsync(pair.end.rec, s->rec.data(), n * sizeof(dbh_live_result),
                               hipMemcpyHostToDevice, s->stream));
    DBH_HIP(hipStreamSynchronize(s->stream));
    *session = s.release();
    return DBH_OK;
}

int live_push(dbh_live_session* s, const int32_t* channels, const int64_t* offsets,
              const int16_t* samples, const uint32_t* flags, dbh_live_result* results,
              dbh_live_end_result* end_results, dbh_live_action* actions, int64_t n_chunks);
}  // namespace

extern "C" {

int dbh_live_create(dbh_model* m, int n_channels, int scan_size, double score_diff,
                    int min_windows, uint32_t flags, int64_t max_round_windows,
                    dbh_live_session** session) {
    if (!m || !session || n_channels < 1 || n_channels > DBH_LIVE_MAX_CHANNELS ||
        max_round_windows < 0)
        return DBH_ERR_INVALID_ARGUMENT;
    return live_create(m, nullptr, n_channels, scan_size, score_diff, min_windows, flags,
                       DBH_REQUIRE_EITHER, max_round_windows, session);
}

int dbh_live_create_pair(dbh_model* start_model, dbh_model* end_model, int n_channels,
                         int scan_size, double score_diff, int min_windows, uint32_t flags,
                         int combine_mode, int64_t max_round_windows,
                         dbh_live_session** session) {
    if (!start_model || !end_model || !session || n_channels < 1 ||
        n_channels > DBH_LIVE_MAX_CHANNELS || max_round_windows < 0 ||
        combine_mode < DBH_REQUIRE_EITHER || combine_mode > DBH_REQUIRE_BOTH)
        return DBH_ERR_INVALID_ARGUMENT;
    if (start_model->device != end_model->device || start_model->n_classes != end_model->n_classes)
        return DBH_ERR_INVALID_ARGUMENT;
    return live_create(start_model, end_model, n_channels, scan_size, score_diff, min_windows,
                       flags, combine_mode, max_round_windows, session);
}

int dbh_live_destroy(dbh_live_session* s) {
    delete s;      // (stream, device state and pinned memory are members that free themselves)
    return DBH_OK;
}

int dbh_live_push(dbh_live_session* s, const int32_t* channels, const int64_t* offsets,
                  const int16_t* samples, const uint32_t* flags, dbh_live_result* results,
                  int64_t n_chunks) {
    return live_push(s, channels, offsets, samples, flags, results, nullptr, nullptr, n_chunks);
}

int dbh_live_push_pair(dbh_live_session* s, const int32_t* channels, const int64_t* offsets,
                       const int16_t* samples, const uint32_t* flags, dbh_live_result* results,
                       dbh_live_end_result* end_results, int64_t n_chunks) {
    if (s && end_results && !s->pair.ring) return DBH_ERR_INVALID_ARGUMENT;
    return live_push(s, channels, offsets, samples, flags, results, end_results, nullptr, n_chunks);
}

int dbh_live_set_policy(dbh_live_session* s, const int32_t* weights, int n_classes,
                        int64_t slack_samples, int undecided_action) {
    if (!s || s->pol.weight || s->pushes != 0 || !weights || n_classes != s->model->n_classes ||
        !dbh_live::policy_ok(weights, n_classes, slack_samples, undecided_action))
        return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipSetDevice(s->model->device));
    const size_t n = (size_t)s->n_channels, C = (size_t)n_classes;
    dbh_live::PolicyArgs pol{};
    int32_t* d_weight = nullptr;
    DBH_HIP(s->policy_block.carve([&](dbh_host::Carve& c) {
        d_weight = c.take<int32_t>(C);
        pol.yield_samples = c.take<long long>(C);
        pol.yield_reads = c.take<long long>(C);
        pol.channel_action = c.take<int32_t>(n);
        pol.actions = c.take<dbh_live_action>(n);
    }));
    DBH_HIP(s->h_out.reserve(n * (sizeof(dbh_live_result) + sizeof(dbh_live_end_result) +
                                  sizeof(dbh_live_action))));
    DBH_HIP(hipMemsetAsync(s->policy_block.get(), 0, s->policy_block.bytes, s->stream));
    DBH_HIP(hipMemcpyAsync(d_weight, weights, C * sizeof(int32_t), hipMemcpyHostToDevice,
                           s->stream));
    DBH_HIP(hipStreamSynchronize(s->stream));
    pol.weight = d_weight;
    pol.n_classes = n_classes;
    pol.slack = slack_samples;
    pol.undecided = undecided_action;
    s->pol = pol;
    return DBH_OK;
}

int dbh_live_push_policy(dbh_live_session* s, const int32_t* channels, const int64_t* offsets,
                         const int16_t* samples, const uint32_t* flags, dbh_live_result* results,
                         dbh_live_end_result* end_results, dbh_live_action* actions,
                         int64_t n_chunks) {
    if (!s || !s->pol.weight || (end_results && !s->pair.ring) || (n_chunks > 0 && !actions))
        return DBH_ERR_INVALID_ARGUMENT;
    return live_push(s, channels, offsets, samples, flags, results, end_results, actions, n_chunks);
}

int dbh_live_yield(dbh_live_session* s, int64_t* samples_host, int64_t* reads_host) {
    if (!s || !s->pol.weight) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipSetDevice(s->model->device));
    const size_t bytes = (size_t)s->pol.n_classes * sizeof(int64_t);
    if (samples_host)
        DBH_HIP(hipMemcpyAsync(samples_host, s->pol.yield_samples, bytes, hipMemcpyDeviceToHost,
                               s->stream));
    if (reads_host)
        DBH_HIP(hipMemcpyAsync(reads_host, s->pol.yield_reads, bytes, hipMemcpyDeviceToHost,
                               s->stream));
    DBH_HIP(hipStreamSynchronize(s->stream));
    return DBH_OK;
}

int dbh_live_set_yield(dbh_live_session* s, const int64_t* samples_host,
                       const int64_t* reads_host) {
    if (!s || !s->pol.weight || !samples_host || !reads_host) return DBH_ERR_INVALID_ARGUMENT;
    for (int c = 0; c < s->pol.n_classes; ++c)
        if (samples_host[c] < 0 || reads_host[c] < 0) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipSetDevice(s->model->device));
    const size_t bytes = (size_t)s->pol.n_classes * sizeof(int64_t);
    DBH_HIP(hipMemcpyAsync(s->pol.yield_samples, samples_host, bytes, hipMemcpyHostToDevice,
                           s->stream));
    DBH_HIP(hipMemcpyAsync(s->pol.yield_reads, reads_host, bytes, hipMemcpyHostToDevice,
                           s->stream));
    DBH_HIP(hipStreamSynchronize(s->stream));
    return DBH_OK;
}

}  // extern "C"

namespace {
int live_push(dbh_live_session* s, const int32_t* channels, const int64_t* offsets,
              const int16_t* samples, const uint32_t* flags, dbh_live_result* results,
              dbh_live_end_result* end_results, dbh_live_action* actions, int64_t n_chunks) {
    if (!s || n_chunks < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_chunks == 0) return DBH_OK;
    if (!channels || !offsets || !samples || !flags || !results || n_chunks > s->n_channels)
        return DBH_ERR_INVALID_ARGUMENT;
    const int64_t push = s->pushes + 1;        // (`seen` is scratch: a refused push leaves no state)
    for (int64_t i = 0; i < n_chunks; ++i) {
        const int32_t ch = channels[i];
        if (ch < 0 || ch >= s->n_channels || s->seen[(size_t)ch] == push ||
            offsets[i + 1] < offsets[i] || (flags[i] & ~(uint32_t)(DBH_LIVE_BEGIN | DBH_LIVE_END))) {
            for (int64_t j = 0; j < i; ++j) s->seen[(size_t)channels[j]] = -1;
            return DBH_ERR_INVALID_ARGUMENT;
        }
        s->seen[(size_t)ch] = push;
    }
    s->pushes = push;
    const dbh_live::Shape& shape = s->shape;
    const dbh_live::Pair& pair = s->pair;
    const bool is_pair = pair.ring != nullptr;
    DBH_HIP(hipSetDevice(s->model->device));
    // the plan: the mirror's copy of every chunk's channel through append, the kept samples placed
    // so that source and row are aligned alike (16-byte copies in the append kernel).  A pair
    // session's chunk is staged whole where the start side's samples and the ring's tail touch
    // (a chunk no longer than cap_e); else the tail is a piece of its own, aligned like its place
    // in the ring.
    const size_t n = (size_t)n_chunks;
    std::vector<dbh_live_result> rec(n);
    std::vector<dbh_live::Gate> gate(n);
    std::vector<dbh_live::Append> plan(n);
    std::vector<dbh_live::Chunk> chunks(n);
    std::vector<dbh_live::Tail> tails(is_pair ? n : 0);
    std::vector<int64_t> end_offsets(is_pair ? n + 1 : 0);
    int64_t staged = 0, total_windows = 0, end_windows = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t ch = (size_t)channels[i];
        rec[i] = s->rec[ch];
        gate[i] = s->gate[ch];
        const int64_t length = offsets[i + 1] - offsets[i];
        plan[i] = dbh_live::append(&rec[i], &gate[i], flags[i], length, shape);
        const int64_t at = staged + ((plan[i].at - staged) & 7);       // at % 8 == plan.at % 8
        chunks[i] = dbh_live::Chunk{at, length, at, channels[i], flags[i]};
        staged = at + plan[i].keep;
        total_windows += plan[i].count;
        if (!is_pair) continue;
        end_offsets[i] = end_windows;
        dbh_live::Tail& tail = tails[i];
        tail = dbh_live::Tail{0, 0, 0, 0};
        if (plan[i].idle) continue;
        tail = dbh_live::tail_store(rec[i].samples - length, length, pair.shape);
        if (plan[i].keep > 0 && tail.from <= plan[i].keep) {           // one piece: the whole chunk
            chunks[i].tail = at + tail.from;
            staged = at + length;
        } else {                                                       // tail % 8 == tail.at % 8
            chunks[i].tail = staged + ((tail.at - staged) & 7);
            staged = chunks[i].tail + tail.keep;
        }
        if (flags[i] & DBH_LIVE_END) end_windows += pair.shape.steps;
    }
    if (is_pair) end_offsets[n] = end_windows;
    const size_t table_bytes = align256(n * sizeof(dbh_live::Chunk));
    const size_t ends_bytes = is_pair ? align256((n + 1) * sizeof(int64_t)) : 0;
    const size_t in_bytes =
        table_bytes + ends_bytes + align256((size_t)staged * sizeof(int16_t) + 16);
    DBH_HIP(s->h_in.reserve(in_bytes));
    DBH_HIP(s->in_block.reserve(in_bytes));
    std::memcpy(s->h_in.get(), chunks.data(), n * sizeof(dbh_live::Chunk));
    if (is_pair)
        std::memcpy(s->h_in.as<char>(table_bytes), end_offsets.data(), (n + 1) * sizeof(int64_t));
    int16_t* h_samples = s->h_in.as<int16_t>(table_bytes + ends_bytes);
    for (size_t i = 0; i < n; ++i) {
        const bool whole = is_pair && tails[i].keep > 0 && plan[i].keep > 0 &&
                           tails[i].from <= plan[i].keep;
        const int64_t head = whole ? offsets[i + 1] - offsets[i] : plan[i].keep;
        if (head > 0)
            std::memcpy(h_samples + chunks[i].src, samples + offsets[i],
                        (size_t)head * sizeof(int16_t));
        if (is_pair && !whole && tails[i].keep > 0)
            std::memcpy(h_samples + chunks[i].tail, samples + offsets[i] + tails[i].from,
                        (size_t)tails[i].keep * sizeof(int16_t));
    }
    hipStream_t stream = s->stream;
    DBH_HIP(hipMemcpyAsync(s->in_block.get(), s->h_in.get(), in_bytes, hipMemcpyHostToDevice,
                           stream));
    const dbh_live::Chunk* d_chunks = s->in_block.as<dbh_live::Chunk>();
    const int64_t* d_end_offsets = s->in_block.as<int64_t>(table_bytes);
    const int16_t* d_in = s->in_block.as<int16_t>(table_bytes + ends_bytes);
    DBH_HIP(dbh_live::append(s->st, shape, pair, d_chunks, d_in, (int)n_chunks, s->d_first,
                             s->d_count, stream));
    DBH_HIP(dbh_live::window_list(s->d_count, (int)n_chunks, s->d_win_offsets, stream));
    for (int64_t w0 = 0; w0 < total_windows; w0 += s->round_windows) {
        const int64_t cnt = std::min(s->round_windows, total_windows - w0);
        DBH_HIP(dbh_live::front(s->st, shape, d_chunks, s->d_first, s->d_win_offsets, (int)n_chunks,
                                w0, cnt, s->d_x, stream));
        DBH_TRY(dbh_predict_dev(s->model, s->d_x, cnt, s->d_probs, (dbh_stream)stream));
        DBH_HIP(dbh_live::fold(live_fold_general(s->model), s->st, shape, d_chunks,
                               s->d_win_offsets, n_chunks, w0, cnt, s->d_probs, stream));
    }
    // the end side of the reads that ended with this push: behind the start side's folds, so that
    // the end record combines with the start record as it stands at END
    for (int64_t w0 = 0; w0 < end_windows; w0 += s->end_round_windows) {
        const int64_t cnt = std::min(s->end_round_windows, end_windows - w0);
        DBH_HIP(dbh_live::end_front(s->st, pair, d_chunks, d_end_offsets, (int)n_chunks, w0, cnt,
                                    s->d_x, stream));
        DBH_TRY(dbh_predict_dev(s->end_model, s->d_x, cnt, s->d_probs, (dbh_stream)stream));
        DBH_HIP(dbh_live::fold(live_fold_general(s->end_model), pair.end, pair.shape, d_chunks,
                               d_end_offsets, n_chunks, w0, cnt, s->d_probs, stream));
    }
    dbh_live_end_result* d_ends = end_results ? s->d_end_results : nullptr;
    DBH_HIP(dbh_live::results(s->st, pair, d_chunks, s->d_first, (int)n_chunks, s->d_results, d_ends,
                              stream));
    DBH_HIP(hipMemcpyAsync(s->h_out.get(), s->d_results, n * sizeof(dbh_live_result),
                           hipMemcpyDeviceToHost, stream));
    dbh_live_end_result* h_ends = s->h_out.as<dbh_live_end_result>(n * sizeof(dbh_live_result));
    if (d_ends)
        DBH_HIP(hipMemcpyAsync(h_ends, d_ends, n * sizeof(dbh_live_end_result),
                               hipMemcpyDeviceToHost, stream));
    // a yield policy: the push's ENDs into the yields, then every chunk's action (two launches)
    dbh_live_action* h_actions = s->h_out.as<dbh_live_action>(
        n * (sizeof(dbh_live_result) + sizeof(dbh_live_end_result)));
    if (s->pol.weight) {
        dbh_live::PolicyArgs pol = s->pol;
        pol.records = s->d_results;
        pol.chunks = d_chunks;
        pol.n_chunks = n_chunks;
        DBH_HIP(dbh_live::policy(pol, stream));
        if (actions)
            DBH_HIP(hipMemcpyAsync(h_actions, pol.actions, n * sizeof(dbh_live_action),
                                   hipMemcpyDeviceToHost, stream));
    }
    DBH_HIP(hipStreamSynchronize(stream));
    std::memcpy(results, s->h_out.get(), n * sizeof(dbh_live_result));
    if (d_ends) std::memcpy(end_results, h_ends, n * sizeof(dbh_live_end_result));
    if (actions) std::memcpy(actions, h_actions, n * sizeof(dbh_live_action));
    for (size_t i = 0; i < n; ++i) {
        if (plan[i].idle) continue;
        s->rec[(size_t)channels[i]] = results[i];       // (the decision is the device's to make)
        s->gate[(size_t)channels[i]] = gate[i];
        s->end_done[(size_t)channels[i]] = is_pair && (flags[i] & DBH_LIVE_END) != 0;
    }
    return DBH_OK;
}
}  // namespace

extern "C" {

int dbh_live_track(dbh_live_session* s, int channel, int32_t* best, double* margin,
                   int32_t* windows) {
    if (!s || !best || !margin || !windows || channel < 0 || channel >= s->n_channels)
        return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipSetDevice(s->model->device));
    const int steps = s->shape.steps;
    DBH_HIP(hipMemcpyAsync(best, s->st.best + (size_t)channel * steps, (size_t)steps * sizeof(int32_t),
                           hipMemcpyDeviceToHost, s->stream));
    DBH_HIP(hipMemcpyAsync(margin, s->st.margin + (size_t)channel * steps,
                           (size_t)steps * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DBH_HIP(hipStreamSynchronize(s->stream));
    *windows = s->rec[(size_t)channel].windows;
    return DBH_OK;
}

int dbh_live_end_track(dbh_live_session* s, int channel, int32_t* best, double* margin,
                       int32_t* windows) {
    if (!s || !s->pair.ring || !best || !margin || !windows || channel < 0 ||
        channel >= s->n_channels)
        return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipSetDevice(s->model->device));
    const int steps = s->pair.shape.steps;
    DBH_HIP(hipMemcpyAsync(best, s->pair.end.best + (size_t)channel * steps,
                           (size_t)steps * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    DBH_HIP(hipMemcpyAsync(margin, s->pair.end.margin + (size_t)channel * steps,
                           (size_t)steps * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DBH_HIP(hipStreamSynchronize(s->stream));
    *windows = s->end_done[(size_t)channel] ? steps : 0;
    return DBH_OK;
}

int dbh_live_fold_dev(const dbh_model* m, const float* window_probs_dev,
                      const int64_t* window_offsets_dev, int64_t n_channels, int64_t n_windows,
                      int steps, double score_diff, int min_windows, uint32_t flags,
                      float* merged_dev, dbh_live_result* state_dev, int32_t* best_dev,
                      double* margin_dev, dbh_stream stream) {
    if (!m || n_channels < 0 || n_windows < 0 || steps < 1) return DBH_ERR_INVALID_ARGUMENT;
    const int half = m->input_size / 2;
    if ((int64_t)steps * half > INT32_MAX) return DBH_ERR_INVALID_ARGUMENT;
    const dbh_live::Shape shape =
        dbh_live::shape_of(m->input_size, steps * half, score_diff, min_windows, flags);
    if (!dbh_live::shape_ok(shape, steps * half)) return DBH_ERR_INVALID_ARGUMENT;
    if (n_channels == 0) return DBH_OK;
    if (!window_offsets_dev || !merged_dev || !state_dev || !best_dev || !margin_dev ||
        (n_windows > 0 && !window_probs_dev))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_windows == 0) return DBH_OK;
    dbh_live::State st{};
    st.rec = state_dev;
    st.merged = merged_dev;
    st.best = best_dev;
    st.margin = margin_dev;
    st.n_classes = m->n_classes;
    DBH_HIP(dbh_live::fold(live_fold_general(m), st, shape, nullptr, window_offsets_dev, n_channels,
                           0, n_windows, window_probs_dev, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_live_plan_host(int input_size, int scan_size, double score_diff, int min_windows,
                       uint32_t flags, const int64_t* lengths, const uint32_t* chunk_flags,
                       int64_t n_chunks, const int32_t* track_best, const double* track_margin,
                       dbh_live_result* results_host, int32_t* new_windows_host) {
    if (n_chunks < 0) return DBH_ERR_INVALID_ARGUMENT;
    const dbh_live::Shape shape =
        dbh_live::shape_of(input_size, scan_size, score_diff, min_windows, flags);
    if (!dbh_live::shape_ok(shape, scan_size)) return DBH_ERR_INVALID_ARGUMENT;
    if (n_chunks == 0) return DBH_OK;
    if (!lengths || !chunk_flags || !track_best || !track_margin || !results_host)
        return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_chunks; ++i)
        if (lengths[i] < 0 || (chunk_flags[i] & ~(uint32_t)(DBH_LIVE_BEGIN | DBH_LIVE_END)))
            return DBH_ERR_INVALID_ARGUMENT;
    dbh_live::plan_channel(shape, (const long long*)lengths, (const unsigned*)chunk_flags,
                           (long long)n_chunks, (const int*)track_best, track_margin, results_host,
                           (int*)new_windows_host);
    return DBH_OK;
}

int dbh_live_tail_plan_host(int end_input_size, int scan_size, const int64_t* lengths,
                            const uint32_t* chunk_flags, int64_t n_chunks, int64_t* store_host,
                            int64_t* samples_host, int32_t* ends_host, int64_t* windows_host) {
    if (n_chunks < 0) return DBH_ERR_INVALID_ARGUMENT;
    const dbh_live::Shape shape = dbh_live::shape_of(end_input_size, scan_size, 0.5, 1, 0);
    if (!dbh_live::shape_ok(shape, scan_size)) return DBH_ERR_INVALID_ARGUMENT;
    if (n_chunks == 0) return DBH_OK;
    if (!lengths || !chunk_flags || !store_host || !samples_host || !ends_host || !windows_host)
        return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_chunks; ++i)
        if (lengths[i] < 0 || (chunk_flags[i] & ~(uint32_t)(DBH_LIVE_BEGIN | DBH_LIVE_END)))
            return DBH_ERR_INVALID_ARGUMENT;
    dbh_live::plan_tail(shape, (const long long*)lengths, (const unsigned*)chunk_flags,
                        (long long)n_chunks, (long long*)store_host, (long long*)samples_host,
                        (int*)ends_host, (long long*)windows_host);
    return DBH_OK;
}

int dbh_live_policy_dev(const dbh_live_result* records_dev, const uint32_t* chunk_flags_dev,
                        const int32_t* channels_dev, int64_t n_chunks, const int32_t* weights_dev,
                        int n_classes, int64_t slack_samples, int undecided_action,
                        int64_t* yield_samples_dev, int64_t* yield_reads_dev,
                        int32_t* channel_action_dev, dbh_live_action* actions_dev,
                        dbh_stream stream) {
    if (n_chunks < 0 || n_chunks > DBH_LIVE_MAX_CHANNELS || n_classes < 1 ||
        n_classes > dbh_live::kMaxClasses || slack_samples < 0 ||
        (undecided_action != DBH_LIVE_ACTION_KEEP && undecided_action != DBH_LIVE_ACTION_EJECT))
        return DBH_ERR_INVALID_ARGUMENT;
    if (!weights_dev || !yield_samples_dev || !yield_reads_dev) return DBH_ERR_INVALID_ARGUMENT;
    if (n_chunks == 0) return DBH_OK;
    if (!records_dev || !chunk_flags_dev || !channels_dev || !channel_action_dev || !actions_dev)
        return DBH_ERR_INVALID_ARGUMENT;
    dbh_live::PolicyArgs pol{};
    pol.records = records_dev;
    pol.chunk_flags = chunk_flags_dev;
    pol.channels = channels_dev;
    pol.n_chunks = n_chunks;
    pol.weight = weights_dev;
    pol.n_classes = n_classes;
    pol.slack = slack_samples;
    pol.undecided = undecided_action;
    pol.yield_samples = (long long*)yield_samples_dev;
    pol.yield_reads = (long long*)yield_reads_dev;
    pol.channel_action = channel_action_dev;
    pol.actions = actions_dev;
    DBH_HIP(dbh_live::policy(pol, (hipStream_t)stream));
    return DBH_OK;
}

int dbh_live_policy_plan_host(const int32_t* weights, int n_classes, int64_t slack_samples,
                              int undecided_action, const int64_t* push_offsets, int64_t n_pushes,
                              const int32_t* channels_host, const uint32_t* chunk_flags_host,
                              const dbh_live_result* records_host, int n_channels,
                              int32_t* channel_action_host, int64_t* yield_samples_host,
                              int64_t* yield_reads_host, dbh_live_action* actions_host,
                              int64_t* yield_trace_host) {
    if (n_pushes < 0 || n_channels < 1 || n_channels > DBH_LIVE_MAX_CHANNELS ||
        n_classes > dbh_live::kMaxClasses ||
        !dbh_live::policy_ok(weights, n_classes, slack_samples, undecided_action))
        return DBH_ERR_INVALID_ARGUMENT;
    if (!channel_action_host || !yield_samples_host || !yield_reads_host)
        return DBH_ERR_INVALID_ARGUMENT;
    for (int c = 0; c < n_classes; ++c)
        if (yield_samples_host[c] < 0 || yield_reads_host[c] < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_pushes == 0) return DBH_OK;
    if (!push_offsets || push_offsets[0] != 0) return DBH_ERR_INVALID_ARGUMENT;
    for (int64_t p = 0; p < n_pushes; ++p)
        if (push_offsets[p + 1] < push_offsets[p] ||
            push_offsets[p + 1] - push_offsets[p] > n_channels)
            return DBH_ERR_INVALID_ARGUMENT;
    const int64_t total = push_offsets[n_pushes];
    if (total > 0 && (!channels_host || !chunk_flags_host || !records_host || !actions_host))
        return DBH_ERR_INVALID_ARGUMENT;
    std::vector<int64_t> seen((size_t)n_channels, -1);          // the push that last named the channel
    for (int64_t p = 0; p < n_pushes; ++p)
        for (int64_t i = push_offsets[p]; i < push_offsets[p + 1]; ++i) {
            const int32_t ch = channels_host[i];
            if (ch < 0 || ch >= n_channels || seen[(size_t)ch] == p ||
                (chunk_flags_host[i] & ~(uint32_t)(DBH_LIVE_BEGIN | DBH_LIVE_END)))
                return DBH_ERR_INVALID_ARGUMENT;
            seen[(size_t)ch] = p;
        }
    for (int64_t p = 0; p < n_pushes; ++p) {
        const int64_t at = push_offsets[p];
        dbh_live::plan_policy_push(weights, n_classes, slack_samples, undecided_action,
                                   channels_host + at, chunk_flags_host + at, records_host + at,
                                   push_offsets[p + 1] - at, channel_action_host,
                                   yield_samples_host, yield_reads_host, actions_host + at);
        if (!yield_trace_host) continue;
        int64_t* trace = yield_trace_host + (size_t)p * 2 * n_classes;
        std::memcpy(trace, yield_samples_host, (size_t)n_classes * sizeof(int64_t));
        std::memcpy(trace + n_classes, yield_reads_host, (size_t)n_classes * sizeof(int64_t));
    }
    return DBH_OK;
}

namespace {
// THE FORWARD STREAM of a device: every queue's forward launches (and the small kernels between
// them) go through this one stream, in the order the queues arrive, so that at most one forward
// kernel is on the GPU at a time.  The forward kernel is persistent - one workgroup per CU for as
// long as the launch lasts: with every queue launching on its own stream two or three of them
// share the CUs, each stretched, the small kernels behind them (merge, combine, the next
// container's fill) wait for whichever ends last, and the queues fall into step: all inflating,
// then all classifying (profiles/r05_k2/steady_state_trace_share0.txt: 16 of every 68 ms with no
// forward kernel on the GPU).  One at a time on 256 - n CUs (dbh_model_reserve_cus), the inflate
// kernels of the containers behind keep the other n CUs busy all the time.
// DEEPBINNER_FORWARD_STREAM=own: every queue on its own stream again (A/B).
// (the streams live as long as the process - the queues of any model may use them - and are left to
// the runtime's teardown on purpose; a device ordinal of kMaxDevices or more keeps every queue on
// its own stream, which is correct, only slower)
constexpr int kMaxDevices = 64;
std::mutex g_forward_mutex[kMaxDevices];
hipStream_t g_forward_stream[kMaxDevices] = {};
bool shared_forward_stream() {
    const char* v = std::getenv("DEEPBINNER_FORWARD_STREAM");
    return !(v && std::strcmp(v, "own") == 0);
}

// One queue's turn on its device's forward stream.  From acquire() to release() the queue holds the
// device's lock; what it launches on `stream` runs behind everything the queue's own stream holds
// so far, and the queue's own stream goes on behind it.  NOTHING ALLOCATES OR FREES WHILE THE LOCK
// IS HELD (but for the forward stream itself, once per device): hipMalloc / hipFree synchronise the
// device, and under the lock that would stall every other queue's launch.  With
// every queue on its own stream (DEEPBINNER_FORWARD_STREAM=own, or a device beyond kMaxDevices)
// both do nothing and `stream` stays the queue's own.
struct ForwardTurn {
    DeflatedQueue& d;
    const int device;
    const bool shared = shared_forward_stream() && device >= 0 && device < kMaxDevices;
    hipStream_t stream = d.stream;       // where the turn's launches go
    std::unique_lock<std::mutex> lock;
    int acquire(dbh_model* const models[2]) {
        if (!shared) return DBH_OK;
        // before the lock: the hand-over's events, and the forward kernel's scratch at the size the
        // launches ask for (its counter zeroed on the queue's stream, which the forward stream awaits)
        hipError_t e = hipSuccess;
        for (dbh_owned::Event* ev : {&d.inflated, &d.classified})
            if (e == hipSuccess && !ev->h) e = hipEventCreateWithFlags(&ev->h, hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(e, "hipEventCreateWithFlags");
        int cus = 0;
        for (int j = 0; j < 2; ++j)
            if (models[j]) cus = std::max(cus, models[j]->cus);
        DBH_HIP(d.tail.reserve(cus, d.stream));
        lock = std::unique_lock<std::mutex>(g_forward_mutex[device]);
        hipStream_t& fs = g_forward_stream[device];
        if (!fs) {
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            e = hipStreamCreateWithPriority(&fs, hipStreamNonBlocking, greatest);
            if (e != hipSuccess) return hip_fail(e, "hipStreamCreateWithPriority");
        }
        stream = fs;
        e = hipEventRecord(d.inflated, d.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, d.inflated, 0);
        return e == hipSuccess ? DBH_OK : hip_fail(e, "handing over to the forward stream");
    }
    // (whatever was launched must be waited for, also behind an error)
    int release() {
        if (!shared) return DBH_OK;
        hipError_t e = hipEventRecord(d.classified, stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(d.stream, d.classified, 0);
        lock.unlock();
        if (e == hipSuccess) return DBH_OK;
        (void)hipStreamSynchronize(stream);      // (with the lock released: the other queues launch on)
        return hip_fail(e, "taking over from the forward stream");
    }
};
}  // namespace

int dbh_classify_pair_deflated(dbh_model* start_model, dbh_model* end_model,
                               const uint8_t* comp_host, int64_t comp_bytes,
                               const dbh_inflate_stream* streams_host, int64_t n_streams,
                               const int64_t* offsets_host, int64_t n_reads, int scan_size,
                               double score_diff, int combine_mode, int32_t* calls_host,
                               int32_t* stream_status_host, int16_t* samples_host,
                               double* stage_ms) {
    return dbh_classify_pair_deflated_verbose(start_model, end_model, comp_host, comp_bytes,
                                              streams_host, n_streams, offsets_host, n_reads,
                                              scan_size, score_diff, combine_mode, calls_host,
                                              stream_status_host, samples_host, stage_ms, nullptr,
                                              nullptr, nullptr, nullptr);
}

int dbh_classify_pair_deflated_verbose(dbh_model* start_model, dbh_model* end_model,
                                       const uint8_t* comp_host, int64_t comp_bytes,
                                       const dbh_inflate_stream* streams_host, int64_t n_streams,
                                       const int64_t* offsets_host, int64_t n_reads, int scan_size,
                                       double score_diff, int combine_mode, int32_t* calls_host,
                                       int32_t* stream_status_host, int16_t* samples_host,
                                       double* stage_ms, int32_t* start_calls_host,
                                       int32_t* end_calls_host, float* start_probs_host,
                                       float* end_probs_host) {
    // ---- validate ----
    dbh_model* const models[2] = {start_model, end_model};
    dbh_model* m = start_model ? start_model : end_model;
    if (!m || n_reads < 0 || n_streams < 0 || comp_bytes < 0 ||
        combine_mode < DBH_REQUIRE_EITHER || combine_mode > DBH_REQUIRE_BOTH)
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!offsets_host || !calls_host || (n_streams > 0 && (!streams_host || !comp_host)) ||
        check_pair(models, scan_size) != DBH_OK)
        return DBH_ERR_INVALID_ARGUMENT;
    const bool both = start_model && end_model;
    const int64_t total_samples = offsets_host[n_reads] - offsets_host[0];
    if (offsets_host[0] != 0 || total_samples < 0) return DBH_ERR_INVALID_ARGUMENT;
    const int64_t out_bytes = total_samples * 2;
    for (int64_t i = 0; i < n_streams; ++i) {
        const dbh_inflate_stream& r = streams_host[i];
        if (r.comp_offset < 0 || r.comp_bytes < 0 || r.out_offset < 0 || r.out_bytes < 0 ||
            (r.out_offset & 1) || r.comp_offset + r.comp_bytes > comp_bytes ||
            r.out_offset + r.out_bytes > out_bytes)
            return DBH_ERR_INVALID_ARGUMENT;
    }
    // ---- layout ----
    DBH_HIP(hipSetDevice(m->device));
    DeflatedQueue& d = m->deflated;
    if (!d.stream) DBH_HIP(hipStreamCreateWithFlags(&d.stream.h, hipStreamNonBlocking));
    const dbh_host::DeflatedSmall small(n_streams, n_reads);
    const size_t probs_bytes = (size_t)n_reads * m->n_classes * sizeof(float);
    const size_t calls_bytes = (size_t)n_reads * sizeof(int32_t);
    const size_t work = pair_workspace_bytes(models, n_reads, scan_size);
    size_t token_bytes = 0;
    DBH_TRY(dbh_inflate_workspace_bytes(out_bytes, n_streams, &token_bytes));
    DBH_HIP(d.h_small.reserve(small.total));
    DBH_HIP(d.d_small.reserve(small.total));
    DBH_HIP(d.d_comp.reserve((size_t)comp_bytes + 64));
    DBH_HIP(d.d_samples.reserve((size_t)out_bytes + 256));
    DBH_HIP(d.d_tokens.reserve(token_bytes));
    DBH_HIP(d.d_out.reserve(2 * probs_bytes + 256));
    if (work) DBH_HIP(d.d_work.reserve(work));
    dbh_owned::Event ev[4];
    if (stage_ms)
        for (dbh_owned::Event& e : ev) DBH_HIP(hipEventCreate(&e.h));
    auto done = [&](int status) -> int {
        (void)hipStreamSynchronize(d.stream);
        return status;
    };
    // ---- stage and upload ----
    // the records go over in record_order, the status comes back in it and is put back below
    char* h = d.h_small.as<char>();
    dbh_host::record_order(streams_host, n_streams, d.order);
    for (int64_t i = 0; i < n_streams; ++i)
        ((dbh_inflate_stream*)(h + small.records))[i] = streams_host[d.order[(size_t)i]];
    std::memcpy(h + small.offsets, offsets_host, (size_t)(n_reads + 1) * sizeof(int64_t));
    if (ev[0]) (void)hipEventRecord(ev[0], d.stream);
    hipError_t e = hipMemcpyAsync(d.d_small.get(), h, small.in_bytes, hipMemcpyHostToDevice, d.stream);
    if (e == hipSuccess && comp_bytes > 0) {
        const void* src = comp_host;
        // the decoder fetches up to 64 bytes beyond the last stream: the loader's buffers carry
        // them; a pageable buffer is staged (and padded) first
        if (!is_pinned(comp_host, (size_t)comp_bytes + 64)) {
            e = d.h_comp.reserve((size_t)comp_bytes + 64);
            if (e != hipSuccess) return done(hip_fail(e, "growing the staging buffer"));
            staged_copy(d.h_comp.get(), comp_host, (size_t)comp_bytes);
            std::memset(d.h_comp.as<char>((size_t)comp_bytes), 0, 64);
            src = d.h_comp.get();
        }
        e = hipMemcpyAsync(d.d_comp.get(), src, (size_t)comp_bytes + 64, hipMemcpyHostToDevice, d.stream);
    }
    if (e != hipSuccess) return done(hip_fail(e, "hipMemcpyAsync H2D"));
    if (ev[1]) (void)hipEventRecord(ev[1], d.stream);
    // ---- decode ----
    // a read without a piece (nothing stored, or nothing readable) must still be zeros
    if (out_bytes > 0) {
        e = hipMemsetAsync(d.d_samples.get(), 0, (size_t)out_bytes, d.stream);
        if (e != hipSuccess) return done(hip_fail(e, "hipMemsetAsync"));
    }
    if (n_streams > 0) {
        const int st = dbh_inflate_dev(d.d_comp.as<uint8_t>(), (int64_t)comp_bytes,
                                       d.d_small.as<dbh_inflate_stream>(small.records), n_streams,
                                       out_bytes, d.d_samples.as<uint8_t>(), d.d_tokens.get(),
                                       d.d_small.as<int32_t>(small.status), 0, (dbh_stream)d.stream);
        if (st != DBH_OK) return done(st);
    }
    if (ev[2]) (void)hipEventRecord(ev[2], d.stream);
    // ---- classify: both models' launches and combine_calls, as one block on the forward stream ----
    {
        const int sides[2] = {DBH_SIDE_START, DBH_SIDE_END};
        float* const d_probs[2] = {d.d_out.as<float>(), d.d_out.as<float>(probs_bytes)};
        int32_t* const d_side[2] = {d.d_small.as<int32_t>(small.side_calls[0]),
                                    d.d_small.as<int32_t>(small.side_calls[1])};
        ForwardTurn turn{d, m->device};
        int st = turn.acquire(models);
        if (st != DBH_OK) return done(st);
        st = classify_pair_dev(models, sides, d.d_samples.as<int16_t>(),
                               d.d_small.as<int64_t>(small.offsets), n_reads, scan_size, score_diff,
                               d_probs, d_side, combine_mode, d.d_small.as<int32_t>(small.final_calls),
                               d.d_work.get(), turn.stream, ReadHints(), &d.tail);
        const int back = turn.release();
        if (back != DBH_OK) return done(back);
        if (st != DBH_OK) return done(st);
    }
    if (ev[3]) (void)hipEventRecord(ev[3], d.stream);
    // ---- download ----
    e = hipMemcpyAsync(h + small.in_bytes, d.d_small.as<char>(small.in_bytes), small.out_bytes,
                       hipMemcpyDeviceToHost, d.stream);
    if (e == hipSuccess && samples_host && out_bytes > 0)
        e = hipMemcpyAsync(samples_host, d.d_samples.get(), (size_t)out_bytes, hipMemcpyDeviceToHost,
                           d.stream);
    // what --verbose prints beside the final call (classify.py:157-171): the sides' probabilities
    float* const side_probs_host[2] = {start_probs_host, end_probs_host};
    for (int j = 0; j < 2; ++j)
        if (e == hipSuccess && side_probs_host[j] && models[j])
            e = hipMemcpyAsync(side_probs_host[j], d.d_out.as<char>((size_t)j * probs_bytes),
                               probs_bytes, hipMemcpyDeviceToHost, d.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    if (e != hipSuccess) return done(hip_fail(e, "dbh_classify_pair_deflated"));
    // ---- scatter: the final calls (one model alone: its own), the sides' own, the status ----
    std::memcpy(calls_host, h + (both ? small.final_calls : small.side_calls[start_model ? 0 : 1]),
                calls_bytes);
    int32_t* const side_calls_host[2] = {start_calls_host, end_calls_host};
    for (int j = 0; j < 2; ++j)
        if (side_calls_host[j] && models[j])
            std::memcpy(side_calls_host[j], h + small.side_calls[j], calls_bytes);
    if (stream_status_host)
        for (int64_t i = 0; i < n_streams; ++i)
            stream_status_host[d.order[(size_t)i]] = ((const int32_t*)(h + small.status))[i];
    if (stage_ms) {
        float ms = 0.f;
        for (int k = 0; k < 3; ++k)
            stage_ms[k] = hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess ? ms : -1.0;
    }
    return done(DBH_OK);
}

void* dbh_host_alloc(size_t bytes, void* user) {
    (void)user;
    void* p = nullptr;
    // portable: the loader's threads allocate with no device of their own chosen, and with
    // several GPUs any of them may be the one that reads the batch
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void dbh_host_release(void* ptr, void* user) {
    (void)user;
    if (ptr) (void)hipHostFree(ptr);
}

int dbh_host_is_pinned(const void* ptr, size_t bytes, int* pinned) {
    if (!pinned) return DBH_ERR_INVALID_ARGUMENT;
    *pinned = is_pinned(ptr, bytes) ? 1 : 0;
    return DBH_OK;
}

int dbh_model_set_host_group(dbh_model* m, int64_t windows_per_group) {
    if (!m || windows_per_group < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_OK;       // (nothing to tune)
    m->host_group_windows = windows_per_group > 0 ? windows_per_group : dbh_model::kDefaultGroup;
    return DBH_OK;
}

int dbh_model_reserve_cus(dbh_model* m, int n_cus) {
    if (!m || n_cus < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_OK;       // (nothing to tune)
    m->cus = m->cus_total - n_cus > 1 ? m->cus_total - n_cus : 1;
    return DBH_OK;
}

int dbh_stage_floats(int stage, int64_t* floats_per_window) {
    if (!floats_per_window || stage < 0 || stage > 7) return DBH_ERR_INVALID_ARGUMENT;
    *floats_per_window = dbh::kStageFloats[stage];
    return DBH_OK;
}

int dbh_debug_forward(dbh_model* m, const float* x_host, int64_t n, int stage, float* out_host) {
    if (!m || n <= 0 || !x_host || !out_host || stage < 0 || stage > 7)
        return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    const size_t per = (size_t)dbh::kStageFloats[stage];
    DBH_HIP(m->in.reserve((size_t)n * dbh::kWindow * sizeof(float)));
    DBH_HIP(m->work.reserve((size_t)n * per * sizeof(float)));
    DBH_HIP(hipMemcpyAsync(m->in.get(), x_host, (size_t)n * dbh::kWindow * sizeof(float),
                           hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemsetAsync(m->work.get(), 0, (size_t)n * per * sizeof(float), 0));
    DBH_TRY(launch_forward(m, m->in.as<float>(), n, nullptr, stage, m->work.as<float>(), 0));
    DBH_HIP(hipMemcpyAsync(out_host, m->work.get(), (size_t)n * per * sizeof(float),
                           hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipStreamSynchronize(0));
    return DBH_OK;
}

int dbh_forward_kernel_info(int* threads_per_block, int* lds_bytes, int* vgprs) {
    hipFuncAttributes attr;
    DBH_HIP(dbh_kernels::forward_attributes(&attr));
    if (threads_per_block) *threads_per_block = dbh::kThreads;
    if (lds_bytes) *lds_bytes = (int)attr.sharedSizeBytes;
    if (vgprs) *vgprs = attr.numRegs;
    return DBH_OK;
}

int dbh_forward_executed_mfmas(int n_classes, int64_t* mfmas_per_window,
                                int64_t* flop_per_window) {
    if (n_classes < 2 || n_classes > dbh::kMaxClasses) return DBH_ERR_INVALID_ARGUMENT;
    const int64_t n = dbh::forward_mfmas(n_classes);
    if (mfmas_per_window) *mfmas_per_window = n;
    if (flop_per_window) *flop_per_window = n * 2048;      // 16 x 16 x 4 multiply-adds
    return DBH_OK;
}

int dbh_forward_truncated_dev(dbh_model* m, const float* x_dev, int64_t n, int last_stage,
                              dbh_stream stream) {
    if (!m || n <= 0 || !x_dev || last_stage < 0 || last_stage > 6) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    return launch_forward(m, x_dev, n, nullptr, 100 + last_stage, nullptr, (hipStream_t)stream);
}

}  // extern "C"

#include "dbh_probes.h"
