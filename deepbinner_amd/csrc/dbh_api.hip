// dbh_api.hip — the core host unit of libdeepbinner_hip.so: the C ABI of include/deepbinner_hip.h but
// for the routes with a unit of their own (dbh_api_sweep / _scan / _locate / _live.hip, which see this
// one through dbh_model.h).  Here: the error state and the runtime's wrappers, the model object,
// predict and the seam entries, launch_forward and the window pass, classify (device, batched, the
// host-buffer pipeline), the deflated path with THE FORWARD STREAM, host memory and introspection -
// everything the benchmark runs.  Uploads the weights dbh_pack.h packs into the kernel's fragment
// order, owns the device buffers and prepares the launches.  Host code only: the forward kernel and
// the seam kernels are built, and launched, in dbh_kernels.hip behind dbh_kernels.h.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>

#include "dbh_kernels.h"
#include "dbh_model.h"
#include "dbh_pack.h"
#include "dbh_probes.h"

namespace {
thread_local std::string g_last_error;
}  // namespace

// (every unit that reports through dbh_last_error() comes here: dbh_status.h)
int dbh_hip::hip_fail(hipError_t e, const char* what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? DBH_ERR_OUT_OF_MEMORY : DBH_ERR_HIP;
}

namespace {

using namespace dbh_api;
using dbh_hip::hip_fail;
using dbh_host::align256;
using dbh_host::staged_copy;

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

// the general path's workspace: per-window probabilities, then, at general_act_offset, the
// activations of one chunk.  Sizing and window_probs_dev place them by the one function.
size_t general_act_offset(const dbh_model* m, int64_t windows) {
    return align256((size_t)windows * m->n_classes * sizeof(float));
}

}  // namespace

size_t dbh_api::general_workspace(const dbh_model* m, int64_t n_reads, int steps) {
    const int64_t windows = n_reads * steps;
    return general_act_offset(m, windows) + dbh_gen::activation_bytes(m->gen, windows);
}

int dbh_api::window_probs_dev(dbh_model* m, const int16_t* samples_dev, const int64_t* offsets_dev,
                              int64_t n_reads, int steps, int side, double score_diff,
                              const ReadHints& hints, TailScratch* tail, void* workspace_dev,
                              hipStream_t stream) {
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

int dbh_api::general_predict(dbh_model* m, const float* x_dev, int64_t n, float* probs_dev,
                             hipStream_t stream, float* evidence_dev) {
    if (n == 0) return DBH_OK;
    DeviceBlock& act = m->gen_scratch[stream];
    DBH_HIP(act.reserve(dbh_gen::activation_bytes(m->gen, n)));
    DBH_HIP(dbh_gen::forward(m->gen, x_dev, nullptr, nullptr, 1, 0, n, probs_dev, evidence_dev,
                             act.get(), stream));
    return DBH_OK;
}

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

}  // namespace

// the host-buffer pipeline (described at its declaration: dbh_model.h)
int dbh_api::host_groups(dbh_model* m, const GroupJob& job, const int16_t* samples_host,
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

namespace {

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
    groups.work_bytes = [&](int64_t cnt) {
        return pair_workspace_bytes(dbh_classify_workspace_bytes, job.model, cnt, scan_size);
    };
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
    const size_t work =
        pair_workspace_bytes(dbh_classify_workspace_bytes, models, n_reads, scan_size);
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
