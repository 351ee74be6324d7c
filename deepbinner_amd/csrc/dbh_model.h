// dbh_model.h — what more than one host unit of libdeepbinner_hip.so (dbh_api.hip with dbh_probes.h,
// dbh_api_sweep / _scan / _locate / _live.hip) needs: dbh_model with the types it is made of, the
// read-length hints, DBH_TRY, the core unit's helpers the routes call (defined in dbh_api.hip unless
// said otherwise) and one resident read batch.  Host code only; none of it a symbol of the library.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <map>
#include <utility>
#include <vector>

#include "../../include/deepbinner_hip.h"
#include "dbh_general.h"
#include "dbh_host_layout.h"
#include "dbh_layout.h"
#include "dbh_owned.h"
#include "dbh_status.h"

#define DBH_TRY(call) \
    do { const int st_ = (call); if (st_ != DBH_OK) return st_; } while (0)

namespace dbh_api __attribute__((visibility("hidden"))) {

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

// "every read is len_hint samples long": offsets[0] belongs to read number read0 of the sample
// buffer, which holds at least hint_cap samples (see dbh_model_set_read_length_hint)
struct ReadHints { int64_t read0 = 0, len_hint = 0, hint_cap = 0; };

// the general path's workspace (its share of dbh_classify_workspace_bytes and of
// dbh_sweep_workspace_bytes): per-window probabilities, then the activations of one chunk
size_t general_workspace(const dbh_model* m, int64_t n_reads, int steps);

// The window pass of either model kind: the probabilities of every window of n_reads reads,
// [n_reads * steps, C], to the front of the workspace.  A general model runs layer by layer with its
// activations behind them; a persistent model's forward kernel slices and normalises its own windows
// and, given no calls pointer, leaves per-window probabilities at one scan step too.  (score_diff
// only travels with the launch: nothing is called here.)
int window_probs_dev(dbh_model* m, const int16_t* samples_dev, const int64_t* offsets_dev,
                     int64_t n_reads, int steps, int side, double score_diff, const ReadHints& hints,
                     TailScratch* tail, void* workspace_dev, hipStream_t stream);

// dbh_predict(_dev) and dbh_evidence_dev on a general model: activations in a per-stream buffer of
// the model (evidence_dev null: the probabilities alone)
int general_predict(dbh_model* m, const float* x_dev, int64_t n, float* probs_dev,
                    hipStream_t stream, float* evidence_dev = nullptr);

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
                const int64_t* offsets_host, int64_t n_reads);

// the input sizes the scan's front and the occlusion's windows take (dbh_api_scan.hip)
bool scan_input_size_ok(int input_size);

// One workspace serves both models of a pair (either may be null), whose kernels follow each other
// on one stream: the larger of what `sizing` (dbh_classify_workspace_bytes, dbh_sweep_workspace_bytes)
// asks for each.  A model `sizing` refuses counts nothing: the callers have checked the pair.
inline size_t pair_workspace_bytes(int (*sizing)(const dbh_model*, int64_t, int, size_t*),
                                   dbh_model* const models[2], int64_t n_reads, int scan_size) {
    size_t bytes = 0, mine = 0;
    for (int j = 0; j < 2; ++j)
        if (models[j] && sizing(models[j], n_reads, scan_size, &mine) == DBH_OK)
            bytes = std::max(bytes, mine);
    return bytes;
}

// One resident read batch: the reads of a host-pointer route (scan, locate, locate --occlude) in ONE
// device block that lives as long as the object - the samples, the offsets made relative to
// offsets_host[0], behind them what the route's lay_out carves.  admit() refuses what no route takes,
// before any device work; upload() sends the samples, then the offsets, on the null stream.
struct ResidentReads {
    DeviceBlock block;
    std::vector<int64_t> rel;             // the offsets from 0, kept until the route has synchronised
    const int16_t* first = nullptr;       // the first read's first sample on the host
    int64_t total_samples = 0;
    int16_t* samples = nullptr;           // on the device
    int64_t* offsets = nullptr;           // ... n_reads + 1 of them: rel

    // for n_reads > 0: no offsets table, offsets that run backwards, samples missing -> refused
    int admit(const int16_t* samples_host, const int64_t* offsets_host, int64_t n_reads) {
        if (!offsets_host || !dbh_host::offsets_run_forwards(offsets_host, n_reads, &total_samples) ||
            (total_samples > 0 && !samples_host))
            return DBH_ERR_INVALID_ARGUMENT;
        rel.resize((size_t)n_reads + 1);
        for (int64_t i = 0; i <= n_reads; ++i) rel[(size_t)i] = offsets_host[i] - offsets_host[0];
        first = total_samples > 0 ? samples_host + offsets_host[0] : nullptr;
        return DBH_OK;
    }
    // lay_out(Carve&): the route's own regions, behind the samples and the offsets
    template <class LayOut>
    int upload(LayOut&& lay_out) {
        DBH_HIP(block.carve([&](dbh_host::Carve& c) {
            samples = c.take<int16_t>((size_t)std::max<int64_t>(total_samples, 1));
            offsets = c.take<int64_t>(rel.size());
            lay_out(c);
        }));
        if (first)
            DBH_HIP(hipMemcpyAsync(samples, first, (size_t)total_samples * sizeof(int16_t),
                                   hipMemcpyHostToDevice, 0));
        DBH_HIP(hipMemcpyAsync(offsets, rel.data(), rel.size() * sizeof(int64_t),
                               hipMemcpyHostToDevice, 0));
        return DBH_OK;
    }
};

}  // namespace dbh_api

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
    dbh_api::DeviceBlock packed;
    dbh_api::DeviceBlock in, work, out;   // workspace of the host-pointer entry points, grown on demand
    // per stream the callers of the *_dev entry points bring (the null stream among them): the
    // forward kernel's scratch, and the general path's activations for dbh_predict(_dev)
    std::map<hipStream_t, dbh_api::TailScratch> tails;
    std::map<hipStream_t, dbh_api::DeviceBlock> gen_scratch;
    dbh_api::DeviceBlock clock;                            // dbh_forward_clock_enable
    bool clock_probe = false;  unsigned clock_grid = 0;
    bool phase_probe = false;      // dbh_forward_phases_enable
    dbh_api::TimingBrackets timing;
    // staging slots of the host-buffer entry points (host_groups: overlapped H2D / kernels / D2H)
    static constexpr int kSlots = 3;
    static constexpr int64_t kDefaultGroup = 32768;
    int64_t host_group_windows = kDefaultGroup;     // dbh_model_set_host_group
    bool host_zero_copy = true;      // DEEPBINNER_HOST_ZERO_COPY=0: copy host samples to HBM first
    dbh_api::HostSlot slot[kSlots];
    // buffers of dbh_classify_pair_deflated (the start model's, or the only model's, are used)
    dbh_api::DeflatedQueue deflated;
    int64_t hint_len = 0, hint_cap = 0;   // dbh_model_set_read_length_hint
    ~dbh_model() { dbh_gen::destroy(&gen); }
};
