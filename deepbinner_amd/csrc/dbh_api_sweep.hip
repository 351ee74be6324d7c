// dbh_api_sweep.hip — the sweep's host unit of libdeepbinner_hip.so: every scan size and threshold
// from one window pass (dbh_sweep_*), the tally and the early tally.  Host code only: the kernels are
// dbh_sweep.hip's (dbh_sweep.h), the early rule dbh_early_core.h's, the window pass and the
// host-buffer pipeline the core unit's (dbh_api.hip, through dbh_model.h).
#include <hip/hip_runtime.h>

#include <cstring>

#include "dbh_early_core.h"
#include "dbh_model.h"
#include "dbh_sweep.h"

namespace {

using namespace dbh_api;

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

// the early tally: the arguments of its three entries (device or host pointers alike) -> P, or 0
// if refused
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

// What both host tallies take to the device, in one block on the calling thread's device, freed
// with the object: each present side's tracks (per_side of best and of margin), the labels and the
// lengths if given, the thresholds, and n_out zeroed int64 to count into.  Absent: a null pointer.
struct TallyInputs {
    DeviceBlock block;
    int32_t *best[2] = {nullptr, nullptr}, *labels = nullptr;
    double *margin[2] = {nullptr, nullptr}, *thresholds = nullptr;
    int64_t *lengths = nullptr, *out = nullptr;
    int upload(const int32_t* const h_best[2], const double* const h_margin[2],
               const int32_t* labels_host, const int64_t* lengths_host, int64_t n_reads,
               size_t per_side, const double* thresholds_host, int n_thresholds, size_t n_out) {
        const size_t n = (size_t)n_reads;
        DBH_HIP(block.carve([&](dbh_host::Carve& c) {
            for (int j = 0; j < 2; ++j) {
                best[j] = c.take<int32_t>(h_best[j] ? per_side : 0);
                margin[j] = c.take<double>(h_best[j] ? per_side : 0);
            }
            labels = c.take<int32_t>(labels_host ? n : 0);
            lengths = c.take<int64_t>(lengths_host ? n : 0);
            thresholds = c.take<double>((size_t)n_thresholds);
            out = c.take<int64_t>(n_out);
        }));
        auto send = [](auto*& dst, const auto* src, size_t count) {      // absent: a null pointer
            if (!src) return dst = nullptr, hipSuccess;
            return hipMemcpy(dst, src, count * sizeof(*src), hipMemcpyHostToDevice);
        };
        for (int j = 0; j < 2; ++j) {
            DBH_HIP(send(best[j], h_best[j], per_side));
            DBH_HIP(send(margin[j], h_best[j] ? h_margin[j] : nullptr, per_side));
        }
        DBH_HIP(send(labels, labels_host, n));
        DBH_HIP(send(lengths, lengths_host, n));
        DBH_HIP(send(thresholds, thresholds_host, (size_t)n_thresholds));
        DBH_HIP(hipMemset(out, 0, n_out * sizeof(int64_t)));
        return DBH_OK;
    }
};

}  // namespace

extern "C" {

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

int dbh_sweep_i16_dev(dbh_model* m, const int16_t* samples_dev, const int64_t* offsets_dev,
                      int64_t n_reads, int side, int max_scan_size, int32_t* best_dev,
                      double* margin_dev, void* workspace_dev, dbh_stream stream) {
    if (!m) return DBH_ERR_INVALID_ARGUMENT;
    return sweep_i16_dev(m, samples_dev, offsets_dev, n_reads, side, max_scan_size, best_dev,
                         margin_dev, workspace_dev, stream, ReadHints{0, m->hint_len, m->hint_cap});
}

// dbh_sweep_pair_i16 through host_groups: per group each model's window pass and fold, a SweepOut -
// (best, margin) of every prefix - coming back
int dbh_sweep_pair_i16(dbh_model* start_model, dbh_model* end_model, const int16_t* samples_host,
                       const int64_t* offsets_host, int64_t n_reads, int max_scan_size,
                       int32_t* start_best_host, double* start_margin_host,
                       int32_t* end_best_host, double* end_margin_host) {
    dbh_model* const models[2] = {start_model, end_model};
    int32_t* const best_host[2] = {start_best_host, end_best_host};
    double* const margin_host[2] = {start_margin_host, end_margin_host};
    dbh_model* m = models[0] ? models[0] : models[1];      // owns the slots
    const int steps = sweep_pair_steps(models, max_scan_size);
    if (!m || n_reads < 0 || steps <= 0) return DBH_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < 2; ++j)
        if (models[j] && n_reads > 0 && (!best_host[j] || !margin_host[j])) return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    int64_t total_samples = 0;
    if (!offsets_host || !dbh_host::offsets_run_forwards(offsets_host, n_reads, &total_samples) ||
        (total_samples > 0 && !samples_host))
        return DBH_ERR_INVALID_ARGUMENT;
    auto layout = [&](const void* base, int64_t cnt) {
        return dbh_host::SweepOut(const_cast<void*>(base), cnt, steps, models[0], models[1]);
    };
    GroupJob groups;
    groups.steps = steps;
    groups.out_bytes = [&](int64_t cnt) { return layout(nullptr, cnt).total; };
    groups.work_bytes = [&](int64_t cnt) {
        return pair_workspace_bytes(dbh_sweep_workspace_bytes, models, cnt, max_scan_size);
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
    const int32_t* const h_best[2] = {start_best_host, end_best_host};
    const double* const h_margin[2] = {start_margin_host, end_margin_host};
    TallyInputs d;
    DBH_TRY(d.upload(h_best, h_margin, labels_host, nullptr, n_reads, per_side, thresholds_host,
                     n_thresholds, cells));
    DBH_HIP(dbh_sweep::tally(d.best[0], d.margin[0], d.best[1], d.margin[1], d.labels, n_reads, steps,
                             n_classes, d.thresholds, n_thresholds, (unsigned long long*)d.out, 0));
    std::vector<int64_t> got(cells);
    DBH_HIP(hipMemcpy(got.data(), d.out, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cells; ++i) counts_host[i] += got[i];
    return DBH_OK;
}

// ---- the early tally: the live decision of every min_windows and threshold (dbh_early_core.h) ----
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
    const int32_t* const h_best[2] = {start_best_host, end_best_host};
    const double* const h_margin[2] = {start_margin_host, end_margin_host};
    TallyInputs d;
    DBH_TRY(d.upload(h_best, h_margin, labels_host, lengths_host, n_reads, per_side,
                     thresholds_host, n_thresholds, n_all));
    int64_t* const d_early = d.out + n_out[0];
    int64_t* const d_windows = d_early + n_out[1];
    DBH_HIP(dbh_sweep::early_tally(
        d.best[0], d.margin[0], d.best[1], d.margin[1], d.labels, d.lengths, n_reads, steps,
        n_classes, input_size, chunk_samples, d.thresholds, n_thresholds, P,
        (unsigned long long*)d.out, (unsigned long long*)d_early, (unsigned long long*)d_windows,
        lengths_host ? (unsigned long long*)(d_windows + n_out[2]) : nullptr, 0));
    std::vector<int64_t> got(n_all);
    DBH_HIP(hipMemcpy(got.data(), d.out, n_all * sizeof(int64_t), hipMemcpyDeviceToHost));
    int64_t* const out[4] = {calls_host, early_host, windows_host, pushes_host};
    size_t at = 0;
    for (int a = 0; a < 4; ++a)
        for (size_t i = 0; i < n_out[a]; ++i) out[a][i] += got[at++];
    return DBH_OK;
}

}  // extern "C"
