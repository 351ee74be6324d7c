// dbh_api_scan.hip — the scan's host unit of libdeepbinner_hip.so: every window of every read, and
// the events of the track (dbh_scan_*).  Host code only: the ragged window front and the event pass
// are dbh_scan.hip's behind dbh_scan.h; the windows go through the public predict and fold entries.
#include "dbh_model.h"
#include "dbh_scan.h"

bool dbh_api::scan_input_size_ok(int input_size) {
    return input_size % 2 == 0 && input_size >= 96 && input_size <= dbh_gen::kMaxInput;
}

using namespace dbh_api;

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
    if (n_reads == 0) {
        *n_events = *n_interior = 0;
        return DBH_OK;
    }
    ResidentReads reads;
    DBH_TRY(reads.admit(samples_host, offsets_host, n_reads));
    const int L = m->input_size, C = m->n_classes;
    int64_t total_windows = 0;
    for (int64_t i = 0; i < n_reads; ++i) {
        const int64_t w = dbh_scan::window_count(offsets_host[i + 1] - offsets_host[i], L);
        if (w > INT32_MAX) return DBH_ERR_INVALID_ARGUMENT;      // (an event's window is an int32)
        total_windows += w;
    }
    DBH_HIP(hipSetDevice(m->device));      // (see dbh_classify_i16)
    // chunks of windows: 256 MiB of fp32 input at the most, and a persistent model's host group
    int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)L * (int64_t)sizeof(float)));
    if (m->kind == DBH_MODEL_KIND_PERSISTENT) chunk = std::min(chunk, std::max<int64_t>(1, m->host_group_windows));
    chunk = std::min(chunk, total_windows);
    // the call's block (freed on return): behind the reads, every window's fold, one chunk of
    // windows and their probabilities, and the event pass's results and workspace
    int64_t *d_window_offsets = nullptr, *d_n_events = nullptr;
    int32_t *d_best = nullptr, *d_interior = nullptr;
    double* d_margin = nullptr;
    float *d_x = nullptr, *d_probs = nullptr;
    dbh_scan_event* d_events = nullptr;
    char* d_work = nullptr;
    DBH_TRY(reads.upload([&](dbh_host::Carve& c) {
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
    DBH_HIP(dbh_scan::window_offsets(reads.offsets, n_reads, L, d_window_offsets, 0));
    for (int64_t w0 = 0; w0 < total_windows; w0 += chunk) {
        const int64_t cnt = std::min(chunk, total_windows - w0);
        DBH_HIP(dbh_scan::windows(reads.samples, reads.offsets, d_window_offsets, n_reads, L, side,
                                  w0, cnt, d_x, 0));
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

}  // extern "C"
