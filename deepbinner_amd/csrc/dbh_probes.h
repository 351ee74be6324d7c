// dbh_probes.h — the instruments of the forward kernel: event brackets around production launches
// (dbh_forward_timing_*), the cycle-stamp build of the kernel (dbh_forward_timeline*), the clock
// and phase marks a production launch leaves (dbh_forward_clock_*, dbh_forward_phases_*).  Host code,
// a part of the core unit (dbh_api.hip includes it once) over the model object of dbh_model.h; the
// cycle-stamp kernel itself is built and launched in dbh_timeline.hip.  Of all this the launch path
// only calls TimingBrackets::begin / end.
#pragma once

#include "dbh_kernels.h"
#include "dbh_model.h"

// Launch number pos of every `every`: pos 0 opens a bracket (start event recorded in front of the
// launch), launches 0 .. span-1 belong to it, the last of them closes it in end().
hipError_t dbh_api::TimingBrackets::begin(hipStream_t stream, int64_t windows) {
    const int64_t pos = launch_counter++ % every;
    if (pos == 0) {
        if (events_used == events.size()) {
            events.emplace_back();
            hipError_t e = hipEventCreate(&events.back().first.h);
            if (e == hipSuccess) e = hipEventCreate(&events.back().second.h);
            if (e != hipSuccess) {
                events.pop_back();
                return e;
            }
        }
        const hipError_t e = hipEventRecord(events[events_used].first, stream);
        if (e != hipSuccess) return e;
        open_stop = events[events_used].second;
        open_windows = 0;
    }
    if (open_stop && pos < span) open_windows += windows;
    return hipSuccess;
}

hipError_t dbh_api::TimingBrackets::end(hipStream_t stream) {
    if (!open_stop || (launch_counter - 1) % every != span - 1) return hipSuccess;
    const hipError_t e = hipEventRecord(std::exchange(open_stop, nullptr), stream);
    if (e != hipSuccess) return e;
    ++events_used;                          // only closed brackets count
    timed_windows += open_windows;
    timed_launches += span;
    return hipSuccess;
}

void dbh_api::TimingBrackets::reset() {
    open_stop = nullptr;
    events_used = 0;
    timed_windows = timed_launches = 0;
}

namespace {

// One launch of the cycle-stamp kernel on the null stream: `a` comes with its input and debug
// stage chosen by the caller; probabilities (and calls, if wanted, behind them) go to the model's
// `out`, the stamps through `work` to stamps_host.
int run_timeline(dbh_model* m, dbh::ForwardArgs a, int64_t n, unsigned grid,
                 bool with_calls, int64_t* stamps_host) {
    const size_t stamp_bytes = (size_t)n * dbh::kWaves * 64 * sizeof(int64_t);
    dbh_api::TailScratch& tail = m->tails[nullptr];
    DBH_HIP(m->work.reserve(stamp_bytes));
    DBH_HIP(m->out.reserve((size_t)n * (m->n_classes + (with_calls ? 1 : 0)) * sizeof(float)));
    DBH_HIP(tail.reserve(grid, nullptr));
    DBH_HIP(hipMemsetAsync(m->work.get(), 0, stamp_bytes, 0));
    a.packed = m->packed.as<float>();
    a.probs = m->out.as<float>();
    a.calls = with_calls ? (int*)(a.probs + n * m->n_classes) : nullptr;
    a.debug_out = m->work.as<float>();
    a.n_windows = (long long)n;
    a.n_classes = m->n_classes;
    a.steps = 1;
    a.tail_scratch = tail.scratch();
    a.win_counter = nullptr;           // (fixed shares: the stamps are indexed by window)
    DBH_HIP(dbh_kernels::launch_forward_timeline(a, grid, 0));
    DBH_HIP(hipMemcpyAsync(stamps_host, m->work.get(), stamp_bytes, hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipStreamSynchronize(0));
    return DBH_OK;
}

// the marks of the last production launch with the clock probe on: per workgroup 4 clock values,
// then kPhaseMarks x kPhaseGroups phase stamps
constexpr size_t kClockPerWg = 4 + dbh::kPhaseMarks * dbh::kPhaseGroups;
int download_clock(dbh_model* m, std::vector<int64_t>& c) {
    if (!m->clock_probe || m->clock_grid == 0 || !m->clock.get()) return DBH_ERR_INVALID_ARGUMENT;
    DBH_HIP(hipSetDevice(m->device));
    DBH_HIP(hipDeviceSynchronize());
    c.resize((size_t)m->clock_grid * kClockPerWg);
    DBH_HIP(hipMemcpy(c.data(), m->clock.get(), c.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    return DBH_OK;
}

}  // namespace

extern "C" {

int dbh_forward_timeline(dbh_model* m, const float* x_host, int64_t n, int64_t* stamps_host) {
    if (!m || n <= 0 || !x_host || !stamps_host) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    DBH_HIP(m->in.reserve((size_t)n * dbh::kWindow * sizeof(float)));
    DBH_HIP(hipMemcpyAsync(m->in.get(), x_host, (size_t)n * dbh::kWindow * sizeof(float),
                           hipMemcpyHostToDevice, 0));
    dbh::ForwardArgs a = {};
    a.x = m->in.as<float>();
    a.debug_stage = 300;
    return run_timeline(m, a, n, (unsigned)((n + dbh::kGroup - 1) / dbh::kGroup), false, stamps_host);
}

int dbh_forward_timeline_i16(dbh_model* m, const int16_t* samples_host, int64_t n,
                             int64_t* stamps_host) {
    if (!m || n <= 0 || !samples_host || !stamps_host) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    const size_t sample_bytes = (size_t)n * dbh::kWindow * sizeof(int16_t);
    const size_t offset_bytes = (size_t)(n + 1) * sizeof(int64_t);
    DBH_HIP(m->in.reserve(sample_bytes + offset_bytes + 16));
    std::vector<int64_t> offsets((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) offsets[(size_t)i] = i * dbh::kWindow;
    char* d_offsets = m->in.as<char>((sample_bytes + 7) & ~(size_t)7);
    DBH_HIP(hipMemcpyAsync(m->in.get(), samples_host, sample_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipMemcpyAsync(d_offsets, offsets.data(), offset_bytes, hipMemcpyHostToDevice, 0));
    DBH_HIP(hipStreamSynchronize(0));
    dbh::ForwardArgs a = {};
    a.samples = m->in.as<int16_t>();
    a.offsets = (const long long*)d_offsets;
    a.score_diff = 0.5;
    a.len_hint = (long long)m->hint_len;
    a.hint_cap = (long long)m->hint_cap;
    // more windows than CUs: a persistent launch, as in production (stamps per window)
    a.debug_stage = n > m->cus ? 301 : 300;
    const int64_t groups = (n + dbh::kGroup - 1) / dbh::kGroup;
    return run_timeline(m, a, n, (unsigned)(n > m->cus && groups > m->cus ? m->cus : groups), true,
                        stamps_host);
}

int dbh_forward_timing_enable_span(dbh_model* m, int every_nth, int span) {
    if (!m || span < 1 || (every_nth > 0 && span > every_nth)) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    m->timing.every = every_nth > 0 ? every_nth : 0;
    m->timing.span = span;
    m->timing.open_windows = 0;
    m->timing.launch_counter = 0;
    m->timing.reset();
    return DBH_OK;
}

int dbh_forward_timing_enable(dbh_model* m, int enable) {
    return dbh_forward_timing_enable_span(m, enable, 1);
}

int dbh_forward_timing_read(dbh_model* m, double* total_ms, int64_t* launches, int64_t* windows) {
    if (!m || !total_ms || !launches || !windows) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    dbh_api::TimingBrackets& t = m->timing;
    double sum = 0.0;
    for (size_t i = 0; i < t.events_used; ++i) {
        DBH_HIP(hipEventSynchronize(t.events[i].second));
        float ms = 0.f;
        DBH_HIP(hipEventElapsedTime(&ms, t.events[i].first, t.events[i].second));
        sum += ms;
    }
    *total_ms = sum;
    *launches = t.timed_launches;
    *windows = t.timed_windows;
    t.reset();
    return DBH_OK;
}

int dbh_forward_clock_enable(dbh_model* m, int enable) {
    if (!m) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    m->clock_probe = enable != 0;
    if (!enable) m->clock_grid = 0;
    return DBH_OK;
}

int dbh_forward_clock_read(dbh_model* m, double* shader_ghz) {
    if (!m || !shader_ghz) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    *shader_ghz = 0.0;
    std::vector<int64_t> c;
    DBH_TRY(download_clock(m, c));
    int wall_khz = 0;      // the rate of s_memrealtime (100 MHz on this hardware)
    DBH_HIP(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, m->device));
    if (wall_khz <= 0) return DBH_ERR_HIP;
    std::vector<double> ratios;
    for (unsigned b = 0; b < m->clock_grid; ++b) {
        const double shader = (double)(c[b * kClockPerWg + 2] - c[b * kClockPerWg]);
        const double wall = (double)(c[b * kClockPerWg + 3] - c[b * kClockPerWg + 1]);
        if (shader > 0 && wall > 0) ratios.push_back(shader / wall);
    }
    if (ratios.empty()) return DBH_ERR_HIP;
    std::nth_element(ratios.begin(), ratios.begin() + ratios.size() / 2, ratios.end());
    *shader_ghz = ratios[ratios.size() / 2] * (double)wall_khz * 1e-6;
    return DBH_OK;
}

int dbh_forward_phases_enable(dbh_model* m, int enable) {
    if (!m) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    m->phase_probe = enable != 0;
    return DBH_OK;
}

int dbh_forward_phases_count(int* count) {
    if (!count) return DBH_ERR_INVALID_ARGUMENT;
    *count = dbh::kPhaseMarks;
    return DBH_OK;
}

int dbh_forward_phases_read(dbh_model* m, double* mean_cycles, int64_t* groups) {
    if (!m || !mean_cycles || !groups) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_PERSISTENT) return DBH_ERR_UNSUPPORTED;
    if (!m->phase_probe) return DBH_ERR_INVALID_ARGUMENT;
    std::vector<int64_t> c;
    DBH_TRY(download_clock(m, c));
    // steady state: not a workgroup's first group (cold), and only groups followed by another one
    // (the last interval runs to the next group's first stamp)
    double sum[dbh::kPhaseMarks] = {};
    int64_t n = 0;
    for (unsigned b = 0; b < m->clock_grid; ++b) {
        const int64_t* s = c.data() + b * kClockPerWg + 4;
        for (int g = 1; g + 1 < dbh::kPhaseGroups; ++g) {
            const int64_t* a = s + g * dbh::kPhaseMarks;
            if (a[0] < 0 || a[dbh::kPhaseMarks] < 0 || a[dbh::kPhaseMarks + 1] < 0) break;
            bool ok = true;
            double d[dbh::kPhaseMarks];
            for (int i = 0; i < 5; ++i) {
                // (the fifth interval runs to the next group's first stamp)
                const int64_t from = a[i], to = i < 4 ? a[i + 1] : a[dbh::kPhaseMarks];
                d[i] = (double)(uint32_t)((uint32_t)to - (uint32_t)from);
                if (d[i] > 4e6) ok = false;                      // (a group that skipped a phase)
            }
            for (int i = 5; i < dbh::kPhaseMarks; ++i) d[i] = (double)a[i];      // (sums of intervals)
            if (!ok) continue;
            for (int i = 0; i < dbh::kPhaseMarks; ++i) sum[i] += d[i];
            ++n;
        }
    }
    for (int i = 0; i < dbh::kPhaseMarks; ++i) mean_cycles[i] = n ? sum[i] / (double)n : 0.0;
    *groups = n;
    return DBH_OK;
}

}  // extern "C"
