// dbh_api_locate.hip — the host unit of locate and of locate --occlude in libdeepbinner_hip.so
// (dbh_evidence_*, dbh_locate_*, dbh_occlude_*).  The two host routes are one body: they share the
// resident reads, LocateGroup's workspace and the group loop.  Host code only: the kernels are
// dbh_locate.hip's (dbh_locate.h) and dbh_occlude.hip's (dbh_occlude.h), the layer chain the general
// path's.
#include <cstdlib>

#include "dbh_locate.h"
#include "dbh_model.h"
#include "dbh_network.h"
#include "dbh_occlude.h"

namespace {

using namespace dbh_api;

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

// the arguments the plan and window entries share
bool occlude_shape_ok(int64_t n_reads, int steps, int input_size, int side) {
    return n_reads >= 0 && steps >= 1 && scan_input_size_ok(input_size) &&
           (int64_t)steps * input_size <= (int64_t)1 << 30 &&
           (side == DBH_SIDE_START || side == DBH_SIDE_END);
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

// dbh_locate_workspace_bytes and, with `occlude`, dbh_locate_occluded_workspace_bytes: one group's
// workspace, through the lay_out calls locate_route carves with
int locate_workspace(const dbh_model* m, int64_t n_reads, int scan_size, bool occlude, size_t* bytes) {
    if (!m || !bytes || n_reads < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_GENERAL) return DBH_ERR_UNSUPPORTED;
    const int steps = dbh_host::model_steps(m->input_size, scan_size);
    if (steps <= 0 || (occlude && !occlude_shape_ok(n_reads, steps, m->input_size, DBH_SIDE_START)))
        return DBH_ERR_INVALID_ARGUMENT;
    const int64_t group = std::min(n_reads, locate_group_reads(m, steps));
    dbh_host::Carve sizing(nullptr);
    LocateGroup().lay_out(sizing, m, group, steps);
    if (occlude) OccludeGroup().lay_out(sizing, m, group, steps);
    *bytes = sizing.used;
    return DBH_OK;
}

// dbh_locate_i16 and, with `occlude`, dbh_locate_occluded_i16.  One block for the call, freed on
// return: the reads, the results of every read, then one group's workspace (and, occluding, the
// group's windows beside it).  The groups follow each other on the null stream, which is what lets
// them share that workspace; nothing is waited for until the results are copied back.
int locate_route(dbh_model* m, const int16_t* samples_host, const int64_t* offsets_host,
                 int64_t n_reads, int side, int scan_size, double score_diff, float* probs_host,
                 int32_t* calls_host, dbh_location* locations_host, bool occlude,
                 dbh_occlusion* occlusions_host) {
    if (!m || n_reads < 0 || (side != DBH_SIDE_START && side != DBH_SIDE_END))
        return DBH_ERR_INVALID_ARGUMENT;
    if (m->kind != DBH_MODEL_KIND_GENERAL) return DBH_ERR_UNSUPPORTED;
    const int steps = dbh_host::model_steps(m->input_size, scan_size);
    if (steps <= 0 || !(score_diff == score_diff) ||
        (occlude && !occlude_shape_ok(n_reads, steps, m->input_size, side)))
        return DBH_ERR_INVALID_ARGUMENT;
    if (n_reads == 0) return DBH_OK;
    if (!probs_host || !calls_host || !locations_host || (occlude && !occlusions_host))
        return DBH_ERR_INVALID_ARGUMENT;
    ResidentReads reads;
    DBH_TRY(reads.admit(samples_host, offsets_host, n_reads));
    DBH_HIP(hipSetDevice(m->device));      // (see dbh_classify_i16)
    const int C = m->n_classes, cells = m->gen.len[7], L = m->input_size;
    const int64_t group = std::min(n_reads, locate_group_reads(m, steps));
    float* d_probs = nullptr;
    int32_t* d_calls = nullptr;
    dbh_location* d_locations = nullptr;
    dbh_occlusion* d_occlusions = nullptr;
    LocateGroup g;
    OccludeGroup o;
    DBH_TRY(reads.upload([&](dbh_host::Carve& c) {
        d_probs = c.take<float>((size_t)n_reads * C);
        d_calls = c.take<int32_t>((size_t)n_reads);
        d_locations = c.take<dbh_location>((size_t)n_reads);
        if (occlude) d_occlusions = c.take<dbh_occlusion>((size_t)n_reads);
        g.lay_out(c, m, group, steps);
        if (occlude) o.lay_out(c, m, group, steps);
    }));
    for (int64_t r0 = 0; r0 < n_reads; r0 += group) {
        const int64_t cnt = std::min(group, n_reads - r0);
        const int64_t* offsets = reads.offsets + r0;
        // The forward with evidence, merge and call, then the rule: a read's results come from its
        // own windows alone, so the grouping does not show in them.  Plain locate lets the front
        // slice the int16 samples; occluding, the group's windows are sliced and normalised once and
        // the unblanked pass runs on them (the front takes an fp32 window as the value it would slice).
        if (occlude) DBH_HIP(dbh_occlude::slice(reads.samples, offsets, cnt, steps, L, side, o.x, 0));
        DBH_HIP(dbh_gen::forward(m->gen, occlude ? o.x : nullptr, occlude ? nullptr : reads.samples,
                                 occlude ? nullptr : offsets, steps, side, cnt * steps, g.wprobs,
                                 g.evidence, g.act, 0));
        DBH_HIP(dbh_gen::merge(g.wprobs, cnt, steps, C, score_diff, d_probs + r0 * C, d_calls + r0,
                               0));
        DBH_HIP(dbh_locate::locate(g.evidence, d_calls + r0, offsets, cnt, steps, cells, C, L, side,
                                   d_locations + r0, 0));
        if (!occlude) continue;
        // the plan, the three variants' windows, and one pass each through the same workspace
        DBH_HIP(dbh_occlude::plan(d_locations + r0, offsets, cnt, steps, L, side, o.plans,
                                  d_occlusions + r0, 0));
        DBH_HIP(dbh_occlude::windows(o.x, offsets, o.plans, cnt, steps, L, side, o.variants, 0));
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
    if (occlude)
        DBH_HIP(hipMemcpyAsync(occlusions_host, d_occlusions, (size_t)n_reads * sizeof(dbh_occlusion),
                               hipMemcpyDeviceToHost, 0));
    DBH_HIP(hipStreamSynchronize(0));
    return DBH_OK;
}

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
    if (!evidence_host || !calls_host || !offsets_host || !locations_host ||
        !dbh_host::offsets_run_forwards(offsets_host, n_reads))
        return DBH_ERR_INVALID_ARGUMENT;
    dbh_locate::locate_host(evidence_host, calls_host, offsets_host, n_reads, steps, cells, n_classes,
                            input_size, side, locations_host);
    return DBH_OK;
}

int dbh_locate_workspace_bytes(const dbh_model* m, int64_t n_reads, int scan_size, size_t* bytes) {
    return locate_workspace(m, n_reads, scan_size, false, bytes);
}

int dbh_locate_i16(dbh_model* m, const int16_t* samples_host, const int64_t* offsets_host,
                   int64_t n_reads, int side, int scan_size, double score_diff, float* probs_host,
                   int32_t* calls_host, dbh_location* locations_host) {
    return locate_route(m, samples_host, offsets_host, n_reads, side, scan_size, score_diff,
                        probs_host, calls_host, locations_host, false, nullptr);
}

// ---- occlude: blank the located span and call the read again (dbh_occlude.hip) -------------------
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
        !dbh_host::offsets_run_forwards(offsets_host, n_reads))
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
        !dbh_host::offsets_run_forwards(offsets_host, n_reads))
        return DBH_ERR_INVALID_ARGUMENT;
    const size_t floats = (size_t)n_reads * steps * input_size;
    float* const out[3] = {variants_host, variants_host + floats, variants_host + 2 * floats};
    dbh_occlude::windows_host(x_host, offsets_host, plans_host, n_reads, steps, input_size, side,
                              out);
    return DBH_OK;
}

int dbh_locate_occluded_workspace_bytes(const dbh_model* m, int64_t n_reads, int scan_size,
                                        size_t* bytes) {
    return locate_workspace(m, n_reads, scan_size, true, bytes);
}

int dbh_locate_occluded_i16(dbh_model* m, const int16_t* samples_host, const int64_t* offsets_host,
                            int64_t n_reads, int side, int scan_size, double score_diff,
                            float* probs_host, int32_t* calls_host, dbh_location* locations_host,
                            dbh_occlusion* occlusions_host) {
    return locate_route(m, samples_host, offsets_host, n_reads, side, scan_size, score_diff,
                        probs_host, calls_host, locations_host, true, occlusions_host);
}

}  // extern "C"
