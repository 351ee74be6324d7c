// dbh_api_live.hip — the live sessions' host unit of libdeepbinner_hip.so (dbh_live_*): the session
// with its host mirror, push, the tracks, the yield policy, and the stand-alone fold, plan and policy
// entries.  Host code only: the kernels are dbh_live.hip's (dbh_live.h), the rules both sides run
// dbh_live_core.h's; the windows go through the public predict entry.
#include <cstring>
#include <memory>
#include <new>

#include "dbh_live.h"
#include "dbh_model.h"

using namespace dbh_api;

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

using dbh_host::align256;
using dbh_host::live_chunk_flags_ok;

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
              dbh_live_end_result* end_results, dbh_live_action* actions, int64_t n_chunks) {
    if (!s || n_chunks < 0) return DBH_ERR_INVALID_ARGUMENT;
    if (n_chunks == 0) return DBH_OK;
    if (!channels || !offsets || !samples || !flags || !results || n_chunks > s->n_channels)
        return DBH_ERR_INVALID_ARGUMENT;
    const int64_t push = s->pushes + 1;        // (`seen` is scratch: a refused push leaves no state)
    for (int64_t i = 0; i < n_chunks; ++i) {
        const int32_t ch = channels[i];
        if (ch < 0 || ch >= s->n_channels || s->seen[(size_t)ch] == push ||
            offsets[i + 1] < offsets[i] || !live_chunk_flags_ok(flags[i])) {
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
        if (lengths[i] < 0 || !live_chunk_flags_ok(chunk_flags[i])) return DBH_ERR_INVALID_ARGUMENT;
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
        if (lengths[i] < 0 || !live_chunk_flags_ok(chunk_flags[i])) return DBH_ERR_INVALID_ARGUMENT;
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
                !live_chunk_flags_ok(chunk_flags_host[i]))
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

}  // extern "C"
