// dbh_live.h — what the library's host code (dbh_api_live.hip) sees of dbh_live.hip: the
// kernels of a live session's push, one launch function each.  No kernel symbol leaves the unit.
// The contract is include/deepbinner_hip.h's ("live"); the rules are dbh_live_core.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dbh_live_core.h"

namespace dbh_live {

constexpr int kMaxClasses = 256;      // the general path's limit (dbh_general.h)

// one chunk of a push as the kernels read it: `length` samples for `channel`, of which the ones
// that the start side keeps lie from in[src] on and the ones the tail ring keeps (a pair session's
// last min(length, cap_e)) from in[tail] on
struct Chunk {
    long long src, length, tail;
    int channel;
    unsigned flags;
};

// the channels' state on the device: sample rows of `stride` int16 (a multiple of 8, so that every
// row begins on a 16-byte boundary), the records and gates, merged [C], the track [steps]
struct State {
    int16_t* samples;
    long long stride;
    dbh_live_result* rec;
    Gate* gate;
    float* merged;
    int32_t* best;
    double* margin;
    int n_classes;
};

// The end side of a pair session: the tail rings, rows of `stride` int16 (a multiple of 8), the END
// model's shape, and as `end` what the fold keeps of the end windows - its record (fresh at END,
// FINAL behind the steps_e windows), merged [C], the end track [steps_e]; end.samples is not used.
// ring null: a start-only session.
struct Pair {
    int16_t* ring;
    long long stride;
    Shape shape;
    State end;
    int combine_mode;
};

// per chunk: reset on BEGIN, the kept samples into the channel's row, the counters; first[i] /
// count[i] get the windows this push made ready (first -1: an idle chunk).  A pair session's chunks
// also store their tails into the ring and make the end fold's record fresh at END.
hipError_t append(const State& st, const Shape& shape, const Pair& pair, const Chunk* chunks,
                  const int16_t* in, int n_chunks, int32_t* first, int32_t* count,
                  hipStream_t stream);

// win_offsets[n_chunks + 1]: the exclusive prefix of count, the total behind it
hipError_t window_list(const int32_t* count, int n_chunks, int64_t* win_offsets,
                       hipStream_t stream);

// x[n][L]: listed windows [w0, w0 + n), cut from the channels' rows, normalised and padded
hipError_t front(const State& st, const Shape& shape, const Chunk* chunks, const int32_t* first,
                 const int64_t* win_offsets, int n_chunks, int64_t w0, int64_t n, float* x,
                 hipStream_t stream);

// Folds listed windows [w0, w0 + n), whose probabilities are probs[n][C], into their channels in
// order: merged, record and track.  chunks null: chunk i is channel i.  general: one workgroup per
// chunk with dbh_trees.h's sums (C <= 256), else 32 lanes per chunk (C <= 32).
hipError_t fold(bool general, const State& st, const Shape& shape, const Chunk* chunks,
                const int64_t* win_offsets, int64_t n_chunks, int64_t w0, int64_t n,
                const float* probs, hipStream_t stream);

// x[n][L_e]: end windows [w0, w0 + n) of the list end_offsets[n_chunks + 1] (steps_e windows for
// every chunk that ended a read), read out of the channels' rings, normalised and padded in front
hipError_t end_front(const State& st, const Pair& pair, const Chunk* chunks,
                     const int64_t* end_offsets, int n_chunks, int64_t w0, int64_t n, float* x,
                     hipStream_t stream);

// results[i]: the record of chunk i's channel, IDLE where first[i] < 0; end_results (may be null;
// pair sessions): the end record beside it
hipError_t results(const State& st, const Pair& pair, const Chunk* chunks, const int32_t* first,
                   int n_chunks, dbh_live_result* results, dbh_live_end_result* end_results,
                   hipStream_t stream);

// The yield policy of a push (dbh_live_core.h, "Yield policies"): the records behind the push with
// either the push's chunk table or, chunks null, the caller's flags and channels; the session's
// yields [n_classes] and the channels' actions, in and out; one action record per chunk.
struct PolicyArgs {
    const dbh_live_result* records;
    const Chunk* chunks;
    const uint32_t* chunk_flags;
    const int32_t* channels;
    long long n_chunks;
    const int32_t* weight;
    int n_classes;
    long long slack;
    int undecided;
    long long* yield_samples;
    long long* yield_reads;
    int32_t* channel_action;
    dbh_live_action* actions;
};

// two launches: the yields of the chunks that ended a read (a workgroup per class), then the floor
// and every chunk's action (a thread per chunk).  n_classes <= kMaxClasses, n_chunks >= 1.
hipError_t policy(const PolicyArgs& args, hipStream_t stream);

}  // namespace dbh_live
