/*
 * deepbinner_hip.h — C ABI of libdeepbinner_hip.so, the MI355X (gfx950) implementation of
 * Deepbinner's classify hot path.
 *
 * The reference has no C ABI on this path: its only device boundary is the Keras call
 *     labels = model.predict(input_signals, batch_size=args.batch_size)   deepbinner/classify.py:361
 * on a model obtained from keras.models.load_model (classify.py:90), wrapped by call_batch
 * (classify.py:325-384).  This header is what a binding for that boundary binds instead; it is
 * modelled on the reference's own ctypes idiom for its one native library
 * (deepbinner/dtw_semi_global.py:30-41: cdll.LoadLibrary, C-contiguous ndpointers, explicit
 * restype/argtypes, caller-allocated outputs, plain-int sizes, scalar return code).
 *
 * Conventions
 *   - every function returns a dbh_status (0 = DBH_OK); nothing throws or exits across the ABI;
 *   - buffers are plain pointers + element counts, C-contiguous, little-endian;
 *   - "_dev" variants take DEVICE pointers and a stream and do not synchronise; the others take
 *     HOST pointers, copy, run and return when the result is in the caller's buffer;
 *   - a model handle belongs to the device that was current when it was created; calls on one
 *     handle must not overlap (the reference host code is single-threaded, classify.py:416-423).
 */
#ifndef DEEPBINNER_HIP_H
#define DEEPBINNER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DBH_OK = 0,
    DBH_ERR_INVALID_ARGUMENT = 1,
    DBH_ERR_NO_DEVICE = 2,        /* no gfx950-capable HIP device visible */
    DBH_ERR_HIP = 3,              /* a HIP runtime call failed; see dbh_last_error() */
    DBH_ERR_BAD_WEIGHTS = 4,      /* blob size does not match the Deepbinner architecture */
    DBH_ERR_UNSUPPORTED = 5,      /* geometry outside the limits (dbh_model_create_ex), or a
                                     persistent-kernel call on a general model */
    DBH_ERR_OUT_OF_MEMORY = 6,
    DBH_ERR_COMM = 7              /* RCCL missing or a collective failed; see dbh_comm_last_error() */
} dbh_status;

typedef struct dbh_model dbh_model;      /* opaque: packed weights resident in HBM */
typedef void* dbh_stream;                /* a hipStream_t */
typedef void* dbh_event;                 /* a hipEvent_t */

#define DBH_SIDE_START 0                 /* classify.py:343-344, windows right-padded  (:355) */
#define DBH_SIDE_END 1                   /* classify.py:345-349, windows left-padded   (:357) */
#define DBH_CALL_NONE 0                  /* barcode call 'none' (classify.py:289-290,295)   */
#define DBH_WINDOW 1024                  /* model input size, classify.py:96                */

/* ---- library / device ------------------------------------------------------------------ */
const char* dbh_version(void);
const char* dbh_status_string(int status);
const char* dbh_last_error(void);                       /* text of the last DBH_ERR_HIP      */
int dbh_device_count(int* count);
int dbh_set_device(int ordinal);                        /* replaces set_tensorflow_threads' device_count, classify.py:416-423 */
int dbh_get_device(int* ordinal);
int dbh_device_name(int ordinal, char* buf, int buf_len);
int dbh_device_synchronize(void);

/* ---- raw device memory (so a host language needs no other GPU library) ----------------- */
int dbh_malloc(void** dev_ptr, size_t bytes);
int dbh_free(void* dev_ptr);
int dbh_malloc_host(void** host_ptr, size_t bytes);     /* pinned, for overlapped H2D        */
int dbh_free_host(void* host_ptr);
/* The address the GPU reaches a pinned host buffer at.  The *_dev entry points take it wherever
 * they take a device pointer for RESULTS (calls, probabilities): the kernels then store them
 * straight into host memory - no copy command between two launches of a stream (one GPU's calls
 * in bench.py; 40 KB per 10,000 reads). */
int dbh_host_device_pointer(void* host_ptr, void** dev_ptr);
int dbh_memcpy_h2d(void* dev_dst, const void* host_src, size_t bytes, dbh_stream stream);
int dbh_memcpy_d2h(void* host_dst, const void* dev_src, size_t bytes, dbh_stream stream);
int dbh_memcpy_d2d(void* dev_dst, const void* dev_src, size_t bytes, dbh_stream stream);
int dbh_stream_create(dbh_stream* stream);
int dbh_stream_destroy(dbh_stream stream);
int dbh_stream_synchronize(dbh_stream stream);
int dbh_event_create(dbh_event* event);
int dbh_event_destroy(dbh_event event);
int dbh_event_record(dbh_event event, dbh_stream stream);
int dbh_event_synchronize(dbh_event event);
/* what is queued on `stream` after this call waits until `event` (recorded on another stream of
 * the device) has happened: the edge between a classification stream and the side stream that
 * gathers and copies its calls (bench.py, sharding.SideGather) */
int dbh_stream_wait_event(dbh_stream stream, dbh_event event);
int dbh_event_elapsed_ms(dbh_event start, dbh_event stop, float* ms);

/* ---- model (replaces keras.models.load_model, classify.py:90) -------------------------- */
/* weights: the canonical flat fp32 blob (deepbinner_amd/model_format.py): for conv 1..20
 * kernel[k][C_in][C_out] then bias[C_out]; for batch-norm 1..7 gamma, beta, mean, variance.
 * n_floats must equal the architecture's parameter count for n_classes (107,197 for 13).
 * RANGE: the persistent forward kernel this call uses holds activations times 2^-60 and takes its
 * ReLU from a [0, 1] clamp, so every activation of the model (the output of every convolution and
 * batch normalisation, on the windows it will see) must stay below 2^60 = 1.15e18; a larger one
 * is cut to 2^60 without an error.  The shipped models reach 2^27 on real reads.  A model that
 * may exceed the limit goes through dbh_model_create_ex with DBH_MODEL_GENERAL: the general path
 * works in plain fp32 and has fp32's own range.  Batch-norm gammas of either sign and of zero are
 * supported by both. */
int dbh_model_create(const float* weights, int64_t n_floats, int n_classes, int input_size,
                     dbh_model** model);
/* Any Deepbinner geometry the reference's own `train` writes: input_size L even, 96 <= L <= 16,384
 * (classify.py:396-407 wants it even; the global average needs one position, so L >= 95), and
 * 2 <= n_classes <= 256 (a 96-barcode kit gives 97).  flags: DBH_MODEL_AUTO runs the persistent
 * forward kernel when L = 1024 and n_classes <= 32 (what dbh_model_create takes) and the GENERAL
 * path otherwise - a layer-by-layer MFMA implicit GEMM over chunks of windows ("General
 * models"); DBH_MODEL_GENERAL forces the general path (A/B runs, tests).  Same blob and n_floats
 * check as dbh_model_create (DBH_ERR_BAD_WEIGHTS); a geometry outside the limits is
 * DBH_ERR_UNSUPPORTED, both before any device work.
 * A general model takes every network entry point (dbh_predict*, dbh_classify_*, the pair calls;
 * scan_size must be a multiple of L/2 and gives scan_size / (L/2) steps); the two models of a pair
 * call may differ in L and kind but not in n_classes.  The tuning calls (set_host_group,
 * reserve_cus, set_read_length_hint) accept it and do nothing; the introspection calls of the
 * persistent kernel (dbh_debug_forward, dbh_forward_truncated_dev, dbh_forward_timeline*,
 * dbh_forward_timing_*, dbh_forward_clock_*, dbh_forward_phases_*) return DBH_ERR_UNSUPPORTED. */
#define DBH_MODEL_AUTO 0
#define DBH_MODEL_GENERAL 1
#define DBH_MODEL_KIND_PERSISTENT 0
#define DBH_MODEL_KIND_GENERAL 1
int dbh_model_create_ex(const float* weights, int64_t n_floats, int n_classes, int input_size,
                        unsigned flags, dbh_model** model);
int dbh_model_kind(const dbh_model* model, int* kind);              /* DBH_MODEL_KIND_*             */
int dbh_model_destroy(dbh_model* model);
int dbh_model_input_size(const dbh_model* model, int* input_size);   /* model.inputs[0].shape[1], classify.py:93-96  */
int dbh_model_output_size(const dbh_model* model, int* n_classes);   /* model.outputs[0].shape[1], classify.py:94-97 */

/* The host-buffer entry points (dbh_predict, dbh_classify_i16) make the model's device the calling
 * thread's current device (HIP keeps that per thread), so a model may be driven from any thread -
 * two models from two threads at once, each on its own streams and staging buffers.  One model is
 * for one caller at a time.  The *_dev entry points work on the caller's device pointers and
 * leave the current device alone; launches of one model queued on DIFFERENT streams may overlap
 * on the device (the per-launch scratch is kept per stream), the host-side calls themselves must
 * still not overlap. */
/* ---- seam b1: model.predict (classify.py:361) ------------------------------------------ */
/* x: n_windows x input_size fp32 (already normalised);  probs: n_windows x n_classes fp32 softmax. */
int dbh_predict(dbh_model* model, const float* x_host, int64_t n_windows, float* probs_host);
int dbh_predict_dev(dbh_model* model, const float* x_dev, int64_t n_windows, float* probs_dev,
                    dbh_stream stream);

/* ---- seam b2: call_batch (classify.py:325-384) ------------------------------------------ */
/* samples: concatenated int16 raw signals; offsets[n_reads+1] delimit each read (any length
 * >= 0).  For each read: scan_size/(input_size/2) windows (classify.py:330-349), normalise
 * (trim_signal.py:61-69, fp64), zero-pad (classify.py:352-357), forward pass, min/max merge
 * (classify.py:368-374), make_sum_to_one (classify.py:387-393) and the top-2 threshold call
 * (classify.py:285-295).  probs: n_reads x n_classes fp32; calls: n_reads int32, 0 = 'none'. */
int dbh_classify_i16(dbh_model* model, const int16_t* samples_host, const int64_t* offsets_host,
                     int64_t n_reads, int side, int scan_size, double score_diff,
                     float* probs_host, int32_t* calls_host);
/* Host buffers that are pinned (dbh_malloc_host / dbh_host_alloc) are read by the GPU's DMA engine
 * where they lie; pageable ones go through a pinned staging copy first.  Either way the reads
 * travel in groups (32,768 windows per model by default: dbh_model_set_host_group) through three
 * slots, so that the upload of one group, the kernels of another and the results of a third
 * overlap. */
int dbh_model_set_host_group(dbh_model* model, int64_t windows_per_group /* 0 = default */);
/* The forward kernel is persistent: one workgroup per CU walks the windows of a launch.  A model
 * whose launches share the GPU with the inflate kernels of the next containers (the streaming
 * path: dbh_classify_pair_deflated on several queues) leaves them n_cus CUs - otherwise those
 * kernels find no CU free until the launch ends, and the workgroups they displaced start late.
 * 0 = all CUs again. */
int dbh_model_reserve_cus(dbh_model* model, int n_cus);

/* The body of the reference's per-batch loop (classify.py:141-171) for one batch of reads and BOTH
 * models in one call: the samples are uploaded once, the start model scans the first and the end
 * model the last scan_size samples of every read (call_batch with side 'start' / 'end',
 * classify.py:325-384), and combine_calls (classify.py:298-322, DBH_REQUIRE_*) gives the final
 * call - all queued on one stream per group, nothing but the calls (and whatever else is asked
 * for) coming back.  Either model may be NULL: calls_host is then the other model's calls.
 * calls_host: n_reads final calls.  Optional (NULL = not wanted): the per-side calls (n_reads
 * int32 each) and per-side probabilities (n_reads x n_classes fp32 each) - what --verbose
 * prints.  Both models must live on the same device and agree on n_classes. */
int dbh_classify_pair_i16(dbh_model* start_model, dbh_model* end_model,
                          const int16_t* samples_host, const int64_t* offsets_host,
                          int64_t n_reads, int scan_size, double score_diff, int combine_mode,
                          int32_t* calls_host, int32_t* start_calls_host, int32_t* end_calls_host,
                          float* start_probs_host, float* end_probs_host);

/* Pinned host memory behind the allocator signature libdeepbinner_fast5.so takes
 * (deepbinner_fast5.h: f5_set_sample_allocator): the loader's threads then write a batch straight
 * into memory the entry points above upload without a staging copy.  `user` is ignored. */
void* dbh_host_alloc(size_t bytes, void* user);
void dbh_host_release(void* ptr, void* user);
int dbh_host_is_pinned(const void* ptr, size_t bytes, int* pinned);

/* Optional hint for the *_dev entry points: "every read in the sample buffer is read_length
 * samples long and the buffer holds at least capacity_samples samples".  The forward kernel then
 * requests a read's samples from read_index * read_length TOGETHER with offsets[read_index]
 * instead of after it (a dependent load costs ~3k cycles at the top of a kernel) and fetches
 * again from the true place wherever the offsets disagree, so a wrong hint costs time, never
 * correctness; speculative addresses beyond capacity_samples are not touched.  read_length 0
 * clears the hint.  dbh_classify_i16 (host buffers) works this out per group by itself. */
int dbh_model_set_read_length_hint(dbh_model* model, int64_t read_length,
                                   int64_t capacity_samples);
/* device-resident variant; workspace_dev must hold dbh_classify_workspace_bytes() bytes (unused,
 * and may be NULL, when scan_size is 512 on a persistent model: the whole read then finishes
 * inside one launch; a general model always needs it - per-window probabilities and the
 * activations of one chunk of windows). */
int dbh_classify_workspace_bytes(const dbh_model* model, int64_t n_reads, int scan_size,
                                 size_t* bytes);
int dbh_classify_i16_dev(dbh_model* model, const int16_t* samples_dev, const int64_t* offsets_dev,
                         int64_t n_reads, int side, int scan_size, double score_diff,
                         float* probs_dev, int32_t* calls_dev, void* workspace_dev,
                         dbh_stream stream);

/* The same job for many reads in batches of batch_size reads (the reference's --batch_size loop,
 * classify.py:130), queued in order on `stream`.  offsets_dev holds n_reads+1 ABSOLUTE offsets
 * into samples_dev.  With scan_size 512 every batch is a single kernel launch (slice + normalise
 * + CNN + renormalise + call); otherwise two (CNN, merge).  Does not block the host. */
int dbh_classify_i16_batched_dev(dbh_model* model, const int16_t* samples_dev,
                                 const int64_t* offsets_dev, int64_t n_reads, int batch_size,
                                 int side, int scan_size, double score_diff, float* probs_dev,
                                 int32_t* calls_dev, dbh_stream stream);

/* combine_calls (classify.py:298-322) for whole arrays of start-model and end-model calls on the
 * device: out[i] is the final call of read i (DBH_CALL_NONE or a barcode number).  Agreement
 * stands; otherwise REQUIRE_BOTH refuses, REQUIRE_START keeps a start call the end model is silent
 * on, REQUIRE_EITHER (the default, deepbinner.py:315-316) keeps whichever side called when the
 * other is silent.  out_dev may alias either input.  Does not block the host. */
#define DBH_REQUIRE_EITHER 0
#define DBH_REQUIRE_START 1
#define DBH_REQUIRE_BOTH 2
int dbh_combine_calls_dev(const int32_t* start_calls_dev, const int32_t* end_calls_dev,
                          int64_t n_reads, int mode, int32_t* out_dev, dbh_stream stream);

/* ---- sweep: the calls of every scan size and every threshold from one window pass ------------ */
/* call_batch (classify.py:325-393) looks at steps = scan_size / (input_size / 2) windows per read
 * end.  Window s is the same samples whatever the scan size (classify.py:337-349), and the merge
 * over windows is a running minimum for class 0 and a running maximum for the barcodes
 * (classify.py:368-374): the merged vector after k windows IS what a run at scan_size =
 * k * input_size / 2 merges.  One window pass at max_scan_size therefore holds the call of every
 * smaller scan size, and - kept as the best class and its lead over the runner-up - of every
 * --score_diff.
 *
 * The fold.  For read r and k = 1 .. steps: merge windows 0 .. k-1, make_sum_to_one in fp64
 * (classify.py:387-393; a read whose barcodes are all zero keeps them zero instead of dividing by
 * their sum), then the top two (classify.py:285-295, ties to the lower class):
 *     best[r][k-1]    int32, the best class; 0 = class 0 leads, no barcode at any threshold
 *     margin[r][k-1]  fp64, best value - second value
 * The call at threshold t is   best != 0 && margin >= t ? best : 0   - to the bit what
 * dbh_classify_i16(_dev) at scan_size = k * input_size / 2 and score_diff = t calls, because the
 * model chooses the form of the fold whose sums run in the order of its own merge (persistent
 * models: 32 lanes per read; general models: one workgroup per read, up to 256 classes).
 *
 * dbh_sweep_windows_dev is the fold alone, over window_probs_dev [n_reads][steps][n_classes] fp32
 * (read-major, as the forward paths leave them), exposed for parity tests as dbh_merge_calls_dev
 * is.  dbh_sweep_i16_dev runs the model's window pass at max_scan_size and then the fold;
 * workspace_dev holds dbh_sweep_workspace_bytes() bytes and is needed at every scan size (one step
 * included: the fold reads per-window probabilities).  best_dev / margin_dev: n_reads x steps.
 * dbh_sweep_pair_i16 takes host buffers through the groups and slots of dbh_classify_pair_i16;
 * either model may be NULL (its two arrays are then not touched), a pair must live on one device
 * and agree on n_classes AND on the input size.  Every argument is checked before any device work
 * - a null pointer, n_reads < 0, steps < 1 or a max_scan_size that is no positive multiple of half
 * the input size, a mismatched pair, offsets that run backwards: DBH_ERR_INVALID_ARGUMENT, nothing
 * written.  n_reads == 0 is DBH_OK.  The _dev entries do not block the host. */
int dbh_sweep_windows_dev(const dbh_model* model, const float* window_probs_dev, int64_t n_reads,
                          int steps, int32_t* best_dev, double* margin_dev, dbh_stream stream);
int dbh_sweep_workspace_bytes(const dbh_model* model, int64_t n_reads, int max_scan_size,
                              size_t* bytes);
int dbh_sweep_i16_dev(dbh_model* model, const int16_t* samples_dev, const int64_t* offsets_dev,
                      int64_t n_reads, int side, int max_scan_size, int32_t* best_dev,
                      double* margin_dev, void* workspace_dev, dbh_stream stream);
int dbh_sweep_pair_i16(dbh_model* start_model, dbh_model* end_model, const int16_t* samples_host,
                       const int64_t* offsets_host, int64_t n_reads, int max_scan_size,
                       int32_t* start_best_host, double* start_margin_host,
                       int32_t* end_best_host, double* end_margin_host);
/* The tally.  From the folds of the start side, the end side or both (a side that is not given is
 * two NULLs), n_thresholds thresholds (fp64) and optional labels (int32 per read: the class the
 * read is known to carry, 0 = known to carry none, negative = unknown; NULL = none known) it ADDS
 * into counts, which the caller zeroed before the first call:
 *     counts[steps][n_thresholds][modes][n_classes + 3]   int64, C order
 *         [0 .. n_classes)   reads whose final call is that class (0 = none)
 *         [n_classes]        right:  labelled reads with call == label (none on label 0 included)
 *         [n_classes + 1]    wrong:  labelled reads with call != label and call != 0
 *         [n_classes + 2]    missed: labelled reads with call == 0 and label != 0
 * modes = 3 with both sides - the final call by combine_calls (classify.py:298-322) under
 * DBH_REQUIRE_EITHER, _START, _BOTH, in that order - and 1 with one side, whose call is final.
 * Only integers are added, so the result depends neither on the launch shape nor on how the reads
 * were split into calls.  A best outside [0, n_classes) counts in no class.  2 <= n_classes <= 256.
 * dbh_sweep_tally (host buffers) works on the calling thread's current device and blocks;
 * dbh_sweep_tally_dev queues on `stream`.  A null thresholds or counts, a side given by half,
 * no side, a count < 1 (n_reads < 0): DBH_ERR_INVALID_ARGUMENT, nothing written. */
int dbh_sweep_tally_dev(const int32_t* start_best_dev, const double* start_margin_dev,
                        const int32_t* end_best_dev, const double* end_margin_dev,
                        const int32_t* labels_dev, int64_t n_reads, int steps, int n_classes,
                        const double* thresholds_dev, int n_thresholds, int64_t* counts_dev,
                        dbh_stream stream);
int dbh_sweep_tally(const int32_t* start_best_host, const double* start_margin_host,
                    const int32_t* end_best_host, const double* end_margin_host,
                    const int32_t* labels_host, int64_t n_reads, int steps, int n_classes,
                    const double* thresholds_host, int n_thresholds, int64_t* counts_host);
/* The early tally: what a live session ("live", below) would have decided EARLY, for every
 * min_windows m = 1 .. steps and every threshold t, read out of the same start track.  A channel's
 * track is the sweep's fold under every chunking, and what decides is integers and comparisons over
 * it and the read's length, so one sweep holds every setting's outcome.  Per read, with L =
 * input_size, h = L / 2, cap = (steps + 1) h, c = chunk_samples, len = its length:
 *     lead(k)         = best[k] != 0 && margin[k] >= t          (a NaN margin leads nowhere)
 *     d               = the smallest k >= m - 1 with lead(k); none: the read is never decided
 *     call            = best[d], decided_windows = d + 1        (never decided: call 0)
 *     final_call      = lead(steps - 1) ? best[steps - 1] : 0
 *     pushes          R = max(1, ceil(len / c)): push r (from 1) brings the read to min(r c, len)
 *                     samples, the last one carries END - as the replay command delivers a read
 *     push            r = min(ceil((d h + L) / c), R), decided_samples = min(r c, len)
 * dbh_sweep_early_pushes gives P = ceil(cap / c), the latest push of any decision; P > 4096 is
 * refused.  The three tally entries ADD int64 into arrays the caller zeroed, all in C order with
 * first axis m - 1:
 *     calls[steps][T][modes][n_classes + 3]   dbh_sweep_tally's cell and its right / wrong / missed,
 *         of the early call; with an end side (both arrays; modes = 3) of combine_calls(early call,
 *         end call at t from end track entry steps - 1) under EITHER, START, BOTH - what a pair
 *         session stopped on its decision reports as read_call.  One side: modes = 1.
 *     early[steps][T][8]     0 decided: reads with a decision         1 agree: call == final_call
 *         2 changed: final_call is neither 0 nor call                 3 lost: final_call == 0
 *         4 late: decided_windows > m       5 windows: sum of decided_windows
 *         6 samples: sum of decided_samples 7 length: sum of len      (all over decided reads;
 *         6 and 7 stay 0 without lengths)
 *     windows[steps][T][steps]   decided reads by decided_windows - 1
 *     pushes[steps][T][P]        decided reads by r - 1; given exactly when lengths is
 * The start side is required; the end side, labels and lengths may be NULL.  A best outside
 * [0, n_classes) leads like any barcode and counts in no class.  A null required pointer, an end
 * side given by half, n_reads < 0, steps < 1, n_classes outside 2 .. 256, an odd or non-positive
 * input_size, chunk_samples < 1, P > 4096, n_thresholds < 1, lengths without pushes or the reverse:
 * DBH_ERR_INVALID_ARGUMENT, nothing written; so is a negative length on the two entries that take
 * host buffers, while dbh_sweep_early_tally_dev - which does not read its inputs on the host - takes
 * a negative length as 0.  n_reads == 0 is DBH_OK.  Only integers are added: the result depends
 * neither on the launch shape nor on how the reads were split into calls.  dbh_sweep_early_tally
 * works on the calling thread's current device and blocks; dbh_sweep_early_host runs the same rule
 * (csrc/dbh_early_core.h) on the host, with no device. */
int dbh_sweep_early_pushes(int input_size, int scan_size, int64_t chunk_samples, int* pushes);
int dbh_sweep_early_tally_dev(const int32_t* start_best_dev, const double* start_margin_dev,
                              const int32_t* end_best_dev, const double* end_margin_dev,
                              const int32_t* labels_dev, const int64_t* lengths_dev,
                              int64_t n_reads, int steps, int n_classes, int input_size,
                              int64_t chunk_samples, const double* thresholds_dev,
                              int n_thresholds, int64_t* calls_dev, int64_t* early_dev,
                              int64_t* windows_dev, int64_t* pushes_dev, dbh_stream stream);
int dbh_sweep_early_tally(const int32_t* start_best_host, const double* start_margin_host,
                          const int32_t* end_best_host, const double* end_margin_host,
                          const int32_t* labels_host, const int64_t* lengths_host, int64_t n_reads,
                          int steps, int n_classes, int input_size, int64_t chunk_samples,
                          const double* thresholds_host, int n_thresholds, int64_t* calls_host,
                          int64_t* early_host, int64_t* windows_host, int64_t* pushes_host);
int dbh_sweep_early_host(const int32_t* start_best_host, const double* start_margin_host,
                         const int32_t* end_best_host, const double* end_margin_host,
                         const int32_t* labels_host, const int64_t* lengths_host, int64_t n_reads,
                         int steps, int n_classes, int input_size, int64_t chunk_samples,
                         const double* thresholds_host, int n_thresholds, int64_t* calls_host,
                         int64_t* early_host, int64_t* windows_host, int64_t* pushes_host);

/* ---- scan: barcode signal in EVERY window of a read, and the events it makes ------------------ */
/* call_batch looks at the first (or last) scan_size samples of a read (classify.py:337-357).  A
 * chimeric read - two molecules in one signal - carries its second adapter and barcode somewhere in
 * the middle, where no window of classify ever lies.  The scan carries the same windows on to the
 * read's other end and says where a barcode class leads.  What it finds with the shipped models are
 * SYNTHETIC junctions (reads packed end to end); nothing here has been validated on real chimeric
 * reads.
 *
 * L = the model's input size, h = L / 2, a read has n samples.
 *   Window count.  W(n) = 1 for n <= L, else ceil((n - L) / h) + 1: the last window reaches the
 *       read's end and holds more than h samples.  dbh_scan_window_count (host only).
 *   Window k, side start: samples [k h, min(k h + L, n)), normalised over the samples present,
 *       zero-padded behind.  Side end: samples [max(n - k h - L, 0), n - k h), padded in front.
 *       For k < scan_size / h these are exactly call_batch's windows (classify.py:337-357).
 *   Normalising is the data set's rule ("device-fed batches", above): S and Q in int64, exact
 *       D = m Q - S^2 over the m samples present, mean = (double)S / m, std = sqrt((double)D) / m,
 *       each value (float)(((double)x - mean) / std), or (float)((double)x - mean) where D == 0; an
 *       empty window (n == 0) is all zeros.
 *   Track.  Per window (best, margin): the sweep's fold at steps = 1 applied to that window alone
 *       - make_sum_to_one, then the top two, ties to the lower class (classify.py:285-295) - which
 *       is dbh_sweep_windows_dev(model, probs, n_windows, 1, ...) with the windows as its reads.
 *   Fire.  Window k fires class b at threshold t when best == b != 0 && margin >= t.
 *   Event.  A maximal run of consecutive windows of ONE read that fire the same class, at least
 *       min_windows long: (read, class, first, last, peak = the highest margin of the run).
 *       Adjacent runs of different classes are separate events.  An event is INTERIOR when
 *       first >= skip_windows (the scan command passes scan_size / h: the windows classify itself
 *       looks at).  Events come back ordered by (read, first).
 *   Capacity.  The first max_events events are written; n_events reports the true total.
 * Events are integers and comparisons only: the result depends neither on the launch shape nor on
 * how the reads were split into chunks.
 *
 * The windows of a batch are numbered through: window_offsets [n_reads + 1] int64 is the exclusive
 * prefix of W over the reads (dbh_scan_window_offsets_dev), global window g of the batch is window
 * g - window_offsets[r] of the read r it falls into.  dbh_scan_windows_dev is the front alone, for
 * parity tests: x_dev [n_windows][input_size] fp32 for global windows [first_window, first_window
 * + n_windows), any even input_size from 96 to 16,384; a window outside the batch is all zeros.
 * dbh_scan_events_dev takes the track in global window order (best int32, margin fp64);
 * per_read_interior_dev (n_reads int32, may be NULL) gets each read's count of interior events,
 * counted whatever the capacity.  It owns a temporary block for the per-read counts, so unlike the
 * other _dev entries it returns when the events are written.
 * dbh_scan_i16: host buffers, blocks.  The windows go through the paths that take normalised
 * windows (what dbh_predict_dev launches) in chunks of at most 256 MiB of fp32 input - and, on a
 * persistent model, of at most dbh_model_set_host_group windows.  best_host / margin_host are
 * optional: the whole ragged track in global window order (the sum of W over the reads each); NULL
 * = not wanted.  events_host holds max_events entries (NULL with max_events == 0); *n_interior
 * counts the interior events, whatever the capacity.
 * Every entry checks its arguments before any device work and writes nothing on error: a null
 * model or pointer, n_reads < 0, a side that is neither DBH_SIDE_START nor DBH_SIDE_END,
 * min_windows < 1, skip_windows < 0, max_events < 0, first_window or n_windows < 0, offsets that
 * run backwards (host entry), an input_size that is odd or outside 96 .. 16,384:
 * DBH_ERR_INVALID_ARGUMENT.  n_reads == 0 is DBH_OK (the host entry then reports no events). */
typedef struct dbh_scan_event {
    int64_t read;
    int32_t cls, first, last, reserved;
    double peak;
} dbh_scan_event;
int dbh_scan_window_count(int input_size, int64_t n_samples, int64_t* count);
int dbh_scan_window_offsets_dev(const int64_t* offsets_dev, int64_t n_reads, int input_size,
                                int64_t* window_offsets_dev, dbh_stream stream);
int dbh_scan_windows_dev(const int16_t* samples_dev, const int64_t* offsets_dev,
                         const int64_t* window_offsets_dev, int64_t n_reads, int input_size,
                         int side, int64_t first_window, int64_t n_windows, float* x_dev,
                         dbh_stream stream);
int dbh_scan_events_dev(const int32_t* best_dev, const double* margin_dev,
                        const int64_t* window_offsets_dev, int64_t n_reads, double threshold,
                        int min_windows, int skip_windows, dbh_scan_event* events_dev,
                        int64_t max_events, int32_t* per_read_interior_dev, int64_t* n_events_dev,
                        dbh_stream stream);
int dbh_scan_i16(dbh_model* model, const int16_t* samples_host, const int64_t* offsets_host,
                 int64_t n_reads, int side, double threshold, int min_windows, int skip_windows,
                 int32_t* best_host, double* margin_host, dbh_scan_event* events_host,
                 int64_t max_events, int64_t* n_events, int64_t* n_interior);

/* ---- locate: where in the signal each barcode call comes from ---------------------------------- */
/* The network ends in conv1d_20 (1x1) -> ReLU -> global average -> softmax
 * (network_architecture.py:91-93), so a class's logit IS the mean, over the positions of stage 7, of
 * that class's post-ReLU conv1d_20 output.  Each position is one cell of 2^7 = 128 samples.  That
 * per-cell value is the class's EVIDENCE: a decomposition of the logit, not a heuristic.  It says
 * where the NETWORK sees the barcode; nothing here has been checked against where the barcode is
 * (whether the call DEPENDS on the located samples is what the occlude section below tests).
 *
 * L = the model's input size, h = L / 2, C its classes, cells = len7 = the positions of stage 7
 * ((L/2)/2/2/2/2, halved rounding up, halved again: 8 at L = 1024), a read has n samples.
 *   Windows.  call_batch's own, per side (classify.py:330-357): steps = scan_size / h.  Window s of
 *       side start begins at read sample o = s h; window s of side end at o = n - s h - L, which may
 *       be negative: the zero pad in front counts as window positions.
 *   Evidence.  e[p][c] = max(0, bias[c] + sum_ci BN7(G)[p][ci] * w20[ci][c]) for p in [0, cells), in
 *       the arithmetic and order of the general path's head; fp32 [window][cells][C], the windows
 *       [read][step].  The mean of e[.][c] over p is class c's logit.
 *   Cell.  Cell p of a window covers window positions [128 p, min(128 (p + 1), L)); in read samples
 *       that range shifted by o and clipped to [0, n).  Positions behind 128 cells belong to no cell
 *       (L = 160 has one cell: positions 128 .. 159 have none).
 *   Rule, per read and side, for the side's call c after merge and score_diff (what
 *       dbh_classify_i16 calls):
 *       c == 0 (or no class of the model): no location - cls 0, every other integer -1, the floats 0.
 *       The deciding window is the one with the largest max_p e[s][p][c], the lowest s among equals.
 *           (Not the window of the highest probability: the probabilities of two overlapping windows
 *           saturate, and rounding would decide.)
 *       The peak cell is the lowest p that holds the maximum.
 *       The span is the longest run of consecutive cells around the peak with e >= 0.5f * peak, an
 *           fp32 comparison (the halving is exact).
 *       share = the sum of e over the span / the sum over all cells of that window and class, both
 *           sums fp64 in cell order, the quotient rounded to float once; 0 where the sum is 0.
 *       All-zero evidence: window 0, peak cell 0, a span of every cell, share 0.
 *       A NaN never wins a '>' (and equals nothing): a NaN cell is never the peak and ends a span.
 *   Result.  dbh_location: samples are [first_sample, end_sample); where clipping empties the range,
 *       end_sample = first_sample.  reserved is 0.
 *
 * A model for locate is general-kind (DBH_MODEL_GENERAL), whatever its geometry: the general path
 * has stage G in memory.  dbh_evidence_floats, dbh_evidence_dev, dbh_locate_workspace_bytes and
 * dbh_locate_i16 on a persistent-kind model return DBH_ERR_UNSUPPORTED.
 * dbh_evidence_floats: cells * C, the evidence floats of one window.
 * dbh_evidence_dev is dbh_predict_dev's twin: x_dev [n_windows][L] -> probs_dev [n_windows][C] and
 * evidence_dev [n_windows][cells][C].  The probabilities are bit-identical to dbh_predict_dev's, and
 * windows cross the chunks of the layer chain exactly as they do there.
 * dbh_locate_dev applies the rule: evidence_dev [n_reads][steps][cells][C], calls_dev int32
 * [n_reads], offsets_dev int64 [n_reads + 1] (the reads' sample offsets; only their differences are
 * read) -> locations_dev [n_reads].  No allocation, no synchronisation.  dbh_locate_host takes the
 * same arguments as host pointers and is the CPU model of the kernel: the same lines, bit for bit.
 * dbh_locate_i16: host buffers, blocks - the whole route: slice, forward with evidence, merge and
 * call (as dbh_classify_i16 on the same model), then the rule.  probs_host [n_reads][C], calls_host
 * and locations_host [n_reads].  Reads go through in groups whose windows fit one chunk of the layer
 * chain; a read's results come from its own windows alone and do not depend on the grouping.
 * dbh_locate_workspace_bytes: the device bytes of one such group - per-window probabilities,
 * evidence, activations - which the groups of a call share (the samples, the offsets and the
 * results of every read come on top).
 * Every entry checks its arguments before any device work and writes nothing on error: a null model
 * or pointer, n_reads < 0, steps < 1, cells that are not the cells of input_size, a geometry outside
 * dbh_model_create_ex's, a side that is neither DBH_SIDE_START nor DBH_SIDE_END, a scan_size that is
 * no positive multiple of h, offsets that run backwards (host entries): DBH_ERR_INVALID_ARGUMENT.
 * n_reads == 0 is DBH_OK. */
typedef struct dbh_location {
    int32_t cls, window, peak_cell, first_cell, last_cell;
    float peak, share;
    int32_t reserved;
    int64_t first_sample, end_sample;
} dbh_location;
int dbh_evidence_floats(const dbh_model* model, int64_t* per_window);
int dbh_evidence_dev(dbh_model* model, const float* x_dev, int64_t n_windows, float* probs_dev,
                     float* evidence_dev, dbh_stream stream);
int dbh_locate_dev(const float* evidence_dev, const int32_t* calls_dev, const int64_t* offsets_dev,
                   int64_t n_reads, int steps, int cells, int n_classes, int input_size, int side,
                   dbh_location* locations_dev, dbh_stream stream);
int dbh_locate_host(const float* evidence_host, const int32_t* calls_host,
                    const int64_t* offsets_host, int64_t n_reads, int steps, int cells,
                    int n_classes, int input_size, int side, dbh_location* locations_host);
int dbh_locate_workspace_bytes(const dbh_model* model, int64_t n_reads, int scan_size,
                               size_t* bytes);
int dbh_locate_i16(dbh_model* model, const int16_t* samples_host, const int64_t* offsets_host,
                   int64_t n_reads, int side, int scan_size, double score_diff, float* probs_host,
                   int32_t* calls_host, dbh_location* locations_host);

/* ---- occlude: blank the located span and call the read again ----------------------------------- */
/* A location says where the network looks; it does not say that the call DEPENDS on those samples.
 * The faithfulness test of an attribution: take the located samples away and see whether the call
 * goes, take away everything else and see whether it stays, take away an equally long stretch
 * elsewhere and see that nothing happens.  "Away" is 0.0f: what the zero pad of a short window is
 * after normalisation (classify.py:330-357), the window's mean - a value the network was trained
 * on.  This tests the attribution against the MODEL, still not against where the barcode is.
 *
 * L, h, n as in the locate section.  Per read and side, after dbh_locate_i16's own pass, for a side
 * whose location has cls = c > 0 and span [first_sample, end_sample) of m > 0 read samples:
 *   Scanned region R.  The read samples the side's `steps` windows cover:
 *       side start: [0, min(n, (steps - 1) h + L));  side end: [max(0, n - (steps - 1) h - L), n).
 *       (A span given from outside is first held to R; dbh_locate_dev's lies inside it.)
 *   Variant.  The side's same `steps` windows, sliced and normalised exactly as for the unblanked
 *       pass, with the statistics of the unblanked samples; then every window position whose read
 *       sample (o + position, o the window's origin of the locate section) lies in the blank set B
 *       is stored as 0.0f.  Pad positions are 0 already.  Nothing is renormalised.
 *       DBH_OCCLUDE_OUT:  B = the span.
 *       DBH_OCCLUDE_ONLY: B = R minus the span.
 *       DBH_OCCLUDE_CTRL: B = a control stretch of m samples: the last m samples of R if the span's
 *           midpoint lies below R's (first_sample + end_sample < R.lo + R.hi, the doubled integers),
 *           otherwise the first m.  If the control stretch overlaps the span there is no control.
 *   Result per variant.  The variant's windows go through the same forward, merge and call as the
 *       unblanked pass: call_v, and p_v = class c's merged, normalised probability - c the
 *       UNBLANKED call, not the variant's.
 *   No result.  A side without a location, m == 0 after clipping (all three variants), or a missing
 *       control (DBH_OCCLUDE_CTRL alone): call = -1, p = NaN, control samples -1, -1.
 *   Record.  dbh_occlusion, 64 bytes: cls (0: no location) and p, class c's probability in the
 *       unblanked pass (NaN where cls == 0); variant[v] = (call_v, p_v); [ctrl_first, ctrl_end) the
 *       control stretch; reserved is 0.
 *   Plan.  dbh_occlude_plan, 64 bytes, what the window kernel reads: per variant an interval
 *       [first[v], end[v]) of read samples, bit v of `invert` set where the variant blanks the read's
 *       samples OUTSIDE its interval (DBH_OCCLUDE_ONLY: the read samples of a window all lie in R),
 *       bit v of `valid` set where the variant has a result.  A variant without a result has an
 *       empty interval and no invert bit: its windows are copies.
 *
 * dbh_occlude_plan_dev / _host: locations [n_reads], offsets int64 [n_reads + 1] (only their
 * differences are read) -> plans [n_reads] and occlusions [n_reads] with cls, the control samples
 * and every "no result" field written (p and the variants of a result are NaN / -1 until the route
 * fills them).  dbh_occlude_windows_dev / _host: x [n_reads][steps][L] normalised windows, offsets,
 * plans -> variants [3][n_reads][steps][L].  Copies and zeros: the _host entries are the CPU models
 * of the kernels, the same lines, bit for bit.  The _dev entries queue and return; no allocation,
 * no synchronisation; pointers need the alignment of their element type only, and x and the
 * variants must not overlap.
 * dbh_locate_occluded_i16: dbh_locate_i16 with the three variant passes added per group: the
 * group's windows are sliced and normalised once, and the four passes follow each other through
 * the group's one workspace.  probs_host, calls_host and locations_host are dbh_locate_i16's to the
 * bit; occlusions_host [n_reads].  No result depends on the grouping.
 * dbh_locate_occluded_workspace_bytes: dbh_locate_workspace_bytes plus the group's four sets of
 * windows, three sets of merged probabilities and calls, and its plans.
 * The entries that take a model are general-kind only (DBH_ERR_UNSUPPORTED otherwise), as locate's.
 * Every entry checks its arguments before any device work and writes nothing on error: a null model
 * or pointer, n_reads < 0, steps < 1, steps * L above 2^30, an input_size that is odd or outside
 * 96 .. 16,384, a side that is neither DBH_SIDE_START nor DBH_SIDE_END, a scan_size that is no
 * positive multiple of h, offsets that run backwards (host entries): DBH_ERR_INVALID_ARGUMENT.
 * n_reads == 0 is DBH_OK. */
#define DBH_OCCLUDE_OUT 0
#define DBH_OCCLUDE_ONLY 1
#define DBH_OCCLUDE_CTRL 2
typedef struct dbh_occlude_plan {
    int64_t first[3], end[3];
    int32_t invert, valid;
    int64_t reserved;
} dbh_occlude_plan;
typedef struct dbh_occlusion_result {
    int32_t call;
    float p;
} dbh_occlusion_result;
typedef struct dbh_occlusion {
    int32_t cls;
    float p;
    dbh_occlusion_result variant[3];
    int64_t ctrl_first, ctrl_end;
    int64_t reserved[2];
} dbh_occlusion;
int dbh_occlude_plan_dev(const dbh_location* locations_dev, const int64_t* offsets_dev,
                         int64_t n_reads, int steps, int input_size, int side,
                         dbh_occlude_plan* plans_dev, dbh_occlusion* occlusions_dev,
                         dbh_stream stream);
int dbh_occlude_plan_host(const dbh_location* locations_host, const int64_t* offsets_host,
                          int64_t n_reads, int steps, int input_size, int side,
                          dbh_occlude_plan* plans_host, dbh_occlusion* occlusions_host);
int dbh_occlude_windows_dev(const float* x_dev, const int64_t* offsets_dev,
                            const dbh_occlude_plan* plans_dev, int64_t n_reads, int steps,
                            int input_size, int side, float* variants_dev, dbh_stream stream);
int dbh_occlude_windows_host(const float* x_host, const int64_t* offsets_host,
                             const dbh_occlude_plan* plans_host, int64_t n_reads, int steps,
                             int input_size, int side, float* variants_host);
int dbh_locate_occluded_workspace_bytes(const dbh_model* model, int64_t n_reads, int scan_size,
                                        size_t* bytes);
int dbh_locate_occluded_i16(dbh_model* model, const int16_t* samples_host,
                            const int64_t* offsets_host, int64_t n_reads, int side, int scan_size,
                            double score_diff, float* probs_host, int32_t* calls_host,
                            dbh_location* locations_host, dbh_occlusion* occlusions_host);

/* ---- live: each read's barcode called while its signal arrives --------------------------------- */
/* Every entry above takes whole reads.  A live session keeps, per sequencer channel, the signal
 * received so far and the fold over the windows that are already complete, so a caller can act on a
 * barcode while the molecule is still in the pore.  Window s of the start side is the same samples
 * whatever comes after it (classify.py:337-349) and the merge is a running min / max
 * (classify.py:368-374), so the merged vector after k windows is what a run at scan_size = k h
 * merges ("sweep", above): the session is that fold, stopped after the windows a push made ready
 * and taken up again at the next.  Checked against the network's answers on prefixes of recorded
 * reads, not on a sequencer; an early call can differ from the final one by construction.
 *
 * L = the model's input size, h = L / 2, steps = scan_size / h, cap = scan_size + h (the last
 * window ends at (steps - 1) h + L = cap).
 *   Session.  One model (persistent or general kind), side start only, 1 <= n_channels <= 16,384,
 *       scan_size a positive multiple of h, 1 <= min_windows <= steps, flags 0 or
 *       DBH_LIVE_STOP_ON_DECISION.  max_round_windows: how many windows one forward round holds,
 *       0 = 64 MiB of fp32 input.  The session owns a stream, its device state and pinned memory.
 *   State per channel, on the device: cap int16 samples; n, every sample received, kept or not;
 *       open, ended, windows_done; the merged fp32 vector; the track best[steps] int32 and
 *       margin[steps] fp64; the decision.
 *   Push.  n_chunks chunks, chunk i for channels[i] (each channel at most once per push) with the
 *       samples [offsets[i], offsets[i + 1]) and flags[i] of DBH_LIVE_BEGIN | DBH_LIVE_END.  Per
 *       chunk, in this order: BEGIN resets the channel and opens a read; the samples are appended
 *       (n grows by the chunk's length, samples are stored only up to cap); END sets ended and
 *       closes the read.  A chunk for a channel with no read open and no BEGIN changes nothing and
 *       reports DBH_LIVE_IDLE.  A channel that is FINAL, or DECIDED under STOP_ON_DECISION, counts
 *       n on but stores and runs nothing more.
 *   Ready.  Window k < steps is ready when k h + L <= n, or when the read has ended (then every
 *       k < steps is: call_batch's short and empty windows).  Its samples are
 *       [min(k h, n), min(k h + L, n)), normalised over the samples present by the scan's front
 *       rule ("scan", above: int64 S and Q, exact D, one fp64 expression per value) and
 *       zero-padded behind.  The windows a push made ready, windows_done .. ready - 1 per channel,
 *       go through what dbh_predict_dev launches, in rounds of at most max_round_windows, and are
 *       folded in order of k: the sweep's fold step, in the form of the model's kind.  (best,
 *       margin) after each window goes into the track.
 *   Decision.  The first k with k + 1 >= min_windows && best != 0 && margin >= score_diff decides:
 *       call = that best, decided_windows = k + 1, decided_samples = n; the call never changes.
 *       Under STOP_ON_DECISION the fold stops behind that window.  windows_done == steps makes the
 *       channel FINAL with final_call = best != 0 && margin >= score_diff ? best : 0.
 *   Result.  dbh_live_result, 48 bytes, one per chunk: the channel's record behind the push (for an
 *       IDLE chunk the record as it stands, with status DBH_LIVE_IDLE).
 * dbh_live_push takes host buffers and blocks once, at its end.  dbh_live_track copies a channel's
 * track to the host (best / margin hold steps entries; *windows of them are valid).
 * dbh_live_fold_dev is the resumable fold alone, for parity tests: window_probs_dev
 * [window_offsets[n_channels]][n_classes] fp32 holds, for channel i, the windows
 * [window_offsets_dev[i], window_offsets_dev[i + 1]) (int64, on the device) that come next;
 * merged_dev [n_channels][n_classes] and state_dev [n_channels] (windows = done, samples as the
 * caller has them) go in and out, best_dev / margin_dev [n_channels][steps] get the new entries.
 * dbh_live_plan_host runs ONE channel's rules on the host (dbh_live_core.h, what the kernels
 * compile): n_chunks pushes of lengths[i] samples with chunk_flags[i], window k folding to
 * (track_best[k], track_margin[k]) -> results_host[i], the record behind push i, and
 * new_windows_host[i] (may be NULL), the windows that push made ready.
 *
 * Pair sessions: the read's full call when it ends.  At the push that carries DBH_LIVE_END the end
 * of the read is known, and the session gives what classify gives: the end model over the last
 * scan_size samples (call_batch with side == 'end', classify.py:343-357) and combine_calls
 * (classify.py:298-322) of the two sides.  _e marks the end model's L, h, steps and cap.
 *   Session.  dbh_live_create_pair: a start and an end model under the pair conditions of
 *       dbh_classify_pair_i16 - both non-NULL here, one device, equal n_classes - of either kind
 *       each; scan_size a positive multiple of h and of h_e; combine_mode one of DBH_REQUIRE_*.
 *       The other arguments and the whole start side are dbh_live_create's.
 *   Tail ring.  cap_e more int16 samples per channel: sample p of a read, counted from BEGIN,
 *       lives at ring[p % cap_e].  A chunk of `length` samples arriving at n stores its last
 *       min(length, cap_e).  Every chunk of an open read stores, also once the start side is FINAL
 *       or stopped on a decision; BEGIN resets nothing in the ring - a read's windows read
 *       positions [max(n - cap_e, 0), n) only, all written by this read.
 *   End windows.  At END, n final, window s = 0 .. steps_e - 1 in this order: samples [a, b) with
 *       a = max(n - (s h_e + L_e), 0), b = max(n - s h_e, 0), m = b - a, read out of the ring
 *       through the wrap, normalised over the m samples present by the scan's front rule, the
 *       values at out[L_e - m .. L_e), zeros in front.  They go through what dbh_predict_dev
 *       launches for the end model, in rounds of at most max_round_windows, and through the same
 *       fold from a fresh record into the end track best[steps_e], margin[steps_e].
 *   End record.  dbh_live_end_result, 40 bytes, one per chunk: IDLE with -1 calls before any read;
 *       PENDING with -1 calls from BEGIN on; behind END status FINAL, end_call = the end track's
 *       last best if it is a barcode leading by score_diff, else 0; start_call = the start
 *       record's final_call if it is FINAL, else its call (the early call of a read stopped on a
 *       decision); read_call = combine_calls(start_call, end_call) under combine_mode.  An IDLE
 *       chunk reports the channel's record as it stands with status DBH_LIVE_IDLE.
 * dbh_live_push_pair is dbh_live_push with the end records beside the start records; end_results
 * may be NULL, and dbh_live_push on a pair session is that: the end side still runs, and its record
 * is read with the channel's next push or through dbh_live_end_track (best / margin hold steps_e
 * entries; *windows is steps_e behind END, 0 from BEGIN until then).  A push in which no chunk
 * carries END launches the kernels of a start-only push, no more; still one synchronise per push.
 * On a session made by dbh_live_create, dbh_live_push_pair with end_results and dbh_live_end_track
 * are DBH_ERR_INVALID_ARGUMENT.
 * dbh_live_tail_plan_host runs ONE channel's ring and end-window rules on the host
 * (dbh_live_core.h), as dbh_live_plan_host does the start side's: for n_chunks pushes of lengths[i]
 * samples with chunk_flags[i] -> store_host[i][4] = (from, keep, at, head): the chunk's samples
 * [from, from + keep) go to ring[at ..], head of them before the wrap (zeros for an IDLE chunk);
 * samples_host[i] = n behind the chunk; ends_host[i] = 1 where the chunk ended an open read, and
 * there windows_host[i][s][4] = (a, m, pad, ring index of a) of end window s (other chunks' entries
 * are left alone).
 *
 * Every entry checks its arguments before any device work and changes no state on error: a null
 * pointer, n_chunks < 0, a channel outside the session or twice in one push, offsets that run
 * backwards, unknown flag bits, the limits of creation, a policy outside its limits, set twice or
 * behind a push, a negative yield (the policy entries are declared further down):
 * DBH_ERR_INVALID_ARGUMENT.  n_chunks == 0 is DBH_OK. */
typedef struct dbh_live_session dbh_live_session;
#define DBH_LIVE_STOP_ON_DECISION 1      /* session flag */
#define DBH_LIVE_BEGIN 1                 /* chunk flags */
#define DBH_LIVE_END 2
#define DBH_LIVE_IDLE 0                  /* status */
#define DBH_LIVE_PENDING 1
#define DBH_LIVE_DECIDED 2
#define DBH_LIVE_FINAL 3
#define DBH_LIVE_MAX_CHANNELS 16384
typedef struct dbh_live_result {
    int32_t status;             /* DBH_LIVE_IDLE .. DBH_LIVE_FINAL */
    int32_t call;               /* 0 until decided */
    int32_t final_call;         /* -1 until FINAL */
    int32_t windows;            /* windows folded: windows_done */
    int32_t decided_windows;    /* 0 until decided */
    int32_t best;               /* of the last window folded */
    double margin;              /* of the last window folded */
    int64_t samples;            /* n */
    int64_t decided_samples;    /* n at the push that decided */
} dbh_live_result;
int dbh_live_create(dbh_model* model, int n_channels, int scan_size, double score_diff,
                    int min_windows, uint32_t flags, int64_t max_round_windows,
                    dbh_live_session** session);
int dbh_live_destroy(dbh_live_session* session);
int dbh_live_push(dbh_live_session* session, const int32_t* channels, const int64_t* offsets,
                  const int16_t* samples, const uint32_t* flags, dbh_live_result* results,
                  int64_t n_chunks);
int dbh_live_track(dbh_live_session* session, int channel, int32_t* best, double* margin,
                   int32_t* windows);
int dbh_live_fold_dev(const dbh_model* model, const float* window_probs_dev,
                      const int64_t* window_offsets_dev, int64_t n_channels, int64_t n_windows,
                      int steps, double score_diff, int min_windows, uint32_t flags,
                      float* merged_dev, dbh_live_result* state_dev, int32_t* best_dev,
                      double* margin_dev, dbh_stream stream);
int dbh_live_plan_host(int input_size, int scan_size, double score_diff, int min_windows,
                       uint32_t flags, const int64_t* lengths, const uint32_t* chunk_flags,
                       int64_t n_chunks, const int32_t* track_best, const double* track_margin,
                       dbh_live_result* results_host, int32_t* new_windows_host);
typedef struct dbh_live_end_result {
    int32_t status;             /* DBH_LIVE_IDLE; DBH_LIVE_PENDING until END; DBH_LIVE_FINAL behind it */
    int32_t end_call;           /* -1 until END */
    int32_t start_call;         /* -1 until END: what went into combine_calls */
    int32_t read_call;          /* -1 until END */
    int32_t end_best;           /* of the last end window folded */
    int32_t end_windows;        /* 0, or steps_e behind END */
    double end_margin;          /* of the last end window folded */
    int64_t samples;            /* n */
} dbh_live_end_result;
int dbh_live_create_pair(dbh_model* start_model, dbh_model* end_model, int n_channels,
                         int scan_size, double score_diff, int min_windows, uint32_t flags,
                         int combine_mode, int64_t max_round_windows, dbh_live_session** session);
int dbh_live_push_pair(dbh_live_session* session, const int32_t* channels, const int64_t* offsets,
                       const int16_t* samples, const uint32_t* flags, dbh_live_result* results,
                       dbh_live_end_result* end_results, int64_t n_chunks);
int dbh_live_end_track(dbh_live_session* session, int channel, int32_t* best, double* margin,
                       int32_t* windows);
int dbh_live_tail_plan_host(int end_input_size, int scan_size, const int64_t* lengths,
                            const uint32_t* chunk_flags, int64_t n_chunks, int64_t* store_host,
                            int64_t* samples_host, int32_t* ends_host, int64_t* windows_host);
/* Yield policies: what to do with the read.  A session with a policy keeps, on the device, how many
 * samples and reads each barcode has yielded so far, and gives with every push an action per chunk:
 * keep the read or eject it.  Integers only (dbh_live_core.h: policy_ok, yield_class, level_of,
 * action_of - the lines the two kernels, the session's host code, dbh_live_policy_plan_host and
 * live_model_check.cpp compile).  A simulation's building block: checked on recorded reads, not on
 * a sequencer.
 *   Policy.  Fixed by dbh_live_set_policy, allowed once, before the first push, on a start-only or
 *       a pair session: int32 weights[n_classes] (n_classes the model's), int64 slack_samples >= 0,
 *       undecided_action DBH_LIVE_ACTION_KEEP or _EJECT.  weight -1: the barcode is always kept and
 *       does not enter the balance; 0: always ejected; 1 .. 1 << 20: balanced with that share.
 *       weights[0] must be -1 (class 0 is never a decided call).
 *   State.  Session: yield_samples[n_classes], yield_reads[n_classes], int64, zero at creation.
 *       Channel: action, int32, NONE from BEGIN on, set once, standing until the next BEGIN.
 *   Per push, behind the last fold, in this order:
 *       1. Yield.  Every chunk that carried END on an open read adds its record's samples to
 *          yield_samples[record.call] and 1 to yield_reads[record.call] (call is 0 until decided).
 *          All ENDs of a push are added before any action of the push is taken.
 *       2. Level.  level[c] = yield_samples[c] / weights[c] (int64, floor) where weights[c] >= 1;
 *          floor = the lowest of these levels, 0 if no class is balanced.
 *       3. Action, for every chunk that is not IDLE and whose channel's action is NONE: a decided
 *          record (decided_windows > 0) with call c gets KEEP (WEIGHT_KEEP) for weight -1, EJECT
 *          (WEIGHT_EJECT) for weight 0, EJECT (OVER_LEVEL) if level[c] - floor > slack_samples,
 *          else KEEP (BALANCED); a record that is FINAL and undecided gets undecided_action
 *          (UNDECIDED); any other stays NONE.
 *       The action changes nothing else: records, end records and tracks are byte for byte those
 *       of the same pushes through a session without a policy.  The caller acts on EJECT; the read
 *       ends when it ends, and yield counts what arrived.
 *   Action record.  dbh_live_action, 32 bytes, one per chunk.  Where the push took the action:
 *       action, reason, klass = the call acted on (0 for UNDECIDED), level = level[klass] (0 where
 *       klass is not balanced) and floor, both as the decision saw them.  Else - an IDLE chunk, a
 *       channel whose action already stands, a read not yet decided - action = the channel's
 *       action as it stands and every other field 0.
 * dbh_live_push_policy is dbh_live_push_pair with `actions` beside the records; end_results is NULL
 * on a start-only session (and may be on a pair session).  dbh_live_push and dbh_live_push_pair on
 * a policy session still run the policy: the action is then read with the channel's next push.  A
 * policy push adds two kernel launches and one download to the push and still synchronises once.
 * On a session without a policy dbh_live_push_policy is DBH_ERR_INVALID_ARGUMENT, and such a
 * session launches what it launched before.
 * dbh_live_yield copies the two yield arrays to the host (either may be NULL); dbh_live_set_yield
 * seeds them (both non-NULL, no negative value): resuming a run, or yield from before the session.
 * dbh_live_policy_dev is the two kernels alone on the caller's device arrays, for parity tests:
 * records_dev [n_chunks] as a push's results hold them (status IDLE = an idle chunk), uint32
 * chunk_flags_dev and int32 channels_dev [n_chunks] (each channel at most once, every one an index
 * into channel_action_dev), int32 weights_dev [n_classes]; yield_samples_dev / yield_reads_dev
 * [n_classes] and channel_action_dev go in and out, actions_dev [n_chunks] comes out.  A chunk
 * whose flags carry BEGIN starts from action NONE.  0 <= n_chunks <= 16,384, 1 <= n_classes <= 256.
 * dbh_live_policy_plan_host runs the same rules on the host over n_pushes pushes:
 * push p holds chunks [push_offsets[p], push_offsets[p + 1]) of channels_host / chunk_flags_host /
 * records_host; channel_action_host [n_channels] and the two yield arrays go in and out (seed them
 * with zeros for a fresh session), actions_host gets one record per chunk; yield_trace_host (may be
 * NULL) gets [n_pushes][2][n_classes]: yield_samples, then yield_reads, behind each push. */
#define DBH_LIVE_ACTION_NONE 0
#define DBH_LIVE_ACTION_KEEP 1
#define DBH_LIVE_ACTION_EJECT 2
#define DBH_LIVE_REASON_NONE 0
#define DBH_LIVE_REASON_WEIGHT_KEEP 1
#define DBH_LIVE_REASON_BALANCED 2
#define DBH_LIVE_REASON_WEIGHT_EJECT 3
#define DBH_LIVE_REASON_OVER_LEVEL 4
#define DBH_LIVE_REASON_UNDECIDED 5
#define DBH_LIVE_MAX_WEIGHT (1 << 20)
typedef struct dbh_live_action {   /* 32 bytes */
    int32_t action;                /* DBH_LIVE_ACTION_NONE 0, _KEEP 1, _EJECT 2 */
    int32_t reason;                /* DBH_LIVE_REASON_* */
    int32_t klass;                 /* the call acted on, 0 for UNDECIDED / NONE */
    int32_t reserved;              /* 0 */
    int64_t level;                 /* level[klass] at the decision, 0 where not balanced */
    int64_t floor;                 /* at the decision */
} dbh_live_action;
int dbh_live_set_policy(dbh_live_session* session, const int32_t* weights, int n_classes,
                        int64_t slack_samples, int undecided_action);
int dbh_live_push_policy(dbh_live_session* session, const int32_t* channels, const int64_t* offsets,
                         const int16_t* samples, const uint32_t* flags, dbh_live_result* results,
                         dbh_live_end_result* end_results, dbh_live_action* actions,
                         int64_t n_chunks);
int dbh_live_yield(dbh_live_session* session, int64_t* samples_host, int64_t* reads_host);
int dbh_live_set_yield(dbh_live_session* session, const int64_t* samples_host,
                       const int64_t* reads_host);
int dbh_live_policy_dev(const dbh_live_result* records_dev, const uint32_t* chunk_flags_dev,
                        const int32_t* channels_dev, int64_t n_chunks, const int32_t* weights_dev,
                        int n_classes, int64_t slack_samples, int undecided_action,
                        int64_t* yield_samples_dev, int64_t* yield_reads_dev,
                        int32_t* channel_action_dev, dbh_live_action* actions_dev,
                        dbh_stream stream);
int dbh_live_policy_plan_host(const int32_t* weights, int n_classes, int64_t slack_samples,
                              int undecided_action, const int64_t* push_offsets, int64_t n_pushes,
                              const int32_t* channels_host, const uint32_t* chunk_flags_host,
                              const dbh_live_result* records_host, int n_channels,
                              int32_t* channel_action_host, int64_t* yield_samples_host,
                              int64_t* yield_reads_host, dbh_live_action* actions_host,
                              int64_t* yield_trace_host);

/* ---- compressed input: the Signal chunks of fast5 files, inflated on the GPU ---------------- */
/* The reference reads `Signal[:]` through h5py (load_fast5s.py:33-43): libhdf5 runs zlib's
 * inflate() over every chunk on the host.  Here the loader may hand over the chunks AS STORED
 * (zlib streams, RFC 1950/1951: the HDF5 "deflate" filter) and the GPU inflates them - thousands
 * of streams side by side, bit-exact with zlib, same accept / reject decisions (tests/
 * test_inflate.py).  A stream is described by where its bytes lie in the compressed buffer and
 * where its output goes in the output buffer; out_bytes is how much of its output is wanted: a
 * stream that holds more is cut there (a partial last chunk), one that ends earlier is
 * zero-extended (MinKNOW's short final chunk, as libhdf5 does it).  DBH_INFLATE_STORED: the
 * bytes are the data itself (an unfiltered chunk, or what the host inflated for the filters the
 * GPU does not do) - copied, zero-extended.  DBH_INFLATE_VBZ: a chunk of ONT's VBZ filter (HDF5
 * filter 32020, version 0) with its zstd stage undone - u32 LE original_size, then the
 * streamvbyte bytes ("VBZ") - unpacked, un-zigzagged and summed into int16 samples by a
 * kernel of its own (dbh_vbz.hip, one wave per stream) in the same call; cut / zero-extended to
 * out_bytes like the others; a stream whose data do not end exactly where it does, or whose
 * original_size is odd, is refused (status != 0, output zeros).
 * status per stream: 0 = ok; anything else = damaged or beyond this decoder (its output is then
 * all zeros): the caller decodes that stream on the host if it wants the verdict of zlib itself.
 * The compressed buffer must be readable for 64 bytes beyond its end (the decoder fetches ahead).
 * Output regions must not overlap; out_offset must be even (samples are int16). */
#define DBH_INFLATE_ZLIB 0
#define DBH_INFLATE_STORED 1
#define DBH_INFLATE_VBZ 2
/* DBH_INFLATE_VBZ_ZSTD: a VBZ chunk as the filter stored it - u32 LE original_size, then the zstd
 * frame (RFC 8878) of the streamvbyte bytes.  A kernel of its own (dbh_zstd.hip, one wave per
 * frame; what it decodes and what it refuses: dbh_zstd_core.h) writes the frame's content into the
 * stream's own slots of the workspace (4 * out_bytes bytes), and the DBH_INFLATE_VBZ kernel reads
 * it from there, with all its self-checks and the same cut / zero-extend rules.  A frame whose
 * content does not fit the slots is refused: none is whose out_bytes covers its original_size.
 * Refused by either stage: status != 0 (16..28: the zstd stage's reason), output zeros. */
#define DBH_INFLATE_VBZ_ZSTD 3
/* HDF5's shuffle filter (filter 2) for int16: the N bytes of a chunk stored as its N/2 low bytes,
 * then its N/2 high bytes - byte j of element i at j * (N/2) + i.  Both modes carry a 4-byte prefix
 * in front of the chunk's bytes, as VBZ does: u32 LE N, the size of the shuffled content.
 * DBH_INFLATE_ZLIB_SHUFFLE: the prefix, then a zlib stream whose content is the N shuffled bytes
 * (the pipeline shuffle + deflate).  The inflate kernels decode it as the DBH_INFLATE_ZLIB stream
 * of comp_bytes - 4 bytes at comp_offset + 4, wanted N, into the stream's own output region; a
 * wave of the kernel behind them (dbh_vbz.hip) copies the N bytes to the stream's slots of the
 * workspace and writes them back de-interleaved: N/2 samples, zeros from N to out_bytes.  Accepted
 * when N is even, 0 <= N <= out_bytes, and the deflate data ENDED with exactly N bytes (the
 * Adler-32 is then checked as for any stream that ends): a stream that holds more or fewer bytes
 * cannot be unshuffled - where its halves meet is unknown.
 * DBH_INFLATE_STORED_SHUFFLE: the prefix, then the N shuffled bytes themselves (comp_bytes == 4 + N,
 * N even).  Sample i is (c[i], c[N/2 + i]) for 2 i < min(N, out_bytes), zeros behind: any
 * out_bytes is taken.
 * Refused: status DBH_INFLATE_SHUFFLE_REFUSED, output zeros - unless the zlib stage has set a
 * status of its own (1..10), which stays. */
#define DBH_INFLATE_ZLIB_SHUFFLE 4
#define DBH_INFLATE_STORED_SHUFFLE 5
#define DBH_INFLATE_SHUFFLE_REFUSED 32
/* the GPU's zstd decoder run on the host: same core, lanes as a loop (tests, tools).  frame must
 * be readable for 64 bytes beyond frame_bytes.  Returns 0 unless an argument is null; *status: 0,
 * or why the frame is refused (16..28, dbh_zstd_core.h), *produced: the content size, 0 if refused. */
int dbh_zstd_decode_host(const uint8_t* frame, size_t frame_bytes, uint8_t* out,
                         size_t out_capacity, size_t* produced, int32_t* status);
/* A row of a POD5 signal table (a `minknow.vbz` value): "svb16", the 16-bit
 * streamvbyte code - ceil(n/8) key bytes, bit i & 7 of key byte i >> 3 (low bit first) saying
 * whether value i takes one byte (0) or two, little-endian (1), then the data bytes;
 * v -> (v >> 1) ^ (0 - (v & 1)) in 16 bits, sample i the sum of values 0..i modulo 2^16 as int16.
 * DBH_INFLATE_SVB16: u32 LE original_size (= 2 n) in front, as DBH_INFLATE_VBZ has, then the
 * svb16 stream (the zstd frame undone by the host) - n int16 at out_offset, cut or zero-extended
 * to out_bytes as the other modes are (an odd out_bytes: whole samples, then one zero byte),
 * decoded by a sibling of the VBZ wave in the same kernel
 * (dbh_vbz.hip: svb16_stream; the rules: csrc/dbh_svb16_core.h).  Refused (status 1, output all
 * zeros, neighbours untouched): comp_bytes < 4, an odd original_size, key bytes beyond the
 * stream, data that would run past its end or that end before it; an output region outside the
 * buffer is not written at all.  The unused bits of the last key byte are not looked at.  Reads
 * stay inside the stream plus 7 bytes.
 * DBH_INFLATE_SVB16_ZSTD: the same prefix, then the zstd frame as the file stores it.  The zstd
 * kernel writes the frame's content into the stream's workspace slots (4 * out_bytes bytes, which
 * cover ceil(n/8) + 2 n whenever out_bytes >= 2 n), the svb16 stage reads it from there; a zstd
 * refusal keeps its own status (16..28), as in DBH_INFLATE_VBZ_ZSTD. */
#define DBH_INFLATE_SVB16 6
#define DBH_INFLATE_SVB16_ZSTD 7
/* the GPU's svb16 decoder run on the host: same core, lanes as a loop (tests, tools).  stream:
 * exactly stream_bytes readable bytes holding the svb16 stream of n values (no prefix); out: n
 * samples.  Returns 0 unless an argument is null or n < 0; *status: 0, or 1 if the stream is
 * refused (out is then all zeros). */
int dbh_svb16_decode_host(const uint8_t* stream, size_t stream_bytes, int64_t n, int16_t* out,
                          int32_t* status);
typedef struct dbh_inflate_stream {
    int64_t comp_offset, comp_bytes;       /* the stream inside the compressed buffer           */
    int64_t out_offset, out_bytes;         /* its output inside the output buffer (bytes)       */
    int32_t mode, reserved;
} dbh_inflate_stream;
const char* dbh_inflate_last_error(void);
/* total_out_bytes = size of the output buffer the streams write into */
int dbh_inflate_workspace_bytes(int64_t total_out_bytes, int64_t n_streams, size_t* bytes);
/* comp_bytes = size of the compressed buffer (the decoder's read-ahead stops 64 bytes behind it).
 * Kernel 1 (Huffman codes -> tokens) gives every stream a wavefront of its own, in the order of
 * the records (the longest first, if the caller can: the launch then ends evenly).
 * streams_per_lane belonged to a retired form of kernel 1: it must be >= 0 and is otherwise ignored.
 * Kernel 2 (tokens -> bytes) reads the output buffer it writes (a match whose source lies more
 * than 8 KiB back is copied from the stream's own flushed output): out_dev must not be mapped
 * write-combined or read-protected.  The two kernels run as ONE launch, a pair of waves per
 * stream, kernel 2 resolving a stream's tokens while kernel 1 still decodes it
 * (DEEPBINNER_INFLATE_PAIR=0: two launches).  The environment variables DEEPBINNER_INFLATE_KERNEL
 * and DEEPBINNER_INFLATE_RESOLVE selected retired forms of the kernels and are no longer read. */
int dbh_inflate_dev(const uint8_t* comp_dev, int64_t comp_bytes,
                    const dbh_inflate_stream* streams_dev, int64_t n_streams,
                    int64_t total_out_bytes, uint8_t* out_dev, void* workspace_dev,
                    int32_t* status_dev, int streams_per_lane, dbh_stream stream);
/* host buffers in, host buffers out (tests, tools); kernel_ms (may be NULL): the two kernels */
int dbh_inflate(const uint8_t* comp_host, size_t comp_bytes, const dbh_inflate_stream* streams_host,
                int64_t n_streams, uint8_t* out_host, size_t out_bytes, int32_t* status_host,
                int streams_per_lane, double* kernel_ms);

/* The whole of a batch from stored chunks to barcode calls in one call: upload of the compressed
 * bytes (in place if they are pinned: the native loader's raw batches are), inflate, the start
 * model over the first and the end model over the last scan_size samples of every read,
 * combine_calls - dbh_classify_pair_i16 for reads that are still deflated.  offsets_host (n_reads
 * + 1, in samples, starting at 0): where each read's signal lies once decoded; the streams'
 * out_offset / out_bytes address the same buffer in bytes.  comp_host must be readable for 64
 * bytes beyond comp_bytes (a pageable buffer is copied and padded, so it need not be).
 * Calls from several threads (one model pair each: the queues of the streaming path) share the
 * device: the inflating of one runs beside the classification of another, but the forward
 * launches of all of them go through ONE stream per device, one launch at a time - the forward
 * kernel is persistent, and two of them on one GPU only stretch each other and everything queued
 * behind them (DEEPBINNER_FORWARD_STREAM=own: each call on its own stream, for comparison).
 * stream_status_host (n_streams, may be NULL): the decoder's verdict per stream - a read one of
 * whose streams failed was classified on zeros; the caller decodes it on the host and asks
 * again.  samples_host (may be NULL): the decoded signals, all of them (realtime's binning).
 * stage_ms (may be NULL, else 3 doubles): upload, inflate, classify in milliseconds on the
 * device (HIP events; tools). */
int dbh_classify_pair_deflated(dbh_model* start_model, dbh_model* end_model,
                               const uint8_t* comp_host, int64_t comp_bytes,
                               const dbh_inflate_stream* streams_host, int64_t n_streams,
                               const int64_t* offsets_host, int64_t n_reads, int scan_size,
                               double score_diff, int combine_mode, int32_t* calls_host,
                               int32_t* stream_status_host, int16_t* samples_host,
                               double* stage_ms);
/* The same call for the reference's verbose table (classify.py:157-171 prints, beside the final
 * call, each side's 2-decimal probabilities and - with two models - each side's own call):
 * optional outputs (NULL = not wanted) as in dbh_classify_pair_i16 - the per-side calls (n_reads
 * int32 each) and per-side merged probabilities (n_reads x n_classes fp32 each).  A side whose
 * model is NULL leaves its arrays untouched. */
int dbh_classify_pair_deflated_verbose(dbh_model* start_model, dbh_model* end_model,
                                       const uint8_t* comp_host, int64_t comp_bytes,
                                       const dbh_inflate_stream* streams_host, int64_t n_streams,
                                       const int64_t* offsets_host, int64_t n_reads, int scan_size,
                                       double score_diff, int combine_mode, int32_t* calls_host,
                                       int32_t* stream_status_host, int16_t* samples_host,
                                       double* stage_ms, int32_t* start_calls_host,
                                       int32_t* end_calls_host, float* start_probs_host,
                                       float* end_probs_host);

/* ---- multi-device: reads shard over the GPUs of one node, calls are all-gathered ---------- */
/* The reference is single-device (its only knob: set_tensorflow_threads, classify.py:416-423).
 * Reads are independent, so every GPU classifies a contiguous shard with its own model replica
 * (dbh_model_create under dbh_set_device) and no data-path collective; the one exchange is an
 * all-gather of the per-read int32 calls over RCCL / xGMI.  Two host
 * models, same entry points:
 *   one process, n devices:  dbh_comm_init_all (ncclCommInitAll); the arrays handed to
 *                            dbh_comm_all_gather_i32 have one entry per device;
 *   one process per GPU:     rank 0 calls dbh_comm_unique_id and ships the DBH_COMM_ID_BYTES bytes
 *                            to the other ranks over any host channel; every rank then calls
 *                            dbh_comm_init_rank with ITS device current; arrays have one entry.
 * librccl.so.1 is looked up at the first of these calls (dlopen), not at load time. */
typedef struct dbh_comm dbh_comm;
#define DBH_COMM_ID_BYTES 128
#define DBH_COMM_RCCL 0                  /* ncclAllGather                                        */
#define DBH_COMM_COPY 1                  /* hipMemcpy(Peer)Async copies, single-process form only:
                                            for boxes where two "devices" are one physical GPU,
                                            which RCCL refuses                                    */
int dbh_comm_available(void);            /* 1 if librccl could be loaded                          */
const char* dbh_comm_last_error(void);
int dbh_comm_init_all(int n_devices, const int* ordinals /* NULL = 0..n-1 */, int transport,
                      dbh_comm** comm);
int dbh_comm_unique_id(void* id_out /* DBH_COMM_ID_BYTES */);
int dbh_comm_init_rank(const void* id, int n_ranks, int rank, dbh_comm** comm);
int dbh_comm_info(const dbh_comm* comm, int* n_ranks, int* n_local, int* transport);
/* recv_dev[i] (n_ranks * count int32 on local device i) = the send_dev blocks of all ranks in rank
 * order; queued on streams[i] behind whatever produced send_dev[i]; does not block the host. */
int dbh_comm_all_gather_i32(dbh_comm* comm, const int32_t* const* send_dev,
                            int32_t* const* recv_dev, int64_t count, const dbh_stream* streams);
int dbh_comm_destroy(dbh_comm* comm);

/* ---- pieces of seam b2, exposed for parity tests ---------------------------------------- */
/* windows_dev: (n_reads * steps) x 1024 fp32, read-major (window index = read*steps + step). */
int dbh_normalise_windows_dev(const int16_t* samples_dev, const int64_t* offsets_dev,
                              int64_t n_reads, int side, int scan_size, float* windows_dev,
                              dbh_stream stream);
int dbh_merge_calls_dev(const float* window_probs_dev, int64_t n_reads, int steps, int n_classes,
                        double score_diff, float* probs_dev, int32_t* calls_dev,
                        dbh_stream stream);

/* ---- training: loss and weight gradients of one batch ----------------------------------------- */
/* The first half of the reference's training step (train_network.py:53-55 compiles build_network,
 * network_architecture.py:18-95, with categorical cross-entropy; train_network.py:66-68 runs
 * fit_generator on batches of deepbinner.py:265's default 20 windows): the network in Keras's
 * TRAINING phase, the loss, and the gradient of the mean loss with respect to every trainable
 * parameter.  The noise, the optimiser (Nadam) and the moving averages are the next section's; the
 * data generator, validation and the `fit` command's pieces the one after.  Any geometry dbh_model_create_ex takes; no model handle: the weights
 * change every step and are read where they lie.
 *   x        n_windows x input_size fp32, already normalised.  The GaussianNoise(0.02) layer
 *            (network_architecture.py:25) is the CALLER's to add to x (dbh_train_noise); this call adds none.
 *   labels   n_windows class numbers in [0, n_classes).
 *   batch normalisation (network_architecture.py:30,39,50,58,73,79,87): batch statistics per channel
 *            over all n_windows x length positions of THIS call (biased variance, epsilon 1e-3,
 *            two passes in fp64), the backward pass through mean and variance.  The blob's moving
 *            mean and variance are not read.  batch_stats: 960 floats, for layers 1..7 in turn the
 *            batch mean [C_i] then the batch variance [C_i] (48,48,48,48,192,48,48 channels), from
 *            which a caller keeps Keras's moving averages.
 *   dropout  (network_architecture.py:31,40,51,59,74,80,88) inverted, rate dropout_rate in [0, 1),
 *            behind each batch normalisation.  Element (layer 1..7, window, position, channel) is
 *            kept by a stateless function of those four and the seed, 32-bit arithmetic:
 *                mix(h): h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16
 *                h = mix(seed_lo + layer * 0x9e3779b9);  h = mix(h ^ seed_hi);  h = mix(h + window);
 *                h = mix(h ^ (position * 256 + channel));   kept <=> (h >> 8) >= floor(rate * 2^24)
 *            and multiplied by (float)(1 / (1 - rate)).  Rate 0 keeps all and multiplies by exactly 1.
 *            The mask does not depend on how the batch is laid over the GPU.
 *   loss     of a window: -log softmax(logits)[label] from a stable log-sum-exp; mean_loss is the
 *            mean over the batch.  Keras clips the probability to [1e-7, 1 - 1e-7] before the
 *            logarithm; this call does not - the one deliberate difference, visible only where
 *            p[label] < 1e-7.  n_correct: windows whose argmax (lowest index on ties) is the label.
 *   grads    n_floats fp32 in the blob's own layout (dbh_model_create): kernel[k][C_in][C_out] and
 *            bias per convolution, gamma and beta per batch normalisation; the moving-mean and
 *            moving-variance slots are zeros.  ReLU'(0) = 0; a max-pool tie sends the gradient to
 *            the first of the pair, the position a 'valid' pool drops gets 0.
 * No atomics: the same call gives the same bits, and a window's contribution does not depend on
 * the workgroup that took it.
 * LIMIT of one call: n_windows * input_size <= 2^20 = 1,048,576 samples (dbh_gradients_max_windows:
 * 1,024 windows of 1,024 samples, 64 of 16,384); more is DBH_ERR_UNSUPPORTED - the statistics are
 * per call, so a batch is never split silently.
 * Errors, all before any device work, nothing written: geometry outside the limits
 * DBH_ERR_UNSUPPORTED; n_floats not the parameter count DBH_ERR_BAD_WEIGHTS; n_windows < 1, a rate
 * outside [0, 1), a null pointer, (host entry) a label outside [0, n_classes):
 * DBH_ERR_INVALID_ARGUMENT. */
int dbh_gradients_max_windows(int input_size, int64_t* n_windows);
int dbh_gradients_workspace_bytes(int n_classes, int input_size, int64_t n_windows, size_t* bytes);
/* host pointers; blocks until the results are in the caller's buffers, like dbh_predict */
int dbh_gradients(const float* weights_host, int64_t n_floats, int n_classes, int input_size,
                  const float* x_host, const int32_t* labels_host, int64_t n_windows,
                  float dropout_rate, uint64_t seed, double* mean_loss, int64_t* n_correct,
                  float* grads_host, float* batch_stats_host);
/* device pointers (weights_dev 16-byte aligned), the caller's workspace of
 * dbh_gradients_workspace_bytes() bytes, queued on `stream`, not synchronised: what a training
 * loop (train_network.py:66-68) calls per step.  The labels are on the device and cannot be
 * checked here: a label outside [0, n_classes) makes mean_loss NaN. */
int dbh_gradients_dev(const float* weights_dev, int64_t n_floats, int n_classes, int input_size,
                      const float* x_dev, const int32_t* labels_dev, int64_t n_windows,
                      float dropout_rate, uint64_t seed, double* mean_loss_dev,
                      int64_t* n_correct_dev, float* grads_dev, float* batch_stats_dev,
                      void* workspace_dev, dbh_stream stream);
/* FROZEN BLOCKS: fine-tuning behind a frozen front.  Block j = 1..7 is what
 * ends at batch_normalization_j; frozen_blocks = f in 0..7 freezes blocks 1..f, and f = 0 is the
 * two calls above, bit for bit.  The head, conv1d_20, is never frozen.
 *   f   frozen in addition      first trainable        the backward pass ends with
 *   1   conv1d_1, bn_1          conv1d_2               conv1d_2's weight and bias gradient (no data
 *                                                      gradient into its input, likewise below)
 *   2   conv1d_2..4, bn_2       conv1d_5               conv1d_5's
 *   3   conv1d_5..7, bn_3       conv1d_8               conv1d_8's
 *   4   conv1d_8, 9, bn_4       conv1d_10, 11, 12, 14  those four's; none of their data gradients,
 *                                                      nothing back through the average pool
 *   5   conv1d_10..16, bn_5     conv1d_17              conv1d_17's
 *   6   conv1d_17, bn_6         conv1d_18              conv1d_18's
 *   7   conv1d_18, 19, bn_7     conv1d_20              conv1d_20's; no data gradient out of the head
 * The phase is Keras 2.1.4's for a layer with trainable = False: the layer leaves
 * trainable_weights and its updates are empty, but in the learning phase its BatchNormalization
 * still normalises by the BATCH's statistics and the Dropout behind it still drops.  So the forward
 * pass is the one above, bit for bit: the same mean_loss, n_correct and all 960 batch_stats.  What
 * changes is which gradients are formed.  Every launch that is kept is the launch of f = 0 (same
 * geometry, same part sizes, same order), so a trainable tensor's gradient has the bits it has at
 * f = 0; the slots of every frozen tensor (kernel, bias, gamma, beta) are written +0.0 like the
 * moving-statistics slots, whatever grads held.  Known consequence: the frozen blocks were trained
 * against their own moving statistics and are fine-tuned against the batch's.  This is this
 * library's contract, stated from Keras 2.1.4's rules; it is not held to a Keras run.
 * frozen_blocks outside 0..7: DBH_ERR_INVALID_ARGUMENT before any device work; otherwise the
 * errors of the calls above. */
int dbh_gradients_frozen(const float* weights_host, int64_t n_floats, int n_classes, int input_size,
                         const float* x_host, const int32_t* labels_host, int64_t n_windows,
                         float dropout_rate, uint64_t seed, double* mean_loss, int64_t* n_correct,
                         float* grads_host, float* batch_stats_host, int frozen_blocks);
int dbh_gradients_frozen_dev(const float* weights_dev, int64_t n_floats, int n_classes,
                             int input_size, const float* x_dev, const int32_t* labels_dev,
                             int64_t n_windows, float dropout_rate, uint64_t seed,
                             double* mean_loss_dev, int64_t* n_correct_dev, float* grads_dev,
                             float* batch_stats_dev, void* workspace_dev, dbh_stream stream,
                             int frozen_blocks);

/* ---- training: a resident trainer (noise, Nadam, moving statistics) ---------------------------- */
/* The second half of the reference's training step, and a trainer that keeps a model's training
 * state on the device: train_network.py:53-55 compiles the network with optimizer='nadam' under
 * Keras 2.1.4 (the version the shipped model files record), network_architecture.py:25 puts
 * GaussianNoise(0.02) in front of conv1d_1.  DESIGN.md section 18.  The data generator with its modify_signal
 * augmentation and validation are the next section's; the checkpoint policy and the command are
 * Python's (deepbinner_amd/fit.py).
 *
 * Defaults (dbh_trainer_default_options): Nadam's configuration as the shipped model files'
 * training_config attribute records it - lr (float)0.002, beta_1 (float)0.9, beta_2 (float)0.999 as
 * the doubles of those fp32 values, epsilon 1e-7, schedule_decay 0.004 - bn_momentum 0.99 (Keras's
 * BatchNormalization default), dropout_rate 0.15, noise_std 0.02, seed 0.
 *
 * One step of a trainer, t0 = the steps already taken (iterations):
 *   step_seed = seed + t0 * 0x9E3779B97F4A7C15 (mod 2^64)
 *   noise     dbh_train_noise(x, noise_std, step_seed): stateless, dbh_gradients' hash with the
 *             free layer number 0.  For sample (window, position), with lo/hi the halves of the seed:
 *                 b1 = bits(lo, hi, layer 0, window, position, channel 0)       24 bits each
 *                 b2 = bits(lo, hi, layer 0, window, position, channel 1)
 *                 u1 = (b1 + 1) / 2^24;  u2 = b2 / 2^24;  z = sqrt(-2 ln u1) * cos((2 pi) u2)
 *                 x' = (float)((double)x + (double)noise_std * z)
 *             in fp64, rounded once: |z| <= sqrt(2 ln 2^24) = 5.77.  noise_std == 0 returns x bit
 *             for bit, no arithmetic done.
 *   gradient  dbh_gradients on x' with dropout_rate and step_seed as its seed.  mean_loss and
 *             n_correct are those of the batch BEFORE the update, as Keras reports them.
 *   update    dbh_nadam_update with the coefficients dbh_nadam_schedule(t0, m_schedule) gives:
 *             one pass over the blob, each element from its own index alone, no atomics.
 *             Keras 2.1.4 Nadam.get_updates; on the host, in double:
 *                 t = t0 + 1
 *                 mu_t  = beta_1 * (1 - 0.5 * 0.96^(t * schedule_decay))
 *                 mu_t1 = beta_1 * (1 - 0.5 * 0.96^((t + 1) * schedule_decay))
 *                 sched_new = m_schedule * mu_t;  sched_next = sched_new * mu_t1;  beta_2_t = beta_2^t
 *             (m_schedule starts at 1 and becomes sched_new), and per trainable element, in fp64 from
 *             the fp32 p, g, m, v, every operation a separate IEEE operation in this order:
 *                 g' = g / (1 - sched_new)
 *                 m  = beta_1 * m + (1 - beta_1) * g;      m' = m / (1 - sched_next)
 *                 v  = beta_2 * v + (1 - beta_2) * (g * g);  v' = v / (1 - beta_2_t)
 *                 p  = p - (lr * ((1 - mu_t) * g' + mu_t1 * m')) / (sqrt(v') + epsilon)
 *             m, v and p are rounded to fp32 once each, where they are stored.  Keras does this in
 *             fp32; fp64 is a deliberate difference (like the unclipped loss): a host can replay it
 *             bit for bit.  Per moving-mean and moving-variance element, Keras 2.1.4's
 *             BatchNormalization:
 *                 new = (float)(old - (old - batch) * (1 - bn_momentum))        in fp64
 *             with batch the fp32 value of dbh_gradients' batch_stats: the BIASED batch variance,
 *             which is what 2.1.4 averages.  Later versions of Keras scale the batch variance by
 *             n / (n - 1 - eps) first; this library does not.  Those elements' m and v are not
 *             touched (they stay zero), and the trainable elements do not read batch_stats.
 * The same state, options and batches give the same bits, also across dbh_trainer_get_state /
 * dbh_trainer_set_state. */
typedef struct dbh_trainer dbh_trainer;
typedef struct dbh_trainer_options {
    double lr, beta_1, beta_2, epsilon, schedule_decay, bn_momentum;
    float dropout_rate, noise_std;
    uint64_t seed;
} dbh_trainer_options;
typedef struct dbh_nadam_coefficients {
    double lr, beta_1, beta_2, epsilon, mu_t, mu_t1, sched_new, sched_next, beta_2_t, bn_momentum;
} dbh_nadam_coefficients;
int dbh_trainer_default_options(dbh_trainer_options* options);
/* Host only, no device: the coefficients of step t0 (>= 0) from the m_schedule before it; hyper
 * null = the defaults.  After the step m_schedule is coefficients->sched_new. */
int dbh_nadam_schedule(int64_t t0, double m_schedule, const dbh_trainer_options* hyper,
                       dbh_nadam_coefficients* coefficients);
/* out = x + noise (see above); n_windows * input_size <= 2^20 samples, input_size <= 16,384 (more:
 * DBH_ERR_UNSUPPORTED); noise_std < 0 or not a number, a null pointer, a count < 1:
 * DBH_ERR_INVALID_ARGUMENT.  Host pointers, blocks; _dev: device pointers (out_dev may be x_dev),
 * queued on `stream`, not synchronised. */
int dbh_train_noise(const float* x_host, int64_t n_windows, int input_size, float noise_std,
                    uint64_t seed, float* out_host);
int dbh_train_noise_dev(const float* x_dev, int64_t n_windows, int input_size, float noise_std,
                        uint64_t seed, float* out_dev, dbh_stream stream);
/* One update in place: params, m, v (n_floats each, the blob's layout) from grads (n_floats) and
 * batch_stats (960 floats, dbh_gradients' layout).  n_classes outside [2, 256]:
 * DBH_ERR_UNSUPPORTED; n_floats not the parameter count: DBH_ERR_BAD_WEIGHTS; a null pointer or
 * bn_momentum outside [0, 1]: DBH_ERR_INVALID_ARGUMENT.  Host pointers: blocks, and the caller's
 * arrays are written only once the whole call has succeeded.  _dev: queued, not synchronised. */
int dbh_nadam_update(float* params_host, const float* grads_host, float* m_host, float* v_host,
                     const float* batch_stats_host, int64_t n_floats, int n_classes,
                     const dbh_nadam_coefficients* coefficients);
int dbh_nadam_update_dev(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev,
                         const float* batch_stats_dev, int64_t n_floats, int n_classes,
                         const dbh_nadam_coefficients* coefficients, dbh_stream stream);
/* The same update with blocks 1..frozen_blocks frozen (see dbh_gradients_frozen): an element of a
 * frozen tensor - kernel, bias, gamma, beta - and of a frozen batch normalisation's moving mean and
 * variance is neither read nor written, p, m and v alike, so a state whose moments there are not
 * zero leaves those weights alone too.  Every other element is dbh_nadam_update's, bit for bit;
 * still one pass over the blob, each element decided from its own index.  frozen_blocks outside
 * 0..7: DBH_ERR_INVALID_ARGUMENT; 0 is the call above. */
int dbh_nadam_update_frozen(float* params_host, const float* grads_host, float* m_host,
                            float* v_host, const float* batch_stats_host, int64_t n_floats,
                            int n_classes, const dbh_nadam_coefficients* coefficients,
                            int frozen_blocks);
int dbh_nadam_update_frozen_dev(float* params_dev, const float* grads_dev, float* m_dev,
                                float* v_dev, const float* batch_stats_dev, int64_t n_floats,
                                int n_classes, const dbh_nadam_coefficients* coefficients,
                                dbh_stream stream, int frozen_blocks);
/* A trainer owns, on the current device: the weights blob, m and v (zeros), the gradient blob, the
 * batch statistics, dbh_gradients' workspace for max_windows windows, and staging for the windows
 * and labels of a batch.  options null = the defaults.  Errors, all before any device work, nothing
 * written: geometry outside the limits, max_windows (or a step's n_windows) over
 * dbh_gradients_max_windows, n_windows > max_windows: DBH_ERR_UNSUPPORTED; n_floats not the
 * parameter count: DBH_ERR_BAD_WEIGHTS; a count < 1, dropout_rate outside [0, 1), noise_std < 0,
 * bn_momentum outside [0, 1], a null pointer, (host entry) a label outside [0, n_classes):
 * DBH_ERR_INVALID_ARGUMENT. */
int dbh_trainer_create(const float* weights_host, int64_t n_floats, int n_classes, int input_size,
                       int64_t max_windows, const dbh_trainer_options* options,
                       dbh_trainer** trainer);
int dbh_trainer_destroy(dbh_trainer* trainer);        /* null is fine */
/* One step on host arrays; blocks until the step is done and mean_loss, n_correct are written. */
int dbh_trainer_step(dbh_trainer* trainer, const float* x_host, const int32_t* labels_host,
                     int64_t n_windows, double* mean_loss, int64_t* n_correct);
/* The same on device arrays, queued on `stream` and never synchronised: a loop of steps keeps the
 * device busy.  The trainer's buffers serve one step at a time: queue a trainer's steps on one
 * stream (or order the streams).  A label outside [0, n_classes) makes mean_loss NaN (and the
 * weights with it).  x_dev is not changed. */
int dbh_trainer_step_dev(dbh_trainer* trainer, const float* x_dev, const int32_t* labels_dev,
                         int64_t n_windows, double* mean_loss_dev, int64_t* n_correct_dev,
                         dbh_stream stream);
/* These wait for the device, then copy.  A state is m, v, the step count and m_schedule; a new
 * trainer created from dbh_trainer_get_weights' blob with the same options and given that state
 * continues bit for bit. */
int dbh_trainer_get_weights(dbh_trainer* trainer, float* weights_host, int64_t n_floats);
int dbh_trainer_get_state(dbh_trainer* trainer, float* m_host, float* v_host, int64_t n_floats,
                          int64_t* iterations, double* m_schedule);
int dbh_trainer_set_state(dbh_trainer* trainer, const float* m_host, const float* v_host,
                          int64_t n_floats, int64_t iterations, double m_schedule);
int dbh_trainer_iterations(dbh_trainer* trainer, int64_t* iterations);
/* Frozen blocks of a trainer (0 when created): every step entry queued after the call - step,
 * step_dev, and the data-set entries of the next section, an epoch queued whole included - uses
 * dbh_gradients_frozen and dbh_nadam_update_frozen with this count; steps already queued keep the
 * count they were queued with.  Allowed between steps.  dbh_trainer_evaluate_dataset (test phase)
 * does not change.  It is an option of the run, not part of a state: dbh_trainer_get_state and
 * dbh_trainer_set_state neither carry nor change it.  Outside 0..7 or a null pointer:
 * DBH_ERR_INVALID_ARGUMENT, nothing changed. */
int dbh_trainer_set_frozen(dbh_trainer* trainer, int frozen_blocks);
int dbh_trainer_get_frozen(dbh_trainer* trainer, int* frozen_blocks);

/* ---- training: device-fed batches, validation -------------------------------------------------- */
/* The reference's data generator (train_network.py:127-193) and Keras's validation pass, without a
 * host loop per sample: a training-data file's windows stay on the device as the int16 samples the
 * file holds, and one kernel per batch gathers, normalises and augments.  DESIGN.md section 19;
 * tests/feed_reference.py restates all of it in NumPy.  bits() below is dbh_gradients' hash before
 * its comparison (24 bits), with the layer numbers 8, 9 and 10 that nothing else uses.
 *
 * Normalise (trim_signal.py:61-69 at train_network.py:144).  For a window of L int16 samples x:
 *     S = sum x, Q = sum x^2 in int64;  D = L * Q - S^2 (exact, < 2^59 for L <= 16,384)
 *     mean = (double)S / L;  std = sqrt((double)D) / L
 *     value = (float)(((double)x - mean) / std),  or (float)((double)x - mean) where D == 0
 * in fp64, each value rounded once; the sums are integers, so no order of summation exists.
 *
 * Augment (modify_signal and augmentation_chance, train_network.py:135,160-193), with s the seed
 * and w the batch SLOT (not the sample) as the hash's window:
 *     slot w is augmented  <=>  bits(s, 8, w, position 0, channel 0) < floor((1 - 1/aug) * 2^24)
 *     (the threshold formed on the host in double; aug = 1: 0, every window copied bit for bit)
 *     key(i) = bits(s, 9, w, i, 0);  rank(i) = the place of (key(i), i) in ascending order (equal
 *     keys rank by index);  half = L / 4 rounded half to even, as Python's round()
 *     position i is written twice where rank < half, dropped where half <= rank < 2 half, once
 *     otherwise; outputs keep the input's order: exactly L of them.
 * That is the reference's law - a uniform subset of 2 half positions, split uniformly - not its
 * random stream.  Every value is a function of its source sample alone, so normalising and
 * augmenting commute.
 *
 * Epoch order (random.shuffle at train_network.py:145,155): dbh_epoch_order, host only, no device:
 * order = the sample indices 0 .. n-1 in a stable ascending sort by
 * bits(seed, 10, sample index, pass mod 2^14, 0).  The sample stream is pass 0's order, then pass
 * 1's, and so on; step t takes stream positions [t B, (t+1) B), so a batch may span two passes.
 * n up to 2^31 (more: DBH_ERR_UNSUPPORTED); n < 1, pass < 0, null: DBH_ERR_INVALID_ARGUMENT.
 *
 * A data set owns one device block: the samples [n][input_size], the labels, mean and std per
 * window (computed once, at creation).  Errors of every entry below come before any device work and
 * nothing is written: a geometry dbh_trainer_create would refuse, n > 2^31 - 1, n_windows *
 * input_size > 2^20: DBH_ERR_UNSUPPORTED; a label outside [0, n_classes), a count < 1, a null
 * pointer, augmentation < 1 or not a number, (host entries) an index outside [0, n):
 * DBH_ERR_INVALID_ARGUMENT.  In the _dev entries an index outside [0, n) gives a window of NaN with
 * the label -1 (so a NaN loss), never a read outside the block. */
typedef struct dbh_dataset dbh_dataset;
int dbh_epoch_order(uint64_t seed, int64_t pass, int64_t n, int64_t* order);
int dbh_dataset_create(const int16_t* samples_host, const int32_t* labels_host, int64_t n,
                       int input_size, int n_classes, dbh_dataset** ds);
int dbh_dataset_destroy(dbh_dataset* ds);             /* null is fine */
int dbh_dataset_count(const dbh_dataset* ds, int64_t* n);
/* Slot w of x [n_windows][input_size] and labels [n_windows] from sample indices[w].  Stateless.
 * Host pointers: blocks (for tests and host loops).  _dev: device pointers, queued on `stream`,
 * not synchronised. */
int dbh_dataset_batch(const dbh_dataset* ds, const int64_t* indices_host, int64_t n_windows,
                      double augmentation, uint64_t seed, float* x_host, int32_t* labels_host);
int dbh_dataset_batch_dev(const dbh_dataset* ds, const int64_t* indices_dev, int64_t n_windows,
                          double augmentation, uint64_t seed, float* x_dev, int32_t* labels_dev,
                          dbh_stream stream);
/* dbh_gradients' forward pass in Keras's TEST phase (what fit_generator's validation and
 * model.evaluate run): each batch normalisation uses the blob's moving mean and variance,
 * 1 / sqrt(var + 1e-3) in fp64, no dropout, no noise; nothing is written to the weights.  The loss of
 * a window as in dbh_gradients (unclipped); loss_sum adds them in window order in fp64, n_correct
 * counts the windows whose argmax (lowest index on ties) is the label.  dbh_gradients' limits,
 * workspace (dbh_gradients_workspace_bytes) and errors.  window_loss (n_windows doubles) may be
 * null.  _dev: queued, not synchronised, and the totals are ADDED to *loss_sum_dev and
 * *n_correct_dev - zero them, then queue a set chunk by chunk and synchronise once. */
int dbh_evaluate(const float* weights_host, int64_t n_floats, int n_classes, int input_size,
                 const float* x_host, const int32_t* labels_host, int64_t n_windows,
                 double* loss_sum, int64_t* n_correct, double* window_loss_host);
int dbh_evaluate_dev(const float* weights_dev, int64_t n_floats, int n_classes, int input_size,
                     const float* x_dev, const int32_t* labels_dev, int64_t n_windows,
                     double* loss_sum_dev, int64_t* n_correct_dev, double* window_loss_dev,
                     void* workspace_dev, dbh_stream stream);
/* A trainer's step on a data set's samples: assemble(indices, augmentation, step_seed) into the
 * trainer's own batch buffers, then the step of dbh_trainer_step_dev - the order is augment, noise,
 * gradients, update, all with the one step_seed.  The data set's input_size and n_classes must be
 * the trainer's (else DBH_ERR_UNSUPPORTED); otherwise the errors of dbh_trainer_step and of
 * dbh_dataset_batch.  The host entry blocks; the _dev entry (indices on the device) is queued on
 * `stream` and never synchronised. */
int dbh_trainer_step_dataset(dbh_trainer* trainer, const dbh_dataset* ds, const int64_t* indices_host,
                             int64_t n_windows, double augmentation, double* mean_loss,
                             int64_t* n_correct);
int dbh_trainer_step_dataset_dev(dbh_trainer* trainer, const dbh_dataset* ds,
                                 const int64_t* indices_dev, int64_t n_windows, double augmentation,
                                 double* mean_loss_dev, int64_t* n_correct_dev, dbh_stream stream);
/* dbh_evaluate on the trainer's resident weights over the samples [first, first + count) in file
 * order, unaugmented, in chunks of max_windows through the step's own buffers (a window's result
 * does not depend on its chunk); one synchronisation at the end.  The weights, m, v and the step
 * count are not touched.  window_loss_host (count doubles) may be null.  first or count outside
 * the set: DBH_ERR_INVALID_ARGUMENT. */
int dbh_trainer_evaluate_dataset(dbh_trainer* trainer, const dbh_dataset* ds, int64_t first,
                                 int64_t count, double* loss_sum, int64_t* n_correct,
                                 double* window_loss_host);

/* ---- training-data text: a file's lines parsed on the GPU ---------------------------------------- */
/* The text that fit and classify read (train_network.py:127-133, classify.py:183-239), one sample
 * per line, to the int16 rows dbh_dataset_create takes.  DESIGN.md section 22;
 * csrc/dbh_text_core.h is the parser, compiled into the kernel and into the host model;
 * tests/text_parse_reference.py restates the grammar with regular expressions.
 *
 * The device parses a STRICT form only; what Python's parser takes beyond it (' 5', '1_0', '+1' or
 * '01' as labels, a lone CR as a line end, digits outside ASCII) is left to the host, which has
 * the last word on every line that is not DBH_TEXT_OK.  A strict line, as bytes:
 *     line  := label TAB value ( ',' value )* [CR] LF
 *     label := '0' | ['-'] [1-9] [0-9]{0,8}        (str(int(label)) == label; fits int32)
 *     value := ['+' | '-'] [0-9]{1,7}
 * A line's kind is the first of these that applies:
 *     DBH_TEXT_FORM   anything outside the grammar: an empty line, a second TAB or none, an empty
 *                     value, a NUL, a byte >= 0x80, a CR that no LF follows, eight digits, ...
 *     DBH_TEXT_COUNT  strict, but the number of values is not input_size
 *     DBH_TEXT_RANGE  strict with input_size values, one of them outside -32768..32767
 *     DBH_TEXT_OK     otherwise
 * A BLOCK is a run of whole lines: n_bytes >= 1 and its last byte is a LF (the caller cuts a file
 * at a LF and appends one to a last line that has none).  Line k is what lies between the k-th LF
 * and the next.  Outputs: samples [n_lines][input_size] int16, labels [n_lines] int32, kinds
 * [n_lines] (one byte each), *n_lines, and *first_bad_line = the smallest k whose kind is not
 * DBH_TEXT_OK, or -1.  The row and the label of a line that is not DBH_TEXT_OK are unspecified.
 * The caller's arrays hold max_lines lines; a block with more gives DBH_ERR_INVALID_ARGUMENT with
 * *n_lines set to the block's count and nothing else written - never a write past the end.
 * Stateless and replayable: a line's result depends on its bytes and input_size alone, not on the
 * block it is in, its place or alignment there, or how the blocks were cut.
 *
 * Errors, before any device work: a null pointer, input_size < 1, n_bytes < 0, max_lines < 0, an
 * empty block or one whose last byte is not a LF: DBH_ERR_INVALID_ARGUMENT; input_size > 2^20 or
 * n_bytes > 2^30: DBH_ERR_UNSUPPORTED.
 *
 * dbh_text_parse: `block` is host memory; uploads it, runs four launches on one stream (the LFs
 * per tile, their prefix, the line starts, one wave per line), synchronises once and downloads the
 * n_lines results.  Every device buffer is sized from n_bytes, input_size and max_lines before the
 * first launch.  dbh_text_parse_host: the same parser on the CPU - the walk in the same 1,024-byte
 * steps and 16-byte pieces - and no device; the two agree bit for bit on kinds, n_lines,
 * first_bad_line and on the rows and labels of DBH_TEXT_OK lines.  dbh_text_stage_ms: what the
 * calling thread's last successful dbh_text_parse spent, in ms - upload and kernels by device
 * events, download by the host's clock. */
#define DBH_TEXT_OK 0
#define DBH_TEXT_FORM 1
#define DBH_TEXT_COUNT 2
#define DBH_TEXT_RANGE 3
int dbh_text_parse(const uint8_t* block_host, int64_t n_bytes, int input_size, int64_t max_lines,
                   int16_t* samples_host, int32_t* labels_host, uint8_t* kinds_host,
                   int64_t* n_lines, int64_t* first_bad_line);
int dbh_text_parse_host(const uint8_t* block_host, int64_t n_bytes, int input_size, int64_t max_lines,
                        int16_t* samples_host, int32_t* labels_host, uint8_t* kinds_host,
                        int64_t* n_lines, int64_t* first_bad_line);
int dbh_text_stage_ms(double* upload, double* kernels, double* download);

/* ---- random signals: the synthetic no-barcode samples of `balance` ------------------------------ */
/* The reference's balance command appends random signals as no-barcode samples (balance.py:155-193):
 * one of four kinds, drawn one random.gauss and one str() per value.  Here value i of signal s is a
 * function of (seed, s, i, input_size) alone - the reference's law, not its Mersenne-Twister
 * stream.  DESIGN.md section 23; csrc/dbh_random_core.h is the generator, compiled into the kernel
 * and into the host model; tests/random_signal_reference.py restates it in NumPy.
 *
 * bits(layer, s, p, c) is dbh_gradients' hash (see "training" above) with the halves of `seed`,
 * the free layer numbers 11..14, s as its window, p as its position and c as its channel: 24 bits.
 * u(b) = b / 2^24.  All arithmetic is fp64, one IEEE operation per operation written here, left to
 * right; a value is truncated toward zero (a C cast, Python's int()).
 *
 * Per signal, b_c = bits(11, s, 0, c):
 *     kind    = b_0 % 4          0 flat, 1 gaussian, 2 multi_gaussian, 3 perlin
 *     level   = b_1 % 1001
 *     mean    = 300 + 300 * u(b_2)          stdev  = 10 + 490 * u(b_3)
 *     octaves = 1 + b_4 % 4                 step   = 0.001 + 0.039 * u(b_5)
 *     start   = u(b_6)                      factor = 10 + 290 * u(b_7)
 * (the ranges of balance.py:164-190).
 *   flat            every value is level.
 *   gaussian        z(i) = sqrt(-2 * log(u1)) * cos(6.283185307179586 * u2) with
 *                   u1 = (bits(13, s, i, 0) + 1) / 2^24 and u2 = bits(13, s, i, 1) / 2^24 - the
 *                   trainer's Box-Muller - and value = trunc(mean + stdev * z(i)).
 *   multi_gaussian  segment k = 0, 1, ... holds 100 + bits(12, s, k, 0) % 401 values, laid end to
 *                   end from value 0, with its own mean = 300 + 300 * u(bits(12, s, k, 1)) and
 *                   stdev = 10 + 490 * u(bits(12, s, k, 2)); value i = trunc(mean_k + stdev_k * z(i))
 *                   of the segment k it lies in.
 *   perlin          gradient noise of noise.pnoise1's construction with hashed gradients (not its
 *                   permutation table).  x = start + i * step; sum = weights = 0; for k = 0 ..
 *                   octaves - 1 in turn, with amp = 0.5^k:
 *                       xk = x * 2^k;  j = floor(xk);  t = xk - j
 *                       g(j) = 2 * u(bits(14, s, j, k)) - 1
 *                       f = t * t * t * (t * (t * 6 - 15) + 10)
 *                       a = g(j) * t;  b = g(j + 1) * (t - 1);  n = a + f * (b - a)
 *                       sum = sum + amp * 2 * n;  weights = weights + amp
 *                   value = trunc(mean + factor * (sum / weights)).
 * Every value lies far inside int16.  log and cos are the math library's: a host and the device
 * may differ in their last place, which moves a truncated value (by one) only where the value
 * before truncation lies on an integer; everything else is bit for bit.
 *
 * out: int16 [n_signals][input_size], signal first_signal + k in row k - a range may be cut into
 * calls anywhere.  Errors, before any device work: a null pointer, n_signals < 1, input_size < 1,
 * first_signal < 0 or first_signal + n_signals > 2^32: DBH_ERR_INVALID_ARGUMENT; input_size > 2^20
 * or n_signals * input_size > 2^30: DBH_ERR_UNSUPPORTED.
 * dbh_random_signals: out is host memory; one launch, one synchronisation, one download.  _dev:
 * device memory, queued on `stream`, never synchronised.  _host: the same generator on the CPU,
 * no device. */
int dbh_random_signals(uint64_t seed, int64_t first_signal, int64_t n_signals, int input_size,
                       int16_t* out_host);
int dbh_random_signals_dev(uint64_t seed, int64_t first_signal, int64_t n_signals, int input_size,
                           int16_t* out_dev, dbh_stream stream);
int dbh_random_signals_host(uint64_t seed, int64_t first_signal, int64_t n_signals, int input_size,
                            int16_t* out_host);

/* ---- training-data text, written: int16 rows to the lines dbh_text_parse reads -------------------- */
/* labels [n_lines] int32 and samples [n_lines][input_size] int16 become the bytes
 *     label TAB v1 ',' v2 ',' ... vL LF          per line, numbers as Python's str() writes them
 * - the strict grammar above, so dbh_text_parse gives the arrays back.  csrc/dbh_format_core.h is
 * the formatter, compiled into the kernels and into the host model; DESIGN.md section 23.
 * A value takes 1 to 6 bytes and the byte behind it; a label is '0' or up to nine digits with an
 * optional '-' (a label outside +-(10^9 - 1): DBH_ERR_INVALID_ARGUMENT).  dbh_text_format_bound:
 * n_lines * (12 + 7 * input_size), which no text exceeds.
 *
 * `out` holds `capacity` bytes; *n_bytes becomes the text's length.  A capacity below it gives
 * DBH_ERR_INVALID_ARGUMENT with *n_bytes set to the need and nothing written - never a write past
 * the end.  Errors, before any device work: a null pointer, n_lines < 1, input_size < 1,
 * capacity < 0: DBH_ERR_INVALID_ARGUMENT; input_size > 2^20 or n_lines * input_size > 2^30:
 * DBH_ERR_UNSUPPORTED.
 *
 * dbh_text_format: host memory; uploads, five launches on one stream (the bytes of each line, one
 * wave per line; their prefix over tiles of 1,024 lines, in three; the bytes themselves, one wave
 * per line), one synchronisation, and
 * the text's bytes downloaded.  Every device buffer is sized from n_lines, input_size and the
 * capacity before the first launch.  _dev: device memory throughout, queued on `stream`, never
 * synchronised; workspace_dev holds dbh_text_format_workspace_bytes(n_lines) bytes, 8-byte
 * aligned; *n_bytes_dev becomes the length, or -1 for a refused label, and nothing is written to
 * out_dev where it is -1 or above the capacity.  _host: the same formatter on the CPU, no device;
 * the three agree byte for byte. */
int dbh_text_format_bound(int64_t n_lines, int input_size, int64_t* bytes);
int dbh_text_format_workspace_bytes(int64_t n_lines, size_t* bytes);
int dbh_text_format(const int32_t* labels_host, const int16_t* samples_host, int64_t n_lines,
                    int input_size, uint8_t* out_host, int64_t capacity, int64_t* n_bytes);
int dbh_text_format_dev(const int32_t* labels_dev, const int16_t* samples_dev, int64_t n_lines,
                        int input_size, uint8_t* out_dev, int64_t capacity, int64_t* n_bytes_dev,
                        void* workspace_dev, dbh_stream stream);
int dbh_text_format_host(const int32_t* labels_host, const int16_t* samples_host, int64_t n_lines,
                         int input_size, uint8_t* out_host, int64_t capacity, int64_t* n_bytes);

/* ---- introspection ------------------------------------------------------------------------ */
/* Activations after stage 'A'..'G'  for n_windows windows, row-major
 * [window][position][channel]; out_host must hold n_windows * dbh_stage_floats(stage) floats. */
int dbh_stage_floats(int stage, int64_t* floats_per_window);
int dbh_debug_forward(dbh_model* model, const float* x_host, int64_t n_windows, int stage,
                      float* out_host);
/* name and static resource use of the forward kernel, for bench/roofline bookkeeping */
int dbh_forward_kernel_info(int* threads_per_block, int* lds_bytes, int* vgprs);
/* Matrix instructions (v_mfma_f32_16x16x4_f32, 2,048 FLOP each) the forward kernel ISSUES per
 * window for a model of n_classes classes - fewer than the 33,629,952 algorithmic FLOP of the
 * direct convolutions because six layers run as Winograd F(4,3) / F(2,3).  A constant of the build
 * (dbh_layout.h), checked against rocprofv3's SQ_INSTS_MFMA in profiles/. */
int dbh_forward_executed_mfmas(int n_classes, int64_t* mfmas_per_window,
                               int64_t* flop_per_window);
/* Run the forward kernel only up to and including stage last_stage (0 = 'A' .. 6 = 'G'), writing
 * nothing: lets a profiler attribute kernel time to stages by differencing. */
int dbh_forward_truncated_dev(dbh_model* model, const float* x_dev, int64_t n_windows,
                              int last_stage, dbh_stream stream);
/* Timeline of one forward launch: every wave of every workgroup stamps the shader cycle counter at
 * each phase boundary (slot meanings: tools/timeline.py).  stamps_host: n_windows x 8 x 64 int64. */
int dbh_forward_timeline(dbh_model* model, const float* x_host, int64_t n_windows,
                         int64_t* stamps_host);
/* The same for the fused seam-b2 mode: n_reads reads of exactly 1,024 int16 samples each (side
 * start, one scan step), so that the slice + normalise front of stage A is on the timeline. */
int dbh_forward_timeline_i16(dbh_model* model, const int16_t* samples_host, int64_t n_reads,
                             int64_t* stamps_host);
/* Live kernel timing: with enable = n > 0, every n-th launch of the forward kernel is bracketed by
 * HIP events on the stream it is launched on (n = 1: every launch; the event pair itself costs a
 * few microseconds of queue time, so sampling keeps the measurement from slowing what it
 * measures); dbh_forward_timing_read synchronises those events, returns the summed kernel time,
 * the number of timed launches and of windows they covered, and resets the tally. 0 = off. */
int dbh_forward_timing_enable(dbh_model* model, int enable);
/* The same with ONE event pair around a run of `span` consecutive launches (span <= every_nth)
 * starting at every every_nth-th launch: the pair's own cost (~2.5 us of dispatch latency lands
 * inside the bracket) is shared by the run, so total_ms / launches is the launch-to-launch period
 * of back-to-back launches, which is what rocprofv3's per-kernel duration plus the dispatch gap
 * adds up to.  Brackets still open at dbh_forward_timing_read are dropped. */
int dbh_forward_timing_enable_span(dbh_model* model, int every_nth, int span);
int dbh_forward_timing_read(dbh_model* model, double* total_ms, int64_t* launches,
                            int64_t* windows);

/* Clock probe.  The MFMA peak of the data sheet assumes 2.4 GHz; under this kernel's load the
 * shader clock runs lower (power management), and "how busy is the matrix pipe" is a ratio of
 * CYCLES.  With the probe on, every workgroup of a production launch of the forward kernel notes
 * the shader clock counter (s_memtime) and the constant-rate wall clock (s_memrealtime,
 * hipDeviceAttributeWallClockRate) at its start and at its end (two stores per workgroup);
 * dbh_forward_clock_read synchronises the device and returns the median ratio of the model's
 * latest launch as a frequency in GHz. */
int dbh_forward_clock_enable(dbh_model* model, int enable);
int dbh_forward_clock_read(dbh_model* model, double* shader_ghz);
/* Phase stamps, asked for on top of the clock probe (dbh_forward_phases_enable; each stamp is a
 * counter read and an LDS word by one lane - ~25 per group, about 1 % of the kernel's time, so they are
 * not part of a timed run): the forward kernel keeps, in LDS, the shader clock at five points of each
 * of a workgroup's first 12 groups of windows (it takes its windows four at a time): the group's
 * start, the end of its stage A-C loop (conv1d_1 .. conv1d_7 of each window), of the stage D-E chain
 * (conv1d_8 .. conv1d_16 of the four together), of its stage F loop (conv1d_17 of each window) and of
 * the batched tail - one lane, right behind a barrier: the kernel measured is the kernel that ships.
 * dbh_forward_phases_read returns the mean cycles of the five intervals (the fifth runs to the next
 * group's start; tail-less groups leave it near zero) over the steady-state groups of the model's
 * latest launch, and how many groups that was.
 * mean_cycles_14[5..8]: stage F's inner intervals as its first wave sees them, summed over the group's
 * windows: to the end of conv1d_17's MFMAs, to behind its barrier, to the end of the reduction, to
 * behind the group's last barrier.  [9..11]: stages A-C's, summed over the group's windows: a window's
 * top to the start of stage B's chain, the chain, conv1d_7 (of all windows but the group's last);
 * [12], [13]: the group's last conv1d_7, and from its end to the start of the stage D-E chain. */
int dbh_forward_phases_enable(dbh_model* model, int enable);
/* how many doubles dbh_forward_phases_read writes (14): size the buffer from this, not from a literal */
int dbh_forward_phases_count(int* count);
int dbh_forward_phases_read(dbh_model* model, double* mean_cycles_14, int64_t* groups);

/* ---- LDS state (test support) --------------------------------------------------------------- */
/* LDS is not cleared between workgroups: a kernel that reads a word of its __shared__ arena before
 * it has written it computes with what the workgroup before it left on that CU.  These two put
 * that state in a test's hands (csrc/dbh_lds_state.hip).
 *
 * dbh_lds_fill: one launch on `device`'s null stream of grid_multiple x (number of CUs) workgroups
 * of 512 threads with all 160 KiB of LDS each (one workgroup per CU at a time); every word of the
 * arena is stored as `pattern`, then the workgroup keeps its CU for hold_us microseconds (a counted
 * wait on the constant-rate clock), so that the grid's later workgroups go to the CUs that had none.
 * The device is synchronised before the call returns.  *cus_seen: distinct CUs a workgroup ran on
 * (by XCC, shader engine and CU id); *cus_total (may be null): the device's CU count.  A fill has
 * reached every CU when the two are equal.
 * dbh_lds_survey: the same shape, but nothing is stored to LDS: the workgroups count the words of
 * the arena that equal `pattern`.  matching[s], looked_at[s] (DBH_LDS_CU_SLOTS int64 each): words
 * that matched and words read on the CU with id s, both 0 where no workgroup ran.
 * grid_multiple 0 and hold_us < 0 ask for the defaults (4 and 50); grid_multiple > 64,
 * hold_us > 10,000 or a null cus_seen / matching / looked_at: DBH_ERR_INVALID_ARGUMENT. */
#define DBH_LDS_CU_SLOTS 1024
int dbh_lds_fill(int device, uint32_t pattern, int grid_multiple, int hold_us, int* cus_seen,
                 int* cus_total);
int dbh_lds_survey(int device, uint32_t pattern, int grid_multiple, int hold_us, int64_t* matching,
                   int64_t* looked_at, int* cus_seen, int* cus_total);

#ifdef __cplusplus
}
#endif
#endif /* DEEPBINNER_HIP_H */
