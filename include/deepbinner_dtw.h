/*
 * deepbinner_dtw.h - C ABI of libdeepbinner_dtw.so: semi-global dynamic time warping on an
 * MI355X (gfx950), SURVEY.md §8f rank 4.
 *
 * Replaces the reference's one native function,
 *   deepbinner/dtw/dtw.h:17-18     double semi_global_dtw(ref, query, ref_len, query_len,
 *                                                        alignment, positions, path_length)
 *   deepbinner/dtw/dtw.cpp:58-151  its implementation (fp64 cost matrix, direction matrix, walk back)
 * which deepbinner/dtw_semi_global.py:30-41 binds with ctypes (LoadLibrary, ndpointer arguments,
 * restype double).  `semi_global_dtw` below has the same name, arguments and results, so that
 * binding works on this library unchanged; `dtw_semi_global_batch` is the form that fills a GPU:
 * many (reference signal, query signal) pairs per call, one wavefront each.
 *
 * Arithmetic: fp64 subtract, multiply, add, compare in the order of dtw.cpp (no fused
 * multiply-add), so distances are bit-identical to the reference's.  One documented difference: an
 * exact tie between LEFT and UP (with the diagonal larger than both) is broken by rand() in the
 * reference (dtw.cpp:40-45) and goes LEFT here; the distance does not depend on it.  A second one,
 * of the rescaled DTW only: a query for which no line can be fitted (the denominator of the normal
 * equations is zero or not finite - a constant query) gets the distance +inf here, where the
 * reference's lstsq returns a minimum-norm fit ("Rescaled DTW" below).
 *
 * All pointers are host pointers; the calls block.  Thread safe (one call at a time runs on the
 * device).  Errors: `semi_global_dtw` returns NaN and leaves path_length[0] = 0;
 * `dtw_semi_global_batch`, `dtw_rescaled_batch` and `dtw_locate_batch` return a status, check every
 * argument before any device work and write nothing on error.
 *
 * ---- prep's signal stage: the contract of dtw_rescaled_batch and dtw_locate_batch ----------------
 * Both are stateless: the results are a function of the arguments alone, the same bits on every
 * call and for every split of the batch, and a NumPy restatement gives those bits
 * (tests/prep_signal_reference.py).  Between upload and download nothing crosses to the host: the
 * launches (normalise; per part pass 1, fit, pass 2; verdict; select) are queued on one stream
 * with one synchronise at the end.
 *
 * Rescaled DTW (reference dtw_semi_global.py:61-95, its two iterations) of a pair (ref, query):
 *   1. pass 1: the DTW above on (ref, query); its alignment has n pairs (i_k, j_k), k = 0 .. n-1 in
 *      STORED order, that is from the end of the alignment backwards.
 *   2. the line y = m x + b through the points x_k = query[j_k], y_k = ref[i_k], by the normal
 *      equations in fp64.  Sums: 64 partial sums per quantity, all starting from +0.0; partial l
 *      takes k = l, l + 64, l + 128, ... in that order,
 *          sx_l += x_k;  sy_l += y_k;  sxx_l += (x_k * x_k);  sxy_l += (x_k * y_k)
 *      (the product rounded, then the sum); then Sx = (((+0.0 + sx_0) + sx_1) + ...) + sx_63, and
 *      Sy, Sxx, Sxy likewise.  This order does not depend on the launch or on the batch.
 *          den = (n * Sxx) - (Sx * Sx)
 *          m   = ((n * Sxy) - (Sx * Sy)) / den
 *          b   = (Sy - (m * Sx)) / n
 *      with n as a double and every operation one IEEE double operation, none fused.
 *   3. query'[j] = (m * query[j]) + b, two roundings.
 *   4. pass 2: the DTW above on (ref, query').  Its distance, positions and alignment are the
 *      result, with the slope m.  If m < 0.75 or m > 1.333 the distance is +inf (reference :91-93).
 *   If den is zero or not finite: no fit.  query' = query, pass 2 runs on it for the positions,
 *   the distance is +inf and the slope NaN.
 *   A reference of one sample: dtw.cpp looks for the end over rows 1 .. ref_len-1, finds none and
 *   returns DBL_MAX with positions 0, 0 and the path along row 0; so does each pass here.  The fit
 *   over that path has y constant, a slope of about 0, and the distance becomes +inf.
 *
 * Normalise (reference trim_signal.py:61-69, over the whole trimmed signal as prep does): the
 * caller forms S = sum x and Q = sum x^2 over the L int16 samples of the trimmed read as exact
 * integers, D = L Q - S^2, mean = (double)S / L (correctly rounded), std = sqrt((double)D) / L.
 * The device forms ((double)x - mean) / std, or (double)x - mean where std == 0 (D == 0), for
 * the samples of the uploaded region only.
 *
 * Locate: job k is (read, from, to, query): the window [from, to) of that read's uploaded,
 * normalised region against queries[query].  Its results are those of the rescaled DTW, positions
 * relative to the window.  An empty window (from == to) is skipped, as the reference's
 * `len(...) > 0` skips it: distance +inf, positions -1, -1, slope NaN.  Consecutive jobs form
 * groups; hits[g] is the index, among all jobs, of the first job of group g in job order whose
 * distance is finite and <= threshold (the reference: 50.0, prep_native_start.py:124), or -1.
 * +inf and NaN never hit.  Every job of a group is computed.
 */
#ifndef DEEPBINNER_DTW_H
#define DEEPBINNER_DTW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTW_OK 0
#define DTW_ERR_ARGUMENT 1     /* null pointer, non-positive length, offsets not ascending */
#define DTW_ERR_NO_DEVICE 2    /* no HIP device / not gfx950 */
#define DTW_ERR_HIP 3          /* a HIP call failed: dtw_last_error() has the text */

const char* dtw_version(void);
const char* dtw_status_string(int status);
const char* dtw_last_error(void);

/* dtw.h:17-18.  alignment: room for 2 * (ref_len + query_len) ints; receives path_length[0] pairs
 * (ref index, query index) from the END of the alignment backwards.  positions[0] / positions[1]:
 * first and last reference index of the aligned region.  Returns the distance (the smallest
 * accumulated cost in the last query column over reference rows 1 .. ref_len-1). */
double semi_global_dtw(const double* ref, const double* query, int ref_len, int query_len,
                       int* alignment, int* positions, int* path_length);

/* n_pairs alignments in one call.  Pair p aligns refs[ref_offsets[p] .. ref_offsets[p+1]) with
 * queries[query_offsets[p] .. query_offsets[p+1]) (both offset arrays have n_pairs + 1 entries,
 * every pair needs at least one sample of each).  Outputs: distances[p]; positions[2p], [2p+1];
 * path_lengths[p]; and, unless `alignment` is NULL, the pairs of p from
 * alignment[2 * (ref_offsets[p] + query_offsets[p])] on, laid out as for semi_global_dtw. */
int dtw_semi_global_batch(const double* refs, const int64_t* ref_offsets, const double* queries,
                          const int64_t* query_offsets, int64_t n_pairs, double* distances,
                          int32_t* positions, int32_t* path_lengths, int32_t* alignment);

/* The rescaled DTW of n_pairs pairs, resident: inputs as for dtw_semi_global_batch (every pair
 * needs at least one sample of each).  Outputs per pair: distances[p]; positions[2p], [2p+1];
 * slopes[p]; unless NULL, rescaled[query_offsets[p] ..): query' of the pair, and path_lengths[p]
 * of pass 2; unless NULL (it needs path_lengths), the alignment of pass 2 laid out as for
 * dtw_semi_global_batch. */
int dtw_rescaled_batch(const double* refs, const int64_t* ref_offsets, const double* queries,
                       const int64_t* query_offsets, int64_t n_pairs, double* distances,
                       int32_t* positions, double* slopes, double* rescaled,
                       int32_t* path_lengths, int32_t* alignment);

/* Locate, as the contract above has it.  Read r's region is samples[region_offsets[r] ..
 * region_offsets[r+1]) (n_reads + 1 offsets, ascending, a region may be empty) with
 * mean_std[2r], mean_std[2r+1] (finite, std >= 0).  Query q is queries[query_offsets[q] ..
 * query_offsets[q+1]) (n_queries + 1 offsets, at least one sample each).  jobs holds four int64
 * per job: read, from, to, query, with 0 <= from <= to <= the region's length.  Group g is jobs
 * group_offsets[g] .. group_offsets[g+1] (n_groups + 1 offsets from 0 to n_jobs, ascending).
 * Outputs: distances, slopes [n_jobs], positions [2 n_jobs], hits [n_groups]. */
int dtw_locate_batch(const int16_t* samples, const int64_t* region_offsets,
                     const double* mean_std, int64_t n_reads, const double* queries,
                     const int64_t* query_offsets, int64_t n_queries, const int64_t* jobs,
                     int64_t n_jobs, const int64_t* group_offsets, int64_t n_groups,
                     double threshold, double* distances, int32_t* positions, double* slopes,
                     int32_t* hits);

/* Device time of the kernels of the last call on this thread's device, in milliseconds (HIP
 * events around the launches), and the number of matrix cells they filled (both passes of the
 * rescaled entries). */
int dtw_last_kernel_time(double* milliseconds, int64_t* cells);

#ifdef __cplusplus
}
#endif
#endif
