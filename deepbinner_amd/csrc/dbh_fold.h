// dbh_fold.h — one step of the fold over a read's windows (include/deepbinner_hip.h, "sweep"), ONE
// text for dbh_sweep.hip, which walks all of a read's windows in one launch, and dbh_live.hip, which
// stops after the windows a push made ready and goes on at the next: window v merged into the running
// vector (class 0 the minimum, the barcodes the maximum; classify.py:368-374), then make_sum_to_one
// in fp64 with the rest == 0 guard (classify.py:387-393), the best class with ties to the lower
// index and its lead over the runner-up (classify.py:285-295).  Two forms, as the two merges sum in
// different orders: 32 lanes per read with dbh_seam.h's reductions, one workgroup per read with
// dbh_trees.h's.  Every lane (thread) of the read gets the result.  Device functions only.
#pragma once

#include <hip/hip_runtime.h>

#include "dbh_seam.h"
#include "dbh_trees.h"

namespace dbh {

// lane c's class of window `v` into its merged value (`first`: the read's first window)
__device__ __forceinline__ float fold_merge(float merged, float v, bool first, int c) {
    return first ? v : (c == 0 ? fminf(merged, v) : fmaxf(merged, v));
}

// 32 lanes per read, lane c = class c, control flow uniform over the 32
__device__ __forceinline__ void fold32_step(float merged, bool valid, int c, int* best,
                                            double* margin) {
    double p = (double)merged;
    const double rest =
        reduce32(RedF64{(valid && c > 0) ? p : 0.0},
                 [](const RedF64& a, const RedF64& b) { return RedF64{a.v + b.v}; }).v;
    const double p0 = __shfl(p, 0, 32);                        // lane 0 of this read's 32
    const double factor = rest > 0.0 ? (1.0 - p0) / rest : 0.0;
    if (c > 0) p = p * factor;
    const RedBest top = reduce32(RedBest{valid ? p : -1.0, c}, [](const RedBest& a, const RedBest& b) {
        return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
    });
    const double second =
        reduce32(RedF64{(valid && c != top.i) ? p : -1.0},
                 [](const RedF64& a, const RedF64& b) { return RedF64{fmax(a.v, b.v)}; }).v;
    *best = top.i;
    *margin = top.v - second;
}

// one workgroup of THREADS per read, thread c = class c; rv, ri: THREADS elements of LDS, first: one.
// (`first` is written again only behind the next step's tree_sum, which has barriers.)
template <int THREADS>
__device__ __forceinline__ void fold256_step(float merged, bool valid, int c, double* rv, int* ri,
                                             double* first, int* best, double* margin) {
    double p = (double)merged;
    const double rest = tree_sum<THREADS>(rv, c, (valid && c > 0) ? p : 0.0);
    if (c == 0) *first = p;
    __syncthreads();
    const double p0 = *first;
    if (c > 0) p = p * (rest > 0.0 ? (1.0 - p0) / rest : 0.0);
    int top_i;
    const double top_v = tree_best<THREADS>(rv, ri, c, valid ? p : -1.0, &top_i);
    const double second = tree_max<THREADS>(rv, c, (valid && c != top_i) ? p : -1.0);
    *best = top_i;
    *margin = top_v - second;
}

}  // namespace dbh
