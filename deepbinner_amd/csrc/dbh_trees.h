// dbh_trees.h — the three halving trees in LDS that finish one read held by one workgroup of THREADS
// threads (thread c = class c): the sum, the best class with ties to the lower index, and the
// maximum.  ONE text for dbh_general.hip's merge_kernel and dbh_sweep.hip's fold256_kernel, whose
// results have to agree to the bit: same pairing (c with c + half), same order (half = THREADS / 2
// down to 1).  Every thread of the workgroup calls each tree; rv (and ri) hold THREADS elements, and
// the closing barrier lets the caller write them again at once.  Device functions only, as
// dbh_seam.h: a kernel defined here would land in every unit that includes this file.
#ifndef DBH_TREES_H
#define DBH_TREES_H
#include <hip/hip_runtime.h>

namespace dbh {

template <int THREADS>
__device__ __forceinline__ double tree_sum(double* rv, int c, double v) {
    rv[c] = v;
    __syncthreads();
    for (int half = THREADS / 2; half >= 1; half >>= 1) {
        if (c < half) rv[c] += rv[c + half];
        __syncthreads();
    }
    const double all = rv[0];
    __syncthreads();
    return all;
}

// highest value, lowest class among equals -> the value, *index its class
template <int THREADS>
__device__ __forceinline__ double tree_best(double* rv, int* ri, int c, double v, int* index) {
    rv[c] = v;
    ri[c] = c;
    __syncthreads();
    for (int half = THREADS / 2; half >= 1; half >>= 1) {
        if (c < half) {
            const double o = rv[c + half];
            const int oi = ri[c + half];
            if (o > rv[c] || (o == rv[c] && oi < ri[c])) {
                rv[c] = o;
                ri[c] = oi;
            }
        }
        __syncthreads();
    }
    const double top = rv[0];
    *index = ri[0];
    __syncthreads();
    return top;
}

template <int THREADS>
__device__ __forceinline__ double tree_max(double* rv, int c, double v) {
    rv[c] = v;
    __syncthreads();
    for (int half = THREADS / 2; half >= 1; half >>= 1) {
        if (c < half) rv[c] = fmax(rv[c], rv[c + half]);
        __syncthreads();
    }
    const double top = rv[0];
    __syncthreads();
    return top;
}

}  // namespace dbh

#endif  // DBH_TREES_H
