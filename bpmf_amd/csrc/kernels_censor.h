// kernels_censor.h -- censored ratings (bpmf_hip_side_set_censored, capi_censor.hip; one translation unit: kcensor.hip).
// DESIGN.md section 16 has the model.
//
//   k_censor_latent    the data-augmentation step of one half-iteration: for every CENSORED rating p of the side (column c, row r,
//                      recorded bound b_p, s_p = +1 for a lower bound / -1 for an upper bound)
//                          m = x_c . y_r,   z_p ~ N(mean + m, 1 / alpha) truncated to (b_p, inf) for s = +1, (-inf, b_p) for s = -1
//                      z has the layout of the side's `vals` and holds the ratings themselves everywhere else; the unchanged
//                      column samplers read it in their place.
//
// The work is cut over the censored entries, not over the ratings: tiles of kProbitTile consecutive entries of the side's lists
// (position, column, row, sign), one tile per workgroup, in the two phases of k_probit_latent (kernels_probit.h):
//   1. the tile's columns and rows go into LDS -- the lists hold the columns, nothing is searched -- and probit_tile_dots forms the
//      dot products as it does for the probit kernels
//   2. thread i owns entry i of the tile: the draw of probit_truncated on the Philox blocks of the rating position p (not of the
//      list index: a draw does not depend on how the censored entries are stored), one 8-byte store to z[p] per lane, ascending
// fp64 throughout; fp32 factors are widened per element.  No atomics: z_p depends on (p, iter, tag, alpha, mean, factors) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_probit.h"     // probit_truncated, kProbitTile, probit_tile_dots (kernels_gather.h)

namespace bpmf {

template <int K, typename T>
__global__ __launch_bounds__(kProbitTile) void k_censor_latent(const int64_t *__restrict__ pos, const int32_t *__restrict__ ccol,
                                                               const int32_t *__restrict__ crow, const int8_t *__restrict__ sign,
                                                               int64_t nlist, const double *__restrict__ vals,
                                                               const T *__restrict__ items, const T *__restrict__ other, int kt,
                                                               uint32_t iter, uint32_t tag, double mean, double sqrt_alpha,
                                                               double inv_sqrt_alpha, double *__restrict__ z,
                                                               unsigned long long *__restrict__ fail)
{
    __shared__ int64_t s_col[kProbitTile];
    __shared__ int32_t s_row[kProbitTile];
    __shared__ double s_m[kProbitTile];
    const int64_t q0 = (int64_t)blockIdx.x * kProbitTile;
    const int n = (int)(nlist - q0 < kProbitTile ? nlist - q0 : kProbitTile);
    const int64_t q = q0 + threadIdx.x;
    if ((int)threadIdx.x < n) { s_col[threadIdx.x] = ccol[q]; s_row[threadIdx.x] = crow[q]; }
    __syncthreads();
    probit_tile_dots<K, T>(s_col, s_row, n, items, other, kt, s_m);
    __syncthreads();
    if ((int)threadIdx.x < n) {
        const int64_t p = pos[q];
        const double s = (double)sign[q], b = vals[p];
        const double e = (b - mean) - s_m[threadIdx.x];
        const double a = s * (sqrt_alpha * e);                       // t ~ N(0, 1) | t > a is sqrt(alpha) s (z - mean - m)
        double d = probit_truncated(p, iter, tag, a);
        if (d < 0.0) { d = kProbitCapValue; *fail = (unsigned long long)p; }      // (plain store: any of the failing ratings)
        z[p] = b + s * (d * inv_sqrt_alpha);
    }
}

}  // namespace bpmf
