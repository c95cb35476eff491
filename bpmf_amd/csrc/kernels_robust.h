// kernels_robust.h -- Student-t noise (bpmf_hip_side_set_robust, capi_robust.hip; one translation unit: krobust.hip).
// DESIGN.md section 21 has the model.
//
//   k_robust_weights     the weight step of one half-iteration: for every rating p of the side (column c, row r, value r_p)
//                            d = r_p - mean,  m = x_c . y_r,  e = d - m,  q = sqrt(alpha) e,  b = (nu + q q) / 2
//                            w_p = g / b,  g ~ Gamma((nu + 1) / 2, 1)
//                        and stores sw_p = sqrt(w_p), zw_p = sw_p d -- the two arrays of a side with per-rating weights (section 20),
//                        which the weighted forms of the column samplers read behind it in the same queue.
//   k_robust_accumulate  wsum[p] += sw[p] sw[p]: the running sum of the posterior-mean weight, one thread per rating.
//
// k_robust_weights has the shape of k_probit_latent (kernels_probit.h): tiles of kProbitTile consecutive ratings, one tile per
// workgroup (work balanced over ratings, not columns), in two phases:
//   1. the columns of the tile's ratings from one search per rating, galloping from the column of the tile's first rating; they and the
//      row indices wait in LDS; probit_tile_dots (kernels_gather.h, unchanged) forms the dot products m.
//   2. thread i owns rating i of the tile: the Gamma draw, two coalesced 8-byte stores per lane.
// fp64 throughout.  Slots k >= kt (a padded num_latent) are skipped.  No atomics: w_p depends on (p, iter, tag, alpha, nu, mean) and
// the factors only, never on the grid.
//
// The draw is Marsaglia-Tsang for a shape a >= 1 (nu >= 1: no boost step) WITHOUT the squeeze test: one comparison per attempt.
// tests/robust_ref.py restates it decision for decision.  Everything in robust_gamma and in phase 2 is compiled with
// `fp contract(off)`: the restatement is numpy, where no product meets a sum in one rounding, so none does here -- c x + 1, the
// four terms of the acceptance bound x x / 2 + dd - dd v + dd ln v, nu + q q, d - m.  (The dot product m itself is a chain of
// fma in probit_tile_dots, as it is for the probit and censored draws; its difference from numpy's sum is what the tests' bar on
// sw / zw covers.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_gather.h"     // kProbitTile, sse_column, probit_tile_dots
#include "philox.h"

namespace bpmf {

constexpr int kRobustMaxAttempts = 64;      // an attempt is accepted with probability >= 0.95 for a >= 1: the cap is reached with probability < 2^-270 per rating

// g ~ Gamma(a, 1), a >= 1, for rating p; dd = a - 1/3 and c = 1 / sqrt(9 dd) come from the host.  Returns g > 0, or -1 when the cap
// was reached.
//   attempt n: x = sqrt(-2 ln u1) cospi(2 u2) from the Philox block (p lo, p hi, iter, 2 n; 42, tag), u1 = 1 - canonical53(w3, w2)
//              in (0, 1], u2 = canonical53(w1, w0);   v = (1 + c x)^3, rejected if v <= 0;
//              u = 1 - canonical53(w1, w0) of the block (p lo, p hi, iter, 2 n + 1; 42, tag);
//              accepted if ln u < x x / 2 + dd - dd v + dd ln v;   then g = dd v
// (cos 2 pi u2 as cospi(2 u2): the argument 2 u2 is exact, no 2 pi to round)
__device__ __forceinline__ double robust_gamma(int64_t p, uint32_t iter, uint32_t tag, double dd, double c)
{
#pragma clang fp contract(off)
    const uint32_t plo = (uint32_t)((uint64_t)p & 0xFFFFFFFFull), phi = (uint32_t)((uint64_t)p >> 32);
    for (int n = 0; n < kRobustMaxAttempts; ++n) {
        const Philox4 w = philox4x32_10(plo, phi, iter, (uint32_t)(2 * n), 42u, tag);
        const double u1 = 1.0 - canonical53(w.w[3], w.w[2]);
        const double u2 = canonical53(w.w[1], w.w[0]);
        const double x = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
        const double t = 1.0 + c * x;
        const double v = (t * t) * t;
        if (v <= 0.0) continue;
        const Philox4 w2 = philox4x32_10(plo, phi, iter, (uint32_t)(2 * n + 1), 42u, tag);
        const double u = 1.0 - canonical53(w2.w[1], w2.w[0]);
        const double bound = ((0.5 * (x * x) + dd) - dd * v) + dd * log(v);
        if (log(u) < bound) return dd * v;
    }
    return -1.0;
}

template <int K, typename T>
__global__ __launch_bounds__(kProbitTile) void k_robust_weights(const int64_t *__restrict__ colptr, int64_t ncols,
                                                                const int32_t *__restrict__ rowidx, const double *__restrict__ vals,
                                                                int64_t nnz, const T *__restrict__ items, const T *__restrict__ other,
                                                                int kt, uint32_t iter, uint32_t tag, double mean, double sqrt_alpha,
                                                                double nu, double dd, double c, double *__restrict__ sw,
                                                                double *__restrict__ zw, unsigned long long *__restrict__ fail)
{
#pragma clang fp contract(off)
    __shared__ int64_t s_col[kProbitTile];
    __shared__ int32_t s_row[kProbitTile];
    __shared__ double s_m[kProbitTile];
    const int64_t p0 = (int64_t)blockIdx.x * kProbitTile;
    const int n = (int)(nnz - p0 < kProbitTile ? nnz - p0 : kProbitTile);
    const int64_t p = p0 + threadIdx.x;
    if ((int)threadIdx.x < n) {
        // the column of the tile's first rating (the same search in every lane: scalar loads), then a gallop from there
        const int64_t c0 = sse_column(colptr, 0, ncols, p0);
        s_col[threadIdx.x] = sse_column(colptr, c0, ncols, p);
        s_row[threadIdx.x] = rowidx[p];
    }
    __syncthreads();
    probit_tile_dots<K, T>(s_col, s_row, n, items, other, kt, s_m);
    __syncthreads();
    if ((int)threadIdx.x < n) {
        const double d = vals[p] - mean;
        const double e = d - s_m[threadIdx.x];
        const double q = sqrt_alpha * e;
        const double b = 0.5 * (nu + q * q);
        const double g = robust_gamma(p, iter, tag, dd, c);
        // the cap, or a residual that is not finite (the draw of g never sees the factors: a NaN factor shows here, in b): w = 1 and
        // the failure word raised (plain store: any of the failing ratings)
        double w = 1.0;
        if (g > 0.0 && b < __builtin_huge_val()) w = g / b;
        else *fail = (unsigned long long)p;
        const double s = sqrt(w);
        sw[p] = s;
        zw[p] = s * d;
    }
}

// (static: not a template)
static __global__ __launch_bounds__(256) void k_robust_accumulate(const double *__restrict__ sw, int64_t nnz, double *__restrict__ wsum)
{
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < nnz) { const double w = sw[p] * sw[p]; wsum[p] = wsum[p] + w; }
}

}  // namespace bpmf
