// kernels_probit.h -- probit likelihood for binary matrices (bpmf_hip_side_set_probit, capi_probit.hip; one translation unit:
// kprobit.hip).  DESIGN.md section 12 has the model.
//
//   k_probit_sign      s_p = +1 if vals[p] > threshold else -1, once per side
//   k_probit_latent    the Albert-Chib step of one half-iteration: for every rating p of the side (column c, row r)
//                          m = x_c . y_r,   z_p ~ N(m, 1) truncated to the half line of s_p
//                      z has the layout of the side's `vals`; the unchanged column samplers read it with mean 0, alpha 1.
//   k_probit_prob      sum[q] += Phi(x_c . y_r) over the entries q of a test matrix (posterior predictive of a positive)
//
// Both gather kernels work on tiles of kProbitTile consecutive ratings, one tile per workgroup (work balanced over ratings,
// not columns, like k_train_sse), in two phases:
//   1. G lanes share a rating: lane l loads vectors l, l + G, ... of both factor columns (16 lanes x 16 B = 256 contiguous
//      bytes per row and load), the G partial dot products meet in a butterfly, lane 0 of the group puts m into LDS.  A group
//      has U ratings in flight (the loads of all U are issued before the first product), which k_train_sse's loop has not.
//      The columns of the tile's ratings come from one search per rating, galloping from the column of the tile's first
//      rating; they and the row indices wait in LDS.
//   2. thread i owns rating i of the tile: draw (or Phi), one coalesced 8-byte store per lane.  The rejection loop of the draw
//      runs on 64 ratings per wave instead of on 64 / G.
// fp64 throughout; fp32 factors are widened per element.  Slots k >= kt (a padded num_latent) are skipped.  No atomics: z_p
// depends on (p, iter, tag) and the factors only, never on the grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_gather.h"     // SseGeo, SseVec, sse_column (shared with k_train_sse); kProbitTile, ProbitGeo, probit_tile_dots (shared with k_link_residual)
#include "philox.h"

namespace bpmf {

constexpr int kProbitMaxAttempts = 64;      // a rejected attempt has probability <= 1/4: the cap is reached with probability < 2^-128 per rating
constexpr double kProbitCapValue = 1.0;     // |z| stored for a rating whose draw ran into the cap (with the failure word raised)

// (static: not a template, and kernels_censor.h brings this header into a second translation unit for probit_truncated)
static __global__ __launch_bounds__(256) void k_probit_sign(const double *__restrict__ vals, int64_t nnz, double threshold, int8_t *__restrict__ sign)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < nnz) sign[p] = vals[p] > threshold ? (int8_t)1 : (int8_t)-1;
}

// t ~ N(0, 1) | t > a for rating p; returns t - a > 0 (so that z = s (t - a) with a = -s m), or -1 when the cap was reached.
//   attempt n: one Philox block (p lo, p hi, iter, n; 42, tag), u1 = 1 - canonical53(w3, w2) in (0, 1], u2 = canonical53(w1, w0)
//   a <= 0: Box-Muller, rho = sqrt(-2 ln u1), t1 = rho cos 2 pi u2, t2 = rho sin 2 pi u2: t1 if t1 > a, else t2 if t2 > a
//   a > 0:  Robert's exponential proposal, lambda = (a + sqrt(a^2 + 4)) / 2, t = a - ln(u1) / lambda, accepted if
//           u2 <= exp(-(t - lambda)^2 / 2)
// (cos 2 pi u2 / sin 2 pi u2 as sincospi(2 u2): the argument 2 u2 is exact, no 2 pi to round)
// (a > 0 and u1 = 1, i.e. the two words of canonical53 both 0: ln u1 = 0, t = a, and an accepted t gives t - a = 0, a score of
//  +-0 that carries the label only in its sign bit.  Probability 2^-64 per tail attempt; the restatement does the same.)
__device__ __forceinline__ double probit_truncated(int64_t p, uint32_t iter, uint32_t tag, double a)
{
    const uint32_t plo = (uint32_t)((uint64_t)p & 0xFFFFFFFFull), phi = (uint32_t)((uint64_t)p >> 32);
    const bool tail = a > 0.0;
    const double lambda = 0.5 * (a + sqrt(a * a + 4.0));
    for (int n = 0; n < kProbitMaxAttempts; ++n) {
        const Philox4 w = philox4x32_10(plo, phi, iter, (uint32_t)n, 42u, tag);
        const double u1 = 1.0 - canonical53(w.w[3], w.w[2]);
        const double u2 = canonical53(w.w[1], w.w[0]);
        const double lg = log(u1);
        if (tail) {
            const double t = a - lg / lambda;
            const double d = t - lambda;
            if (u2 <= exp(-0.5 * (d * d))) return t - a;
        } else {
            const double rho = sqrt(-2.0 * lg);
            double sn, cs;
            sincospi(2.0 * u2, &sn, &cs);
            const double t1 = rho * cs, t2 = rho * sn;
            if (t1 > a) return t1 - a;
            if (t2 > a) return t2 - a;
        }
    }
    return -1.0;
}

template <int K, typename T>
__global__ __launch_bounds__(kProbitTile) void k_probit_latent(const int64_t *__restrict__ colptr, int64_t ncols,
                                                               const int32_t *__restrict__ rowidx, const int8_t *__restrict__ sign,
                                                               int64_t nnz, const T *__restrict__ items, const T *__restrict__ other,
                                                               int kt, uint32_t iter, uint32_t tag, double *__restrict__ z,
                                                               unsigned long long *__restrict__ fail)
{
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
        const double s = (double)sign[p];
        const double mu = s * s_m[threadIdx.x];
        double d = probit_truncated(p, iter, tag, -mu);
        if (d < 0.0) { d = kProbitCapValue; *fail = (unsigned long long)p; }      // (plain store: any of the failing ratings)
        z[p] = s * d;
    }
}

// Phi(m) = erfc(-m / sqrt 2) / 2
template <int K, typename T>
__global__ __launch_bounds__(kProbitTile) void k_probit_prob(const int32_t *__restrict__ tcol, const int32_t *__restrict__ trow,
                                                             int64_t nnz, const T *__restrict__ items, const T *__restrict__ other,
                                                             int kt, double *__restrict__ sum)
{
    __shared__ int64_t s_col[kProbitTile];
    __shared__ int32_t s_row[kProbitTile];
    __shared__ double s_m[kProbitTile];
    const int64_t q0 = (int64_t)blockIdx.x * kProbitTile;
    const int n = (int)(nnz - q0 < kProbitTile ? nnz - q0 : kProbitTile);
    const int64_t q = q0 + threadIdx.x;
    if ((int)threadIdx.x < n) { s_col[threadIdx.x] = tcol[q]; s_row[threadIdx.x] = trow[q]; }
    __syncthreads();
    probit_tile_dots<K, T>(s_col, s_row, n, items, other, kt, s_m);
    __syncthreads();
    if ((int)threadIdx.x < n) sum[q] += 0.5 * erfc(-s_m[threadIdx.x] * 0.70710678118654752440);
}

}  // namespace bpmf
