// kernels_ordinal.h -- ordinal probit likelihood with C levels and C - 1 cutpoints (bpmf_hip_side_set_ordinal, capi_ordinal.hip;
// one translation unit: kordinal.hip).  DESIGN.md section 23 has the model.
//
//   k_ordinal_latent   the latent step of one half-iteration: for every rating p of the side (column c, row r, level y)
//                          m = x_c . y_r,   z_p ~ N(m, 1) truncated to (g[y], g[y + 1]]
//                      z has the layout of the side's `vals`; the unchanged column samplers read it with mean 0, alpha 1.
//   k_ordinal_loglik   sum_p log[Phi(g[y + 1] - m) - Phi(g[y] - m)] for two cutpoint tables g and g' in one pass: one pair of
//                      partials per workgroup (a fixed tree), k_ordinal_loglik_final adds the pairs in a fixed order.  No atomics.
//   k_ordinal_prob     sum[c * nnz + q] += Phi(g[c + 1] - m_q) - Phi(g[c] - m_q) over the entries q of a test matrix and the levels c
//
// g is the table of C + 1 doubles g[0] = -inf < g[1] < ... < g[C - 1] < g[C] = +inf (C <= kOrdinalMaxLevels).  A workgroup
// copies it into LDS once: the level of a rating differs per lane, and an array among the kernel arguments indexed per lane
// would be copied to scratch.
//
// The three kernels work on tiles of kProbitTile consecutive ratings in the two phases of kernels_probit.h (phase 1, the
// gathered dot products, is probit_tile_dots itself).  fp64 throughout; fp32 factors are widened per element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_gather.h"     // sse_column, kProbitTile, probit_tile_dots
#include "philox.h"

namespace bpmf {

constexpr int kOrdinalMaxLevels = 16;
constexpr double kOrdinalTail = 37.0;                       // beyond it erfc(a / sqrt 2) leaves the normal range of a double
constexpr double kOrdinalRsqrt2 = 0.70710678118654752440;   // 1 / sqrt 2
constexpr double kOrdinalSqrt2 = 1.41421356237309504880;
constexpr double kOrdinalHalfLog2Pi = 0.91893853320467274178;
constexpr double kOrdinalTiny = 2.2250738585072014e-308;    // the smallest normal double

// log of the upper tail 1 - Phi(a) for a > kOrdinalTail: the asymptotic series phi(a) / a (1 - 1/a^2 + 3/a^4 - 15/a^6 + 105/a^8),
// whose first dropped term is 945 / a^10 < 2e-13
__device__ __forceinline__ double ordinal_log_tail(double a)
{
    const double r = 1.0 / (a * a);
    const double s = fma(r, fma(r, fma(r, fma(r, 105.0, -15.0), 3.0), -1.0), 1.0);
    return -0.5 * a * a - log(a) - kOrdinalHalfLog2Pi + log(s);
}

// log[Phi(b) - Phi(a)] for a < b (either may be infinite, not both).  The interval is reflected to the side where its ends are
// the larger in magnitude on the right (a + b >= 0): both erfc are then small numbers and their difference loses nothing to a 1.
//   a <= kOrdinalTail: log((erfc(a / sqrt 2) - erfc(b / sqrt 2)) / 2)
//   a >  kOrdinalTail: log_tail(a) + log1p(-exp(log_tail(b) - log_tail(a)))
__device__ __forceinline__ double ordinal_logmass(double a, double b)
{
    if (a + b < 0.0) { const double t = a; a = -b; b = -t; }
    if (a > kOrdinalTail) {
        const double la = ordinal_log_tail(a);
        if (!(b < INFINITY)) return la;
        return la + log1p(-exp(ordinal_log_tail(b) - la));
    }
    return log(0.5 * (erfc(a * kOrdinalRsqrt2) - erfc(b * kOrdinalRsqrt2)));
}

// Phi(b) - Phi(a), the same reflection (the far tail is below the smallest double that matters for a probability: exp of the above)
__device__ __forceinline__ double ordinal_mass(double a, double b)
{
    if (a + b < 0.0) { const double t = a; a = -b; b = -t; }
    if (a > kOrdinalTail) return exp(ordinal_logmass(a, b));
    return 0.5 * (erfc(a * kOrdinalRsqrt2) - erfc(b * kOrdinalRsqrt2));
}

// t ~ N(0, 1) | a < t <= b for rating p, by inversion: ONE Philox block (p lo, p hi, iter, 0; 42, tag), u = canonical53(w1, w0)
// in [0, 1), no rejection loop.  After the reflection of ordinal_logmass, with E_x = erfc(x / sqrt 2):
//   a <= kOrdinalTail: v = (1 - u) E_a + u E_b, a convex combination of two numbers of one sign (no cancellation), at least the
//                      smallest normal double;  t = sqrt 2 erfcinv(v).
//                      v > 1 (possible for a < 0 only: t lies left of 0, where v closes in on 2 and its spacing 2^-52 is all the
//                      resolution the draw has): the same map through the other tail, v' = 2 - v = (1 - u) erfc(-a / sqrt 2) +
//                      u erfc(-b / sqrt 2) formed from its own two erfc, t = -sqrt 2 erfcinv(v').
//   a >  kOrdinalTail: the density on (a, b) is e^{-a (t - a)} to 1 / (2 a^2):  t = a - log1p(-u (1 - e^{-a (b - a)})) / a
// t is clamped to [a, b] and reflected back.  Finite for all finite a or b.
__device__ __forceinline__ double ordinal_truncated(int64_t p, uint32_t iter, uint32_t tag, double a, double b)
{
    const uint32_t plo = (uint32_t)((uint64_t)p & 0xFFFFFFFFull), phi = (uint32_t)((uint64_t)p >> 32);
    const Philox4 w = philox4x32_10(plo, phi, iter, 0u, 42u, tag);
    const double u = canonical53(w.w[1], w.w[0]);
    const bool refl = a + b < 0.0;
    if (refl) { const double t = a; a = -b; b = -t; }
    double t;
    if (a > kOrdinalTail) {
        const double span = -expm1(-a * (b - a));                      // 1 - e^{-a (b - a)} in (0, 1]; b = +inf: 1
        t = a - log1p(-u * span) / a;
    } else {
        const double v = fma(1.0 - u, erfc(a * kOrdinalRsqrt2), u * erfc(b * kOrdinalRsqrt2));
        if (v > 1.0) {
            const double v2 = fma(1.0 - u, erfc(-a * kOrdinalRsqrt2), u * erfc(-b * kOrdinalRsqrt2));
            t = -kOrdinalSqrt2 * erfcinv(fmax(v2, kOrdinalTiny));
        } else {
            t = kOrdinalSqrt2 * erfcinv(fmax(v, kOrdinalTiny));
        }
    }
    t = fmin(fmax(t, a), b);
    return refl ? -t : t;
}

// the cutpoint table of the workgroup: C + 1 doubles from global memory into LDS (the caller synchronises)
__device__ __forceinline__ void ordinal_stage(const double *__restrict__ g, int nlev, double *s_g)
{
    if ((int)threadIdx.x <= nlev) s_g[threadIdx.x] = g[threadIdx.x];
}

template <int K, typename T>
__global__ __launch_bounds__(kProbitTile) void k_ordinal_latent(const int64_t *__restrict__ colptr, int64_t ncols,
                                                                const int32_t *__restrict__ rowidx, const uint8_t *__restrict__ level,
                                                                int64_t nnz, const T *__restrict__ items, const T *__restrict__ other,
                                                                int kt, uint32_t iter, uint32_t tag, const double *__restrict__ g, int nlev,
                                                                double *__restrict__ z, unsigned long long *__restrict__ fail)
{
    __shared__ int64_t s_col[kProbitTile];
    __shared__ int32_t s_row[kProbitTile];
    __shared__ double s_m[kProbitTile];
    __shared__ double s_g[kOrdinalMaxLevels + 1];
    const int64_t p0 = (int64_t)blockIdx.x * kProbitTile;
    const int n = (int)(nnz - p0 < kProbitTile ? nnz - p0 : kProbitTile);
    const int64_t p = p0 + threadIdx.x;
    ordinal_stage(g, nlev, s_g);
    if ((int)threadIdx.x < n) {
        const int64_t c0 = sse_column(colptr, 0, ncols, p0);
        s_col[threadIdx.x] = sse_column(colptr, c0, ncols, p);
        s_row[threadIdx.x] = rowidx[p];
    }
    __syncthreads();
    probit_tile_dots<K, T>(s_col, s_row, n, items, other, kt, s_m);
    __syncthreads();
    if ((int)threadIdx.x < n) {
        const int y = level[p];                                         // < nlev (checked on the host when the side was set)
        const double lo = s_g[y], hi = s_g[y + 1];
        const double m = s_m[threadIdx.x];
        double zz;
        if (m - m == 0.0) {                                             // m is finite
            zz = m + ordinal_truncated(p, iter, tag, lo - m, hi - m);
            zz = fmin(fmax(zz, lo), hi);                                // (the sum may round across an end by an ulp)
        } else {
            zz = 0.0; *fail = (unsigned long long)p;                    // (plain store: any of the failing ratings)
        }
        z[p] = zz;
    }
}

// partial[2 b] / partial[2 b + 1]: the sums of workgroup b under the tables g0 / g1
template <int K, typename T>
__global__ __launch_bounds__(kProbitTile) void k_ordinal_loglik(const int64_t *__restrict__ colptr, int64_t ncols,
                                                                const int32_t *__restrict__ rowidx, const uint8_t *__restrict__ level,
                                                                int64_t nnz, const T *__restrict__ items, const T *__restrict__ other,
                                                                int kt, const double *__restrict__ g0, const double *__restrict__ g1, int nlev,
                                                                double *__restrict__ partial)
{
    __shared__ int64_t s_col[kProbitTile];
    __shared__ int32_t s_row[kProbitTile];
    __shared__ double s_m[kProbitTile];
    __shared__ double s_g[2][kOrdinalMaxLevels + 1];
    __shared__ double red[2][kProbitTile / 64];
    static_assert(kProbitTile == 256, "the tree below adds the partials of exactly four waves");
    const int64_t p0 = (int64_t)blockIdx.x * kProbitTile;
    const int n = (int)(nnz - p0 < kProbitTile ? nnz - p0 : kProbitTile);
    const int64_t p = p0 + threadIdx.x;
    ordinal_stage(g0, nlev, s_g[0]);
    ordinal_stage(g1, nlev, s_g[1]);
    if ((int)threadIdx.x < n) {
        const int64_t c0 = sse_column(colptr, 0, ncols, p0);
        s_col[threadIdx.x] = sse_column(colptr, c0, ncols, p);
        s_row[threadIdx.x] = rowidx[p];
    }
    __syncthreads();
    probit_tile_dots<K, T>(s_col, s_row, n, items, other, kt, s_m);
    __syncthreads();
    double l0 = 0.0, l1 = 0.0;
    if ((int)threadIdx.x < n) {
        const int y = level[p];
        const double m = s_m[threadIdx.x];
        l0 = ordinal_logmass(s_g[0][y] - m, s_g[0][y + 1] - m);
        l1 = ordinal_logmass(s_g[1][y] - m, s_g[1][y + 1] - m);
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) { l0 += __shfl_xor(l0, sh); l1 += __shfl_xor(l1, sh); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = l0; red[1][threadIdx.x >> 6] = l1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partial[2 * (size_t)blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// one workgroup: thread i adds the pairs i, i + 256, ... in index order, then the tree of k_ordinal_loglik; out[0], out[1]
static __global__ __launch_bounds__(kProbitTile) void k_ordinal_loglik_final(const double *__restrict__ partial, int64_t n, double *__restrict__ out)
{
    __shared__ double red[2][kProbitTile / 64];
    static_assert(kProbitTile == 256, "the tree below adds the partials of exactly four waves");
    double l0 = 0.0, l1 = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kProbitTile) { l0 += partial[2 * i]; l1 += partial[2 * i + 1]; }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) { l0 += __shfl_xor(l0, sh); l1 += __shfl_xor(l1, sh); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = l0; red[1][threadIdx.x >> 6] = l1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        out[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

template <int K, typename T>
__global__ __launch_bounds__(kProbitTile) void k_ordinal_prob(const int32_t *__restrict__ tcol, const int32_t *__restrict__ trow,
                                                              int64_t nnz, const T *__restrict__ items, const T *__restrict__ other,
                                                              int kt, const double *__restrict__ g, int nlev, double *__restrict__ sum)
{
    __shared__ int64_t s_col[kProbitTile];
    __shared__ int32_t s_row[kProbitTile];
    __shared__ double s_m[kProbitTile];
    __shared__ double s_g[kOrdinalMaxLevels + 1];
    const int64_t q0 = (int64_t)blockIdx.x * kProbitTile;
    const int n = (int)(nnz - q0 < kProbitTile ? nnz - q0 : kProbitTile);
    const int64_t q = q0 + threadIdx.x;
    ordinal_stage(g, nlev, s_g);
    if ((int)threadIdx.x < n) { s_col[threadIdx.x] = tcol[q]; s_row[threadIdx.x] = trow[q]; }
    __syncthreads();
    probit_tile_dots<K, T>(s_col, s_row, n, items, other, kt, s_m);
    __syncthreads();
    if ((int)threadIdx.x < n) {
        const double m = s_m[threadIdx.x];
        for (int c = 0; c < nlev; ++c) sum[(size_t)c * (size_t)nnz + (size_t)q] += ordinal_mass(s_g[c] - m, s_g[c + 1] - m);
    }
}

}  // namespace bpmf
