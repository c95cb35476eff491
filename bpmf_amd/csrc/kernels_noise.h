// kernels_noise.h -- sum of squared training residuals for the adaptive noise precision (bpmf_hip_train_sse, capi_noise.hip;
// one translation unit: knoise.hip).
//
//   SSE = sum over the ratings (r, c, v) of one side of (v - (mean + x_c . y_r))^2
//
// x = the side's current factors, y = the other side's.  Read-only; no atomics, one fixed order of summation, so the
// result is the same bits on every call.
//
//   k_train_sse        the ratings are cut into equal contiguous chunks, one per workgroup (work balanced over ratings, not
//                      columns: a side of 483 500 columns with ~1.7 ratings each and one of 5 775 with ~142 cost the same per
//                      rating).  G lanes share a rating: lane l loads vectors l, l + G, ... of both factor columns (16 lanes x
//                      16 B = 256 contiguous bytes per row and load), the G partial dot products meet in a butterfly.  The
//                      column of a rating comes from the column pointers: a galloping search from the column of the group's
//                      previous rating (the first one from column 0).  fp64 throughout; fp32 factors are widened per element,
//                      as k_predict does.  Slots k >= kt (a padded num_latent) are skipped.  One partial per workgroup.
//   k_train_sse_final  one workgroup sums the partials in a fixed order
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_gather.h"      // SseGeo, SseVec, sse_column (shared with kernels_probit.h)

namespace bpmf {

constexpr int kSseThreads = 256;

template <int K, typename T>
__global__ __launch_bounds__(kSseThreads) void k_train_sse(const int64_t *__restrict__ colptr, int64_t ncols,
                                                           const int32_t *__restrict__ rowidx, const double *__restrict__ vals,
                                                           int64_t nnz, int64_t span, const T *__restrict__ items,
                                                           const T *__restrict__ other, int kt, double mean,
                                                           double *__restrict__ partial)
{
    using Geo = SseGeo<K, T>;
    using Vec = typename SseVec<T>::type;
    constexpr int G = Geo::G, RPW = kSseThreads / G;
    __shared__ double red[kSseThreads / 64];
    const int grp = threadIdx.x / G, lane = threadIdx.x % G;
    const int64_t p0 = (int64_t)blockIdx.x * span;
    const int64_t p1 = p0 + span < nnz ? p0 + span : nnz;
    double acc = 0.0;
    int64_t col = 0;
    for (int64_t p = p0 + grp; p < p1; p += RPW) {
        col = sse_column(colptr, col, ncols, p);
        const Vec *x = reinterpret_cast<const Vec *>(items + (size_t)col * K);
        const Vec *y = reinterpret_cast<const Vec *>(other + (size_t)rowidx[p] * K);
        double d = 0.0;
#pragma unroll
        for (int v = 0; v < Geo::V; ++v) {
            const int q = lane + G * v, e = q * Geo::E;
            const Vec a = x[q], b = y[q];
            if constexpr (Geo::E == 2) {
                if (e < kt) d = fma(a.x, b.x, d);
                if (e + 1 < kt) d = fma(a.y, b.y, d);
            } else {
                if (e < kt) d = fma((double)a.x, (double)b.x, d);
                if (e + 1 < kt) d = fma((double)a.y, (double)b.y, d);
                if (e + 2 < kt) d = fma((double)a.z, (double)b.z, d);
                if (e + 3 < kt) d = fma((double)a.w, (double)b.w, d);
            }
        }
#pragma unroll
        for (int sh = G / 2; sh >= 1; sh >>= 1) d += __shfl_xor(d, sh);   // (a + b == b + a: every lane of the group holds the same sum)
        if (lane == 0) {
            const double r = vals[p] - (d + mean);
            acc = fma(r, r, acc);
        }
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) acc += __shfl_xor(acc, sh);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kSseThreads) void k_train_sse_final(const double *__restrict__ partial, int n, double *__restrict__ out)
{
    __shared__ double red[kSseThreads / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kSseThreads) s += partial[i];
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace bpmf
