// kernels_gather.h -- what the kernels that visit every rating of a side share (k_train_sse in kernels_noise.h, the probit
// kernels in kernels_probit.h, k_link_residual in kernels_link.h): the lane geometry of a gathered dot product x_c . y_r, the search
// for a rating's column, and the dot products of a tile of consecutive ratings.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmf {

template <int K, typename T>
struct SseGeo {
    static constexpr int E = sizeof(T) == 8 ? 2 : 4;       // elements per vector load (double2 / float4)
    static constexpr int NV = K / E;                       // vector loads per factor column
    static constexpr int G = NV < 16 ? NV : 16;            // lanes per rating (a power of two that divides 64)
    static constexpr int V = NV / G;                       // vector loads per lane and operand
    static_assert(NV % G == 0 && 64 % G == 0, "SseGeo");
};

// the largest c in [lo, ncols) with cp[c] <= p, given cp[lo] <= p < cp[ncols]: empty columns are stepped over
__device__ __forceinline__ int64_t sse_column(const int64_t *__restrict__ cp, int64_t lo, int64_t ncols, int64_t p)
{
    int64_t step = 1, hi = lo + 1;
    while (hi < ncols && cp[hi] <= p) { lo = hi; step <<= 1; hi = lo + step; }
    if (hi > ncols) hi = ncols;
    while (hi - lo > 1) {
        const int64_t m = (lo + hi) >> 1;
        if (cp[m] <= p) lo = m; else hi = m;
    }
    return lo;
}

template <typename T> struct SseVec;
template <> struct SseVec<double> { using type = double2; };
template <> struct SseVec<float> { using type = float4; };


constexpr int kProbitTile = 256;            // ratings per workgroup = threads per workgroup

// ratings a group of G lanes keeps in flight: 2 operands x V vector loads x 4 VGPRs each, at most 64 VGPRs of loads
template <int K, typename T>
struct ProbitGeo {
    using S = SseGeo<K, T>;
    static constexpr int U = S::V >= 4 ? 2 : 4;
    static constexpr int RPW = kProbitTile / S::G;          // groups per workgroup
    static constexpr int PER = kProbitTile / RPW;           // ratings per group and tile (= G)
    static_assert(PER % U == 0, "ProbitGeo");
};

// phase 1: m[i] = items[col[i]] . other[row[i]] for the n <= kProbitTile ratings of a tile whose columns / rows wait in LDS
template <int K, typename T>
__device__ __forceinline__ void probit_tile_dots(const int64_t *col, const int32_t *row, int n, const T *__restrict__ items,
                                                 const T *__restrict__ other, int kt, double *m)
{
    using Geo = SseGeo<K, T>;
    using PG = ProbitGeo<K, T>;
    using Vec = typename SseVec<T>::type;
    constexpr int G = Geo::G, V = Geo::V, U = PG::U;
    const int grp = threadIdx.x / G, lane = threadIdx.x % G;
    for (int j0 = 0; j0 < PG::PER; j0 += U) {
        if (grp + PG::RPW * j0 >= n) break;                                    // (uniform over the group)
        Vec a[U][V], b[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = grp + PG::RPW * (j0 + u);
            const int ii = i < n ? i : n - 1;                                  // (a ragged tail repeats the last rating: in bounds, not stored)
            const Vec *x = reinterpret_cast<const Vec *>(items + (size_t)col[ii] * K);
            const Vec *y = reinterpret_cast<const Vec *>(other + (size_t)row[ii] * K);
#pragma unroll
            for (int v = 0; v < V; ++v) { a[u][v] = x[lane + G * v]; b[u][v] = y[lane + G * v]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double d = 0.0;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int e = (lane + G * v) * Geo::E;
                if constexpr (Geo::E == 2) {
                    if (e < kt) d = fma(a[u][v].x, b[u][v].x, d);
                    if (e + 1 < kt) d = fma(a[u][v].y, b[u][v].y, d);
                } else {
                    if (e < kt) d = fma((double)a[u][v].x, (double)b[u][v].x, d);
                    if (e + 1 < kt) d = fma((double)a[u][v].y, (double)b[u][v].y, d);
                    if (e + 2 < kt) d = fma((double)a[u][v].z, (double)b[u][v].z, d);
                    if (e + 3 < kt) d = fma((double)a[u][v].w, (double)b[u][v].w, d);
                }
            }
#pragma unroll
            for (int sh = G / 2; sh >= 1; sh >>= 1) d += __shfl_xor(d, sh);
            const int i = grp + PG::RPW * (j0 + u);
            if (lane == 0 && i < n) m[i] = d;
        }
    }
}

}  // namespace bpmf
