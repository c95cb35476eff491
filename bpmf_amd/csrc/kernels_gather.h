// kernels_gather.h -- what the kernels that visit every rating of a side share (k_train_sse in kernels_noise.h, the probit
// kernels in kernels_probit.h): the lane geometry of a gathered dot product x_c . y_r and the search for a rating's column.
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

}  // namespace bpmf
