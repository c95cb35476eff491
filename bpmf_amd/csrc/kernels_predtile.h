// kernels_predtile.h -- what k_predict_block (kernels_predblock.h) and k_topn_scored (kernels_topn_score.h) share: the staged
// 64 x 64 tile of per-sample predictions and its running moments.  Device functions only, so that both translation units can
// include it; the two kernels run the same expressions in the same order, which is what makes their moments equal bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmf {

typedef double pred_d4 __attribute__((ext_vector_type(4)));
typedef double pred_d2 __attribute__((ext_vector_type(2)));

constexpr int kPredTile = 64;               // queries and candidates per workgroup
constexpr int kPredStep = 16;               // rows of k staged per slice (4 MFMA k-steps)
constexpr int kPredPitch = kPredStep + 2;   // row pitch in LDS (doubles): the 32 lanes of a half-wave's 8-byte read fall into 32 different bank pairs

// one staged slice (kPredStep rows of k) into the four 16 x 16 tiles of wave w: lane (kq, li) holds k = 4 kk + kq of query row li
// and of candidate row li of every tile (lane layout: link_mfma, kernels_link.h)
__device__ __forceinline__ void pred_slice_mfma(const double (*sQ)[kPredPitch], const double (*sC)[kPredPitch], int w, int li, int kq,
                                                pred_d4 (&acc)[4])
{
#pragma unroll
    for (int kk = 0; kk < kPredStep / 4; ++kk) {
        const double av = sQ[w * 16 + li][kk * 4 + kq];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, sC[j * 16 + li][kk * 4 + kq], acc[j], 0, 0, 0);
    }
}

// sample s + 1 = n of every element: the deviation from the mean of the n - 1 before it, then the sum (Welford written on the sum)
__device__ __forceinline__ void pred_fold(int s, const pred_d4 (&acc)[4], pred_d4 (&sum)[4], pred_d4 (&m2)[4])
{
    const double c1 = s > 0 ? 1.0 / (double)s : 0.0, c2 = (double)s / (double)(s + 1);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double p = acc[j][r], d = p - sum[j][r] * c1;
            m2[j][r] = fma(d * d, c2, m2[j][r]);
            sum[j][r] += p;
        }
}

}  // namespace bpmf
