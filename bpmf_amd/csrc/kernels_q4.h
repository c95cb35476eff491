// k_sample4<K>: four columns per wave, the whole column update on the 4x4x4 f64 MFMA shape.
//
// v_mfma_f64_4x4x4_4b_f64 computes four INDEPENDENT 4x4x4 products.  k_sample1 gives the four
// blocks four different groups of ratings of ONE column (and has to add the four partial Grams,
// then factorises on the VALU).  Here block b belongs to COLUMN b of a group of four work items:
//   * Gram: an instruction adds 4 ratings of each of the 4 columns to one 4x4 block (g, g') of
//     their Grams -- the same 36 instructions per 16 ratings, no cross-block sum afterwards, and
//     the 36 accumulator registers now hold FOUR matrices;
//   * Lambda* = LambdaF + alpha G stays in those registers.  Blocked right-looking Cholesky
//     Lambda* = R^T R with 4x4 blocks, the four columns in lockstep: the 4x4 diagonal block is
//     factored and inverted redundantly by the 16 lanes of its column (its 10 entries arrive through
//     ds_bpermute), the panel  R_sJ = W^T A_sJ  and the trailing updates  A_IJ -= R_sI^T R_sJ  are
//     MFMAs whose operands are accumulator registers as they are (a D-layout register used as the
//     A operand is the transposed block, which is exactly what both products need);
//   * the forward solve rides in the same loop on a ninth "block column" (b as 4x4 blocks with one
//     live column), the backward solve needs the blocks of R untransposed: one bpermute each;
//   * natural (contiguous) 4-index blocks, so R is THE Cholesky factor of the reference's
//     Lambda* and x = R^-1 (R^-T b + z) is the reference's sample for the same z (c++/sample.cpp:306-323).
// Per column this replaces ~1 900 VALU instructions of assembly + factorisation + solves by ~600
// (of which ~230 are the normal draw) plus ~46 MFMAs.
//
// Lane l = 16 k + 4 b + x:  operand view (k, b, x): A_b[i = x][k], B_b[k][j = x];
//                           result view  (i = l >> 4, b, j = l & 3): D_b[i][j].
#pragma once
#include "kernels.h"

namespace bpmf {

template <int K>
struct Geo4 {
    static constexpr int NG = K / 4;                      // 4-index blocks per dimension
    static constexpr int NB = NG * (NG + 1) / 2;          // upper blocks incl. diagonal
    static constexpr int PART = (NB + NG) * 16;           // doubles one chunk of a heavy column parks (its 16 lanes)
    __host__ __device__ static constexpr int blk(int g, int g2) { return g * NG - (g * (g - 1)) / 2 + (g2 - g); }
    static constexpr int WPS = K == 32 ? 2 : 4;           // K = 32: 72 accumulators + two blocks of gathered operands (128 registers)
};

__device__ __forceinline__ double mfma44n(double a, double b, double c)   // c - a^T-view * b: the A operand negated
{
    return __builtin_amdgcn_mfma_f64_4x4x4f64(-a, b, c, 0, 0, 0);
}

// value held by lane (x = T) of every quad, to all four lanes of the quad (DPP quad_perm)
template <int T>
__device__ __forceinline__ int quad_bcast_i(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, T * 0x55, 0xF, 0xF, true);
}
template <int T>
__device__ __forceinline__ double quad_bcast_d(double v)
{
    const long long w = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)w, T * 0x55, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(w >> 32), T * 0x55, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

#define BPMF_Q4_KERNEL k_sample4
#define BPMF_Q4_WEIGHTED 0
#include "kernels_q4.inc"
#undef BPMF_Q4_KERNEL
#undef BPMF_Q4_WEIGHTED

// four columns per wave with per-rating weights (instantiated in units of their own, kw8.hip .. kw32.hip)
#define BPMF_Q4_KERNEL k_sample4w
#define BPMF_Q4_WEIGHTED 1
#include "kernels_q4.inc"
#undef BPMF_Q4_KERNEL
#undef BPMF_Q4_WEIGHTED

}  // namespace bpmf
