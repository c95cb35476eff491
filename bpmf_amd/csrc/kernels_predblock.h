// kernels_predblock.h -- dense blocks of posterior predictions from two sample rings, and what the prediction of rows unseen in
// training needs beside them (bpmf_hip_predict_block / bpmf_hip_newrows_*, capi_newrows.hip; one translation unit:
// kpredblock.hip).  DESIGN.md section 17 has the model.
//
// Both rings have the layout of bpmf_ring (ext_state.h): column c, sample s, row k at c * stride + s * Kp + k, fp64, Kp a
// multiple of 4, pad rows zero, stride = max_samples * Kp >= S * Kp.  For a query q and a candidate c, p_s = e_s(q) . v_s(c):
//   mean(q, c) = mean_rating + (1/S) sum_s p_s
//   var(q, c)  = sum_s (p_s - mean)^2 / (S - 1)  [0 for S = 1]  + w[c] / S  [when w is given]
//   std(q, c)  = sqrt(var)
// w[c] / S is the spread of a cold row's factors around their conditional mean (the second term of the law of total variance);
// w = NULL for two in-matrix rings.  The observation noise 1 / alpha is NOT part of std: a predictive interval for a rating adds it.
//
//   k_predict_block    a workgroup of four waves = 64 queries x 64 candidates; wave w owns queries 16 w .. 16 w + 15 and four
//                      16-wide candidate tiles.  Per sample the four tiles of p_s are accumulated on v_mfma_f64_16x16x4_f64 over
//                      Kp (lane layout: link_mfma, kernels_link.h); the operand slices (kPredStep rows of k of 64 queries and
//                      64 candidates) are staged ONCE per workgroup in LDS, the global loads of the next slice -- of the next
//                      sample after a sample's last -- are in flight while this one is multiplied (two LDS buffers, one
//                      barrier per slice).  After a sample's last slice every lane folds its 16 products into two running
//                      moments per element, in registers: the plain sum, and M2 by Welford's update written on the sum,
//                          M2 += (n - 1) / n * (p_n - sum_{n-1} / (n - 1))^2,   sum += p_n
//                      which keeps its digits when |p_s| >> spread (sum p, sum p^2 does not).  mean_rating stays out of the
//                      moments and is added at the store.  No nq x nc x S intermediate, no atomics: element (q, c) is
//                      accumulated in the order s ascending, k ascending inside the MFMA chain, whatever the ranges or the grid.
//                      Queries / candidates past the edge and slices past Kp are staged as zeros and not stored.
//   k_rowsq_add        w[c] += sum_j Y[c][j]^2, j ascending: with Y = V R^-1 (Lambda = R^T R; k_link_gemm_nn) this is the quadratic
//                      form v(c)^T Lambda^-1 v(c) = |R^-T v(c)|^2 (k_quadform_add of the design)
//   k_ring_add_mu      ring[i][slot][k] += mu[k], k < Kt: the mean of a projected row (the product F beta sits in the slot)
#pragma once
#include "kernels_predtile.h"               // the staged tile product and the moment update, shared with k_topn_scored

namespace bpmf {

struct PredBlockArgs {
    const double *qring, *cring;            // sample rings of the queries / the candidates
    int64_t qstride, cstride;               // doubles per column of either ring
    int Kp, S;
    double mean_rating;
    int64_t q_from, nq, c_from, nc;         // queries [q_from, q_from + nq), candidates [c_from, c_from + nc)
    const double *w;                        // per candidate column (indexed by the candidate's id), or NULL
    double *mean, *std;                     // nq x nc, row-major
};

__global__ __launch_bounds__(256) void k_predict_block(PredBlockArgs a)
{
    __shared__ __attribute__((aligned(16))) double sQ[2][kPredTile][kPredPitch];
    __shared__ __attribute__((aligned(16))) double sC[2][kPredTile][kPredPitch];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kPredTile, c0 = (int64_t)blockIdx.y * kPredTile;
    // staging role: row lr of either operand, four consecutive k from lk
    const int lr = t >> 2, lk = (t & 3) * 4;
    const bool q_ok = q0 + lr < a.nq, c_ok = c0 + lr < a.nc;
    const double *qrow = a.qring + (a.q_from + (q_ok ? q0 + lr : 0)) * a.qstride + lk;
    const double *crow = a.cring + (a.c_from + (c_ok ? c0 + lr : 0)) * a.cstride + lk;
    const int nk = (a.Kp + kPredStep - 1) / kPredStep;
    pred_d4 rq, rc;
    int ls = 0, lks = 0;                                                   // sample and slice of the next load
    auto load = [&]() {
        const int k = lks * kPredStep;
        const bool in = k + lk < a.Kp;                                     // (Kp is a multiple of 4: a 4-chunk is wholly in or out)
        const int64_t off = (int64_t)ls * a.Kp + k;
        rq = (q_ok && in) ? *reinterpret_cast<const pred_d4 *>(qrow + off) : pred_d4{0.0, 0.0, 0.0, 0.0};
        rc = (c_ok && in) ? *reinterpret_cast<const pred_d4 *>(crow + off) : pred_d4{0.0, 0.0, 0.0, 0.0};
        if (++lks == nk) { lks = 0; ++ls; }
    };
    auto store = [&](int buf) {
        // (a row starts at a multiple of 16 bytes, not of 32: two 16-byte stores per operand)
        *reinterpret_cast<pred_d2 *>(&sQ[buf][lr][lk]) = pred_d2{rq[0], rq[1]};
        *reinterpret_cast<pred_d2 *>(&sQ[buf][lr][lk + 2]) = pred_d2{rq[2], rq[3]};
        *reinterpret_cast<pred_d2 *>(&sC[buf][lr][lk]) = pred_d2{rc[0], rc[1]};
        *reinterpret_cast<pred_d2 *>(&sC[buf][lr][lk + 2]) = pred_d2{rc[2], rc[3]};
    };
    pred_d4 sum[4], m2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { sum[j] = pred_d4{0.0, 0.0, 0.0, 0.0}; m2[j] = pred_d4{0.0, 0.0, 0.0, 0.0}; }
    load();
    store(0);
    __syncthreads();
    int buf = 0;
    for (int s = 0; s < a.S; ++s) {
        pred_d4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = pred_d4{0.0, 0.0, 0.0, 0.0};
        for (int ks = 0; ks < nk; ++ks) {
            const bool more = ls < a.S;                                    // (uniform over the workgroup)
            if (more) load();
            pred_slice_mfma(sQ[buf], sC[buf], w, li, kq, acc);
            if (more) store(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
        pred_fold(s, acc, sum, m2);
    }
    const double S = (double)a.S;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t c = c0 + j * 16 + li;
        if (c >= a.nc) continue;
        const double wc = a.w ? a.w[a.c_from + c] / S : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t q = q0 + w * 16 + kq + 4 * r;
            if (q >= a.nq) continue;
            const double var = (a.S > 1 ? m2[j][r] / (S - 1.0) : 0.0) + wc;
            a.mean[q * a.nc + c] = a.mean_rating + sum[j][r] / S;
            a.std[q * a.nc + c] = sqrt(var);
        }
    }
}

// one thread per column: w[c] += Y[c][0]^2 + Y[c][1]^2 + ... in that order
__global__ __launch_bounds__(256) void k_rowsq_add(const double *__restrict__ Y, int64_t ldy, int n, int64_t ncols, double *__restrict__ w)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    const double *y = Y + c * ldy;
    double s = 0.0;
    for (int j = 0; j < n; ++j) s = fma(y[j], y[j], s);
    w[c] += s;
}

__global__ __launch_bounds__(256) void k_ring_add_mu(double *__restrict__ ring, int64_t stride, int slot, int Kp, int Kt, int64_t nrows,
                                                     const double *__restrict__ mu)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nrows * Kt) return;
    const int64_t i = e / Kt;
    const int k = (int)(e - i * Kt);
    ring[i * stride + (int64_t)slot * Kp + k] += mu[k];
}

}  // namespace bpmf
