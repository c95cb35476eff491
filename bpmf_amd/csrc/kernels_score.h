// kernels_score.h -- model comparison: the log pointwise predictive density and its WAIC correction for a list of observed cells over
// two sample rings (bpmf_hip_score_cells).  capi_score.hip; one translation unit: kscore.hip.  DESIGN.md section 30 has the
// definitions, the order of additions and the measurements.
//
// For a cell i = (q, c) with the observed value y_i, over the S kept samples of the two rings, with d_s = u_s(q) . v_s(c),
// p_s = mean_rating + d_s and l_s = log p(y_i | sample s):
//   lpd_i = log((1/S) sum_s exp l_s)           pw_i = sum_s (l_s - lbar)^2 / (S - 1)   [0 for S = 1]
//   gaussian              l_s = c0_s + (1/2) log w_i - (1/2) (a_s w_i) (y_i - p_s)^2         c0_s = (1/2) log(alpha_s / 2 pi),  a_s = alpha_s
//   gaussian, flag +-1    l_s = log Phi(flag sa_s (p_s - y_i))                               sa_s = sqrt(alpha_s)
//   student               l_s = c0_s - ((nu + 1) / 2) log1p(a_s (y_i - p_s)^2)               c0_s = lgamma((nu + 1) / 2) - lgamma(nu / 2)
//                                                                                                   + (1/2) log(alpha_s / (nu pi)),  a_s = alpha_s / nu
//   probit                l_s = log Phi(flag p_s)                                            flag = +1 for a positive label, else -1
// c0, a and sa are S doubles each, computed once on the host.
//
//   k_cells_logdens<G, KIND>   the walk of k_predict_cells<G, false> (kernels_predcells.h: the same grouping by query, staging of the
//       query's ring row through LDS, lane groups, 16-byte loads and order of additions, restated here so that that kernel is left
//       alone): mean and std come out of the same Welford recurrence.  After the butterfly every lane of a group holds d_s of the
//       group's kScoreCellsR cells; lane pl < PL = min(G, kScoreCellsR) of the group takes cells pl, pl + PL, .. and forms l_s for
//       them (one exp per cell and sample, and the log1p / erfc / erfcx of the kind), as the PROB form of k_predict_cells spreads its
//       erfc.  l_s is folded in s order into a streaming log-sum-exp -- a running maximum M and a sum Sg of exp(l - M): l > M rescales
//       Sg by exp(M - l), adds 1 and moves M, otherwise exp(l - M) is added -- and into a second Welford recurrence, whose sum of
//       squared deviations is pw_i (S - 1).  lpd_i = M + log Sg - log S.  No per-sample value is stored and no atomics are used:
//       the bits of a cell depend on the cell, Kp, S and the kind alone.  The kinds are compile-time: the plain Gaussian form carries
//       no erfc and no log1p.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmf {

// the shape of k_predict_cells' walk (kernels_predcells.h: kCellsR, kCellsLds, pc_group, pc_chunk, pc_segment), restated: that header
// defines kernels that are not templates and belongs to one translation unit
constexpr int kScoreCellsR = 4;                // cells a lane group carries side by side
constexpr int kScoreLds = 2048;                // doubles of the staged query row (16 KiB per workgroup)
__host__ __device__ inline int sc_group(int Kp) { int g = 2; while (2 * g <= Kp / 2 && g < 64) g *= 2; return g; }
__host__ __device__ inline int sc_chunk(int Kp) { return kScoreLds / Kp; }
__host__ __device__ inline int sc_segment(int Kp) { return kScoreCellsR * 256 / sc_group(Kp); }

enum { kScoreGauss = 0, kScoreGaussFlags = 1, kScoreStudent = 2, kScoreProbit = 3 };

// log Phi(x), finite and accurate in both tails.  Left of -1 the scaled erfcx keeps the tail that erfc loses to underflow near
// x = -38: Phi(x) = erfcx(-x / sqrt 2) exp(-x^2 / 2) / 2.  Otherwise Phi(x) = 1 - erfc(x / sqrt 2) / 2 with at most 0.84 taken
// from 1, through log1p: the upper tail keeps its own relative accuracy down to where it underflows, and the result is then -0.
__device__ __forceinline__ double score_log_phi(double x)
{
    const double t = x * 0.70710678118654752440;
    if (x < -1.0) return log(0.5 * erfcx(-t)) - 0.5 * (x * x);
    return log1p(-0.5 * erfc(t));
}

struct ScoreCellsArgs {
    const double *qring, *cring;               // sample rings of the query / candidate side
    int64_t qstride, cstride;                  // doubles per column of either ring (max_samples x Kp)
    int Kp, S;
    double mean_rating;
    const int32_t *seg_q, *seg_beg, *seg_cnt;  // per workgroup: its query, its first cell in the sorted list, its cells (1 .. sc_segment)
    const int32_t *cand, *orig;                // per sorted cell: its candidate, its place in the caller's list
    const double *y, *w;                       // caller's order; w may be NULL (1)
    const int8_t *flag;                        // caller's order: kScoreGaussFlags -1 / 0 / +1, kScoreProbit -1 / +1; else unused
    const double *c0, *as, *sa;                // per sample (see above); sa for kScoreGaussFlags alone
    double hnu1;                               // (nu + 1) / 2, kScoreStudent
    double *mean, *std, *lpd, *pw;             // caller's order
};

template <int G, int KIND>
__global__ __launch_bounds__(256) void k_cells_logdens(ScoreCellsArgs a)
{
    __shared__ __attribute__((aligned(16))) double urow[kScoreLds];
    constexpr int NG = 256 / G;
    const int tid = threadIdx.x, grp = tid / G, g = tid % G;
    const int Kp = a.Kp, S = a.S, K2 = Kp >> 1, SC = sc_chunk(Kp);
    const int cnt = a.seg_cnt[blockIdx.x], beg = a.seg_beg[blockIdx.x];
    const double *uq = a.qring + (int64_t)a.seg_q[blockIdx.x] * a.qstride;

    const double2 *vrow[kScoreCellsR];
    bool ok[kScoreCellsR];
    constexpr int PL = G < kScoreCellsR ? G : kScoreCellsR, NP = kScoreCellsR / PL;   // the densities of a group's cells are shared by PL of its lanes
    const int pl = g % PL;
    double m[kScoreCellsR], m2[kScoreCellsR];
    double yv[NP], wv[NP], hlw[NP], fl[NP];                     // of the lane's own cells: y, w, (1/2) log w, the flag
    double lM[NP], lS[NP], lm[NP], lm2[NP];                     // log-sum-exp (maximum, sum) and Welford (mean, squared deviations) of l
#pragma unroll
    for (int r = 0; r < kScoreCellsR; ++r) {
        const int i = r * NG + grp;
        ok[r] = i < cnt;
        vrow[r] = reinterpret_cast<const double2 *>(a.cring + (int64_t)(ok[r] ? a.cand[beg + i] : 0) * a.cstride);
        m[r] = 0.0; m2[r] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int i = (k * PL + pl) * NG + grp;
        const bool have = i < cnt;
        const int o = have ? a.orig[beg + i] : 0;
        yv[k] = have ? a.y[o] : 0.0;
        wv[k] = 1.0; hlw[k] = 0.0; fl[k] = 0.0;
        if ((KIND == kScoreGauss || KIND == kScoreGaussFlags) && a.w && have) { wv[k] = a.w[o]; hlw[k] = 0.5 * log(wv[k]); }
        if (KIND == kScoreGaussFlags || KIND == kScoreProbit) fl[k] = have ? (double)a.flag[o] : (KIND == kScoreProbit ? 1.0 : 0.0);
        lM[k] = -__builtin_huge_val(); lS[k] = 0.0; lm[k] = 0.0; lm2[k] = 0.0;
    }

    for (int s0 = 0; s0 < S; s0 += SC) {
        const int sc = S - s0 < SC ? S - s0 : SC;
        __syncthreads();                                        // the previous chunk is read
        {
            const double2 *src = reinterpret_cast<const double2 *>(uq + (int64_t)s0 * Kp);
            double2 *dst = reinterpret_cast<double2 *>(urow);
            for (int e = tid; e < sc * K2; e += 256) dst[e] = src[e];
        }
        __syncthreads();
        for (int s = 0; s < sc; ++s) {
            const double2 *us = reinterpret_cast<const double2 *>(urow) + s * K2;
            const int64_t vo = (int64_t)(s0 + s) * K2;
            double part[kScoreCellsR];
#pragma unroll
            for (int r = 0; r < kScoreCellsR; ++r) part[r] = 0.0;
            for (int j = g; j < K2; j += G) {
                const double2 uu = us[j];
                double2 vv[kScoreCellsR];
#pragma unroll
                for (int r = 0; r < kScoreCellsR; ++r) if (ok[r]) vv[r] = vrow[r][vo + j];
#pragma unroll
                for (int r = 0; r < kScoreCellsR; ++r) if (ok[r]) part[r] = fma(uu.y, vv[r].y, fma(uu.x, vv[r].x, part[r]));
            }
#pragma unroll
            for (int r = 0; r < kScoreCellsR; ++r) {
#pragma unroll
                for (int off = G / 2; off >= 1; off >>= 1) part[r] += __shfl_xor(part[r], off);
                const double d = part[r], dl = d - m[r];
                m[r] += dl / (double)(s0 + s + 1);
                m2[r] = fma(dl, d - m[r], m2[r]);
            }
            const double c0 = a.c0[s0 + s];                     // (the same in every lane)
            const double as = KIND == kScoreProbit ? 0.0 : a.as[s0 + s];
            const double sa = KIND == kScoreGaussFlags ? a.sa[s0 + s] : 0.0;
#pragma unroll
            for (int k = 0; k < NP; ++k) {                      // every lane of the group holds d of its cells: lane pl takes cells pl, pl + PL, ..
                double d = part[k * PL];
#pragma unroll
                for (int x = 1; x < PL; ++x) d = pl == x ? part[k * PL + x] : d;
                const double p = a.mean_rating + d;
                double l;
                if (KIND == kScoreProbit) {
                    l = score_log_phi(fl[k] * p);
                } else if (KIND == kScoreStudent) {
                    const double e = yv[k] - p;
                    l = c0 - a.hnu1 * log1p(as * (e * e));
                } else {
                    const double e = yv[k] - p;
                    l = (c0 + hlw[k]) - 0.5 * (as * wv[k]) * (e * e);
                    if (KIND == kScoreGaussFlags) { if (fl[k] != 0.0) l = score_log_phi(fl[k] * sa * (p - yv[k])); }
                }
                const bool up = l > lM[k];
                const double t = exp(up ? lM[k] - l : l - lM[k]);
                lS[k] = up ? fma(lS[k], t, 1.0) : lS[k] + t;
                lM[k] = up ? l : lM[k];
                const double dl = l - lm[k];
                lm[k] += dl / (double)(s0 + s + 1);
                lm2[k] = fma(dl, l - lm[k], lm2[k]);
            }
        }
    }
    if (g == 0) {
#pragma unroll
        for (int r = 0; r < kScoreCellsR; ++r) {
            if (!ok[r]) continue;
            const int o = a.orig[beg + r * NG + grp];
            a.mean[o] = a.mean_rating + m[r];
            a.std[o] = S > 1 ? sqrt(m2[r] / (double)(S - 1)) : 0.0;
        }
    }
    if (g < PL) {
        const double logS = log((double)S);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = (k * PL + g) * NG + grp;
            if (i >= cnt) continue;
            const int o = a.orig[beg + i];
            a.lpd[o] = (lM[k] + log(lS[k])) - logS;
            a.pw[o] = S > 1 ? lm2[k] / (double)(S - 1) : 0.0;
        }
    }
}

}  // namespace bpmf
