// kernels_loo.h -- PSIS-LOO cross-validation: Pareto-smoothed importance sampling of the per-sample log densities of a list of observed
// cells over two sample rings (bpmf_hip_loo_cells) and of traces of log densities given by the host (bpmf_hip_loo_traces).
// capi_loo.hip; one translation unit: kloo.hip.  DESIGN.md section 32 has the rule, the order of additions and the measurements.
//
// For one trace l_0 .. l_{S-1} (the log density of the cell under kept sample s), 1 <= S <= kLooMaxSamples, let a_0 <= .. <= a_{S-1} be
// the l_s in increasing order.  Position i of that order holds the (i + 1)-th largest importance ratio, rho_i = a_0 - a_i <= 0 (the
// log ratio -l_s shifted so that its maximum is 0).
//   M = min(floor(S / 5), ceil(3 sqrt S)) <= kLooMaxTail, the tail: positions 0 .. M - 1; the cutoff c = rho_M, ec = exp(c)
//   x_j = exp(rho_{M-j}) - ec, j = 1 .. M, increasing: the excesses a generalised Pareto distribution is fitted to (Zhang & Stephens 2009)
//       m = 30 + floor(sqrt M) <= 64 (one lane each), x* = x_{floor(M/4 + 1/2)}
//       theta_j = 1 / x_M + (1 - sqrt(m / (j - 1/2))) / (3 x*),  k_j = (1/M) sum_i log1p(-theta_j x_i),  L_j = M (log(-theta_j / k_j) - k_j - 1)
//       w_j = exp(L_j - max L) / sum_j exp(L_j - max L),  theta^ = sum_j w_j theta_j,  k = (1/M) sum_i log1p(-theta^ x_i),  sigma = -k / theta^
//       khat = (k M + 5) / (M + 10)
//   lw_i = min(log(q_j + ec), 0) at the tail position i = M - j, q_j = sigma expm1(khat t_j) / khat (sigma t_j for |khat| < kLooTinyK),
//       t_j = -log1p(-(j - 1/2) / M); lw_i = rho_i at every other position
//   elpd_loo = logsumexp_i(lw_i + a_i) - logsumexp_i(lw_i),  lpd = logsumexp_i(a_i) - log S
// No smoothing (lw_i = rho_i everywhere) and khat = +infinity: M < 5, x_M = x_1, x* = 0, or an L_j, theta^, k, sigma or khat that is not
// finite.  A trace holding a value that is not finite gives NaN for its three outputs.
//
//   k_trace_psis<KIND>   one wave per trace, 64 * W threads per workgroup, P = loo_lds_doubles(S) doubles of LDS per wave (S rounded up to
//       a power of two, at least 128; W = 4 while the dynamic LDS stays <= 64 KiB: S <= 2048, else 2).  Phase 1 forms l_s from the d_s
//       = u_s . v_s that k_cell_traces left in the trace buffer, by the four forms of kernels_score.h (KIND = kLooTraces: l_s is loaded
//       as given).  Phase 2 sorts the wave's P values (+infinity behind the S) with a bitonic network in LDS -- log2 P (log2 P + 1) / 2
//       stages of P / 128 compare-exchanges per lane -- so that every later sum runs over the positions of the sorted order and does
//       not depend on where ties came from.  The tail's a_i stay in three registers per lane and their places in LDS take the x_j.
//       Lane j - 1 owns theta_j and adds its M terms in increasing i; every other sum adds positions (or j) lane, lane + 64, .. in
//       increasing order in a lane and then runs the butterfly xor 32 .. 1 of iv_wave_sum, so every lane holds the same bits and all
//       control flow is wave-uniform.  Every loop's trip count is fixed by S, M and m.  No atomics, no scratch; the bits of a trace
//       depend on the trace, S, the kind and its parameters alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_score.h"

namespace bpmf {

constexpr int kLooMaxSamples = 4096;           // a trace is at most 32 KiB of LDS
constexpr int kLooMaxTail = 192;               // M at kLooMaxSamples: three tail positions per lane
constexpr double kLooTinyK = 1e-30;            // below it expm1(khat t) / khat is t to the last bit
constexpr int kLooTraces = 4;                  // KIND beside kScoreGauss .. kScoreProbit: the traces hold l_s

__host__ __device__ inline int loo_lds_doubles(int S) { int p = 128; while (p < S) p *= 2; return p; }       // per wave
__host__ __device__ inline int loo_waves(int S) { return 4 * loo_lds_doubles(S) * 8 <= 65536 ? 4 : 2; }      // waves (traces) per workgroup
__host__ __device__ inline int loo_tail(int S)
{
    int r = 0;
    while ((int64_t)r * r < (int64_t)9 * S) ++r;                // ceil(3 sqrt S) = ceil(sqrt(9 S)), in integers
    const int f = S / 5;
    return f < r ? f : r;
}
__host__ __device__ inline int loo_isqrt(int M) { int r = 0; while ((r + 1) * (r + 1) <= M) ++r; return r; }

struct TracePsisArgs {
    const double *traces;                      // ntr x S, row-major: d_s, or l_s for kLooTraces
    int64_t ntr;
    int S;
    const int32_t *orig;                       // per trace: its place in y, w, flag and the outputs (NULL: the trace's own number)
    double mean_rating;
    const double *y, *w;                       // per place (kernels_score.h); w may be NULL (1)
    const int8_t *flag;                        // kScoreGaussFlags -1 / 0 / +1, kScoreProbit -1 / +1
    const double *c0, *as, *sa;                // per sample (kernels_score.h)
    double hnu1;                               // (nu + 1) / 2, kScoreStudent
    double *elpd, *khat, *lpd;                 // per place
};

__device__ inline double loo_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ inline double loo_wave_max(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
// what one stage of the network wrote is read by other lanes of the same wave in the next
__device__ inline void loo_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ inline bool loo_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }   // false for NaN and for either infinity

// blockDim.x = 64 * loo_waves(S), dynamic LDS = loo_waves(S) * loo_lds_doubles(S) doubles
template <int KIND>
__global__ __launch_bounds__(256) void k_trace_psis(TracePsisArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double loo_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * nwaves + wave;
    if (t >= a.ntr) return;                                     // (no workgroup barrier below: a wave works in its own LDS alone)
    const int S = a.S, P = loo_lds_doubles(S);
    double *d = loo_lds + (size_t)wave * P;
    const int64_t o = a.orig ? (int64_t)a.orig[t] : t;
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");

    // phase 1: l_s, +infinity behind them
    bool finite = true;
    {
        const double *x = a.traces + t * S;
        double yv = 0.0, wv = 1.0, hlw = 0.0, fl = 0.0;
        if (KIND != kLooTraces) {
            yv = a.y[o];
            if ((KIND == kScoreGauss || KIND == kScoreGaussFlags) && a.w) { wv = a.w[o]; hlw = 0.5 * log(wv); }
            if (KIND == kScoreGaussFlags || KIND == kScoreProbit) fl = (double)a.flag[o];
        }
        for (int s = lane; s < P; s += 64) {
            double l = inf;
            if (s < S) {
                l = x[s];
                if (KIND != kLooTraces) {
                    const double p = a.mean_rating + l;
                    if (KIND == kScoreProbit) {
                        l = score_log_phi(fl * p);
                    } else if (KIND == kScoreStudent) {
                        const double e = yv - p;
                        l = a.c0[s] - a.hnu1 * log1p(a.as[s] * (e * e));
                    } else {
                        const double e = yv - p;
                        // (the fma is written out: an uncensored cell gets the same bits from the plain instance and from the one with flags)
                        l = fma(-0.5 * (a.as[s] * wv), e * e, a.c0[s] + hlw);
                        if (KIND == kScoreGaussFlags) { if (fl != 0.0) l = score_log_phi(fl * a.sa[s] * (p - yv)); }
                    }
                }
                finite = finite && loo_finite(l);
            }
            d[s] = l;
        }
    }
    if (__any(!finite)) {                                       // wave-uniform
        if (lane == 0) { a.elpd[o] = nan; a.khat[o] = nan; a.lpd[o] = nan; }
        return;
    }
    loo_wave_sync();

    // phase 2: the bitonic network, increasing
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int e = lane; e < (P >> 1); e += 64) {
                const int i1 = ((e & ~(j - 1)) << 1) | (e & (j - 1)), i2 = i1 | j;
                const double u = d[i1], v = d[i2];
                const bool sw = (i1 & k) == 0 ? u > v : u < v;
                d[i1] = sw ? v : u;
                d[i2] = sw ? u : v;
            }
            loo_wave_sync();
        }
    }

    const int M = loo_tail(S);
    const double a0 = d[0], amax = d[S - 1], dS = (double)S, dM = (double)M;
    const double c = M < S ? a0 - d[M] : 0.0, ec = exp(c);      // (M < S always; the guard keeps the address inside the trace)

    // the tail's a_i to registers; the x_j to LDS, x_j at position M - j
    double at[3], lwt[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = lane + 64 * r;
        at[r] = i < M ? d[i] : 0.0;
        lwt[r] = a0 - at[r];                                    // rho_i: what stays without smoothing
    }
    bool smooth = M >= 5;
    double khat = inf;
    if (smooth) {                                               // wave-uniform
        loo_wave_sync();
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = lane + 64 * r;
            if (i < M) d[i] = exp(lwt[r]) - ec;
        }
        loo_wave_sync();
        const double xM = d[0], x1 = d[M - 1], xs = d[M - (int)(0.25 * dM + 0.5)];
        smooth = !(xM == x1) && !(xs == 0.0);
        if (smooth) {
            const int m = 30 + loo_isqrt(M);
            const double dm = (double)m;
            const bool mine = lane < m;
            const double theta = 1.0 / xM + (1.0 - sqrt(dm / ((double)(lane + 1) - 0.5))) / (3.0 * xs);
            double acc = 0.0;
            for (int j = 1; j <= M; ++j) acc += log1p(-theta * d[M - j]);
            const double kj = acc / dM;
            const double L = dM * ((log(-theta / kj) - kj) - 1.0);
            smooth = !__any(mine && !loo_finite(L));
            const double Lmax = loo_wave_max(mine ? L : -inf);
            const double ej = mine ? exp(L - Lmax) : 0.0;
            const double wj = ej / loo_wave_sum(ej);
            const double th = loo_wave_sum(mine ? wj * theta : 0.0);
            double ks = 0.0;
            for (int j = lane + 1; j <= M; j += 64) ks += log1p(-th * d[M - j]);
            const double kk = loo_wave_sum(ks) / dM;
            const double sigma = -kk / th;
            const double kh = (kk * dM + 5.0) / (dM + 10.0);
            smooth = smooth && loo_finite(th) && loo_finite(kk) && loo_finite(sigma) && loo_finite(kh);   // the same bits in every lane
            if (smooth) {
                khat = kh;
                const bool tiny = fabs(kh) < kLooTinyK;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int i = lane + 64 * r;                // j = M - i
                    const double pj = ((double)(M - i) - 0.5) / dM;
                    const double tj = -log1p(-pj);
                    const double q = tiny ? sigma * tj : sigma * expm1(kh * tj) / kh;
                    if (i < M) lwt[r] = fmin(log(q + ec), 0.0);
                }
            }
        }
    }

    // the three log-sum-exps over the positions of the sorted order: tail positions from the registers, the others from LDS
    double m0 = -inf, m1 = -inf;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = lane + 64 * r;
        if (i < S) {
            const double ai = i < M ? at[r] : d[i], lw = i < M ? lwt[r] : a0 - ai;
            m0 = fmax(m0, lw); m1 = fmax(m1, lw + ai);
        }
    }
    for (int i = lane + 192; i < S; i += 64) {
        const double ai = d[i], lw = a0 - ai;
        m0 = fmax(m0, lw); m1 = fmax(m1, lw + ai);
    }
    m0 = loo_wave_max(m0); m1 = loo_wave_max(m1);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = lane + 64 * r;
        if (i < S) {
            const double ai = i < M ? at[r] : d[i], lw = i < M ? lwt[r] : a0 - ai;
            s0 += exp(lw - m0); s1 += exp((lw + ai) - m1); s2 += exp(ai - amax);
        }
    }
    for (int i = lane + 192; i < S; i += 64) {
        const double ai = d[i], lw = a0 - ai;
        s0 += exp(lw - m0); s1 += exp((lw + ai) - m1); s2 += exp(ai - amax);
    }
    s0 = loo_wave_sum(s0); s1 = loo_wave_sum(s1); s2 = loo_wave_sum(s2);
    if (lane == 0) {
        a.elpd[o] = (m1 + log(s1)) - (m0 + log(s0));
        a.khat[o] = khat;
        a.lpd[o] = (amax + log(s2)) - log(dS);
    }
}

}  // namespace bpmf
