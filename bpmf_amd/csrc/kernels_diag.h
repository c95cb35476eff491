// kernels_diag.h -- convergence diagnostics of predictions: split-Rhat and the effective sample size of the traces of a list of cells
// over two sample rings (bpmf_hip_diag_cells) and of traces given by the host (bpmf_hip_diag_traces).  capi_diag.hip; one translation
// unit: kdiag.hip.  DESIGN.md section 29 has the estimator, the shape of the work and the measurements.
//
// The estimator, for one trace x_0 .. x_{S-1} in chronological order, 8 <= S <= kDiagMaxSamples (the split-chain estimator of
// Vehtari et al. 2021 without rank normalisation):
//   n = floor(S / 2);  A = x[0, n), B = x[S - n, S)  (an odd S drops the middle sample)
//   per half h: the mean m_h (of a half whose values are all equal: that value), d = x - m_h, c_h(t) = (1/n) sum_{i=0}^{n-1-t} d_i d_{i+t};
//   c(t) = (c_A(t) + c_B(t)) / 2                      -- two passes; sum x^2 - n m^2 is never formed
//   W = c(0) n / (n - 1);  Bv = (m_A - m_B)^2 / 2;  var+ = c(0) + Bv;  rhat = sqrt(var+ / W)
//   rho_0 = 1, rho_t = 1 - (W - c(t)) / var+
//   P_0 = rho_0 + rho_1;  for k = 1, 2, .. while 2k + 1 <= n - 3:  p = rho_2k + rho_2k+1;  stop unless p > 0;  P_k = min(p, P_k-1)
//   tau = max(-1 + 2 sum_k P_k, 1 / log10(2n));  ess = 2n / tau
// W not > 0 (a constant trace, or one with a value that is not finite): rhat = ess = NaN.  Every loop has a trip count fixed by n,
// and the one early exit is taken when `p > 0` is false, which NaN makes false.
//
//   k_cell_traces<G>   the walk of k_predict_cells<G, false> (kernels_predcells.h: the same grouping by query, staging, lane groups,
//       16-byte loads and order of additions, restated here so that that kernel is left alone): mean and std come out of the same
//       Welford recurrence, and every d_s = u_s(q) . v_s(c) is also stored, cell-major: trace[(cell's place among the sorted cells of
//       the batch) * S + s].  Lane 0 of a group stores 8 bytes per sample; the eight stores of a 64-byte line follow one another
//       within a few hundred cycles and meet in the L2, and k_trace_diag then reads whole lines.
//   k_trace_diag       one wave per trace, 64 * W threads per workgroup (W = 4 for 2n <= 2048, else 2: at most 64 KiB of dynamic LDS).
//       The two centred halves live in the wave's 2n doubles of LDS.  A lag's sum: lane l adds i = l, l + 64, .. ascending with fma,
//       then a butterfly xor 32 .. 1 (both lanes of a pair add the same two numbers), so every lane holds the same bits and the loop
//       over k is wave-uniform.  Two lags (2k, 2k + 1) of both halves share one pass over d.  No atomics; the bits of a trace depend
//       on the trace alone.  Worst case (n / 2) n multiply-adds per half.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmf {

// the shape of k_predict_cells' walk (kernels_predcells.h: kCellsR, kCellsLds, pc_group, pc_chunk, pc_segment), restated: that header
// defines kernels that are not templates and belongs to one translation unit
constexpr int kTraceCellsR = 4;                // cells a lane group carries side by side
constexpr int kTraceLds = 2048;                // doubles of the staged query row (16 KiB per workgroup)
__host__ __device__ inline int ct_group(int Kp) { int g = 2; while (2 * g <= Kp / 2 && g < 64) g *= 2; return g; }
__host__ __device__ inline int ct_chunk(int Kp) { return kTraceLds / Kp; }
__host__ __device__ inline int ct_segment(int Kp) { return kTraceCellsR * 256 / ct_group(Kp); }

constexpr int kDiagMinSamples = 8;
constexpr int kDiagMaxSamples = 4096;          // BPMF_HIP_DIAG_MAX_SAMPLES: a trace's two halves are 32 KiB of LDS

__host__ __device__ inline int diag_waves(int S) { return (S & ~1) <= 2048 ? 4 : 2; }          // waves (traces) per workgroup
__host__ __device__ inline int diag_lds_doubles(int S) { return S & ~1; }                      // per wave: 2n, a multiple of 16 bytes

struct CellTracesArgs {
    const double *qring, *cring;               // sample rings of the query / candidate side
    int64_t qstride, cstride;                  // doubles per column of either ring (max_samples x Kp)
    int Kp, S;
    double mean_rating;
    const int32_t *seg_q, *seg_beg, *seg_cnt;  // per workgroup: its query, its first cell in the sorted list, its cells (1 .. ct_segment)
    const int32_t *cand, *orig;                // per sorted cell: its candidate, its place in the caller's list
    double *mean, *std;                        // caller's order
    double *trace;                             // (sorted cells of the batch) x S
    int64_t tbase;                             // the batch's first cell in the sorted list
};

template <int G>
__global__ __launch_bounds__(256) void k_cell_traces(CellTracesArgs a)
{
    __shared__ __attribute__((aligned(16))) double urow[kTraceLds];
    constexpr int NG = 256 / G;
    const int tid = threadIdx.x, grp = tid / G, g = tid % G;
    const int Kp = a.Kp, S = a.S, K2 = Kp >> 1, SC = ct_chunk(Kp);
    const int cnt = a.seg_cnt[blockIdx.x], beg = a.seg_beg[blockIdx.x];
    const double *uq = a.qring + (int64_t)a.seg_q[blockIdx.x] * a.qstride;

    const double2 *vrow[kTraceCellsR];
    double *tr[kTraceCellsR];
    bool ok[kTraceCellsR];
    double m[kTraceCellsR], m2[kTraceCellsR];
#pragma unroll
    for (int r = 0; r < kTraceCellsR; ++r) {
        const int i = r * NG + grp;
        ok[r] = i < cnt;
        vrow[r] = reinterpret_cast<const double2 *>(a.cring + (int64_t)(ok[r] ? a.cand[beg + i] : 0) * a.cstride);
        tr[r] = a.trace + ((int64_t)beg - a.tbase + (ok[r] ? i : 0)) * S;
        m[r] = 0.0; m2[r] = 0.0;
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
            double part[kTraceCellsR];
#pragma unroll
            for (int r = 0; r < kTraceCellsR; ++r) part[r] = 0.0;
            for (int j = g; j < K2; j += G) {
                const double2 uu = us[j];
                double2 vv[kTraceCellsR];
#pragma unroll
                for (int r = 0; r < kTraceCellsR; ++r) if (ok[r]) vv[r] = vrow[r][vo + j];
#pragma unroll
                for (int r = 0; r < kTraceCellsR; ++r) if (ok[r]) part[r] = fma(uu.y, vv[r].y, fma(uu.x, vv[r].x, part[r]));
            }
#pragma unroll
            for (int r = 0; r < kTraceCellsR; ++r) {
#pragma unroll
                for (int off = G / 2; off >= 1; off >>= 1) part[r] += __shfl_xor(part[r], off);
                const double d = part[r], dl = d - m[r];
                m[r] += dl / (double)(s0 + s + 1);
                m2[r] = fma(dl, d - m[r], m2[r]);
                if (g == 0 && ok[r]) tr[r][s0 + s] = d;
            }
        }
    }
    if (g == 0) {
#pragma unroll
        for (int r = 0; r < kTraceCellsR; ++r) {
            if (!ok[r]) continue;
            const int o = a.orig[beg + r * NG + grp];
            a.mean[o] = a.mean_rating + m[r];
            a.std[o] = S > 1 ? sqrt(m2[r] / (double)(S - 1)) : 0.0;
        }
    }
}

__device__ inline double diag_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// c(t) and c(t + 1) from the centred halves dA, dB (n doubles each); t + 1 <= n - 1
__device__ inline void diag_lag_pair(const double *dA, const double *dB, int n, int t, int lane, double *c_t, double *c_t1)
{
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    const int last = n - 1 - t;                                 // lag t pairs i <= last, lag t + 1 pairs i < last
    for (int i = lane; i <= last; i += 64) {
        const double xa = dA[i], xb = dB[i];
        a0 = fma(xa, dA[i + t], a0);
        b0 = fma(xb, dB[i + t], b0);
        if (i < last) {
            a1 = fma(xa, dA[i + t + 1], a1);
            b1 = fma(xb, dB[i + t + 1], b1);
        }
    }
    a0 = diag_wave_sum(a0); b0 = diag_wave_sum(b0); a1 = diag_wave_sum(a1); b1 = diag_wave_sum(b1);
    const double dn = (double)n;
    *c_t = 0.5 * (a0 / dn + b0 / dn);
    *c_t1 = 0.5 * (a1 / dn + b1 / dn);
}

// traces: ntr x S row-major; the results of trace t go to place orig[t] (orig NULL: t).  blockDim.x = 64 * diag_waves(S),
// dynamic LDS = diag_waves(S) * diag_lds_doubles(S) doubles.
__global__ __launch_bounds__(256) void k_trace_diag(const double *__restrict__ traces, int64_t ntr, int S, const int32_t *__restrict__ orig,
                                                    double *__restrict__ rhat, double *__restrict__ ess)
{
    extern __shared__ __attribute__((aligned(16))) double diag_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * nwaves + wave;
    const bool live = t < ntr;
    const int n = S >> 1;
    double *dA = diag_lds + (size_t)wave * diag_lds_doubles(S), *dB = dA + n;
    double mean[2] = {0.0, 0.0};
    if (live) {
        const double *x = traces + t * S;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double *xh = x + (h ? S - n : 0);
            double sum = 0.0, mn = __builtin_huge_val(), mx = -__builtin_huge_val();
            for (int i = lane; i < n; i += 64) {
                const double v = xh[i];
                sum += v; mn = fmin(mn, v); mx = fmax(mx, v);
            }
            sum = diag_wave_sum(sum);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { mn = fmin(mn, __shfl_xor(mn, off)); mx = fmax(mx, __shfl_xor(mx, off)); }
            const double mh = mn == mx ? mn : sum / (double)n;
            mean[h] = mh;
            double *dh = h ? dB : dA;
            for (int i = lane; i < n; i += 64) dh[i] = xh[i] - mh;
        }
    }
    __syncthreads();                                            // (a wave reads what its own lanes wrote)
    if (!live) return;

    const double dn = (double)n, nan = __builtin_nan("");
    double c0, c1;
    diag_lag_pair(dA, dB, n, 0, lane, &c0, &c1);
    const double W = c0 * dn / (dn - 1.0);
    const double dm = mean[0] - mean[1];
    const double varp = c0 + 0.5 * (dm * dm);
    double r_out = nan, e_out = nan;
    if (W > 0.0) {
        r_out = sqrt(varp / W);
        double Pprev = 1.0 + (1.0 - (W - c1) / varp), acc = Pprev;
        for (int k = 1; 2 * k + 1 <= n - 3; ++k) {
            double ce, co;
            diag_lag_pair(dA, dB, n, 2 * k, lane, &ce, &co);
            const double p = (1.0 - (W - ce) / varp) + (1.0 - (W - co) / varp);
            if (!(p > 0.0)) break;
            Pprev = p < Pprev ? p : Pprev;
            acc += Pprev;
        }
        const double tau = -1.0 + 2.0 * acc, floor_tau = 1.0 / log10(2.0 * dn);
        e_out = 2.0 * dn / (tau < floor_tau ? floor_tau : tau);
    }
    if (lane == 0) {
        const int64_t o = orig ? (int64_t)orig[t] : t;
        rhat[o] = r_out; ess[o] = e_out;
    }
}

}  // namespace bpmf
