// kernels_diag_mc.h -- convergence diagnostics over several chains: the rank-normalised split-Rhat, the bulk and the tail effective
// sample size of Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021) of the traces of a list of cells over two pooled sample rings
// (bpmf_hip_diag_cells_mc) and of traces given by the host (bpmf_hip_diag_traces_mc).  capi_diag.hip; one translation unit:
// kdiagmc.hip.  DESIGN.md section 33 has the estimator, the shape of the work and the measurements.  kernels_diag.h is left alone:
// k_cell_traces writes the traces this kernel reads, k_trace_diag keeps the bits of section 29.
//
// A trace is C * S doubles, chain-major: chain c is x[c S, (c + 1) S), chronological inside.  1 <= C <= 64, S >= 8, C S <= 4096.
//   n = floor(S / 2); half-chain 2c = x_c[0, n), half-chain 2c + 1 = x_c[S - n, S)  (an odd S drops the middle draw);
//   M = 2C half-chains, N = M n kept values, kept value g = h n + i.
//   est(y) for N values y in that layout:
//     per half-chain the mean m_h (of a half whose values are all equal: that value) and d = y - m_h, in two passes;
//     c(t) = (1 / N) sum_h sum_{i=0}^{n-1-t} d_{h,i} d_{h,i+t};  W = c(0) n / (n - 1);  mbar = sum m_h / M;
//     Bv = sum (m_h - mbar)^2 / (M - 1);  var+ = c(0) + Bv;  rhat = sqrt(var+ / W);  rho_t = 1 - (W - c(t)) / var+;
//     P_0 = 1 + rho_1;  for k = 1, 2, .. while 2k + 1 <= n - 3:  p = rho_2k + rho_2k+1;  stop unless p > 0;  P_k = min(p, P_k-1);
//     tau = max(-1 + 2 sum_k P_k, 1 / log10 N);  ess = N / tau;  W not > 0: rhat = ess = NaN
//   z(y): r = the rank of y_g among the N values (1-based, the average rank for values that compare equal), a = min(r, N + 1 - r),
//     z = -+ sqrt 2 erfcinv((2a - 0.75) / (N + 0.25)): negative for r < (N + 1) / 2, 0 at r = (N + 1) / 2
//   rhat = max(est(z(x)).rhat, est(z(|x - med|)).rhat), med = the mean of the two middle order statistics; NaN if either is
//   ess_bulk = est(z(x)).ess
//   ess_tail = min over p in {0.05, 0.95} of est(1[x <= x_(floor((N - 1) p) + 1)]).ess  (1-based order statistic); NaN if either is
//   a value that is not finite anywhere in the C S values: NaN for all three
//
//   k_trace_diag_mc    one wave per trace, 64 * W threads per workgroup (W = 4, 2 or 1: at most 64 KiB of dynamic LDS).  A wave owns
//       P doubles (P: N padded to a power of two), M doubles of means and P 16-bit ranks, and no wave waits for another: the only
//       barriers are wave barriers.  The values are sorted by a bitonic network (+infinity behind the N) and the trace is read again
//       from memory for a value's rank: two binary searches of log2 P + 1 steps in the sorted array give the count of values below and
//       the count of values not above, twice the average rank is their sum plus one and fits 16 bits -- so no position travels through
//       the network, and the z scores then overwrite the sorted array in the layout est wants.  A lag's sum: lane l adds the products of
//       g = l, l + 64, .. ascending with fma (a pair that would cross into the next half-chain is skipped), then a butterfly xor
//       32 .. 1, so every lane holds the same bits and the loop over k is wave-uniform.  A half-chain's mean: the 64 / G half-chains of
//       a round side by side, G = the power of two >= min(n, 64) lanes each, lane j of a group adds i = j, j + G, .. ascending, then a
//       butterfly xor G / 2 .. 1.  Every loop has a trip count fixed by (C, S) but the one `p > 0` exit.  No atomics, no scratch; the
//       bits of a trace depend on the trace alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmf {

constexpr int kDiagMcMaxChains = 64;
constexpr int kDiagMcMinSamples = 8;             // per chain
constexpr int kDiagMcMaxValues = 4096;           // C * S at most: the sorted array is 32 KiB of LDS

__host__ __device__ inline int dmc_kept(int C, int S) { return 2 * C * (S >> 1); }
__host__ __device__ inline int dmc_pad(int N) { int p = 8; while (p < N) p *= 2; return p; }
// per wave: P doubles, 2C doubles, P 16-bit ranks (a multiple of 16 bytes)
__host__ __device__ inline int dmc_lds_bytes(int C, int S) { const int P = dmc_pad(dmc_kept(C, S)); return 8 * P + 16 * C + 2 * P; }
__host__ __device__ inline int dmc_waves(int C, int S) { int w = 4; while (w > 1 && w * dmc_lds_bytes(C, S) > 65536) w >>= 1; return w; }
__host__ __device__ inline bool dmc_shape_ok(int C, int S)
{
    return C >= 1 && C <= kDiagMcMaxChains && S >= kDiagMcMinSamples && S <= kDiagMcMaxValues && (int64_t)C * S <= kDiagMcMaxValues;
}

struct TraceDiagMcArgs {
    const double *traces;                      // ntr x (C S), row-major
    int64_t ntr;
    int C, S;
    const int32_t *orig;                       // the results of trace t go to place orig[t] (NULL: t)
    double *rhat, *ess_bulk, *ess_tail;
};

__device__ inline void dmc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ inline bool dmc_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }   // false for NaN and for either infinity

__device__ inline double dmc_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the place of kept value g in the chain-major trace
__device__ inline int dmc_src(int g, int n, int S)
{
    const int h = g / n, i = g - h * n;
    return (h >> 1) * S + ((h & 1) ? S - n : 0) + i;
}

// the bitonic network over v[0, P), increasing
__device__ inline void dmc_sort(double *v, int P, int lane)
{
#pragma nounroll
    for (int k = 2; k <= P; k <<= 1) {
#pragma nounroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
#pragma unroll 2
            for (int e = lane; e < (P >> 1); e += 64) {
                const int i1 = ((e & ~(j - 1)) << 1) | (e & (j - 1)), i2 = i1 | j;
                const double a = v[i1], b = v[i2];
                const bool sw = (i1 & k) == 0 ? a > b : a < b;
                v[i1] = sw ? b : a;
                v[i2] = sw ? a : b;
            }
            dmc_wave_sync();
        }
    }
}

// twice the average rank of the value `key` among the N values of the sorted v[0, P) (+infinity behind the N): the count of values
// below + the count of values not above + 1
__device__ inline int dmc_rank2(const double *v, int P, int N, double key)
{
    int lo = 0, hi = 0;
#pragma nounroll
    for (int step = P >> 1; step >= 1; step >>= 1) {
        if (v[lo + step - 1] < key) lo += step;
        if (v[hi + step - 1] <= key) hi += step;
    }
    lo += v[lo] < key ? 1 : 0;
    hi += v[hi] <= key ? 1 : 0;
    hi = hi < N ? hi : N;                                       // (a key that overflowed to +infinity meets the pad)
    return lo + hi + 1;
}

// (not inlined: inside the loop over the values the compiler would hoist erfcinv's several hundred polynomial constants into
// registers of the whole kernel and spill them)
__device__ __attribute__((noinline)) double dmc_zscore(int r2, int N)
{
    const int a2 = r2 < 2 * N + 2 - r2 ? r2 : 2 * N + 2 - r2;
    const double z = 1.41421356237309504880 * erfcinv(((double)a2 - 0.75) / ((double)N + 0.25));
    return r2 < N + 1 ? -z : (r2 > N + 1 ? z : 0.0);
}

// sum over the half-chains of sum_i d_i d_{i+t} and the same at t + 1; t + 1 <= n - 1.  i0 = lane % n, step = 64 % n.
__device__ inline void dmc_lag_pair(const double *d, int N, int n, int t, int lane, int i0, int step, double *s_t, double *s_t1)
{
    double a0 = 0.0, a1 = 0.0;
    const int last = n - 1 - t;                                 // lag t pairs i <= last, lag t + 1 pairs i < last
    int i = i0;
#pragma unroll 2
    for (int g = lane; g < N; g += 64) {
        if (i <= last) {
            const double xa = d[g];
            a0 = fma(xa, d[g + t], a0);
            if (i < last) a1 = fma(xa, d[g + t + 1], a1);
        }
        i += step;
        i = i >= n ? i - n : i;
    }
    *s_t = dmc_wave_sum(a0);
    *s_t1 = dmc_wave_sum(a1);
}

// est of the N = M n values of d (centred in place); mh: M doubles.  The wave's stores to d are visible (dmc_wave_sync) on entry.
__device__ inline void dmc_est(double *d, double *mh, int n, int M, int lane, double *rhat, double *ess)
{
    const int N = n * M;
    const double dn = (double)n, dN = (double)N, dM = (double)M, nan = __builtin_nan("");
    int G = 4;
    while (G < n && G < 64) G *= 2;
    const int grp = lane / G, j = lane - grp * G, R = 64 / G;
#pragma nounroll
    for (int h0 = 0; h0 < M; h0 += R) {
        const int h = h0 + grp;
        const bool on = h < M;
        double *dh = d + (on ? h : 0) * n;
        double sum = 0.0, mn = __builtin_huge_val(), mx = -__builtin_huge_val();
        if (on)
            for (int i = j; i < n; i += G) {
                const double v = dh[i];
                sum += v; mn = fmin(mn, v); mx = fmax(mx, v);
            }
        for (int off = G >> 1; off >= 1; off >>= 1) {
            sum += __shfl_xor(sum, off); mn = fmin(mn, __shfl_xor(mn, off)); mx = fmax(mx, __shfl_xor(mx, off));
        }
        const double m = mn == mx ? mn : sum / dn;
        if (on) {
            for (int i = j; i < n; i += G) dh[i] -= m;          // (the values this lane read)
            if (j == 0) mh[h] = m;
        }
    }
    dmc_wave_sync();

    double s = 0.0;
    for (int h = lane; h < M; h += 64) s += mh[h];
    const double mbar = dmc_wave_sum(s) / dM;
    double q = 0.0;
    for (int h = lane; h < M; h += 64) { const double e = mh[h] - mbar; q = fma(e, e, q); }
    const double Bv = dmc_wave_sum(q) / (dM - 1.0);

    const int i0 = lane % n, step = 64 % n;
    double s0, s1;
    dmc_lag_pair(d, N, n, 0, lane, i0, step, &s0, &s1);
    const double c0 = s0 / dN, c1 = s1 / dN;
    const double W = c0 * dn / (dn - 1.0);
    const double varp = c0 + Bv;
    *rhat = nan; *ess = nan;
    if (W > 0.0) {
        *rhat = sqrt(varp / W);
        double Pprev = 1.0 + (1.0 - (W - c1) / varp), acc = Pprev;
#pragma nounroll
        for (int k = 1; 2 * k + 1 <= n - 3; ++k) {
            double se, so;
            dmc_lag_pair(d, N, n, 2 * k, lane, i0, step, &se, &so);
            const double p = (1.0 - (W - se / dN) / varp) + (1.0 - (W - so / dN) / varp);
            if (!(p > 0.0)) break;
            Pprev = p < Pprev ? p : Pprev;
            acc += Pprev;
        }
        const double tau = -1.0 + 2.0 * acc, floor_tau = 1.0 / log10(dN);
        *ess = dN / (tau < floor_tau ? floor_tau : tau);
    }
    dmc_wave_sync();                                            // the caller overwrites d
}

// blockDim.x = 64 * dmc_waves(C, S), dynamic LDS = dmc_waves(C, S) * dmc_lds_bytes(C, S) bytes
__global__ __launch_bounds__(256, 4) void k_trace_diag_mc(TraceDiagMcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dmc_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * nwaves + wave;
    if (t >= a.ntr) return;                                     // (no workgroup barrier anywhere)
    const int C = a.C, S = a.S, n = S >> 1, M = 2 * C, N = M * n, P = dmc_pad(N);
    unsigned char *mine = dmc_lds + (size_t)wave * (size_t)dmc_lds_bytes(C, S);
    double *v = reinterpret_cast<double *>(mine), *mh = v + P;
    uint16_t *rk = reinterpret_cast<uint16_t *>(mh + M);
    const double *x = a.traces + t * ((int64_t)C * S);
    const int64_t o = a.orig ? (int64_t)a.orig[t] : t;
    const double nan = __builtin_nan(""), inf = __builtin_huge_val();

    bool finite = true;
    for (int s = lane; s < C * S; s += 64) finite = finite && dmc_finite(x[s]);
    if (__any(!finite)) {                                       // wave-uniform
        if (lane == 0) { a.rhat[o] = nan; a.ess_bulk[o] = nan; a.ess_tail[o] = nan; }
        return;
    }

    // the order statistics of x, the ranks, the z scores
    for (int g = lane; g < P; g += 64) v[g] = g < N ? x[dmc_src(g, n, S)] : inf;
    dmc_wave_sync();
    dmc_sort(v, P, lane);
    const double med = 0.5 * (v[N / 2 - 1] + v[N / 2]);
    const double cut_lo = v[(N - 1) * 5 / 100], cut_hi = v[(N - 1) * 95 / 100];
    for (int g = lane; g < N; g += 64) rk[g] = (uint16_t)dmc_rank2(v, P, N, x[dmc_src(g, n, S)]);
    dmc_wave_sync();
    for (int g = lane; g < N; g += 64) v[g] = dmc_zscore((int)rk[g], N);
    dmc_wave_sync();
    double r_bulk, e_bulk;
    dmc_est(v, mh, n, M, lane, &r_bulk, &e_bulk);

    // folded
    for (int g = lane; g < P; g += 64) v[g] = g < N ? fabs(x[dmc_src(g, n, S)] - med) : inf;
    dmc_wave_sync();
    dmc_sort(v, P, lane);
    for (int g = lane; g < N; g += 64) rk[g] = (uint16_t)dmc_rank2(v, P, N, fabs(x[dmc_src(g, n, S)] - med));
    dmc_wave_sync();
    for (int g = lane; g < N; g += 64) v[g] = dmc_zscore((int)rk[g], N);
    dmc_wave_sync();
    double r_fold, e_fold;
    dmc_est(v, mh, n, M, lane, &r_fold, &e_fold);

    // the two tails
    double e_lo = 0.0, e_hi = 0.0;
#pragma nounroll
    for (int k = 0; k < 2; ++k) {
        const double cut = k ? cut_hi : cut_lo;
        for (int g = lane; g < N; g += 64) v[g] = x[dmc_src(g, n, S)] <= cut ? 1.0 : 0.0;
        dmc_wave_sync();
        double r_tail, e_tail;
        dmc_est(v, mh, n, M, lane, &r_tail, &e_tail);
        if (k) e_hi = e_tail; else e_lo = e_tail;
    }

    if (lane == 0) {
        a.rhat[o] = (r_bulk == r_bulk && r_fold == r_fold) ? (r_bulk > r_fold ? r_bulk : r_fold) : nan;
        a.ess_bulk[o] = e_bulk;
        a.ess_tail[o] = (e_lo == e_lo && e_hi == e_hi) ? (e_lo < e_hi ? e_lo : e_hi) : nan;
    }
}

}  // namespace bpmf
