// kernels_interval.h -- predictive intervals: the probability integral transform and up to kIntervalMaxQuantiles quantiles of the posterior
// predictive mixture of a list of cells over two sample rings (bpmf_hip_interval_cells) and of traces given by the host
// (bpmf_hip_interval_traces).  capi_interval.hip; one translation unit: kinterval.hip.  DESIGN.md section 31.
//
// For one trace d_0 .. d_{S-1} (d_s = u_s . v_s, what k_cell_traces stores: without mean_rating), 1 <= S <= kIntervalMaxSamples, and
// r_s = sqrt(alpha_s w):
//   F(x) = (1/S) sum_s Phi((x - d_s) r_s),  f(x) = (1/S) sum_s r_s phi((x - d_s) r_s),  Phi(t) = erfc(-t / sqrt 2) / 2
//   pit = F(y - mean_rating);  q(tau) = mean_rating + x with F(x) = tau.  Everything is solved in d-space, so a large mean_rating costs no bits.
// A root: tau <= 1/2 solves h(x) = F(x) - tau = 0, tau > 1/2 solves h(x) = (1 - tau) - (1/S) sum_s Phi(-t_s) = 0 (1 - tau is exact), so
// that both tails keep their relative precision; h increases in x either way.  The bracket is [min_s, max_s] of the component quantiles
// d_s + z / r_s, z = Phi^-1(tau) from the host: at its lower end every component's CDF is <= tau, at its upper end >= tau.  Its ends are
// not evaluated: if rounding puts h(lo) above 0, every step moves hi and the iteration ends at lo (and likewise at hi).  The first point
// is the moment-matched Gaussian's quantile, clamped into the bracket; then Newton steps x - h / f, replaced by the bracket's midpoint
// whenever the step leaves the bracket, f is not > 0, or the bracket has not halved in two steps.  It stops at h = 0, at a step of at most
// 2 ulp, at a bracket without a double inside, or after kIntervalMaxSteps evaluations with the bracket's midpoint.  Several quantiles are
// solved in increasing tau, the previous root being the next lower end, so they never decrease.  Every comparison that keeps a loop going
// is false for NaN; a trace holding a value that is not finite gives NaN for its own outputs and is not iterated at all.
//
//   k_trace_quantiles   one wave per trace, 64 * W threads per workgroup (W = 4 while the dynamic LDS stays <= 64 KiB: S <= 2048, else 2).  The
//       trace lives in the wave's LDS.  One evaluation gives F (or the survival function) and f in one pass: lane l adds s = l, l + 64, ..
//       ascending, then a butterfly xor 32 .. 1 (both lanes of a pair add the same two numbers), so every lane holds the same bits and
//       all control flow is wave-uniform.  No atomics; the bits of a trace depend on the trace, S, the alphas, the weight, y and the taus alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmf {

constexpr int kIntervalMaxSamples = 4096;      // a trace is at most 32 KiB of LDS
constexpr int kIntervalMaxQuantiles = 8;
constexpr int kIntervalMaxSteps = 128;         // evaluations of one root at most

__host__ __device__ inline int interval_lds_doubles(int S) { return (S + 1) & ~1; }           // per wave: a multiple of 16 bytes
__host__ __device__ inline int interval_waves(int S) { return 4 * interval_lds_doubles(S) * 8 <= 65536 ? 4 : 2; }   // waves (traces) per workgroup

struct TraceQuantArgs {
    const double *traces;                      // ntr x S, row-major
    int64_t ntr;
    int S;
    const int32_t *orig;                       // per trace: its place in y, w and the outputs (NULL: the trace's own number)
    double mean_rating;
    const double *y, *w;                       // per place: the observed value (NULL: no pit), the weight (NULL: 1)
    const double *sa;                          // sqrt(alpha_s), S doubles, or NULL: sa0 for every sample
    double sa0;
    int nq;
    double tau[kIntervalMaxQuantiles], z[kIntervalMaxQuantiles];       // increasing; z = Phi^-1(tau)
    double *pit, *quant;                       // per place: 1, nq doubles
};

__device__ inline double iv_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ inline double iv_wave_min(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}
__device__ inline double iv_wave_max(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

// r_s = sqrt(alpha_s) sqrt(w)
__device__ inline double iv_rate(const double *sa, double sa0, double sw, int s) { return (sa ? sa[s] : sa0) * sw; }

// P = (1/S) sum_s Phi(sgn t_s) and f = (1/S) sum_s r_s phi(t_s), t_s = (x - d_s) r_s; the same bits in every lane
__device__ inline void iv_eval(const double *d, const double *sa, double sa0, double sw, int S, int lane, double x, double sgn, double *P, double *f)
{
    constexpr double kRsqrt2 = 0.70710678118654752440, kRsqrt2Pi = 0.39894228040143267794;
    double p = 0.0, g = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double r = iv_rate(sa, sa0, sw, s);
        const double t = (x - d[s]) * r;
        p += 0.5 * erfc(-sgn * t * kRsqrt2);
        g = fma(r, exp(-0.5 * t * t), g);
    }
    p = iv_wave_sum(p); g = iv_wave_sum(g);
    *P = p / (double)S;
    *f = g * kRsqrt2Pi / (double)S;
}

// blockDim.x = 64 * interval_waves(S), dynamic LDS = interval_waves(S) * interval_lds_doubles(S) doubles
__global__ __launch_bounds__(256) void k_trace_quantiles(TraceQuantArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double iv_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * nwaves + wave;
    const bool live = t < a.ntr;
    const int S = a.S;
    double *d = iv_lds + (size_t)wave * interval_lds_doubles(S);
    double sum = 0.0;
    bool finite = true;
    if (live) {
        const double *x = a.traces + t * S;
        for (int s = lane; s < S; s += 64) {
            const double v = x[s];
            d[s] = v;
            sum += v;
            finite = finite && fabs(v) <= 1.79769313486231570815e308;  // false for NaN and for either infinity
        }
    }
    __syncthreads();                                            // (a wave reads what its own lanes wrote)
    if (!live) return;

    const int64_t o = a.orig ? (int64_t)a.orig[t] : t;
    const int nq = a.nq;
    const double nan = __builtin_nan("");
    if (__any(!finite)) {                                       // wave-uniform
        if (lane == 0) {
            if (a.y) a.pit[o] = nan;
            for (int j = 0; j < nq; ++j) a.quant[o * nq + j] = nan;
        }
        return;
    }
    const double sw = a.w ? sqrt(a.w[o]) : 1.0;
    const double dS = (double)S;

    if (a.y) {
        double P, f;
        iv_eval(d, a.sa, a.sa0, sw, S, lane, a.y[o] - a.mean_rating, 1.0, &P, &f);
        if (lane == 0) a.pit[o] = P;
    }
    if (nq == 0) return;

    // the mixture's first two moments (two passes; sum x^2 - S m^2 is never formed)
    const double m = iv_wave_sum(sum) / dS;
    double var = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double c = d[s] - m, r = iv_rate(a.sa, a.sa0, sw, s);
        var += fma(c, c, 1.0 / (r * r));
    }
    const double sd = sqrt(iv_wave_sum(var) / dS);

    double prev = -__builtin_huge_val();
    for (int j = 0; j < nq; ++j) {
        const double tau = a.tau[j], z = a.z[j];
        const bool upper = tau > 0.5;
        const double tail = upper ? 1.0 - tau : tau, sgn = upper ? -1.0 : 1.0;
        double lo = __builtin_huge_val(), hi = -__builtin_huge_val();
        for (int s = lane; s < S; s += 64) {
            const double c = d[s] + z / iv_rate(a.sa, a.sa0, sw, s);
            lo = fmin(lo, c); hi = fmax(hi, c);
        }
        lo = iv_wave_min(lo); hi = iv_wave_max(hi);
        lo = lo < prev ? prev : lo;
        hi = hi < lo ? lo : hi;
        double x = fma(z, sd, m);
        x = !(x >= lo) ? lo : !(x <= hi) ? hi : x;              // NaN: lo
        double w1 = __builtin_huge_val(), w2 = w1;              // the bracket's width one and two steps ago
        double root = x;
        bool done = !(hi > lo);                                 // (all components alike: lo = hi is the root)
        for (int it = 0; it < kIntervalMaxSteps && !done; ++it) {
            double P, f;
            iv_eval(d, a.sa, a.sa0, sw, S, lane, x, sgn, &P, &f);
            const double h = upper ? tail - P : P - tail;
            if (h == 0.0) { root = x; break; }
            if (h < 0.0) lo = x; else hi = x;
            const double width = hi - lo, mid = lo + 0.5 * width;
            root = mid;                                         // what the cap leaves
            if (!(mid > lo && mid < hi)) break;                 // no double inside the bracket
            double xn = x - h / f;
            if (!(f > 0.0 && xn > lo && xn < hi && width <= 0.5 * w2)) xn = mid;
            w2 = w1; w1 = width;
            if (!(fabs(xn - x) > 0x1p-52 * fabs(x))) { root = xn; break; }   // a step of at most 2 ulp
            x = xn;
        }
        prev = root;
        if (lane == 0) a.quant[o * nq + j] = a.mean_rating + root;
    }
}

}  // namespace bpmf
