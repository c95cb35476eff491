// kernels_topn.h -- posterior top-N ranking (bpmf_hip_topn, capi_topn.hip; one translation unit: ktopn.hip).
//
// The S kept samples of a column sit in the side's sample ring as ONE fp64 vector of length L = S Kp (Kp = num_latent
// rounded up to 4, pad rows zero), so the posterior-mean score of a pair is one dot product of length L:
//   mean(q, c) = mean_rating + (1/S) sum_s u_s(q) . v_s(c)
// and ranking every candidate for a block of queries is a dense fp64 product with inner dimension L, fused with the
// selection so that no nq x nc score matrix ever exists.
//
//   k_samples_add   current factors -> slot `slot` of the ring (fp32 factors widened), pad rows zeroed
//   k_topn_score    a workgroup = 64 queries x a range of candidates.  Wave w owns queries 16 w .. 16 w + 15; per step of
//                   64 candidates it accumulates four 16 x 16 tiles on v_mfma_f64_16x16x4_f64 over the whole of L, the
//                   operands streamed from the rings in 16-wide K slices (one 32-byte load per lane and operand per slice:
//                   the candidate slices are shared by the four waves through the vector L1).  The step's 64 x 64 scores
//                   go to LDS (the excluded / out-of-range ones as -inf); then four threads per query merge the scores that
//                   beat the query's current N-th best into its sorted LDS list of N by rank (deterministic: the order
//                   (mean desc, candidate asc) is total, no atomics).  The rated candidates are removed by walking the
//                   query's sorted rating list alongside the candidate steps (four threads per query, a 64-bit mask per step).
//   k_topn_merge    the candidate range of a query block is split over workgroups when there are few queries: one thread
//                   per query merges the per-split lists in split order (the merge is exact, so the result is the same for
//                   any split count)
//   k_topn_std      one wave per selected pair: the S dot products of length Kp, then sum (p_s - mean)^2 around the known mean
#pragma once
#include "kernels.h"

namespace bpmf {

constexpr int kTopnQ = 64;                 // queries per workgroup (four waves x 16)
constexpr int kTopnC = 64;                 // candidates per step (four 16-wide tiles)
constexpr int kTopnScLd = kTopnC + 1;      // row pitch of the score tile in LDS (doubles)
constexpr int kTopnMaxN = 32;
constexpr int kTopnNone = 0x7fffffff;      // candidate id of an empty slot (with mean -inf: worse than every candidate)

struct TopnArgs {
    const double *qring, *cring;           // sample rings of the query / candidate side
    int64_t qstride, cstride;              // doubles per column of either ring (max_samples x Kp)
    int L, S, n;                           // L = S Kp
    double mean_rating;
    int64_t q_from, nq, nc, cspan;         // queries [q_from, q_from + nq); candidates [0, nc) in splits of cspan
    const int64_t *ex_ptr;                 // exclusion: rated candidates of query column q are ex_rows[ex_ptr[q] .. ex_ptr[q + 1]), sorted; NULL: none
    const int32_t *ex_rows;
    double *part_mean;                     // nsplit x nq x n
    int32_t *part_idx;
};

__device__ __forceinline__ bool topn_better(double ma, int ia, double mb, int ib)
{
    return ma > mb || (ma == mb && ia < ib);
}

template <typename T>
__global__ __launch_bounds__(256) void k_samples_add(const T *__restrict__ items, int ld, int Kt, int Kp, int64_t ncols,
                                                     double *__restrict__ ring, int64_t stride, int slot)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ncols * Kp) return;
    const int64_t c = e / Kp;
    const int k = (int)(e - c * Kp);
    ring[c * stride + (int64_t)slot * Kp + k] = k < Kt ? (double)items[c * ld + k] : 0.0;
}

// dynamic LDS: score tile [64][65] | top means [64][n] | exclusion masks [64] | top ids [64][n]
__global__ __launch_bounds__(256, 2) void k_topn_score(TopnArgs a)
{
    extern __shared__ double lds_topn[];
    const int n = a.n;
    double *sc = lds_topn;
    double *top_m = sc + kTopnQ * kTopnScLd;
    unsigned long long *exm = reinterpret_cast<unsigned long long *>(top_m + kTopnQ * n);
    int *top_i = reinterpret_cast<int *>(exm + kTopnQ);
    const double NEG = -__builtin_inf();

    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, kq = lane >> 4, li = lane & 15;
    const int64_t qb = (int64_t)blockIdx.x * kTopnQ;
    const int64_t c_beg = (int64_t)blockIdx.y * a.cspan;
    const int64_t c_end = c_beg + a.cspan < a.nc ? c_beg + a.cspan : a.nc;

    // selection role: query sq of the block, part j of its four threads (the four are neighbouring lanes of one wave)
    const int sq = tid >> 2, j = tid & 3;
    const bool sel_ok = qb + sq < a.nq;
    for (int r = j; r < n; r += 4) { top_m[sq * n + r] = NEG; top_i[sq * n + r] = kTopnNone; }
    int64_t ep = 0, ee = 0;                                   // the query's rated candidates not passed yet
    if (a.ex_ptr && sel_ok) {
        const int64_t gq = a.q_from + qb + sq;
        ep = a.ex_ptr[gq]; ee = a.ex_ptr[gq + 1];
        int64_t lo = ep, hi = ee;                             // first rated candidate >= c_beg
        while (lo < hi) { const int64_t m = (lo + hi) >> 1; if ((int64_t)a.ex_rows[m] < c_beg) lo = m + 1; else hi = m; }
        ep = lo;
    }

    // product role: row li of wave w's query tile
    const int64_t aq = qb + 16 * w + li;
    const bool a_ok = aq < a.nq;
    const double *arow = a.qring + (a_ok ? a.q_from + aq : 0) * a.qstride;
    __syncthreads();

    for (int64_t c0 = c_beg; c0 < c_end; c0 += kTopnC) {
        // (1) the rated candidates of this step: thread j walks entries ep + j, ep + j + 4, ...
        unsigned long long bits = 0;
        int64_t stop = ee;
        if (a.ex_ptr && sel_ok) {
            for (int64_t p = ep + j; p < ee; p += 4) {
                const int64_t r = a.ex_rows[p];
                if (r >= c0 + kTopnC) { stop = p; break; }
                if (r >= c0) bits |= 1ull << (r - c0);
            }
        }
        bits |= __shfl_xor(bits, 1); bits |= __shfl_xor(bits, 2);
        { long long s2 = __shfl_xor((long long)stop, 1); stop = s2 < stop ? s2 : stop; }
        { long long s2 = __shfl_xor((long long)stop, 2); stop = s2 < stop ? s2 : stop; }
        ep = stop;

        // (2) scores of wave w's 16 queries x the step's 64 candidates over the whole stacked inner dimension
        d4 acc[4];
        const double *brow[4];
        bool b_ok[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[t] = d4{0.0, 0.0, 0.0, 0.0};
            const int64_t bc = c0 + 16 * t + li;
            b_ok[t] = bc < c_end;
            brow[t] = a.cring + (b_ok[t] ? bc : 0) * a.cstride;
        }
        for (int k0 = 0; k0 < a.L; k0 += 16) {
            // lane (kq, li) holds k = k0 + 4 kq + r in sub-step r, for the query and the candidates alike
            const int kk = k0 + 4 * kq;
            const bool k_ok = kk < a.L;                       // (L is a multiple of 4: a 4-chunk is wholly in or out)
            d4 av = d4{0.0, 0.0, 0.0, 0.0}, bv[4];
            if (a_ok && k_ok) av = *reinterpret_cast<const d4 *>(arow + kk);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                bv[t] = d4{0.0, 0.0, 0.0, 0.0};
                if (b_ok[t] && k_ok) bv[t] = *reinterpret_cast<const d4 *>(brow[t] + kk);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = mfma16(av[r], bv[t][r], acc[t]);
        }
        if (j == 0) exm[sq] = bits;
        __syncthreads();                                      // the previous step's selection is done with sc; exm is written

        // (3) the step's scores to LDS: D[i = kq + 4 reg][j = li] of tile t
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 16 * w + kq + 4 * r, c = 16 * t + li;
                const bool ok = qb + q < a.nq && c0 + c < c_end && !((exm[q] >> c) & 1ull);
                sc[q * kTopnScLd + c] = ok ? a.mean_rating + acc[t][r] / (double)a.S : NEG;
            }
        __syncthreads();

        // (4) merge the step's survivors into the query's list of n by rank
        const double *row = sc + sq * kTopnScLd;
        double *tm = top_m + sq * n;
        int *ti = top_i + sq * n;
        const double th_m = tm[n - 1];
        const int th_i = ti[n - 1];
        auto survives = [&](double v, int c) { return v != NEG && topn_better(v, (int)(c0 + c), th_m, th_i); };
        int any = 0;
        for (int e = j; e < kTopnC; e += 4) any |= survives(row[e], e) ? 1 : 0;
        any |= __shfl_xor(any, 1); any |= __shfl_xor(any, 2);
        int rk_new[kTopnC / 4], rk_top[kTopnMaxN / 4];
        double old_m[kTopnMaxN / 4];
        int old_i[kTopnMaxN / 4];
        if (any) {
#pragma unroll
            for (int e = 0; e < kTopnC / 4; ++e) {
                const int c = j + 4 * e;
                const double v = row[c];
                rk_new[e] = -1;
                if (!survives(v, c)) continue;
                const int gi = (int)(c0 + c);
                int rk = 0;
                for (int r = 0; r < n; ++r) rk += topn_better(tm[r], ti[r], v, gi) ? 1 : 0;
                for (int c2 = 0; c2 < kTopnC; ++c2) {
                    const double v2 = row[c2];
                    rk += (survives(v2, c2) && topn_better(v2, (int)(c0 + c2), v, gi)) ? 1 : 0;
                }
                rk_new[e] = rk;
            }
#pragma unroll
            for (int e = 0; e < kTopnMaxN / 4; ++e) {
                const int r = j + 4 * e;
                rk_top[e] = -1;
                if (r >= n) continue;
                old_m[e] = tm[r]; old_i[e] = ti[r];
                int rk = r;
                for (int c2 = 0; c2 < kTopnC; ++c2) {
                    const double v2 = row[c2];
                    rk += (survives(v2, c2) && topn_better(v2, (int)(c0 + c2), old_m[e], old_i[e])) ? 1 : 0;
                }
                rk_top[e] = rk;
            }
        }
        __syncthreads();                                      // every list read before any is rewritten
        if (any) {
#pragma unroll
            for (int e = 0; e < kTopnC / 4; ++e)
                if (rk_new[e] >= 0 && rk_new[e] < n) { tm[rk_new[e]] = row[j + 4 * e]; ti[rk_new[e]] = (int)(c0 + j + 4 * e); }
#pragma unroll
            for (int e = 0; e < kTopnMaxN / 4; ++e)
                if (rk_top[e] >= 0 && rk_top[e] < n) { tm[rk_top[e]] = old_m[e]; ti[rk_top[e]] = old_i[e]; }
        }
        __syncthreads();
    }
    if (sel_ok) {
        const size_t o = ((size_t)blockIdx.y * (size_t)a.nq + (size_t)(qb + sq)) * (size_t)n;
        for (int r = j; r < n; r += 4) { a.part_mean[o + r] = top_m[sq * n + r]; a.part_idx[o + r] = top_i[sq * n + r]; }
    }
}

// one thread per query: the split lists merged in split order; empty slots -> id -1, mean 0
__global__ __launch_bounds__(256) void k_topn_merge(const double *__restrict__ part_mean, const int32_t *__restrict__ part_idx,
                                                    int nsplit, int64_t nq, int n, double *__restrict__ out_mean, int32_t *__restrict__ out_idx)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    double cm[kTopnMaxN], tm[kTopnMaxN];
    int ci[kTopnMaxN], ti[kTopnMaxN];
    for (int r = 0; r < n; ++r) { cm[r] = part_mean[q * n + r]; ci[r] = part_idx[q * n + r]; }
    for (int s = 1; s < nsplit; ++s) {
        const size_t o = ((size_t)s * (size_t)nq + (size_t)q) * (size_t)n;
        int x = 0, y = 0;
        for (int r = 0; r < n; ++r) {
            const double ym = part_mean[o + y];
            const int yi = part_idx[o + y];
            if (topn_better(cm[x], ci[x], ym, yi)) { tm[r] = cm[x]; ti[r] = ci[x]; ++x; }
            else { tm[r] = ym; ti[r] = yi; ++y; }
        }
        for (int r = 0; r < n; ++r) { cm[r] = tm[r]; ci[r] = ti[r]; }
    }
    for (int r = 0; r < n; ++r) {
        const bool empty = ci[r] == kTopnNone;
        out_mean[q * n + r] = empty ? 0.0 : cm[r];
        out_idx[q * n + r] = empty ? -1 : ci[r];
    }
}

// one wave per selected pair (four per workgroup): std around the known mean, in a fixed order
__global__ __launch_bounds__(256) void k_topn_std(const double *__restrict__ qring, const double *__restrict__ cring, int64_t qstride,
                                                  int64_t cstride, int Kp, int S, double mean_rating, int64_t q_from, int64_t npairs, int n,
                                                  const double *__restrict__ mean, const int32_t *__restrict__ idx, double *__restrict__ std_out)
{
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pair >= npairs) return;
    const int c = idx[pair];
    if (c < 0 || S < 2) { if (lane == 0) std_out[pair] = 0.0; return; }
    const double *u = qring + (q_from + pair / n) * qstride;
    const double *v = cring + (int64_t)c * cstride;
    const double m = mean[pair];
    double ss = 0.0;
    for (int s = 0; s < S; ++s) {
        double part = 0.0;
        for (int k = lane; k < Kp; k += 64) part = fma(u[(int64_t)s * Kp + k], v[(int64_t)s * Kp + k], part);
        for (int off = 32; off >= 1; off >>= 1) part += __shfl_down(part, off);
        const double d = (mean_rating + __shfl(part, 0)) - m;
        ss = fma(d, d, ss);
    }
    if (lane == 0) std_out[pair] = sqrt(ss / (double)(S - 1));
}

}  // namespace bpmf
