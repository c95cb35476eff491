// kernels_topn_score.h -- posterior top-N by an acquisition score (bpmf_hip_topn_scored, capi_topn.hip; one translation unit:
// ktopnscore.hip).  DESIGN.md section 18 has the definitions and the measurements.
//
// With p_s = mean_rating + u_s(q) . v_s(c) over the S kept samples of the two rings (layout: kernels_predblock.h), mean and std
// as k_predict_block with w = NULL, z_s = (p_s - t) / sigma:
//   ucb    mean + kappa std
//   prob   (1/S) sum_s Phi(z_s)                                 sigma = 0: (1/S) #{s : p_s > t}
//   ei     (1/S) sum_s [(p_s - t) Phi(z_s) + sigma phi(z_s)]    sigma = 0: (1/S) sum_s max(p_s - t, 0)
// None of them is a function of the stacked dot product of k_topn_score: they need every p_s.
//
//   k_topn_scored<KIND, NOISY>
//       a workgroup of four waves = 64 queries x a span of candidates, in steps of 64 candidates.  Per step and per sample the
//       64 x 64 tile of p_s is accumulated exactly as in k_predict_block (pred_slice_mfma / pred_fold of kernels_predtile.h:
//       kPredStep slices staged once per workgroup in two LDS buffers, one barrier per slice, the next slice -- of the next sample,
//       of the next step -- in flight meanwhile), so element (q, c) sees s ascending, k ascending inside the MFMA chain whatever
//       q_from, the split or its place in the tile.  prob / ei also fold the sample's score term into a third running sum, in s
//       order; the kind and sigma > 0 (NOISY) are template parameters: ucb has no erfc, the sigma = 0 forms have none either.
//       After the last sample the lanes keep mean and std of their 16 elements in registers and write the scores to the LDS
//       score tile (excluded / past the edge / past the span: -inf).  Selection is k_topn_score's: the exclusion walk (four
//       threads per query, a 64-bit mask per step) and the merge by rank into the query's sorted list (score desc, id asc: a total
//       order, no atomics).  A list entry has four fields (score, id, mean, std).  The selection threads move score and id -- and
//       all four fields of the entries already listed -- and leave the rank of every newly listed element in a byte tile; in a
//       second phase the lane that owns the element writes its mean and std to that rank.  No second pass over the picks.
//   k_topn_scored_merge   one thread per query merges the four-field lists of the splits in split order; empty slots -> id -1, zeros
//
// LDS (dynamic), n = list length:
//   staging   2 operands x 2 buffers x 64 x kPredPitch doubles      36 864 B
//   score tile 64 x 65 doubles                                      33 280 B   ALIASED onto the staging buffers
//   lists     64 x n x (3 doubles + 1 int)                           1 792 n B
//   exclusion masks 64 x 8 B, rank tile 64 x 64 B                    4 608 B
//   total     41 472 + 1 792 n: 59 392 B at n = 10, 98 816 B at n = 32.  Above 64 KB (n > 13) the launcher asks for the larger
//   dynamic limit (hipFuncAttributeMaxDynamicSharedMemorySize); a CU has 160 KB.
// Hazards of the alias: the score tile is written only after the barrier that ends the step's last slice (every wave is done
// reading both staging buffers; the next step's first slice is prefetched into REGISTERS only and not stored), and the staging
// buffer 0 is stored again only behind the barrier that follows the last read of the score tile (the list rewrite).
#pragma once
#include "kernels_predtile.h"

namespace bpmf {

constexpr int kTsQ = kPredTile;            // queries per workgroup (four waves x 16)
constexpr int kTsC = kPredTile;            // candidates per step (four 16-wide tiles)
constexpr int kTsScLd = kTsC + 1;          // row pitch of the score tile in LDS (doubles)
constexpr int kTsMaxN = 32;
constexpr int kTsNone = 0x7fffffff;        // candidate id of an empty slot (with score -inf: worse than every candidate)
constexpr int kTsStage = 4 * kPredTile * kPredPitch;   // doubles of the staging buffers
static_assert(kTsQ * kTsScLd <= kTsStage, "the score tile must fit into the staging buffers it aliases");

enum { kScoreUcb = 0, kScoreProb = 1, kScoreEi = 2 };

struct TopnScoredArgs {
    const double *qring, *cring;           // sample rings of the query / candidate side
    int64_t qstride, cstride;              // doubles per column of either ring (max_samples x Kp)
    int Kp, S, n;
    double mean_rating, param, sigma;      // param: kappa (ucb) or the threshold t (prob, ei)
    int64_t q_from, nq, nc, cspan;         // queries [q_from, q_from + nq); candidates [0, nc) in splits of cspan
    const int64_t *ex_ptr;                 // exclusion lists as in TopnArgs (kernels_topn.h); NULL: none
    const int32_t *ex_rows;
    double *part_score, *part_mean, *part_std;   // nsplit x nq x n
    int32_t *part_idx;
};

__host__ __device__ inline size_t topn_scored_lds(int n)
{
    return sizeof(double) * ((size_t)kTsStage + 3 * (size_t)kTsQ * n + kTsQ) + sizeof(int) * (size_t)kTsQ * n + (size_t)kTsQ * kTsC;
}

__device__ __forceinline__ bool ts_better(double sa, int ia, double sb, int ib)
{
    return sa > sb || (sa == sb && ia < ib);
}

// the score term of one sample; Phi(z) = erfc(-z / sqrt 2) / 2 as k_probit_prob
template <int KIND, bool NOISY>
__device__ __forceinline__ double ts_term(double p, double t, double sigma, double inv_sigma)
{
    const double d = p - t;
    if (KIND == kScoreProb) {
        if (!NOISY) return d > 0.0 ? 1.0 : 0.0;
        return 0.5 * erfc(-(d * inv_sigma) * 0.70710678118654752440);
    } else {
        if (!NOISY) return d > 0.0 ? d : 0.0;
        const double z = d * inv_sigma;
        const double Phi = 0.5 * erfc(-z * 0.70710678118654752440);
        const double phi = 0.39894228040143267794 * exp(-0.5 * z * z);
        return d * Phi + sigma * phi;
    }
}

template <int KIND, bool NOISY>
__global__ __launch_bounds__(256) void k_topn_scored(TopnScoredArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds_ts[];
    typedef double stage_t[kPredTile][kPredPitch];
    const int n = a.n;
    stage_t *sQ = reinterpret_cast<stage_t *>(lds_ts);                      // [2]
    stage_t *sC = sQ + 2;                                                   // [2]
    double *sc = lds_ts;                                                    // aliases sQ / sC (see the header)
    double *top_s = lds_ts + kTsStage;
    double *top_mu = top_s + kTsQ * n;
    double *top_sd = top_mu + kTsQ * n;
    unsigned long long *exm = reinterpret_cast<unsigned long long *>(top_sd + kTsQ * n);
    int *top_i = reinterpret_cast<int *>(exm + kTsQ);
    unsigned char *pos = reinterpret_cast<unsigned char *>(top_i + kTsQ * n);
    const double NEG = -__builtin_inf();

    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    const int64_t qb = (int64_t)blockIdx.x * kTsQ;
    const int64_t c_beg = (int64_t)blockIdx.y * a.cspan;
    const int64_t c_end = c_beg + a.cspan < a.nc ? c_beg + a.cspan : a.nc;

    // selection role: query sq of the block, part sj of its four threads (the four are neighbouring lanes of one wave)
    const int sq = t >> 2, sj = t & 3;
    const bool sel_ok = qb + sq < a.nq;
    for (int r = sj; r < n; r += 4) {
        top_s[sq * n + r] = NEG; top_i[sq * n + r] = kTsNone; top_mu[sq * n + r] = 0.0; top_sd[sq * n + r] = 0.0;
    }
    int64_t ep = 0, ee = 0;                                                 // the query's rated candidates not passed yet
    if (a.ex_ptr && sel_ok) {
        const int64_t gq = a.q_from + qb + sq;
        ep = a.ex_ptr[gq]; ee = a.ex_ptr[gq + 1];
        int64_t lo = ep, hi = ee;                                           // first rated candidate >= c_beg
        while (lo < hi) { const int64_t m = (lo + hi) >> 1; if ((int64_t)a.ex_rows[m] < c_beg) lo = m + 1; else hi = m; }
        ep = lo;
    }

    // staging role: row lr of either operand, four consecutive k from lk
    const int lr = t >> 2, lk = (t & 3) * 4;
    const bool q_ok = qb + lr < a.nq;
    const double *qrow = a.qring + (a.q_from + (q_ok ? qb + lr : 0)) * a.qstride + lk;
    const int nk = (a.Kp + kPredStep - 1) / kPredStep;
    pred_d4 rq, rc;
    int64_t lc0 = c_beg;                                                    // step, sample and slice of the next load
    int ls = 0, lks = 0;
    bool c_ok = lc0 + lr < c_end;
    const double *crow = a.cring + (c_ok ? lc0 + lr : 0) * a.cstride + lk;
    auto load = [&]() {
        const int k = lks * kPredStep;
        const bool in = k + lk < a.Kp;                                      // (Kp is a multiple of 4: a 4-chunk is wholly in or out)
        const int64_t off = (int64_t)ls * a.Kp + k;
        rq = (q_ok && in) ? *reinterpret_cast<const pred_d4 *>(qrow + off) : pred_d4{0.0, 0.0, 0.0, 0.0};
        rc = (c_ok && in) ? *reinterpret_cast<const pred_d4 *>(crow + off) : pred_d4{0.0, 0.0, 0.0, 0.0};
        if (++lks == nk) {
            lks = 0;
            if (++ls == a.S) {
                ls = 0; lc0 += kTsC;
                c_ok = lc0 + lr < c_end;
                crow = a.cring + (c_ok ? lc0 + lr : 0) * a.cstride + lk;
            }
        }
    };
    auto store = [&](int buf) {
        *reinterpret_cast<pred_d2 *>(&sQ[buf][lr][lk]) = pred_d2{rq[0], rq[1]};
        *reinterpret_cast<pred_d2 *>(&sQ[buf][lr][lk + 2]) = pred_d2{rq[2], rq[3]};
        *reinterpret_cast<pred_d2 *>(&sC[buf][lr][lk]) = pred_d2{rc[0], rc[1]};
        *reinterpret_cast<pred_d2 *>(&sC[buf][lr][lk + 2]) = pred_d2{rc[2], rc[3]};
    };
    const double S = (double)a.S;
    const double inv_sigma = NOISY ? 1.0 / a.sigma : 0.0;

    load();
    store(0);
    __syncthreads();
    for (int64_t c0 = c_beg; c0 < c_end; c0 += kTsC) {
        // (1) the rated candidates of this step: thread sj walks entries ep + sj, ep + sj + 4, ...
        unsigned long long bits = 0;
        int64_t stop = ee;
        if (a.ex_ptr && sel_ok) {
            for (int64_t p = ep + sj; p < ee; p += 4) {
                const int64_t r = a.ex_rows[p];
                if (r >= c0 + kTsC) { stop = p; break; }
                if (r >= c0) bits |= 1ull << (r - c0);
            }
        }
        bits |= __shfl_xor(bits, 1); bits |= __shfl_xor(bits, 2);
        { long long s2 = __shfl_xor((long long)stop, 1); stop = s2 < stop ? s2 : stop; }
        { long long s2 = __shfl_xor((long long)stop, 2); stop = s2 < stop ? s2 : stop; }
        ep = stop;
        if (sj == 0) exm[sq] = bits;                                        // (read behind the barriers of the slices below)

        // (2) the moments of the step's 64 x 64 pairs over the samples
        pred_d4 sum[4], m2[4], ts[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sum[j] = pred_d4{0.0, 0.0, 0.0, 0.0}; m2[j] = pred_d4{0.0, 0.0, 0.0, 0.0}; ts[j] = pred_d4{0.0, 0.0, 0.0, 0.0};
        }
        int buf = 0;
        for (int s = 0; s < a.S; ++s) {
            pred_d4 acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = pred_d4{0.0, 0.0, 0.0, 0.0};
            for (int ks = 0; ks < nk; ++ks) {
                const bool more = lc0 < c_end;                              // (uniform over the workgroup)
                const bool last = s == a.S - 1 && ks == nk - 1;             // the next slice is the next step's first: kept in registers
                if (more) load();
                pred_slice_mfma(sQ[buf], sC[buf], w, li, kq, acc);
                if (more && !last) store(buf ^ 1);
                __syncthreads();
                buf ^= 1;
            }
            pred_fold(s, acc, sum, m2);
            if (KIND != kScoreUcb) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ts[j][r] += ts_term<KIND, NOISY>(a.mean_rating + acc[j][r], a.param, a.sigma, inv_sigma);
            }
        }

        // (3) mean and std as k_predict_block stores them (kept in sum / m2), the scores to LDS: D[i = kq + 4 r][j = li] of tile j.
        //     Every wave is past the last slice's barrier: the staging buffers are free to hold the score tile.
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 16 * w + kq + 4 * r, c = 16 * j + li;
                const double var = a.S > 1 ? m2[j][r] / (S - 1.0) : 0.0;
                const double mu = a.mean_rating + sum[j][r] / S, sd = sqrt(var);
                sum[j][r] = mu; m2[j][r] = sd;
                const double score = KIND == kScoreUcb ? mu + a.param * sd : ts[j][r] / S;
                const bool ok = qb + q < a.nq && c0 + c < c_end && !((exm[q] >> c) & 1ull);
                sc[q * kTsScLd + c] = ok ? score : NEG;
            }
        __syncthreads();

        // (4) ranks of the step's survivors and of the listed entries in the merged order
        const double *row = sc + sq * kTsScLd;
        double *tm = top_s + sq * n;
        int *ti = top_i + sq * n;
        const double th_m = tm[n - 1];
        const int th_i = ti[n - 1];
        auto survives = [&](double v, int c) { return v != NEG && ts_better(v, (int)(c0 + c), th_m, th_i); };
        int any = 0;
        for (int e = sj; e < kTsC; e += 4) any |= survives(row[e], e) ? 1 : 0;
        any |= __shfl_xor(any, 1); any |= __shfl_xor(any, 2);
        int rk_new[kTsC / 4], rk_top[kTsMaxN / 4];
        double old_s[kTsMaxN / 4], old_mu[kTsMaxN / 4], old_sd[kTsMaxN / 4];
        int old_i[kTsMaxN / 4];
#pragma unroll
        for (int e = 0; e < kTsC / 4; ++e) rk_new[e] = -1;
#pragma unroll
        for (int e = 0; e < kTsMaxN / 4; ++e) rk_top[e] = -1;
        if (any) {
#pragma unroll
            for (int e = 0; e < kTsC / 4; ++e) {
                const int c = sj + 4 * e;
                const double v = row[c];
                if (!survives(v, c)) continue;
                const int gi = (int)(c0 + c);
                int rk = 0;
                for (int r = 0; r < n; ++r) rk += ts_better(tm[r], ti[r], v, gi) ? 1 : 0;
                for (int c2 = 0; c2 < kTsC; ++c2) {
                    const double v2 = row[c2];
                    rk += (survives(v2, c2) && ts_better(v2, (int)(c0 + c2), v, gi)) ? 1 : 0;
                }
                rk_new[e] = rk;
            }
#pragma unroll
            for (int e = 0; e < kTsMaxN / 4; ++e) {
                const int r = sj + 4 * e;
                if (r >= n) continue;
                old_s[e] = tm[r]; old_i[e] = ti[r]; old_mu[e] = top_mu[sq * n + r]; old_sd[e] = top_sd[sq * n + r];
                int rk = r;
                for (int c2 = 0; c2 < kTsC; ++c2) {
                    const double v2 = row[c2];
                    rk += (survives(v2, c2) && ts_better(v2, (int)(c0 + c2), old_s[e], old_i[e])) ? 1 : 0;
                }
                rk_top[e] = rk;
            }
        }
        // every list read before any is rewritten; a step without a survivor in the whole block (the common one, late in a long
        // span) skips the rewrite
        const int blk_any = __syncthreads_or(any);
        if (blk_any) {
            // (5) the lists rewritten; the rank of every newly listed element left for the lane that owns it
#pragma unroll
            for (int e = 0; e < kTsC / 4; ++e) {
                const int c = sj + 4 * e;
                const bool in = rk_new[e] >= 0 && rk_new[e] < n;
                if (in) { tm[rk_new[e]] = row[c]; ti[rk_new[e]] = (int)(c0 + c); }
                pos[sq * kTsC + c] = in ? (unsigned char)rk_new[e] : (unsigned char)0xff;
            }
#pragma unroll
            for (int e = 0; e < kTsMaxN / 4; ++e)
                if (rk_top[e] >= 0 && rk_top[e] < n) {
                    tm[rk_top[e]] = old_s[e]; ti[rk_top[e]] = old_i[e];
                    top_mu[sq * n + rk_top[e]] = old_mu[e]; top_sd[sq * n + rk_top[e]] = old_sd[e];
                }
            __syncthreads();
            // (6) mean and std of the newly listed elements, from the registers of their lanes
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = 16 * w + kq + 4 * r, c = 16 * j + li;
                    const int p = pos[q * kTsC + c];
                    if (p != 0xff) { top_mu[q * n + p] = sum[j][r]; top_sd[q * n + p] = m2[j][r]; }
                }
        }
        // the score tile is read no more (5 is behind a barrier when it ran): the next step's first slice, loaded during the
        // step's last, goes to buffer 0
        if (c0 + kTsC < c_end) store(0);
        __syncthreads();
    }
    if (sel_ok) {
        const size_t o = ((size_t)blockIdx.y * (size_t)a.nq + (size_t)(qb + sq)) * (size_t)n;
        for (int r = sj; r < n; r += 4) {
            a.part_score[o + r] = top_s[sq * n + r]; a.part_idx[o + r] = top_i[sq * n + r];
            a.part_mean[o + r] = top_mu[sq * n + r]; a.part_std[o + r] = top_sd[sq * n + r];
        }
    }
}

// one thread per query: the split lists merged in split order (exact, so the result is the same for any split count);
// empty slots -> id -1 and zeros
__global__ __launch_bounds__(256) void k_topn_scored_merge(const double *__restrict__ part_score, const double *__restrict__ part_mean,
                                                           const double *__restrict__ part_std, const int32_t *__restrict__ part_idx,
                                                           int nsplit, int64_t nq, int n, double *__restrict__ out_score,
                                                           double *__restrict__ out_mean, double *__restrict__ out_std,
                                                           int32_t *__restrict__ out_idx)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    // the merged list so far: entry r is entry cp[r] of the partial lists (a flat index), so the four fields move only once
    double cs[kTsMaxN], tsc[kTsMaxN];
    int ci[kTsMaxN], ti[kTsMaxN];
    int64_t cp[kTsMaxN], tp[kTsMaxN];
    for (int r = 0; r < n; ++r) { cp[r] = q * n + r; cs[r] = part_score[cp[r]]; ci[r] = part_idx[cp[r]]; }
    for (int s = 1; s < nsplit; ++s) {
        const int64_t o = ((int64_t)s * nq + q) * n;
        int x = 0, y = 0;
        for (int r = 0; r < n; ++r) {
            const double ys = part_score[o + y];
            const int yi = part_idx[o + y];
            if (ts_better(cs[x], ci[x], ys, yi)) { tsc[r] = cs[x]; ti[r] = ci[x]; tp[r] = cp[x]; ++x; }
            else { tsc[r] = ys; ti[r] = yi; tp[r] = o + y; ++y; }
        }
        for (int r = 0; r < n; ++r) { cs[r] = tsc[r]; ci[r] = ti[r]; cp[r] = tp[r]; }
    }
    for (int r = 0; r < n; ++r) {
        const bool empty = ci[r] == kTsNone;
        out_score[q * n + r] = empty ? 0.0 : cs[r];
        out_mean[q * n + r] = empty ? 0.0 : part_mean[cp[r]];
        out_std[q * n + r] = empty ? 0.0 : part_std[cp[r]];
        out_idx[q * n + r] = empty ? -1 : ci[r];
    }
}

}  // namespace bpmf
