// kernels_similar.h -- similar columns of ONE side by a rotation-invariant posterior similarity (bpmf_hip_similar,
// bpmf_hip_similar_block, capi_similar.hip; one translation unit: ksimilar.hip).  DESIGN.md section 27 has the definitions, the
// rotation argument, the error bounds and the measurements.
//
// The side's ring (layout: kernels_predblock.h) holds S samples; column c of sample s is v_s(c), Kp doubles, pad rows zero.
//   d_s = v_s(q) . v_s(c)        n_s(c) = sum_k v_s(c)_k^2        r_s(c) = 1 / sqrt(n_s(c)), 0 where n_s(c) = 0
//   cosine  x_s = clamp(d_s * (r_s(q) * r_s(c)), -1, 1)      the product of the inverse norms first: x_s(q, c) and x_s(c, q) have equal bits
//   euclid  x_s = -max((n_s(q) + n_s(c)) - 2 d_s, 0)         the sum of the norms first; 2 d_s is exact, so a fused subtraction rounds alike
//   mean = (1/S) sum_s x_s, std = sqrt(M2 / (S - 1)) [0 for S = 1] by pred_fold in s order;  score = mean - kappa std (product rounded,
//   then the difference: no fused form, so that mean - kappa * std of the block's doubles has the same bits)
// Supported range: every n_s(c) is 0 or within [2^-900, 2^900] for cosine and within [2^-500, 2^500] for euclid, whose variance squares
// a squared norm; beyond it a norm, an inverse-norm product, d_s or a squared deviation may overflow or lose its digits to underflow.
// Nothing traps: an element whose score is -inf or not a number is never listed, and the block stores what it computed.
//
//   k_ring_norms          one thread per (column, sample): n = fma(v_k, v_k, n) for k = 0, 1, ..., Kp - 1 in that order, one chain, no
//                         atomics, so the bits are the same on every call.  Table: column c at tab + c * 2 S, n_s at [s], r_s at [S + s].
//                         Rebuilt by every call of the entry points (one pass over the ring, a few percent of a ranking); nothing is
//                         cached on the side, so samples_add / _set / _reserve have nothing to drop.
//   k_similar_topn<KIND>  the workgroup of k_topn_scored (kernels_topn_score.h): four waves = 64 queries x a span of candidates in
//                         steps of 64.  Per step and sample the 64 x 64 tile of d_s through pred_slice_mfma from the two LDS staging
//                         buffers (both operands are rows of the same ring); each lane then turns its 16 d_s into x_s with the table
//                         entries of its four query rows and four candidate columns (loaded ahead of the sample's slices, so the
//                         MFMA chain hides them) and folds them with pred_fold.  After the last sample: mean, std, score; the
//                         selection of k_topn_scored restated (see DESIGN section 27 for why restated, not shared): ranks in the merged
//                         order (score desc, id asc), a sorted four-field list per query, mean / std written by the owning lane.
//                         The 64-bit mask of a query and step is the step's candidate word -- a ballot of (inside the span, cand_ok) over
//                         the 64 candidates, formed by every wave for itself -- without the query's own bit (the diagonal).
//   k_similar_merge       one thread per query merges the lists of the splits in split order (k_topn_scored_merge restated)
//   k_similar_block<KIND> the workgroup of k_predict_block with the same element code, no selection: mean and std of a dense block,
//                         diagonal included, bit for bit the values the lists carry
// The bits of a pair depend on its two columns only: d_s is accumulated s ascending, k ascending inside the MFMA chain from a zero
// accumulator in both kernels, the table entries are per column, and a * b = b * a, a + b = b + a in IEEE arithmetic.
//
// LDS of k_similar_topn (dynamic), n = list length: as k_topn_scored without the exclusion words
//   staging 2 operands x 2 buffers x 64 x kPredPitch doubles 36 864 B; score tile 64 x 65 doubles 33 280 B ALIASED onto it;
//   lists 64 x n x (3 doubles + 1 int) 1 792 n B; rank tile 4 096 B: 40 960 + 1 792 n, 58 880 B at n = 10, 98 304 B at n = 32.
// Hazards of the alias, as in kernels_topn_score.h: the score tile is written only after the barrier that ends the step's last
// slice (the next step's first slice is prefetched into REGISTERS only), and staging buffer 0 is stored again only behind the
// barrier that follows the last read of the score tile (the list rewrite).
#pragma once
#include "kernels_predtile.h"

namespace bpmf {

constexpr int kSimQ = kPredTile;            // queries per workgroup (four waves x 16)
constexpr int kSimC = kPredTile;            // candidates per step
constexpr int kSimScLd = kSimC + 1;         // row pitch of the score tile in LDS (doubles)
constexpr int kSimMaxN = 32;
constexpr int kSimNone = 0x7fffffff;        // id of an empty slot (with score -inf: worse than every candidate)
constexpr int kSimStage = 4 * kPredTile * kPredPitch;
static_assert(kSimQ * kSimScLd <= kSimStage, "the score tile must fit into the staging buffers it aliases");

enum { kSimCosine = 0, kSimEuclid = 1 };

struct SimilarArgs {
    const double *ring; int64_t stride;    // the side's ring, doubles per column
    const double *tab;                     // k_ring_norms' table, 2 S doubles per column
    int Kp, S, n;
    double kappa;
    int64_t q_from, nq, nc, cspan;         // queries [q_from, q_from + nq); candidates [0, nc) in splits of cspan
    const uint8_t *cand_ok;                // per candidate, != 0: eligible; NULL: all
    double *part_score, *part_mean, *part_std;   // nsplit x nq x n
    int32_t *part_idx;
};

struct SimilarBlockArgs {
    const double *ring; int64_t stride;
    const double *tab;
    int Kp, S;
    int64_t q_from, nq, c_from, nc;        // queries [q_from, q_from + nq), candidates [c_from, c_from + nc)
    double *mean, *std;                    // nq x nc, row-major
};

__host__ __device__ inline size_t similar_lds(int n)
{
    return sizeof(double) * ((size_t)kSimStage + 3 * (size_t)kSimQ * n) + sizeof(int) * (size_t)kSimQ * n + (size_t)kSimQ * kSimC;
}

__device__ __forceinline__ bool sim_better(double sa, int ia, double sb, int ib)
{
    return sa > sb || (sa == sb && ia < ib);
}

// one thread per (column, sample)
__global__ __launch_bounds__(256) void k_ring_norms(const double *__restrict__ ring, int64_t stride, int Kp, int S, int64_t ncols,
                                                    double *__restrict__ tab)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ncols * S) return;
    const int64_t c = e / S;
    const int s = (int)(e - c * S);
    const double *v = ring + c * stride + (int64_t)s * Kp;
    double n = 0.0;
    for (int k = 0; k < Kp; ++k) n = fma(v[k], v[k], n);
    tab[c * 2 * S + s] = n;
    tab[c * 2 * S + S + s] = n > 0.0 ? 1.0 / sqrt(n) : 0.0;
}

// x_s of one pair: tq / tc are r_s (cosine) or n_s (euclid) of the query / the candidate
template <int KIND>
__device__ __forceinline__ double sim_x(double d, double tq, double tc)
{
    if (KIND == kSimCosine) return fmin(fmax(d * (tq * tc), -1.0), 1.0);
    return -fmax((tq + tc) - 2.0 * d, 0.0);
}

// the sample's d_s in acc -> x_s in acc: lane (kq, li) of wave w holds D[kq + 4 r][li] of tile j
template <int KIND>
__device__ __forceinline__ void sim_elements(pred_d4 (&acc)[4], const double (&tq)[4], const double (&tc)[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[j][r] = sim_x<KIND>(acc[j][r], tq[r], tc[j]);
}

__device__ __forceinline__ void sim_moments(int S, double sum, double m2, double *mu, double *sd)
{
    const double Sd = (double)S;
    const double var = S > 1 ? m2 / (Sd - 1.0) : 0.0;
    *mu = sum / Sd; *sd = sqrt(var);
}

template <int KIND>
__global__ __launch_bounds__(256) void k_similar_topn(SimilarArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds_sim[];
    typedef double stage_t[kPredTile][kPredPitch];
    const int n = a.n;
    stage_t *sQ = reinterpret_cast<stage_t *>(lds_sim);                     // [2]
    stage_t *sC = sQ + 2;                                                   // [2]
    double *sc = lds_sim;                                                   // aliases sQ / sC (see the header)
    double *top_s = lds_sim + kSimStage;
    double *top_mu = top_s + kSimQ * n;
    double *top_sd = top_mu + kSimQ * n;
    int *top_i = reinterpret_cast<int *>(top_sd + kSimQ * n);
    unsigned char *pos = reinterpret_cast<unsigned char *>(top_i + kSimQ * n);
    const double NEG = -__builtin_inf();

    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    const int64_t qb = (int64_t)blockIdx.x * kSimQ;
    const int64_t c_beg = (int64_t)blockIdx.y * a.cspan;
    const int64_t c_end = c_beg + a.cspan < a.nc ? c_beg + a.cspan : a.nc;

    // selection role: query sq of the block, part sj of its four threads
    const int sq = t >> 2, sj = t & 3;
    const bool sel_ok = qb + sq < a.nq;
    for (int r = sj; r < n; r += 4) {
        top_s[sq * n + r] = NEG; top_i[sq * n + r] = kSimNone; top_mu[sq * n + r] = 0.0; top_sd[sq * n + r] = 0.0;
    }

    // staging role: row lr of either operand, four consecutive k from lk
    const int lr = t >> 2, lk = (t & 3) * 4;
    const bool q_ok = qb + lr < a.nq;
    const double *qrow = a.ring + (a.q_from + (q_ok ? qb + lr : 0)) * a.stride + lk;
    const int nk = (a.Kp + kPredStep - 1) / kPredStep;
    pred_d4 rq, rc;
    int64_t lc0 = c_beg;                                                    // step, sample and slice of the next load
    int ls = 0, lks = 0;
    bool c_ok = lc0 + lr < c_end;
    const double *crow = a.ring + (c_ok ? lc0 + lr : 0) * a.stride + lk;
    auto load = [&]() {
        const int k = lks * kPredStep;
        const bool in = k + lk < a.Kp;                                      // (Kp is a multiple of 4: a 4-chunk is wholly in or out)
        const int64_t off = (int64_t)ls * a.Kp + k;
        rq = (q_ok && in) ? *reinterpret_cast<const pred_d4 *>(qrow + off) : pred_d4{0.0, 0.0, 0.0, 0.0};
        rc = (c_ok && in) ? *reinterpret_cast<const pred_d4 *>(crow + off) : pred_d4{0.0, 0.0, 0.0, 0.0};
        if (++lks == nk) {
            lks = 0;
            if (++ls == a.S) {
                ls = 0; lc0 += kSimC;
                c_ok = lc0 + lr < c_end;
                crow = a.ring + (c_ok ? lc0 + lr : 0) * a.stride + lk;
            }
        }
    };
    auto store = [&](int buf) {
        *reinterpret_cast<pred_d2 *>(&sQ[buf][lr][lk]) = pred_d2{rq[0], rq[1]};
        *reinterpret_cast<pred_d2 *>(&sQ[buf][lr][lk + 2]) = pred_d2{rq[2], rq[3]};
        *reinterpret_cast<pred_d2 *>(&sC[buf][lr][lk]) = pred_d2{rc[0], rc[1]};
        *reinterpret_cast<pred_d2 *>(&sC[buf][lr][lk + 2]) = pred_d2{rc[2], rc[3]};
    };

    // element role: the table rows of the lane's four queries (past the edge: query 0's, never listed)
    const int toff = KIND == kSimCosine ? a.S : 0;                          // r_s or n_s
    const double *tqp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t q = qb + 16 * w + kq + 4 * r;
        tqp[r] = a.tab + (a.q_from + (q < a.nq ? q : 0)) * 2 * a.S + toff;
    }

    load();
    store(0);
    __syncthreads();
    for (int64_t c0 = c_beg; c0 < c_end; c0 += kSimC) {
        // (1) the step's candidate word: inside the span and eligible (every wave forms it for itself)
        const bool cin = c0 + l < c_end;
        const unsigned long long cword = __ballot(cin && (!a.cand_ok || a.cand_ok[c0 + l] != 0));
        const double *tcp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t c = c0 + 16 * j + li;
            tcp[j] = a.tab + (c < c_end ? c : c_beg) * 2 * a.S + toff;
        }

        // (2) the moments of the step's 64 x 64 pairs over the samples
        pred_d4 sum[4], m2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { sum[j] = pred_d4{0.0, 0.0, 0.0, 0.0}; m2[j] = pred_d4{0.0, 0.0, 0.0, 0.0}; }
        int buf = 0;
        for (int s = 0; s < a.S; ++s) {
            double tq[4], tc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { tq[r] = tqp[r][s]; tc[r] = tcp[r][s]; }
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
            sim_elements<KIND>(acc, tq, tc);
            pred_fold(s, acc, sum, m2);
        }

        // (3) mean and std as k_similar_block stores them (kept in sum / m2), the scores to LDS: D[i = kq + 4 r][j = li] of tile j.
        //     Every wave is past the last slice's barrier: the staging buffers are free to hold the score tile.
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 16 * w + kq + 4 * r;
            const int64_t dq = a.q_from + qb + q - c0;                      // the query's own place in the step, if it has one
            const unsigned long long okw = (dq >= 0 && dq < kSimC) ? cword & ~(1ull << dq) : cword;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 16 * j + li;
                double mu, sd;
                sim_moments(a.S, sum[j][r], m2[j][r], &mu, &sd);
                sum[j][r] = mu; m2[j][r] = sd;
                const double score = __dsub_rn(mu, __dmul_rn(a.kappa, sd));
                const bool ok = qb + q < a.nq && ((okw >> c) & 1ull);
                sc[q * kSimScLd + c] = ok ? score : NEG;
            }
        }
        __syncthreads();

        // (4) ranks of the step's survivors and of the listed entries in the merged order
        const double *row = sc + sq * kSimScLd;
        double *tm = top_s + sq * n;
        int *ti = top_i + sq * n;
        const double th_m = tm[n - 1];
        const int th_i = ti[n - 1];
        auto survives = [&](double v, int c) { return v != NEG && sim_better(v, (int)(c0 + c), th_m, th_i); };
        int any = 0;
        if (sel_ok)
            for (int e = sj; e < kSimC; e += 4) any |= survives(row[e], e) ? 1 : 0;
        any |= __shfl_xor(any, 1); any |= __shfl_xor(any, 2);
        int rk_new[kSimC / 4], rk_top[kSimMaxN / 4];
        double old_s[kSimMaxN / 4], old_mu[kSimMaxN / 4], old_sd[kSimMaxN / 4];
        int old_i[kSimMaxN / 4];
#pragma unroll
        for (int e = 0; e < kSimC / 4; ++e) rk_new[e] = -1;
#pragma unroll
        for (int e = 0; e < kSimMaxN / 4; ++e) rk_top[e] = -1;
        if (any) {
#pragma unroll
            for (int e = 0; e < kSimC / 4; ++e) {
                const int c = sj + 4 * e;
                const double v = row[c];
                if (!survives(v, c)) continue;
                const int gi = (int)(c0 + c);
                int rk = 0;
                for (int r = 0; r < n; ++r) rk += sim_better(tm[r], ti[r], v, gi) ? 1 : 0;
                for (int c2 = 0; c2 < kSimC; ++c2) {
                    const double v2 = row[c2];
                    rk += (survives(v2, c2) && sim_better(v2, (int)(c0 + c2), v, gi)) ? 1 : 0;
                }
                rk_new[e] = rk;
            }
#pragma unroll
            for (int e = 0; e < kSimMaxN / 4; ++e) {
                const int r = sj + 4 * e;
                if (r >= n) continue;
                old_s[e] = tm[r]; old_i[e] = ti[r]; old_mu[e] = top_mu[sq * n + r]; old_sd[e] = top_sd[sq * n + r];
                int rk = r;
                for (int c2 = 0; c2 < kSimC; ++c2) {
                    const double v2 = row[c2];
                    rk += (survives(v2, c2) && sim_better(v2, (int)(c0 + c2), old_s[e], old_i[e])) ? 1 : 0;
                }
                rk_top[e] = rk;
            }
        }
        // every list read before any is rewritten; a step without a survivor in the whole block skips the rewrite
        const int blk_any = __syncthreads_or(any);
        if (blk_any) {
            // (5) the lists rewritten; the rank of every newly listed element left for the lane that owns it
#pragma unroll
            for (int e = 0; e < kSimC / 4; ++e) {
                const int c = sj + 4 * e;
                const bool in = rk_new[e] >= 0 && rk_new[e] < n;
                if (in) { tm[rk_new[e]] = row[c]; ti[rk_new[e]] = (int)(c0 + c); }
                pos[sq * kSimC + c] = in ? (unsigned char)rk_new[e] : (unsigned char)0xff;
            }
#pragma unroll
            for (int e = 0; e < kSimMaxN / 4; ++e)
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
                    const int p = pos[q * kSimC + c];
                    if (p != 0xff) { top_mu[q * n + p] = sum[j][r]; top_sd[q * n + p] = m2[j][r]; }
                }
        }
        // the score tile is read no more (5 is behind a barrier when it ran): the next step's first slice, loaded during the
        // step's last, goes to buffer 0
        if (c0 + kSimC < c_end) store(0);
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
__global__ __launch_bounds__(256) void k_similar_merge(const double *__restrict__ part_score, const double *__restrict__ part_mean,
                                                       const double *__restrict__ part_std, const int32_t *__restrict__ part_idx,
                                                       int nsplit, int64_t nq, int n, double *__restrict__ out_score,
                                                       double *__restrict__ out_mean, double *__restrict__ out_std,
                                                       int32_t *__restrict__ out_idx)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    // the merged list so far: entry r is entry cp[r] of the partial lists (a flat index), so the four fields move only once
    double cs[kSimMaxN], tsc[kSimMaxN];
    int ci[kSimMaxN], ti[kSimMaxN];
    int64_t cp[kSimMaxN], tp[kSimMaxN];
    for (int r = 0; r < n; ++r) { cp[r] = q * n + r; cs[r] = part_score[cp[r]]; ci[r] = part_idx[cp[r]]; }
    for (int s = 1; s < nsplit; ++s) {
        const int64_t o = ((int64_t)s * nq + q) * n;
        int x = 0, y = 0;
        for (int r = 0; r < n; ++r) {
            const double ys = part_score[o + y];
            const int yi = part_idx[o + y];
            if (sim_better(cs[x], ci[x], ys, yi)) { tsc[r] = cs[x]; ti[r] = ci[x]; tp[r] = cp[x]; ++x; }
            else { tsc[r] = ys; ti[r] = yi; tp[r] = o + y; ++y; }
        }
        for (int r = 0; r < n; ++r) { cs[r] = tsc[r]; ci[r] = ti[r]; cp[r] = tp[r]; }
    }
    for (int r = 0; r < n; ++r) {
        const bool empty = ci[r] == kSimNone;
        out_score[q * n + r] = empty ? 0.0 : cs[r];
        out_mean[q * n + r] = empty ? 0.0 : part_mean[cp[r]];
        out_std[q * n + r] = empty ? 0.0 : part_std[cp[r]];
        out_idx[q * n + r] = empty ? -1 : ci[r];
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_similar_block(SimilarBlockArgs a)
{
    __shared__ __attribute__((aligned(16))) double sQ[2][kPredTile][kPredPitch];
    __shared__ __attribute__((aligned(16))) double sC[2][kPredTile][kPredPitch];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kPredTile, c0 = (int64_t)blockIdx.y * kPredTile;
    // staging role: row lr of either operand, four consecutive k from lk
    const int lr = t >> 2, lk = (t & 3) * 4;
    const bool q_ok = q0 + lr < a.nq, c_ok = c0 + lr < a.nc;
    const double *qrow = a.ring + (a.q_from + (q_ok ? q0 + lr : 0)) * a.stride + lk;
    const double *crow = a.ring + (a.c_from + (c_ok ? c0 + lr : 0)) * a.stride + lk;
    const int nk = (a.Kp + kPredStep - 1) / kPredStep;
    pred_d4 rq, rc;
    int ls = 0, lks = 0;                                                   // sample and slice of the next load
    auto load = [&]() {
        const int k = lks * kPredStep;
        const bool in = k + lk < a.Kp;
        const int64_t off = (int64_t)ls * a.Kp + k;
        rq = (q_ok && in) ? *reinterpret_cast<const pred_d4 *>(qrow + off) : pred_d4{0.0, 0.0, 0.0, 0.0};
        rc = (c_ok && in) ? *reinterpret_cast<const pred_d4 *>(crow + off) : pred_d4{0.0, 0.0, 0.0, 0.0};
        if (++lks == nk) { lks = 0; ++ls; }
    };
    auto store = [&](int buf) {
        *reinterpret_cast<pred_d2 *>(&sQ[buf][lr][lk]) = pred_d2{rq[0], rq[1]};
        *reinterpret_cast<pred_d2 *>(&sQ[buf][lr][lk + 2]) = pred_d2{rq[2], rq[3]};
        *reinterpret_cast<pred_d2 *>(&sC[buf][lr][lk]) = pred_d2{rc[0], rc[1]};
        *reinterpret_cast<pred_d2 *>(&sC[buf][lr][lk + 2]) = pred_d2{rc[2], rc[3]};
    };
    // element role: the table rows of the lane's four queries and four candidates (past the edge: the range's first, never stored)
    const int toff = KIND == kSimCosine ? a.S : 0;
    const double *tqp[4], *tcp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t q = q0 + 16 * w + kq + 4 * r, c = c0 + 16 * r + li;
        tqp[r] = a.tab + (a.q_from + (q < a.nq ? q : 0)) * 2 * a.S + toff;
        tcp[r] = a.tab + (a.c_from + (c < a.nc ? c : 0)) * 2 * a.S + toff;
    }
    pred_d4 sum[4], m2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { sum[j] = pred_d4{0.0, 0.0, 0.0, 0.0}; m2[j] = pred_d4{0.0, 0.0, 0.0, 0.0}; }
    load();
    store(0);
    __syncthreads();
    int buf = 0;
    for (int s = 0; s < a.S; ++s) {
        double tq[4], tc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { tq[r] = tqp[r][s]; tc[r] = tcp[r][s]; }
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
        sim_elements<KIND>(acc, tq, tc);
        pred_fold(s, acc, sum, m2);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t c = c0 + j * 16 + li;
        if (c >= a.nc) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t q = q0 + w * 16 + kq + 4 * r;
            if (q >= a.nq) continue;
            double mu, sd;
            sim_moments(a.S, sum[j][r], m2[j][r], &mu, &sd);
            a.mean[q * a.nc + c] = mu;
            a.std[q * a.nc + c] = sd;
        }
    }
}

}  // namespace bpmf
