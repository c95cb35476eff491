// kernels_rank.h -- ranks of held-out candidates among all the candidates a query has not rated (bpmf_hip_rank_eval,
// capi_topn.hip; one translation unit: krank.hip).  DESIGN.md section 24.
//
// The score is k_topn_score's (kernels_topn.h): mean_rating + (1/S) of the dot product of the two stacked ring vectors, one
// 16 x 16 x 4 fp64 MFMA chain per tile element over the whole of L, k ascending.  The chain of an element does not depend on where
// its tile sits (query block, candidate step, split), which is what makes the two sweeps below -- and bpmf_hip_topn -- agree bit
// for bit.  The product loop, the exclusion walk and the layout of the score tile are copies of k_topn_score's steps (1) - (3).
//
//   k_rank_eval<false>   sweep 1: the score of every held-out entry.  The held-out candidates of a query are sorted, so four threads
//                        per query walk them alongside the candidate steps as the exclusion walk does and copy the entry's score
//                        out of the step's LDS tile.  A step in which no query of the block has a held-out candidate skips the
//                        products.  Every entry is written by exactly one thread of exactly one split.
//   k_rank_eval<true>    sweep 2: per step, thread j of a query counts, for its entries j, j + 4, ..., the scores of the tile that
//                        beat the entry (topn_better: score desc, candidate asc -- a total order, and strict, so the entry never
//                        counts itself) into the split's integer partial of the entry, which that thread alone owns.  Excluded
//                        and out-of-range scores are -inf and never count.  The candidates left (not -inf) are counted on the way.
//                        No atomics, no nq x nc buffer, no cap on the entries of a query.
//   k_rank_merge         rank = 1 + the sum of the split partials; ncand = the sum of the split counts
#pragma once
#include "kernels.h"

namespace bpmf {

// the workgroup of k_topn_score (kernels_topn.h is not included: its kernels are no templates and live in ktopn.hip alone)
constexpr int kRankQ = 64;                 // queries per workgroup (four waves x 16)
constexpr int kRankC = 64;                 // candidates per step (four 16-wide tiles)
constexpr int kRankScLd = kRankC + 1;      // row pitch of the score tile in LDS (doubles)

// topn_better of kernels_topn.h: score descending, lower candidate first
__device__ __forceinline__ bool rank_better(double ma, int ia, double mb, int ib)
{
    return ma > mb || (ma == mb && ia < ib);
}

struct RankArgs {
    const double *qring, *cring;           // sample rings of the query / candidate side
    int64_t qstride, cstride;              // doubles per column of either ring (max_samples x Kp)
    int L, S;                              // L = S Kp
    double mean_rating;
    int64_t q_from, nq, nc, cspan;         // queries [q_from, q_from + nq); candidates [0, nc) in splits of cspan
    const int64_t *ex_ptr;                 // exclusion lists as in TopnArgs, indexed by the query's column; NULL: none
    const int32_t *ex_rows;
    const int64_t *tptr;                   // held-out entries of query q (0 .. nq - 1): tcand[tptr[q] .. tptr[q + 1]), ascending
    const int32_t *tcand;
    int64_t nt;                            // tptr[nq]
    double *tscore;                        // nt: written by sweep 1, read by sweep 2
    int32_t *part_cnt;                     // nsplit x nt, zero before sweep 2
    int32_t *part_ncand;                   // nsplit x nq
};

// dynamic LDS: score tile [64][65] | exclusion masks [64]
template <bool COUNT>
__global__ __launch_bounds__(256, 2) void k_rank_eval(RankArgs a)
{
    extern __shared__ double lds_rank[];
    double *sc = lds_rank;
    unsigned long long *exm = reinterpret_cast<unsigned long long *>(sc + kRankQ * kRankScLd);
    const double NEG = -__builtin_inf();

    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, kq = lane >> 4, li = lane & 15;
    const int64_t qb = (int64_t)blockIdx.x * kRankQ;
    const int64_t c_beg = (int64_t)blockIdx.y * a.cspan;
    const int64_t c_end = c_beg + a.cspan < a.nc ? c_beg + a.cspan : a.nc;

    // selection role: query sq of the block, part j of its four threads (the four are neighbouring lanes of one wave)
    const int sq = tid >> 2, j = tid & 3;
    const bool sel_ok = qb + sq < a.nq;
    int64_t ep = 0, ee = 0;                                   // the query's rated candidates not passed yet
    if (a.ex_ptr && sel_ok) {
        const int64_t gq = a.q_from + qb + sq;
        ep = a.ex_ptr[gq]; ee = a.ex_ptr[gq + 1];
        int64_t lo = ep, hi = ee;                             // first rated candidate >= c_beg
        while (lo < hi) { const int64_t m = (lo + hi) >> 1; if ((int64_t)a.ex_rows[m] < c_beg) lo = m + 1; else hi = m; }
        ep = lo;
    }
    int64_t tb = 0, te = 0, tp = 0;                           // the query's held-out entries; sweep 1: those not passed yet
    if (sel_ok) {
        tb = a.tptr[qb + sq]; te = a.tptr[qb + sq + 1];
        tp = tb;
        if (!COUNT) {
            int64_t lo = tb, hi = te;                         // first held-out candidate >= c_beg
            while (lo < hi) { const int64_t m = (lo + hi) >> 1; if ((int64_t)a.tcand[m] < c_beg) lo = m + 1; else hi = m; }
            tp = lo;
        }
    }
    int left = 0;                                             // sweep 2: candidates of this split the query has not rated (thread j's share)

    // product role: row li of wave w's query tile
    const int64_t aq = qb + 16 * w + li;
    const bool a_ok = aq < a.nq;
    const double *arow = a.qring + (a_ok ? a.q_from + aq : 0) * a.qstride;

    for (int64_t c0 = c_beg; c0 < c_end; c0 += kRankC) {
        // (1) the rated candidates of this step: thread j walks entries ep + j, ep + j + 4, ...
        unsigned long long bits = 0;
        int64_t stop = ee;
        if (a.ex_ptr && sel_ok) {
            for (int64_t p = ep + j; p < ee; p += 4) {
                const int64_t r = a.ex_rows[p];
                if (r >= c0 + kRankC) { stop = p; break; }
                if (r >= c0) bits |= 1ull << (r - c0);
            }
        }
        bits |= __shfl_xor(bits, 1); bits |= __shfl_xor(bits, 2);
        { long long s2 = __shfl_xor((long long)stop, 1); stop = s2 < stop ? s2 : stop; }
        { long long s2 = __shfl_xor((long long)stop, 2); stop = s2 < stop ? s2 : stop; }
        ep = stop;

        if (!COUNT) {
            // sweep 1: a step without a held-out candidate in the whole block has nothing to store (tcand is ascending, tp is the
            // same in the query's four threads: the first entry not passed decides).  The barrier also ends the previous step's reads of sc.
            const int mine = tp < te && (int64_t)a.tcand[tp] < c0 + kRankC;
            if (!__syncthreads_or(mine)) continue;
        }

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
        __syncthreads();                                      // the previous step's reads of sc are done; exm is written

        // (3) the step's scores to LDS: D[i = kq + 4 reg][j = li] of tile t
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 16 * w + kq + 4 * r, c = 16 * t + li;
                const bool ok = qb + q < a.nq && c0 + c < c_end && !((exm[q] >> c) & 1ull);
                sc[q * kRankScLd + c] = ok ? a.mean_rating + acc[t][r] / (double)a.S : NEG;
            }
        __syncthreads();

        const double *row = sc + sq * kRankScLd;
        if (!COUNT) {
            // (4a) the held-out entries of this step: thread j takes entries tp + j, tp + j + 4, ...
            int64_t tstop = te;
            for (int64_t p = tp + j; p < te; p += 4) {
                const int64_t r = a.tcand[p];
                if (r >= c0 + kRankC) { tstop = p; break; }
                a.tscore[p] = row[r - c0];
            }
            { long long s2 = __shfl_xor((long long)tstop, 1); tstop = s2 < tstop ? s2 : tstop; }
            { long long s2 = __shfl_xor((long long)tstop, 2); tstop = s2 < tstop ? s2 : tstop; }
            tp = tstop;
        } else {
            // (4b) the candidates of this step that beat each of thread j's entries
            for (int e = j; e < kRankC; e += 4) left += row[e] != NEG ? 1 : 0;
            for (int64_t p = tb + j; p < te; p += 4) {
                const double v = a.tscore[p];
                const int gi = a.tcand[p];
                int cnt = 0;
                for (int c = 0; c < kRankC; ++c) {
                    const double v2 = row[c];
                    cnt += (v2 != NEG && rank_better(v2, (int)(c0 + c), v, gi)) ? 1 : 0;
                }
                a.part_cnt[(size_t)blockIdx.y * (size_t)a.nt + (size_t)p] += cnt;   // (zeroed by the launcher; this thread alone writes it)
            }
        }
    }
    if (COUNT) {
        left += __shfl_xor(left, 1); left += __shfl_xor(left, 2);
        if (sel_ok && j == 0) a.part_ncand[(size_t)blockIdx.y * (size_t)a.nq + (size_t)(qb + sq)] = left;
    }
}

// one thread per held-out entry, then one per query: the integer partials of the splits summed
__global__ __launch_bounds__(256) void k_rank_merge(const int32_t *__restrict__ part_cnt, const int32_t *__restrict__ part_ncand, int nsplit,
                                                    int64_t nt, int64_t nq, int32_t *__restrict__ rank, int32_t *__restrict__ ncand)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nt) {
        int32_t r = 1;
        for (int s = 0; s < nsplit; ++s) r += part_cnt[(size_t)s * (size_t)nt + (size_t)e];
        rank[e] = r;
    }
    if (e < nq) {
        int32_t n = 0;
        for (int s = 0; s < nsplit; ++s) n += part_ncand[(size_t)s * (size_t)nq + (size_t)e];
        ncand[e] = n;
    }
}

}  // namespace bpmf
