// kernels_predcells.h -- predictions for a list of (query, candidate) cells from two sample rings (bpmf_hip_predict_cells), and the
// repacking of a sample ring for its read-back and load (bpmf_hip_side_samples_get / _set).  capi_model.hip; one translation unit:
// kpredcells.hip.  DESIGN.md section 26 has the definitions, the shape of the work and the measurements.
//
// With d_s = u_s(q) . v_s(c) over the S kept samples of the two rings (layout: kernels_topn.h; Kp = num_latent rounded up to 4, pad
// rows zero) and p_s = mean_rating + d_s:
//   mean = mean_rating + (1/S) sum_s d_s      std = sqrt(sum_s (d_s - dbar)^2 / (S - 1))  [0 for S = 1]
//   prob = (1/S) sum_s Phi((p_s - t) / sigma)                       sigma < DBL_MIN: (1/S) #{s : p_s > t}
// mean and the deviations are carried by Welford's recurrence over d_s in s order (as kernels_predtile.h): mean_rating is added once
// at the end, so it never enters a difference, and no sum of squares is formed.
//
//   k_predict_cells<G, PROB>   (PROB: with the exceedance probability; the plain form carries no erfc and fewer registers)
//       The host has grouped the list by query (stable counting sort) and cut every query's run into segments of at most
//       kCellsR * 256 / G cells.  A workgroup of four waves takes one segment.  G = the largest power of two <= Kp / 2 (2 .. 64) lanes
//       share a cell: lane g of the group takes the 16-byte pairs g, g + G, ... of a sample's Kp doubles, so a wave-wide load
//       covers 64 / G cells at once and no lane idles at small Kp (at Kp = 4 a wave reads 32 cells per load, at Kp = 128 one).
//       Every group carries kCellsR cells side by side (independent loads in flight).  The query's ring row is staged in LDS
//       once per workgroup, in chunks of pc_chunk(Kp) samples (S has no upper bound); the candidates' rows are streamed from
//       global memory, 16 bytes per lane and load (ring rows are 32-byte aligned: Kp is a multiple of 4).
//       Order of additions of a cell: per sample the pairs of a lane ascending (fma), then a butterfly over the G lanes (xor G / 2
//       .. 1; both lanes of a pair add the same two numbers, so every lane of the group holds the same bits), then Welford in s
//       order; the probability terms of a group's cells are spread over four of its lanes (one erfc per lane and sample), each
//       cell's summed in s order by its lane.  It all depends on Kp and S alone: not on the other cells, the cell's place in the list or the grid.  No atomics.
//       Results go to the caller's order through the permutation of the sort.
//   k_samples_pack / k_samples_unpack   slots [s_from, s_from + n) of columns [c_from, c_from + nc) of a ring <-> nc x n x Kt doubles
//       without the pad rows; unpack writes the pad rows as zeros
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmf {

constexpr int kCellsR = 4;                     // cells a lane group carries side by side
constexpr int kCellsLds = 2048;                // doubles of the staged query row (16 KiB per workgroup)

__host__ __device__ inline int pc_group(int Kp) { int g = 2; while (2 * g <= Kp / 2 && g < 64) g *= 2; return g; }
__host__ __device__ inline int pc_chunk(int Kp) { return kCellsLds / Kp; }     // samples per staged chunk (Kp <= 128: >= 16)
__host__ __device__ inline int pc_segment(int Kp) { return kCellsR * 256 / pc_group(Kp); }

struct PredCellsArgs {
    const double *qring, *cring;               // sample rings of the query / candidate side
    int64_t qstride, cstride;                  // doubles per column of either ring (max_samples x Kp)
    int Kp, S;
    double mean_rating, t, sigma;
    const int32_t *seg_q, *seg_beg, *seg_cnt;  // per workgroup: its query, its first cell in the sorted list, its cells (1 .. pc_segment)
    const int32_t *cand, *orig;                // per sorted cell: its candidate, its place in the caller's list
    double *mean, *std, *prob;                 // caller's order; prob may be NULL
};

template <int G, bool PROB>
__global__ __launch_bounds__(256) void k_predict_cells(PredCellsArgs a)
{
    __shared__ __attribute__((aligned(16))) double urow[kCellsLds];
    constexpr int NG = 256 / G;                                 // lane groups of the workgroup
    const int tid = threadIdx.x, grp = tid / G, g = tid % G;
    const int Kp = a.Kp, S = a.S, K2 = Kp >> 1, SC = pc_chunk(Kp);
    const int cnt = a.seg_cnt[blockIdx.x], beg = a.seg_beg[blockIdx.x];
    const double *uq = a.qring + (int64_t)a.seg_q[blockIdx.x] * a.qstride;

    const double2 *vrow[kCellsR];
    bool ok[kCellsR];
    constexpr int PL = G < kCellsR ? G : kCellsR, NP = kCellsR / PL;   // the probability terms of a group's cells are shared by PL of its lanes
    const int pl = g % PL;
    double m[kCellsR], m2[kCellsR], ps[NP];
#pragma unroll
    for (int r = 0; r < kCellsR; ++r) {
        const int i = r * NG + grp;                             // the cell of the segment (the groups fill before a second cell)
        ok[r] = i < cnt;
        vrow[r] = reinterpret_cast<const double2 *>(a.cring + (int64_t)(ok[r] ? a.cand[beg + i] : 0) * a.cstride);
        m[r] = 0.0; m2[r] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) ps[k] = 0.0;
    const bool noisy = a.sigma >= 2.2250738585072014e-308;
    const double inv_sigma = noisy ? 1.0 / a.sigma : 0.0;

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
            double part[kCellsR];
#pragma unroll
            for (int r = 0; r < kCellsR; ++r) part[r] = 0.0;
            for (int j = g; j < K2; j += G) {
                const double2 uu = us[j];
                double2 vv[kCellsR];
#pragma unroll
                for (int r = 0; r < kCellsR; ++r) if (ok[r]) vv[r] = vrow[r][vo + j];
#pragma unroll
                for (int r = 0; r < kCellsR; ++r) if (ok[r]) part[r] = fma(uu.y, vv[r].y, fma(uu.x, vv[r].x, part[r]));
            }
#pragma unroll
            for (int r = 0; r < kCellsR; ++r) {
#pragma unroll
                for (int off = G / 2; off >= 1; off >>= 1) part[r] += __shfl_xor(part[r], off);
                const double d = part[r], dl = d - m[r];
                m[r] += dl / (double)(s0 + s + 1);
                m2[r] = fma(dl, d - m[r], m2[r]);
            }
            if (PROB) {                                         // every lane of the group holds d of its kCellsR cells: lane pl takes cells pl, pl + PL, ..
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    double d = part[k * PL];
#pragma unroll
                    for (int x = 1; x < PL; ++x) d = pl == x ? part[k * PL + x] : d;
                    const double e = (a.mean_rating + d) - a.t;
                    ps[k] += noisy ? 0.5 * erfc(-(e * inv_sigma) * 0.70710678118654752440) : (e > 0.0 ? 1.0 : 0.0);
                }
            }
        }
    }
    if (g == 0) {
#pragma unroll
        for (int r = 0; r < kCellsR; ++r) {
            if (!ok[r]) continue;
            const int o = a.orig[beg + r * NG + grp];
            a.mean[o] = a.mean_rating + m[r];
            a.std[o] = S > 1 ? sqrt(m2[r] / (double)(S - 1)) : 0.0;
        }
    }
    if (PROB && g < PL) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = (k * PL + g) * NG + grp;
            if (i < cnt) a.prob[a.orig[beg + i]] = ps[k] / (double)S;
        }
    }
}

// packed[(c * n + s) * Kt + k] = ring[(c_from + c) * stride + (s_from + s) * Kp + k]
__global__ __launch_bounds__(256) void k_samples_pack(const double *__restrict__ ring, int64_t stride, int Kp, int Kt, int64_t c_from,
                                                      int64_t nc, int s_from, int n, double *__restrict__ packed)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nc * n * Kt) return;
    const int64_t cs = e / Kt;
    const int k = (int)(e - cs * Kt);
    const int64_t c = cs / n;
    const int s = (int)(cs - c * n);
    packed[e] = ring[(c_from + c) * stride + (int64_t)(s_from + s) * Kp + k];
}

// the inverse into slots [0, n); pad rows Kt .. Kp - 1 zero
__global__ __launch_bounds__(256) void k_samples_unpack(const double *__restrict__ packed, int64_t stride, int Kp, int Kt, int64_t c_from,
                                                        int64_t nc, int n, double *__restrict__ ring)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nc * n * Kp) return;
    const int64_t cs = e / Kp;
    const int k = (int)(e - cs * Kp);
    const int64_t c = cs / n;
    const int s = (int)(cs - c * n);
    ring[(c_from + c) * stride + (int64_t)s * Kp + k] = k < Kt ? packed[cs * Kt + k] : 0.0;
}

}  // namespace bpmf
