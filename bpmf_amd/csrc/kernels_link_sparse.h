// kernels_link_sparse.h -- side information with a SPARSE feature matrix F (N x D, fp64 values or all ones): the link matrix is
// drawn by K conjugate-gradient solves in lockstep on a noise-injected right-hand side, G = F^T F + lambda I is never formed
// (bpmf_hip_side_set_features_sparse, capi_link_sparse.hip; one translation unit: klinksp.hip).  DESIGN.md section 14.
//
//   k_sp_rows          C[r] = sum over the nonzeros of row r, IN INDEX ORDER, of val * V[index] (+ lambda P[r]): the one gather
//                      product.  F row-compressed gives F V (N x n), F column-compressed (= F^T row-compressed) gives F^T X
//                      (D x n).  No scatter, no atomic.  Rows of more than kSpChunk nonzeros are left to the next two kernels.
//   k_sp_chunks        part[q] = the same sum over chunk q (kSpChunk nonzeros) of a long row
//   k_sp_sum_long      C[r] = part[first] + part[first + 1] + ... IN CHUNK ORDER (+ lambda P[r]) for the long rows
//   k_cg_dot           partial[b][k] = sum over the kCgBlock rows of block b of a[d][k] b[d][k], fixed order inside the block
//   k_cg_init / k_cg_alpha / k_cg_beta   one workgroup: the per-column scalars from the partials, added IN BLOCK ORDER; they
//                      stay on the device.  k_cg_init / k_cg_beta write the number of active columns to the host's word.
//   k_cg_xr            x += alpha p, r -= alpha q on the active columns, fused with the partials of the new |r|^2
//   k_cg_p             p = r + beta p on the active columns
//   k_link_noise_rows  row i of a noise matrix: the first kt normals of the polar method on Philox4x32-10(counter = {i lo, i hi,
//                      it, attempt}, key = {42, key word}), times R^-T, scaled and added to (base - 1 bvec^T)
//
// Every result depends on the operands only, never on the grid: a row's sum runs over its nonzeros in index order whatever the
// unrolling (one fma chain), a long row's chunks are fixed by kSpChunk, a scalar's blocks by kCgBlock and the column width CW.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace bpmf {

constexpr int kSpChunk = 512;               // nonzeros per partial of a long row (fixed: the summation order)
constexpr int kCgBlock = 256;               // rows of a D x n array per partial of a CG scalar (fixed: the summation order)
constexpr int kCgMaxN = 128;                // columns solved in lockstep

// the per-column scalars of a solve (device memory; copied to the host once per solve for the statistics)
struct CgState {
    double bb[kCgMaxN], rr[kCgMaxN], alpha[kCgMaxN], beta[kCgMaxN];
    int active[kCgMaxN], iters[kCgMaxN];
    int nactive, pad_;
};

// sum over p in [beg, end) of val[p] * V[idx[p]][l (, l + 64)], one fma per nonzero in index order; four gathers in flight
template <int LPR>
__device__ __forceinline__ void sp_row_sum(const int32_t *__restrict__ idx, const double *__restrict__ vals, int64_t beg, int64_t end,
                                           const double *__restrict__ V, int64_t ldv, int n, int l, double &a0, double &a1)
{
    constexpr bool TWO = LPR == 64;
    const bool on0 = l < n, on1 = TWO && l + 64 < n;
    int64_t p = beg;
    for (; p + 4 <= end; p += 4) {
        int32_t j[4];
        double v[4], x0[4], x1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { j[u] = idx[p + u]; v[u] = vals ? vals[p + u] : 1.0; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            x0[u] = on0 ? V[(int64_t)j[u] * ldv + l] : 0.0;
            x1[u] = on1 ? V[(int64_t)j[u] * ldv + l + 64] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { a0 = fma(v[u], x0[u], a0); a1 = fma(v[u], x1[u], a1); }
    }
    for (; p < end; ++p) {
        const int32_t j = idx[p];
        const double v = vals ? vals[p] : 1.0;
        a0 = fma(v, on0 ? V[(int64_t)j * ldv + l] : 0.0, a0);
        a1 = fma(v, on1 ? V[(int64_t)j * ldv + l + 64] : 0.0, a1);
    }
}

// LPR lanes per row (8 .. 64, ncw <= LPR or LPR = 64 and ncw <= 128), 256 / LPR rows per group, wg_groups consecutive groups per
// workgroup (BPMF_LINK_WG_CHUNKS: the grid, never the bits).  Columns n .. ncw - 1 of C are written as exact zeros.
template <int LPR>
__global__ __launch_bounds__(256) void k_sp_rows(const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx, const double *__restrict__ vals,
                                                 int64_t nrows, const double *__restrict__ V, int64_t ldv, int n, int ncw, double *C,
                                                 int64_t ldc, double lambda, const double *P, int64_t ldp, int wg_groups)   // (P may be C)
{
    constexpr int RPW = 256 / LPR;
    const int l = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    for (int g = 0; g < wg_groups; ++g) {
        const int64_t r = ((int64_t)blockIdx.x * wg_groups + g) * RPW + sub;
        if (r >= nrows) return;
        const int64_t beg = ptr[r], end = ptr[r + 1];
        if (end - beg > kSpChunk) continue;                                // a long row: k_sp_chunks + k_sp_sum_long
        double a0 = 0.0, a1 = 0.0;
        sp_row_sum<LPR>(idx, vals, beg, end, V, ldv, n, l, a0, a1);
        if (l < ncw) C[r * ldc + l] = l < n ? (P ? fma(lambda, P[r * ldp + l], a0) : a0) : 0.0;
        if (LPR == 64 && l + 64 < ncw) C[r * ldc + l + 64] = l + 64 < n ? (P ? fma(lambda, P[r * ldp + l + 64], a1) : a1) : 0.0;
    }
}

// chunk q of the long rows: nonzeros [cbeg[q], cend[q]); part[q][0 .. n)
template <int LPR>
__global__ __launch_bounds__(256) void k_sp_chunks(const int64_t *__restrict__ cbeg, const int64_t *__restrict__ cend, int64_t nchunks,
                                                   const int32_t *__restrict__ idx, const double *__restrict__ vals, const double *__restrict__ V,
                                                   int64_t ldv, int n, double *__restrict__ part, int wg_groups)
{
    constexpr int RPW = 256 / LPR;
    const int l = threadIdx.x % LPR, sub = threadIdx.x / LPR;
    for (int g = 0; g < wg_groups; ++g) {
        const int64_t q = ((int64_t)blockIdx.x * wg_groups + g) * RPW + sub;
        if (q >= nchunks) return;
        double a0 = 0.0, a1 = 0.0;
        sp_row_sum<LPR>(idx, vals, cbeg[q], cend[q], V, ldv, n, l, a0, a1);
        if (l < n) part[q * n + l] = a0;
        if (LPR == 64 && l + 64 < n) part[q * n + l + 64] = a1;
    }
}

// long row j (row number lrow[j]) owns the chunks lfirst[j] .. lfirst[j + 1) - 1; one thread per (j, column < ncw)
__global__ __launch_bounds__(256) void k_sp_sum_long(const int32_t *__restrict__ lrow, const int64_t *__restrict__ lfirst, int nlong,
                                                     const double *__restrict__ part, int n, int ncw, double *C, int64_t ldc,
                                                     double lambda, const double *P, int64_t ldp)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)nlong * ncw) return;
    const int j = (int)(e / ncw), col = (int)(e % ncw);
    const int64_t r = lrow[j];
    double s = 0.0;
    if (col < n) {
        for (int64_t q = lfirst[j]; q < lfirst[j + 1]; ++q) s += part[q * n + col];
        if (P) s = fma(lambda, P[r * ldp + col], s);
    }
    C[r * ldc + col] = s;
}

// ---- conjugate gradients: K systems in lockstep ---------------------------------------------------------------------------
// CW: the smallest power of two >= n (8 .. 128), fixed by n.  Thread (c, rl) of a block adds rows rl, rl + RL, ... of its column
// in row order, the RL row-lanes are added by a fixed tree.
template <int CW>
__device__ __forceinline__ double cg_block_reduce(double acc, double *s)
{
    constexpr int RL = 256 / CW;
    const int t = threadIdx.x, rl = t / CW;
    s[t] = acc;
    __syncthreads();
#pragma unroll
    for (int h = RL / 2; h >= 1; h >>= 1) {
        if (rl < h) s[t] += s[t + h * CW];
        __syncthreads();
    }
    return s[t % CW];
}

template <int CW>
__global__ __launch_bounds__(256) void k_cg_dot(const double *__restrict__ a, const double *__restrict__ b, int64_t ld, int64_t D, int n,
                                                double *__restrict__ partial)
{
    constexpr int RL = 256 / CW;
    __shared__ double s[256];
    const int c = threadIdx.x % CW, rl = threadIdx.x / CW;
    const int64_t d0 = (int64_t)blockIdx.x * kCgBlock;
    double acc = 0.0;
    if (c < n)
        for (int q = rl; q < kCgBlock; q += RL) {
            const int64_t d = d0 + q;
            if (d < D) acc = fma(a[d * ld + c], b[d * ld + c], acc);
        }
    const double tot = cg_block_reduce<CW>(acc, s);
    if (rl == 0 && c < n) partial[(int64_t)blockIdx.x * n + c] = tot;
}

__device__ __forceinline__ double cg_sum_blocks(const double *__restrict__ partial, int64_t nblocks, int n, int k)
{
    double s = 0.0;
    for (int64_t b = 0; b < nblocks; ++b) s += partial[b * n + k];
    return s;
}

// the number of active columns, counted by thread 0 in column order, to the state and to the host's word
__device__ __forceinline__ void cg_publish(CgState *st, int n, int *__restrict__ word)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        int na = 0;
        for (int k = 0; k < n; ++k) na += st->active[k];
        st->nactive = na;
        if (word) *word = na;
    }
}

// rr = bb = |rhs_k|^2 from the partials of k_cg_dot(r, r); a column starts active iff rr > tol2 * bb (never for rhs_k = 0)
__global__ __launch_bounds__(kCgMaxN) void k_cg_init(const double *__restrict__ partial, int64_t nblocks, int n, double tol2, CgState *st,
                                                     int *__restrict__ word)
{
    const int k = threadIdx.x;
    if (k < n) {
        const double s = cg_sum_blocks(partial, nblocks, n, k);
        st->bb[k] = s; st->rr[k] = s; st->alpha[k] = 0.0; st->beta[k] = 0.0;
        st->active[k] = s > tol2 * s ? 1 : 0;
        st->iters[k] = 0;
    }
    cg_publish(st, n, word);
}

// alpha_k = rr_k / p_k . q_k from the partials of k_cg_dot(p, q); 0 for a frozen column
__global__ __launch_bounds__(kCgMaxN) void k_cg_alpha(const double *__restrict__ partial, int64_t nblocks, int n, CgState *st)
{
    const int k = threadIdx.x;
    if (k >= n) return;
    st->alpha[k] = st->active[k] ? st->rr[k] / cg_sum_blocks(partial, nblocks, n, k) : 0.0;
}

template <int CW>
__global__ __launch_bounds__(256) void k_cg_xr(double *__restrict__ x, double *__restrict__ r, const double *__restrict__ p,
                                               const double *__restrict__ q, int64_t ld, int64_t D, int n, const CgState *__restrict__ st,
                                               double *__restrict__ partial)
{
    constexpr int RL = 256 / CW;
    __shared__ double s[256];
    const int c = threadIdx.x % CW, rl = threadIdx.x / CW;
    const int64_t d0 = (int64_t)blockIdx.x * kCgBlock;
    double acc = 0.0;
    if (c < n && st->active[c]) {
        const double al = st->alpha[c];
        for (int i = rl; i < kCgBlock; i += RL) {
            const int64_t d = d0 + i;
            if (d < D) {
                const int64_t e = d * ld + c;
                x[e] = fma(al, p[e], x[e]);
                const double rn = fma(-al, q[e], r[e]);
                r[e] = rn;
                acc = fma(rn, rn, acc);
            }
        }
    }
    const double tot = cg_block_reduce<CW>(acc, s);
    if (rl == 0 && c < n) partial[(int64_t)blockIdx.x * n + c] = tot;
}

// the new |r_k|^2 of the active columns from the partials of k_cg_xr: beta_k, one iteration charged, the next active mask
__global__ __launch_bounds__(kCgMaxN) void k_cg_beta(const double *__restrict__ partial, int64_t nblocks, int n, double tol2, CgState *st,
                                                     int *__restrict__ word)
{
    const int k = threadIdx.x;
    if (k < n) {
        if (st->active[k]) {
            const double rn = cg_sum_blocks(partial, nblocks, n, k);
            st->beta[k] = rn / st->rr[k];
            st->rr[k] = rn;
            st->iters[k] += 1;
            st->active[k] = rn > tol2 * st->bb[k] ? 1 : 0;
        } else
            st->beta[k] = 0.0;
    }
    cg_publish(st, n, word);
}

__global__ __launch_bounds__(256) void k_cg_p(double *__restrict__ p, const double *__restrict__ r, int64_t ld, int64_t D, int n,
                                              const CgState *__restrict__ st)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= D * n) return;
    const int64_t d = e / n;
    const int c = (int)(e % n);
    if (!st->active[c]) return;
    const int64_t o = d * ld + c;
    p[o] = fma(st->beta[c], p[o], r[o]);
}

// x = 0, p = r on the n columns of the D x ld arrays (r holds the right-hand side)
__global__ __launch_bounds__(256) void k_cg_start(double *__restrict__ x, double *__restrict__ p, const double *__restrict__ r, int64_t ld,
                                                  int64_t D, int n)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= D * n) return;
    const int64_t o = (e / n) * ld + (e % n);
    x[o] = 0.0;
    p[o] = r[o];
}

// ---- noise rows -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sp_polar_r2(double x, double y)
{
#pragma clang fp contract(off)
    return x * x + y * y;      // two roundings + add, as the un-fused host restatement evaluates it
}

// One wave per row, four rows per workgroup.  out[i][j] = (base ? base[i][j] - bvec[j] : 0) + scale * sum_{m >= j} z[m] Rinv[j][m],
// j < kt (Rinv: kt x kt row-major upper triangular, or NULL for the normals themselves); kt <= 128.
__global__ __launch_bounds__(256) void k_link_noise_rows(int64_t nrows, int kt, uint32_t it, uint32_t key1, const double *__restrict__ Rinv,
                                                         const double *__restrict__ base, int64_t ldb, const double *__restrict__ bvec,
                                                         double scale, double *__restrict__ out, int64_t ldo)
{
    __shared__ double sz[4][kCgMaxN];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + w;
    if (i < nrows) {                                                       // (wave-uniform)
        const uint32_t c0 = (uint32_t)((uint64_t)i & 0xFFFFFFFFull), c1 = (uint32_t)((uint64_t)i >> 32);
        int produced = 0;
        uint32_t b0 = 0;
        while (produced < kt) {                                            // attempt a <-> block a; normal j = the j-th accepted attempt
            const Philox4 b = philox4x32_10(c0, c1, it, b0 + (uint32_t)lane, 42u, key1);
            const double x = 2.0 * canonical53(b.w[3], b.w[2]) - 1.0;
            const double y = 2.0 * canonical53(b.w[1], b.w[0]) - 1.0;
            const double r2 = sp_polar_r2(x, y);
            const bool acc = !(r2 > 1.0 || r2 == 0.0);
            const unsigned long long m = __ballot(acc);
            const int rank = produced + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (acc && rank < kt) sz[w][rank] = y * polar_mult(r2);
            produced += __popcll(m);
            b0 += 64u;
        }
    }
    __syncthreads();
    if (i >= nrows) return;
    for (int j = lane; j < kt; j += 64) {
        double s;
        if (Rinv) {
            s = 0.0;
            for (int m = j; m < kt; ++m) s = fma(sz[w][m], Rinv[j * kt + m], s);
        } else
            s = sz[w][j];
        const double b = base ? base[i * ldb + j] - bvec[j] : 0.0;
        out[i * ldo + j] = fma(scale, s, b);                               // (scale 1, no base: s itself)
    }
}

}  // namespace bpmf
