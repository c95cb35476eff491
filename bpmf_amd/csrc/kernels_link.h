// kernels_link.h -- side information: the link between a side's feature matrix F (N x D, row-major, fp64) and the prior of its
// factors (bpmf_hip_side_set_features / bpmf_hip_link_sample, capi_link.hip; one translation unit: klink.hip).  DESIGN.md
// section 13 has the model.
//
//   k_link_gemm_tn     part[chunk] = A[chunk rows]^T (B - 1 bvec^T)[chunk rows]: A (N x D), B (N x n), both row-major, the
//                      reduction runs over the LONG dimension N, cut into chunks of kLinkChunk rows.  F^T (U - 1 mu^T), F^T F,
//                      beta^T beta.
//   k_link_sum_chunks  C = sum of the partials IN CHUNK ORDER (no floating-point atomics: C depends on N, never on the grid)
//   k_link_gemm_nn     C (N x n) = A (N x Dr) B (Dr x n), row-major: the offsets M = F beta in the factors' layout, and
//                      beta = [G^-1 | L_G^-T] [P ; E]
//   k_link_residual    r~_p = r_p - m_c . y_r for every rating p of the side (column c, row r): k_probit_latent without the draw
//   k_link_shift       U = U~ + M, and the partial sums of |U|^2 of fixed blocks of kLinkShiftBlock elements
//
// Both products run on v_mfma_f64_16x16x4_f64.  A workgroup of four waves owns a 64-row strip of the result and up to 128
// columns (NT tiles of 16 per wave); the operand slices of one step (kLinkStep rows of the reduction) are staged ONCE per
// workgroup in LDS and read from there by all four waves, the global loads of step s + 1 are in flight while step s is
// multiplied (two LDS buffers, one barrier per step).  Rows / columns past the edge of an operand are staged as zeros, so any
// N, D, n works and the pad columns of a result (num_latent padded to the instantiated size) are exactly zero.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_gather.h"     // probit_tile_dots, kProbitTile, sse_column

namespace bpmf {

typedef double link_d4 __attribute__((ext_vector_type(4)));

constexpr int kLinkChunk = 2048;            // rows of the long dimension per partial of k_link_gemm_tn (fixed: the summation order)
constexpr int kLinkStep = 16;               // rows of the reduction staged per step (4 MFMA k-steps)
constexpr int kLinkRows = 64;               // rows of the result per workgroup (16 per wave)
constexpr int kLinkShiftBlock = 4096;       // elements per workgroup of k_link_shift (fixed: the order of the norm)

// lane l: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; D[i = (l >> 4) + 4 reg][j = l & 15]
__device__ __forceinline__ link_d4 link_mfma(double a, double b, link_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// ---- C = A^T B over the long dimension ------------------------------------------------------------------------------------
// grid (ceil(D / 64), ceil(nchunks / wg_chunks)); workgroup (bx, by) computes, one after the other, the partials of the chunks
// by * wg_chunks .. of rows bx * 64 .. of the result.  part[chunk][d][j], d < D, j < n.
template <int NT>
__global__ __launch_bounds__(256) void k_link_gemm_tn(const double *__restrict__ A, int64_t lda, const double *__restrict__ B, int64_t ldb,
                                                      const double *__restrict__ bvec, int64_t N, int D, int n, int wg_chunks,
                                                      double *__restrict__ part)
{
    constexpr int NC = NT * 16, PA = kLinkRows + 16, PB = NC + 16;       // (pitches: the four k-rows of an operand read fall into different banks)
    __shared__ double sA[2][kLinkStep][PA];
    __shared__ double sB[2][kLinkStep][PB];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    const int d0 = blockIdx.x * kLinkRows;
    const int64_t nchunks = (N + kLinkChunk - 1) / kLinkChunk;
    double ra[4], rb[NT];
    for (int cc = 0; cc < wg_chunks; ++cc) {
        const int64_t chunk = (int64_t)blockIdx.y * wg_chunks + cc;
        if (chunk >= nchunks) break;                                       // (uniform over the workgroup)
        const int64_t r0 = chunk * kLinkChunk, r1 = r0 + kLinkChunk < N ? r0 + kLinkChunk : N;
        const int nsteps = (int)((r1 - r0 + kLinkStep - 1) / kLinkStep);
        auto load = [&](int s) {
            const int64_t i0 = r0 + (int64_t)s * kLinkStep;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = t + 256 * q, row = e / kLinkRows, col = e % kLinkRows;
                const int64_t i = i0 + row;
                ra[q] = (i < r1 && d0 + col < D) ? A[i * lda + d0 + col] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const int e = t + 256 * q, row = e / NC, col = e % NC;
                const int64_t i = i0 + row;
                rb[q] = (i < r1 && col < n) ? B[i * ldb + col] - (bvec ? bvec[col] : 0.0) : 0.0;
            }
        };
        auto store = [&](int buf) {
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int e = t + 256 * q; sA[buf][e / kLinkRows][e % kLinkRows] = ra[q]; }
#pragma unroll
            for (int q = 0; q < NT; ++q) { const int e = t + 256 * q; sB[buf][e / NC][e % NC] = rb[q]; }
        };
        link_d4 acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = link_d4{0.0, 0.0, 0.0, 0.0};
        __syncthreads();                                                   // (the previous chunk's last step may still be read)
        load(0);
        store(0);
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
            const int buf = s & 1;
            if (s + 1 < nsteps) load(s + 1);
#pragma unroll
            for (int kk = 0; kk < kLinkStep / 4; ++kk) {
                const double a = sA[buf][kk * 4 + kq][w * 16 + li];
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = link_mfma(a, sB[buf][kk * 4 + kq][j * 16 + li], acc[j]);
            }
            if (s + 1 < nsteps) store(buf ^ 1);
            __syncthreads();
        }
        double *out = part + (size_t)chunk * (size_t)D * (size_t)n;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int d = d0 + w * 16 + kq + 4 * reg, col = j * 16 + li;
                if (d < D && col < n) out[(size_t)d * n + col] = acc[j][reg];
            }
    }
}

// C[d][j] = part[0][d][j] + part[1][d][j] + ... in chunk order
__global__ __launch_bounds__(256) void k_link_sum_chunks(const double *__restrict__ part, int64_t nchunks, int D, int n, double *__restrict__ C,
                                                         int64_t ldc)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, tot = (int64_t)D * n;
    if (e >= tot) return;
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) s += part[c * tot + e];
    C[(e / n) * ldc + (e % n)] = s;
}

// ---- C = A B, the reduction over the short dimension ----------------------------------------------------------------------
// grid ceil(N / 64).  Columns n .. ncw - 1 of C (ncw <= NT * 16) are written as exact zeros: the pad slots of the factors' layout.
template <int NT>
__global__ __launch_bounds__(256) void k_link_gemm_nn(const double *__restrict__ A, int64_t lda, const double *__restrict__ B, int64_t ldb,
                                                      int64_t N, int Dr, int n, double *__restrict__ C, int64_t ldc, int ncw)
{
    constexpr int NC = NT * 16, PA = kLinkStep + 4, PB = NC + 16;
    __shared__ double sA[2][kLinkRows][PA];
    __shared__ double sB[2][kLinkStep][PB];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * kLinkRows;
    const int nsteps = (Dr + kLinkStep - 1) / kLinkStep;
    double ra[4], rb[NT];
    auto load = [&](int s) {
        const int k0 = s * kLinkStep;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + 256 * q, row = e / kLinkStep, col = e % kLinkStep;
            ra[q] = (i0 + row < N && k0 + col < Dr) ? A[(i0 + row) * lda + k0 + col] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int e = t + 256 * q, row = e / NC, col = e % NC;
            rb[q] = (k0 + row < Dr && col < n) ? B[(int64_t)(k0 + row) * ldb + col] : 0.0;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int e = t + 256 * q; sA[buf][e / kLinkStep][e % kLinkStep] = ra[q]; }
#pragma unroll
        for (int q = 0; q < NT; ++q) { const int e = t + 256 * q; sB[buf][e / NC][e % NC] = rb[q]; }
    };
    link_d4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = link_d4{0.0, 0.0, 0.0, 0.0};
    load(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) load(s + 1);
#pragma unroll
        for (int kk = 0; kk < kLinkStep / 4; ++kk) {
            const double a = sA[buf][w * 16 + li][kk * 4 + kq];
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = link_mfma(a, sB[buf][kk * 4 + kq][j * 16 + li], acc[j]);
        }
        if (s + 1 < nsteps) store(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t i = i0 + w * 16 + kq + 4 * reg;
            const int col = j * 16 + li;
            if (i < N && col < ncw) C[i * ldc + col] = acc[j][reg];
        }
}

// ---- residuals ------------------------------------------------------------------------------------------------------------
// One tile of kProbitTile consecutive ratings per workgroup; `offs` (the side's offsets M) and `other` have the factors' layout.
template <int K>
__global__ __launch_bounds__(kProbitTile) void k_link_residual(const int64_t *__restrict__ colptr, int64_t ncols,
                                                               const int32_t *__restrict__ rowidx, const double *__restrict__ vals,
                                                               int64_t nnz, const double *__restrict__ offs, const double *__restrict__ other,
                                                               int kt, double *__restrict__ out)
{
    __shared__ int64_t s_col[kProbitTile];
    __shared__ int32_t s_row[kProbitTile];
    __shared__ double s_m[kProbitTile];
    const int64_t p0 = (int64_t)blockIdx.x * kProbitTile;
    const int n = (int)(nnz - p0 < kProbitTile ? nnz - p0 : kProbitTile);
    const int64_t p = p0 + threadIdx.x;
    if ((int)threadIdx.x < n) {
        const int64_t c0 = sse_column(colptr, 0, ncols, p0);
        s_col[threadIdx.x] = sse_column(colptr, c0, ncols, p);
        s_row[threadIdx.x] = rowidx[p];
    }
    __syncthreads();
    probit_tile_dots<K, double>(s_col, s_row, n, offs, other, kt, s_m);
    __syncthreads();
    if ((int)threadIdx.x < n) out[p] = vals[p] - s_m[threadIdx.x];
}

// ---- shift ----------------------------------------------------------------------------------------------------------------
// items[e] += offs[e] for the `total` elements of the factors' layout; partial[block] = sum of the new items[e]^2 of the block's
// kLinkShiftBlock elements, added per thread in element order and over the threads by a fixed tree.
__global__ __launch_bounds__(256) void k_link_shift(double *__restrict__ items, const double *__restrict__ offs, int64_t total,
                                                    double *__restrict__ partial)
{
    __shared__ double s_sum[256];
    const int64_t base = (int64_t)blockIdx.x * kLinkShiftBlock;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kLinkShiftBlock / 256; ++q) {
        const int64_t e = base + threadIdx.x + 256 * q;
        if (e < total) { const double v = items[e] + offs[e]; items[e] = v; s = fma(v, v, s); }
    }
    s_sum[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) s_sum[threadIdx.x] += s_sum[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s_sum[0];
}

}  // namespace bpmf
