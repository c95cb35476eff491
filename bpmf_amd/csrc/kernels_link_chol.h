// kernels_link_chol.h -- side information with a sampled lambda_beta: G(lambda) = F^T F + lambda I changes
// every half-iteration, so it is factored and solved against on the device (one translation unit: klinkchol.hip).
//
// Everything works on a PADDED copy Lp (Dp x Dp, Dp = 64 ceil(D / 64), row-major): rows and columns past D carry zeros and a unit
// diagonal, so every block is a whole 64 x 64 block and no kernel below has an edge.  The lower blocks of Lp become L (G = L L^T);
// the upper blocks receive L^T as the panels are finished, so every product below reads both operands along rows:
//
//   k_chol_form    Lp = [F^T F + lambda I, 0; 0, I]
//   k_chol_diag    block (j, j): L_jj by the row-oriented dot-product form in LDS (one wave, one row per lane), then L_jj^-1 by
//                  forward substitution (one column per lane); writes L_jj (upper half: L_jj^T), Linv[j] and LinvT[j] = L_jj^-T.
//                  A pivot that is not positive and finite raises *flag by an ordinary store and is replaced by 1.
//   k_chol_panel   blocks (i, j), i > j: L_ij = A_ij L_jj^-T, written in place and transposed into block (j, i)
//   k_chol_trail   blocks (i, k), i >= k > j: A_ik -= L_ij L_kj^T  (right-looking)
//   k_chol_pack    the right-hand sides into padded Dp x 128 arrays (zeros past D x n)
//   k_chol_solve   one block row of  L Y = P (forward, ascending j)  or  L^T X = Y + E (backward, descending; E_j joins Y_j as the
//                  block is read):  X_j = Dinv_j (X_j [+ E_j] - sum over the finished blocks), in place, 32 columns per workgroup
//   k_chol_unpack  rows < D, columns < ncw of the padded result into the caller's layout (columns n .. ncw - 1 zero)
//
// The products run on v_mfma_f64_16x16x4_f64 with the staging of k_link_gemm_nn (kernels_link.h): four waves own 16 rows each of
// a 64-row strip, the operand slices of 16 reduction rows are staged once per workgroup in one of two LDS buffers while the
// previous slice is multiplied.  No atomics; every sum runs in program order: the results are the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmf {

typedef double chol_d4 __attribute__((ext_vector_type(4)));

constexpr int kCholStep = 16;               // rows of the reduction staged per step (4 MFMA k-steps), as kCholStep

constexpr int kCholBlock = 64;              // block size of the factorisation: one 64-row strip of the products
constexpr int kCholRhs = 128;               // leading dimension of the padded right-hand sides
constexpr int kCholSolveCols = 32;          // right-hand-side columns per workgroup of k_chol_solve

// lane l: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; D[i = (l >> 4) + 4 reg][j = l & 15]
__device__ __forceinline__ chol_d4 chol_mfma(double a, double b, chol_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// acc (64 x NT * 16, rows w * 16 .. of wave w) += A (64 x 16 nsteps, leading dimension lda) B (16 nsteps x NT * 16, ldb).  No edges.
template <int NT>
__device__ __forceinline__ void chol_mac(const double *A, int64_t lda, const double *B, int64_t ldb, int nsteps,
                                         chol_d4 (&acc)[NT], double (&sA)[2][kCholBlock][kCholStep + 4],
                                         double (&sB)[2][kCholStep][NT * 16 + 16])
{
    constexpr int NC = NT * 16;
    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    if (nsteps <= 0) return;                                               // (uniform over the workgroup)
    double ra[4], rb[NT];
    auto load = [&](int s) {
        const int k0 = s * kCholStep;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int e = t + 256 * q; ra[q] = A[(int64_t)(e / kCholStep) * lda + k0 + e % kCholStep]; }
#pragma unroll
        for (int q = 0; q < NT; ++q) { const int e = t + 256 * q; rb[q] = B[(int64_t)(k0 + e / NC) * ldb + e % NC]; }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int e = t + 256 * q; sA[buf][e / kCholStep][e % kCholStep] = ra[q]; }
#pragma unroll
        for (int q = 0; q < NT; ++q) { const int e = t + 256 * q; sB[buf][e / NC][e % NC] = rb[q]; }
    };
    load(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) load(s + 1);
#pragma unroll
        for (int kk = 0; kk < kCholStep / 4; ++kk) {
            const double a = sA[buf][w * 16 + li][kk * 4 + kq];
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = chol_mfma(a, sB[buf][kk * 4 + kq][j * 16 + li], acc[j]);
        }
        if (s + 1 < nsteps) store(buf ^ 1);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_chol_form(const double *__restrict__ FtF, int D, double lambda, double *__restrict__ Lp, int Dp)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Dp * Dp) return;
    const int r = (int)(e / Dp), c = (int)(e % Dp);
    double v = r == c ? 1.0 : 0.0;
    if (r < D && c < D) v = FtF[(int64_t)r * D + c] + (r == c ? lambda : 0.0);
    Lp[e] = v;
}

__global__ __launch_bounds__(64) void k_chol_diag(double *Lp, int Dp, int j, double *__restrict__ Linv, double *__restrict__ LinvT,
                                                  int *__restrict__ flag)
{
    // One array holds both triangles: l_rc (r >= c) at sL[r * P + c], and x_ic of X = L^-1 (i >= c) at sL[c * P + i + 1], above the
    // diagonal (the pad column of the pitch takes i = 63).  Pitch 65: a lane per row reads and writes conflict-free.
    constexpr int B = kCholBlock, P = B + 1;
    __shared__ double sL[B * P];
    __shared__ double s_d;
    const int t = threadIdx.x;
    double *blk = Lp + ((int64_t)j * B) * Dp + (int64_t)j * B;
    for (int r = 0; r < B; ++r) sL[r * P + t] = blk[(int64_t)r * Dp + t];
    __syncthreads();
    for (int c = 0; c < B; ++c) {                                          // lane t >= c: l_tc = (a_tc - sum_{k < c} l_tk l_ck) / l_cc
        double s = sL[t * P + c];
        for (int k = 0; k < c; ++k) s -= sL[t * P + k] * sL[c * P + k];
        if (t == c) {
            if (!(s > 0.0) || !isfinite(s)) { *flag = 1; s = 1.0; }
            s_d = sqrt(s);
        }
        __syncthreads();
        if (t >= c) sL[t * P + c] = t == c ? s_d : s / s_d;
        __syncthreads();
    }
    for (int i = t; i < B; ++i) {                                          // lane t: column t of X by forward substitution, rows t ..
        double s = i == t ? 1.0 : 0.0;
        for (int k = t; k < i; ++k) s -= sL[i * P + k] * sL[t * P + k + 1];
        sL[t * P + i + 1] = s / sL[i * P + i];
    }
    __syncthreads();
    double *inv = Linv + (int64_t)j * B * B, *invT = LinvT + (int64_t)j * B * B;
    for (int r = 0; r < B; ++r) {
        blk[(int64_t)r * Dp + t] = t <= r ? sL[r * P + t] : sL[t * P + r];
        inv[r * B + t] = t <= r ? sL[t * P + r + 1] : 0.0;
        invT[r * B + t] = r <= t ? sL[r * P + t + 1] : 0.0;
    }
}

// grid nb - 1 - j: block row i = j + 1 + blockIdx.x
__global__ __launch_bounds__(256) void k_chol_panel(double *Lp, int Dp, int j, const double *__restrict__ LinvT)
{
    constexpr int B = kCholBlock, NT = 4;
    __shared__ double sA[2][kCholBlock][kCholStep + 4];
    __shared__ double sB[2][kCholStep][NT * 16 + 16];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    const int i = j + 1 + blockIdx.x;
    double *blk = Lp + ((int64_t)i * B) * Dp + (int64_t)j * B;              // (i, j)
    double *blkT = Lp + ((int64_t)j * B) * Dp + (int64_t)i * B;             // (j, i)
    chol_d4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = chol_d4{0.0, 0.0, 0.0, 0.0};
    chol_mac<NT>(blk, Dp, LinvT + (int64_t)j * B * B, B, B / kCholStep, acc, sA, sB);   // (ends with a barrier: every read of blk is done)
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = w * 16 + kq + 4 * reg, c = q * 16 + li;
            blk[(int64_t)r * Dp + c] = acc[q][reg];
            blkT[(int64_t)c * Dp + r] = acc[q][reg];
        }
}

// grid (m, m), m = nb - 1 - j: block (i, k) = (j + 1 + blockIdx.x, j + 1 + blockIdx.y), the lower ones only
__global__ __launch_bounds__(256) void k_chol_trail(double *Lp, int Dp, int j)
{
    constexpr int B = kCholBlock, NT = 4;
    __shared__ double sA[2][kCholBlock][kCholStep + 4];
    __shared__ double sB[2][kCholStep][NT * 16 + 16];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    const int i = j + 1 + blockIdx.x, k = j + 1 + blockIdx.y;
    if (k > i) return;
    const double *a = Lp + ((int64_t)i * B) * Dp + (int64_t)j * B;          // L_ij
    const double *b = Lp + ((int64_t)j * B) * Dp + (int64_t)k * B;          // L_kj^T
    double *c = Lp + ((int64_t)i * B) * Dp + (int64_t)k * B;
    chol_d4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = chol_d4{0.0, 0.0, 0.0, 0.0};
    chol_mac<NT>(a, Dp, b, Dp, B / kCholStep, acc, sA, sB);
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t o = (int64_t)(w * 16 + kq + 4 * reg) * Dp + q * 16 + li;
            c[o] -= acc[q][reg];
        }
}

__global__ __launch_bounds__(256) void k_chol_pack(const double *__restrict__ src, int64_t ld, int D, int n, double *__restrict__ dst, int Dp)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Dp * kCholRhs) return;
    const int r = (int)(e / kCholRhs), c = (int)(e % kCholRhs);
    dst[e] = (src && r < D && c < n) ? src[(int64_t)r * ld + c] : 0.0;
}

__global__ __launch_bounds__(256) void k_chol_unpack(const double *__restrict__ Xp, int D, int n, double *__restrict__ dst, int64_t ld, int ncw)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)D * ncw) return;
    const int r = (int)(e / ncw), c = (int)(e % ncw);
    dst[(int64_t)r * ld + c] = c < n ? Xp[(int64_t)r * kCholRhs + c] : 0.0;
}

// grid ceil(n / 32).  BACK = false: X_j = Linv_j (X_j - sum_{k < j} L_jk X_k);  true: X_j = LinvT_j (X_j + E_j - sum_{k > j} L_kj^T X_k).
// Dinv: Linv (forward) or LinvT (backward), nb blocks.  X, E: Dp x kCholRhs.
template <bool BACK>
__global__ __launch_bounds__(256) void k_chol_solve(const double *__restrict__ Lp, int Dp, int j, const double *__restrict__ Dinv,
                                                    double *X, const double *__restrict__ E)
{
    constexpr int B = kCholBlock, NT = kCholSolveCols / 16, NC = NT * 16;
    __shared__ double sA[2][kCholBlock][kCholStep + 4];
    __shared__ double sB[2][kCholStep][NC + 16];
    __shared__ double sT[B][NC + 16];
    const int t = threadIdx.x, w = t >> 6, l = t & 63, li = l & 15, kq = l >> 4;
    const int c0 = blockIdx.x * NC, nb = Dp / B;
    const int first = BACK ? j + 1 : 0, nblk = BACK ? nb - 1 - j : j;       // the finished blocks: first .. first + nblk - 1
    chol_d4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = chol_d4{0.0, 0.0, 0.0, 0.0};
    chol_mac<NT>(Lp + ((int64_t)j * B) * Dp + (int64_t)first * B, Dp, X + ((int64_t)first * B) * kCholRhs + c0, kCholRhs,
                 nblk * (B / kCholStep), acc, sA, sB);
    double *xj = X + ((int64_t)j * B) * kCholRhs + c0;
    const double *ej = (BACK && E) ? E + ((int64_t)j * B) * kCholRhs + c0 : nullptr;
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = w * 16 + kq + 4 * reg, c = q * 16 + li;
            const double y = xj[(int64_t)r * kCholRhs + c];
            sT[r][c] = (ej ? y + ej[(int64_t)r * kCholRhs + c] : y) - acc[q][reg];
        }
    __syncthreads();
    const double *dinv = Dinv + (int64_t)j * B * B + (int64_t)(w * 16 + li) * B;
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = chol_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < B / 4; ++kk) {
        const double a = dinv[kk * 4 + kq];
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[q] = chol_mfma(a, sT[kk * 4 + kq][q * 16 + li], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) xj[(int64_t)(w * 16 + kq + 4 * reg) * kCholRhs + q * 16 + li] = acc[q][reg];
}

}  // namespace bpmf
