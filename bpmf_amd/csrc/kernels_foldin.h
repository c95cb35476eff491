// kernels_foldin.h -- fold-in: the factors of rows that arrive after training with a few ratings and no features, drawn against the
// kept posterior samples (bpmf_hip_foldin, capi_foldin.hip; one translation unit: kfoldin.hip).  DESIGN.md section 19 has the model.
//
//   k_foldin<KP>   one workgroup per (new row i, kept sample s):
//                      Lambda* = Lambda_s + alpha_s sum_j v_js v_js^T,   b = Lambda_s mu_s + alpha_s sum_j (r_ij - mean) v_js
//                      Lambda* = L L^T,   u_is = L^-T (L^-1 b + z),   z ~ N(0, I) or 0
//                  v_js: row j of sample s of the candidate side's ring; (alpha_s, Lambda_s, Lambda_s mu_s): slot s of the hyper ring.
//
// The phases of an item, all in LDS:
//   1. Gram and right-hand side.  The ratings are taken in chunks of kFoldinChunk: the chunk's ring rows (kp contiguous doubles each)
//      are staged, then every thread adds the chunk's products to the elements it owns, in rating order.  An element is owned by
//      one thread and summed in one order: no atomics, the same bits from every call and in every batch.
//   2. Cholesky factorisation of the packed lower triangle (row r at r (r + 1) / 2), right-looking: column j is scaled by the root
//      of its pivot and copied into a vector, a TX x TY tile of threads sweeps the trailing triangle.  A pivot that is not positive
//      and finite ends the item: zeros are written and the failure word is raised to the row (plain store, any failing row).
//   3. y = L^-1 b by columns, y += z, u = L^-T y by rows of L; one barrier per column.
// The normals: Philox block (i lo, i hi, s, n; 42, tag) gives components 2 n and 2 n + 1 by Box-Muller on u1 = 1 - canonical53(w3,
// w2), u2 = canonical53(w1, w0) (the uniforms of probit_truncated): a draw depends on (i, s, tag) and the inputs only.
// fp64 throughout.  KP is the context's device num_latent (8 .. 128); components k >= kt (a padded num_latent) are skipped and the
// ring's pad components kt .. kp - 1 are written as zeros.  K <= 32: a single wave per item; above: four.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace bpmf {

constexpr int kFoldinChunk = 8;             // ratings staged per pass over the Gram (K = 128: 8 KiB beside the 64.5 KiB triangle, two workgroups per CU)

struct FoldinArgs {
    const int64_t *rowptr; const int32_t *colidx; const double *vals;   // the new rows by rows: columns of the candidate side, ascending
    const double *cring; int64_t cstride;                               // the candidate side's sample ring, doubles per column
    const double *alpha, *lam, *lmu;                                    // the hyper ring: S | S x kt x kt (row-major, lower triangle read) | S x kt
    double mean_rating;
    int S, kt, kp;
    uint32_t tag; int draw;
    double *out;                                                        // n_new x S x kp
    unsigned long long *fail;                                           // raised to a row whose pivot was not positive and finite
};

__device__ __forceinline__ int foldin_tri(int r) { return r * (r + 1) / 2; }

// row of element e of the packed lower triangle (e < 2^23: the float root is exact enough for the two corrections to finish it)
__device__ __forceinline__ int foldin_row(int e)
{
    int r = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while (foldin_tri(r) > e) --r;
    while (foldin_tri(r + 1) <= e) ++r;
    return r;
}

template <int KP>
__global__ __launch_bounds__(KP <= 32 ? 64 : 256) void k_foldin(const FoldinArgs a)
{
    constexpr int NT = KP <= 32 ? 64 : 256, TX = KP <= 32 ? 8 : 16, TY = NT / TX;
    __shared__ double s_a[KP * (KP + 1) / 2];
    __shared__ double s_v[kFoldinChunk * KP];
    __shared__ double s_r[kFoldinChunk];
    __shared__ double s_b[KP], s_c[KP], s_d[KP];
    const int tid = (int)threadIdx.x, tx = tid % TX, ty = tid / TX;
    const int kt = a.kt, kp = a.kp, S = a.S;
    const int64_t i = (int64_t)blockIdx.x / S;
    const int s = (int)((int64_t)blockIdx.x - i * S);
    const int ne = foldin_tri(kt);

    // 1. sum_j v v^T and sum_j (r - mean) v
    for (int e = tid; e < ne; e += NT) s_a[e] = 0.0;
    for (int k = tid; k < kt; k += NT) s_b[k] = 0.0;
    const int64_t p0 = a.rowptr[i], p1 = a.rowptr[i + 1];
    const double *vs = a.cring + (int64_t)s * kp;
    for (int64_t p = p0; p < p1; p += kFoldinChunk) {
        const int nc = (int)(p1 - p < kFoldinChunk ? p1 - p : kFoldinChunk);
        __syncthreads();                                                // (the readers of the chunk before are done)
        for (int q = tid; q < nc * kp; q += NT) {
            const int c = q / kp, k = q - c * kp;
            s_v[c * KP + k] = vs[(int64_t)a.colidx[p + c] * a.cstride + k];
        }
        if (tid < nc) s_r[tid] = a.vals[p + tid] - a.mean_rating;
        __syncthreads();
        for (int e = tid; e < ne; e += NT) {
            const int r = foldin_row(e), c2 = e - foldin_tri(r);
            double acc = s_a[e];
            for (int c = 0; c < nc; ++c) acc = fma(s_v[c * KP + r], s_v[c * KP + c2], acc);
            s_a[e] = acc;
        }
        for (int k = tid; k < kt; k += NT) {
            double acc = s_b[k];
            for (int c = 0; c < nc; ++c) acc = fma(s_r[c], s_v[c * KP + k], acc);
            s_b[k] = acc;
        }
    }
    {
        const double al = a.alpha[s];
        const double *lam = a.lam + (int64_t)s * kt * kt, *lmu = a.lmu + (int64_t)s * kt;
        for (int e = tid; e < ne; e += NT) {
            const int r = foldin_row(e), c2 = e - foldin_tri(r);
            s_a[e] = fma(al, s_a[e], lam[r * kt + c2]);
        }
        for (int k = tid; k < kt; k += NT) s_b[k] = fma(al, s_b[k], lmu[k]);
    }

    // 2. Lambda* = L L^T in place; the roots of the pivots go to s_d (the diagonal of s_a keeps the pivots)
    bool bad = false;
    for (int j = 0; j < kt; ++j) {
        __syncthreads();
        const double d = s_a[foldin_tri(j) + j];                        // (one word for every thread: the branch is uniform)
        if (!(d > 0.0 && d < __builtin_huge_val())) { bad = true; break; }
        const double root = sqrt(d);
        if (tid == 0) s_d[j] = root;
        for (int r = j + 1 + tid; r < kt; r += NT) {
            const double v = s_a[foldin_tri(r) + j] / root;
            s_a[foldin_tri(r) + j] = v;
            s_c[r] = v;
        }
        __syncthreads();
        for (int r = j + 1 + ty; r < kt; r += TY) {
            const double cr = s_c[r];
            double *row = s_a + foldin_tri(r);
            for (int c = j + 1 + tx; c <= r; c += TX) row[c] = fma(-cr, s_c[c], row[c]);
        }
    }

    if (!bad) {
        // 3. y = L^-1 b into s_c
        for (int j = 0; j < kt; ++j) {
            __syncthreads();
            const double yj = s_b[j] / s_d[j];
            for (int r = j + 1 + tid; r < kt; r += NT) s_b[r] = fma(-s_a[foldin_tri(r) + j], yj, s_b[r]);
            if (tid == 0) s_c[j] = yj;
        }
        __syncthreads();
        if (a.draw && 2 * tid < kt) {
            const uint32_t ilo = (uint32_t)((uint64_t)i & 0xFFFFFFFFull), ihi = (uint32_t)((uint64_t)i >> 32);
            const Philox4 w = philox4x32_10(ilo, ihi, (uint32_t)s, (uint32_t)tid, 42u, a.tag);
            const double u1 = 1.0 - canonical53(w.w[3], w.w[2]);
            const double u2 = canonical53(w.w[1], w.w[0]);
            const double rho = sqrt(-2.0 * log(u1));
            s_c[2 * tid] += rho * cospi(2.0 * u2);
            if (2 * tid + 1 < kt) s_c[2 * tid + 1] += rho * sinpi(2.0 * u2);
        }
        // u = L^-T y into s_b
        for (int j = kt - 1; j >= 0; --j) {
            __syncthreads();
            const double xj = s_c[j] / s_d[j];
            const double *row = s_a + foldin_tri(j);
            for (int c = tid; c < j; c += NT) s_c[c] = fma(-row[c], xj, s_c[c]);
            if (tid == 0) s_b[j] = xj;
        }
        __syncthreads();
    } else if (tid == 0) {
        *a.fail = (unsigned long long)i;                                // (plain store: any of the failing rows)
    }
    double *out = a.out + ((int64_t)i * S + s) * kp;
    for (int k = tid; k < kp; k += NT) out[k] = (bad || k >= kt) ? 0.0 : s_b[k];
}

}  // namespace bpmf
