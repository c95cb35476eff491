// kernels_bias.h -- row and column bias terms (bpmf_hip_side_set_bias, capi_bias.hip; one translation unit: kbias.hip).
// DESIGN.md section 28 has the model: r_ij ~ N(mean + b_i + c_j + u_i . v_j, 1 / alpha), b_a ~ N(0, 1 / lambda).
//
// The bias step of one half-iteration of side A (columns a, ratings p, the other side's biases c) is four launches in one queue:
//   k_bias_resid<K>     e_p = ((r_p - mean) - c[row p]) - x_col(p) . y_row(p) for every rating of the side.  The shape of k_robust_weights
//                       (kernels_robust.h): tiles of kProbitTile consecutive ratings, one tile per workgroup (work balanced over ratings,
//                       not columns), the columns from sse_column, the dot products from probit_tile_dots.  An e_p that is not finite
//                       raises the side's fail word to p.
//   k_bias_piece_sums   every column of more than kBiasLight = 16 ratings is cut into pieces of kBiasPiece consecutive ratings (the last one
//                       ragged); one wave per piece.  (A lighter column has no piece: a wave per column of two ratings is what the users'
//                       side of a ChEMBL-shaped matrix would otherwise spend.)
//                       The order inside a piece: lane l adds e[64 j + l], j = 0 .. 3, in ascending j to 0.0; the 64 lane sums meet in
//                       the butterfly xor 32, 16, 8, 4, 2, 1.  The piece partial is parked in part[piece].  A column of thousands of
//                       ratings is spread over as many waves as it has pieces.
//   k_bias_draw         one thread per column: S_a = the column's piece partials added to 0.0 in piece order -- or, for a column of at most
//                       kBiasLight ratings, its residuals added to 0.0 in rating order;
//                           prec = lambda + alpha n_a,   b_a = (alpha S_a) / prec + xi_a / sqrt(prec)
//                       xi_a = sqrt(-2 ln u1) cospi(2 u2) from the Philox block (a lo, a hi, iter, 0; 42, tag), u1 = 1 - canonical53(w3, w2),
//                       u2 = canonical53(w1, w0): the normal of robust_gamma (kernels_robust.h).  A column without ratings has no piece:
//                       S = 0, prec = lambda, a draw from the prior.  lambda is read from a device word.
//   k_bias_values       z_p = (r_p - b[col p]) - c[row p] for every rating, one rating per thread: coalesced 8-byte stores.  The
//                       unchanged column samplers read z in place of the ratings, with the side's own mean rating.
// fp64 throughout, nothing is fused (`fp contract(off)`: tests/bias_ref.py restates the step in numpy, where no product meets a sum in
// one rounding).  No floating-point atomics: every sum has the fixed order above, whatever the grid.
//
//   k_bias_accumulate   bsum[a] += b[a] (the posterior mean of the biases)
//   k_predict_bias<K, NT>   k_predict (kernels.h) with pred = ((x . y + mean) + b[col]) + c[row]; the fused twin copy gets the same two
//                       additions behind its own mean.  fp64 factors only.  Same block partials, ticket and publishing as k_predict.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"            // TwinArgs (args.h), BPMF_RLX_AGENT / BPMF_RLX_SYSTEM
#include "kernels_gather.h"     // kProbitTile, sse_column, probit_tile_dots
#include "kernels_robust.h"     // robust_gamma
#include "philox.h"

namespace bpmf {

constexpr int kBiasPiece = 256;             // consecutive ratings of a column per piece: four per lane of a wave
constexpr int kBiasLight = 16;              // a column of at most this many ratings has no piece: its thread of k_bias_draw adds them itself

template <int K>
__global__ __launch_bounds__(kProbitTile) void k_bias_resid(const int64_t *__restrict__ colptr, int64_t ncols,
                                                            const int32_t *__restrict__ rowidx, const double *__restrict__ vals,
                                                            int64_t nnz, const double *__restrict__ items, const double *__restrict__ other,
                                                            int kt, double mean, const double *__restrict__ cbias,
                                                            double *__restrict__ e, unsigned long long *__restrict__ fail)
{
#pragma clang fp contract(off)
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
    probit_tile_dots<K, double>(s_col, s_row, n, items, other, kt, s_m);
    __syncthreads();
    if ((int)threadIdx.x < n) {
        const double d = vals[p] - mean;
        const double t = d - cbias[s_row[threadIdx.x]];
        const double r = t - s_m[threadIdx.x];
        e[p] = r;
        if (!(__builtin_fabs(r) < __builtin_huge_val())) *fail = (unsigned long long)p;      // (plain store: any of the failing ratings)
    }
}

// pieceptr[a]: the first piece of column a (ncols + 1 entries; pieceptr[ncols] = npieces).  Four waves per workgroup, one piece each.
static __global__ __launch_bounds__(256) void k_bias_piece_sums(const int64_t *__restrict__ colptr, const int64_t *__restrict__ pieceptr,
                                                                int64_t ncols, int64_t npieces, const double *__restrict__ e,
                                                                double *__restrict__ part)
{
#pragma clang fp contract(off)
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= npieces) return;                                          // (uniform over the wave)
    const int64_t a = sse_column(pieceptr, 0, ncols, g);               // columns without a piece are stepped over
    const int64_t p0 = colptr[a] + (g - pieceptr[a]) * kBiasPiece;
    const int64_t left = colptr[a + 1] - p0;
    const int n = (int)(left < kBiasPiece ? left : kBiasPiece);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kBiasPiece / 64; ++j) {
        const int i = 64 * j + lane;
        if (i < n) s = s + e[p0 + i];
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s = s + __shfl_xor(s, sh);
    if (lane == 0) part[g] = s;
}

static __global__ __launch_bounds__(256) void k_bias_draw(const int64_t *__restrict__ colptr, const int64_t *__restrict__ pieceptr,
                                                          int64_t ncols, const double *__restrict__ e, const double *__restrict__ part,
                                                          const double *__restrict__ lambda_word, double alpha, uint32_t iter, uint32_t tag,
                                                          double *__restrict__ b)
{
#pragma clang fp contract(off)
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= ncols) return;
    const int64_t p0 = colptr[a], p1 = colptr[a + 1];
    double S = 0.0;
    if (p1 - p0 <= kBiasLight) {                                       // light: the residuals themselves, in rating order
        for (int64_t p = p0; p < p1; ++p) S = S + e[p];
    } else {                                                           // the parked piece partials, in piece order
        for (int64_t g = pieceptr[a]; g < pieceptr[a + 1]; ++g) S = S + part[g];
    }
    const double na = (double)(p1 - p0);
    const double prec = *lambda_word + alpha * na;
    const Philox4 w = philox4x32_10((uint32_t)((uint64_t)a & 0xFFFFFFFFull), (uint32_t)((uint64_t)a >> 32), iter, 0u, 42u, tag);
    const double u1 = 1.0 - canonical53(w.w[3], w.w[2]);
    const double u2 = canonical53(w.w[1], w.w[0]);
    const double xi = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
    b[a] = (alpha * S) / prec + xi / sqrt(prec);
}

static __global__ __launch_bounds__(256) void k_bias_values(const int64_t *__restrict__ colptr, int64_t ncols, const int32_t *__restrict__ rowidx,
                                                            const double *__restrict__ vals, int64_t nnz, const double *__restrict__ b,
                                                            const double *__restrict__ cbias, double *__restrict__ z)
{
#pragma clang fp contract(off)
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    const int64_t p = p0 + threadIdx.x;
    if (p >= nnz) return;
    const int64_t c0 = sse_column(colptr, 0, ncols, p0);
    const int64_t a = sse_column(colptr, c0, ncols, p);
    const double t = vals[p] - b[a];
    z[p] = t - cbias[rowidx[p]];
}

constexpr unsigned long long kBiasLambdaFailed = ~0ull - 1ull;      // the value the fail word takes when the draw of lambda fails

// The draw of a side's bias precision (only with a prior, bpmf_hip_side_bias_prior): lambda ~ Gamma(a0 + N / 2, rate b0 + sum_a b_a^2 / 2).
// One workgroup.  The sum of squares in chunks of 256 columns: thread t squares b[chunk 256 + t], the 256 squares meet in the LDS tree
// of strides 128 .. 1, thread 0 adds the chunk sums to 0.0 in chunk order.  g ~ Gamma(a, 1) from robust_gamma (kernels_robust.h:
// Marsaglia-Tsang, a >= 1) on the Philox blocks (~0, ~0, iter, attempt; 42, tag) -- no column has the index 2^64 - 1, so no block is
// shared with a bias draw of the same iteration and tag.  dd = a - 1 / 3 and c = 1 / sqrt(9 dd) come from the host.  lambda = g / rate goes
// to the side's lambda word and to trace[iter] (iter < cap).  The attempt cap, or a rate that is not finite and > 0: the word keeps its
// value and the fail word is raised.
static __global__ __launch_bounds__(256) void k_bias_lambda(const double *__restrict__ b, int64_t ncols, double dd, double c, double b0,
                                                            uint32_t iter, uint32_t tag, double *__restrict__ lambda_word,
                                                            double *__restrict__ trace, int cap, unsigned long long *__restrict__ fail)
{
#pragma clang fp contract(off)
    __shared__ double s[256];
    double total = 0.0;
    for (int64_t c0 = 0; c0 < ncols; c0 += 256) {
        const int64_t a = c0 + threadIdx.x;
        const double v = a < ncols ? b[a] : 0.0;
        s[threadIdx.x] = v * v;
        __syncthreads();
        for (int st = 128; st >= 1; st >>= 1) {
            if ((int)threadIdx.x < st) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) total = total + s[0];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double rate = b0 + 0.5 * total;
    const double g = robust_gamma((int64_t)-1, iter, tag, dd, c);
    double lam = *lambda_word;
    if (g > 0.0 && rate > 0.0 && rate < __builtin_huge_val()) lam = g / rate;
    else *fail = kBiasLambdaFailed;
    *lambda_word = lam;
    if ((int)iter < cap) trace[iter] = lam;
}

// Two extra rows behind the Kt factor rows of ring slot `slot` of every column: role 0 writes (b_a, 1), role 1 writes (1, b_a), so that
// the ring dot product of a query column and a candidate column of opposite roles is u . v + b + c (rows Kt + 2 .. Kp - 1 stay zero).
static __global__ __launch_bounds__(256) void k_samples_add_bias(const double *__restrict__ b, int64_t ncols, int role, int Kt,
                                                                 double *__restrict__ ring, int64_t stride, int Kp, int slot)
{
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= ncols) return;
    double *col = ring + (size_t)a * (size_t)stride + (size_t)slot * (size_t)Kp + (size_t)Kt;
    col[role] = b[a];
    col[1 - role] = 1.0;
}

static __global__ __launch_bounds__(256) void k_bias_accumulate(const double *__restrict__ b, int64_t ncols, double *__restrict__ bsum)
{
#pragma clang fp contract(off)
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a < ncols) bsum[a] = bsum[a] + b[a];
}

template <int K, int NT>
__global__ __launch_bounds__(NT) void k_predict_bias(const int32_t *__restrict__ tcol, const int32_t *__restrict__ trow,
                                                      const double *__restrict__ tval, int64_t nnz,
                                                      const double *__restrict__ items, const double *__restrict__ other,
                                                      const double *__restrict__ bcol, const double *__restrict__ brow,
                                                      double mean, int n, double *__restrict__ pavg,
                                                      double *__restrict__ pm2, double *partial, double *__restrict__ out,
                                                      unsigned *ticket, unsigned *flag, unsigned seq, TwinArgs tw)
{
    // (compiled like k_predict, products and sums contracted where it contracts them: with b = c = 0 the bytes are k_predict's)
    __shared__ double red[4][NT / 64];
    __shared__ double fin[4][NT];
    __shared__ unsigned last;
    auto wsum = [](const double (&r)[NT / 64]) { if constexpr (NT == 256) return (r[0] + r[1]) + (r[2] + r[3]); else return r[0]; };
    const int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x;
    double se = 0.0, se_avg = 0.0, se_t = 0.0, se_avg_t = 0.0;
    if (q < nnz) {
        double d0 = 0.0, d1 = 0.0;
        const int32_t tc = tcol[q], tr = trow[q];
        const double2 *m = reinterpret_cast<const double2 *>(items + (size_t)tc * K);
        const double2 *u = reinterpret_cast<const double2 *>(other + (size_t)tr * K);
#pragma unroll
        for (int t = 0; t < K / 2; ++t) {
            const double2 a = m[t], b = u[t];
            d0 = fma(a.x, b.x, d0);
            d1 = fma(a.y, b.y, d1);
        }
        const double bc = bcol[tc], br = brow[tr];
        const double pred = (((d0 + d1) + mean) + bc) + br;
        const double v = tval[q];
        se = (v - pred) * (v - pred);
        double avg = pavg[q];
        const double delta = pred - avg;
        avg = (n == 0) ? pred : (avg + delta / n);
        pavg[q] = avg;
        pm2[q] = (n == 0) ? 0.0 : pm2[q] + delta * (pred - avg);
        se_avg = (v - avg) * (v - avg);
        if (tw.perm) {
            const int qt = tw.perm[q];
            const double pred_t = (((d0 + d1) + tw.mean) + bc) + br;
            se_t = (v - pred_t) * (v - pred_t);
            double avg_t = tw.pavg[qt];
            const double delta_t = pred_t - avg_t;
            avg_t = (n == 0) ? pred_t : (avg_t + delta_t / n);
            tw.pavg[qt] = avg_t;
            tw.pm2[qt] = (n == 0) ? 0.0 : tw.pm2[qt] + delta_t * (pred_t - avg_t);
            se_avg_t = (v - avg_t) * (v - avg_t);
        }
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        se += __shfl_xor(se, sh);
        se_avg += __shfl_xor(se_avg, sh);
        se_t += __shfl_xor(se_t, sh);
        se_avg_t += __shfl_xor(se_avg_t, sh);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wv] = se; red[1][wv] = se_avg; red[2][wv] = se_t; red[3][wv] = se_avg_t; }
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(&partial[2 * blockIdx.x], wsum(red[0]), BPMF_RLX_AGENT);
        __hip_atomic_store(&partial[2 * blockIdx.x + 1], wsum(red[1]), BPMF_RLX_AGENT);
        if (tw.perm) {
            __hip_atomic_store(&tw.partial[2 * blockIdx.x], wsum(red[2]), BPMF_RLX_AGENT);
            __hip_atomic_store(&tw.partial[2 * blockIdx.x + 1], wsum(red[3]), BPMF_RLX_AGENT);
        }
        // the last block to arrive adds the block partials up (fixed-shape tree) and publishes the sums, as in k_predict
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, BPMF_RLX_AGENT);
        last = (t == gridDim.x - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    const int64_t nblocks = gridDim.x;
    double a = 0.0, b = 0.0, at = 0.0, bt = 0.0;
    for (int64_t w = threadIdx.x; w < nblocks; w += NT) {
        a += __hip_atomic_load(&partial[2 * w], BPMF_RLX_AGENT);
        b += __hip_atomic_load(&partial[2 * w + 1], BPMF_RLX_AGENT);
        if (tw.perm) {
            at += __hip_atomic_load(&tw.partial[2 * w], BPMF_RLX_AGENT);
            bt += __hip_atomic_load(&tw.partial[2 * w + 1], BPMF_RLX_AGENT);
        }
    }
    fin[0][threadIdx.x] = a; fin[1][threadIdx.x] = b; fin[2][threadIdx.x] = at; fin[3][threadIdx.x] = bt;
    __syncthreads();
    for (int st = NT / 2; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) {
#pragma unroll
            for (int c = 0; c < 4; ++c) fin[c][threadIdx.x] += fin[c][threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&out[0], fin[0][0], BPMF_RLX_SYSTEM);
        __hip_atomic_store(&out[1], fin[1][0], BPMF_RLX_SYSTEM);
        if (tw.perm) {
            __hip_atomic_store(&tw.out[0], fin[2][0], BPMF_RLX_SYSTEM);
            __hip_atomic_store(&tw.out[1], fin[3][0], BPMF_RLX_SYSTEM);
        }
        __hip_atomic_store(ticket, 0u, BPMF_RLX_AGENT);              // re-arm
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(flag, seq, BPMF_RLX_SYSTEM);
        if (tw.perm) __hip_atomic_store(tw.flag, tw.seq, BPMF_RLX_SYSTEM);
    }
}

}  // namespace bpmf
