// kernels.h -- hand-written HIP kernels for gfx950 (CDNA4, wave64) behind the C ABI.
//
// The path (c++/sample.cpp:248-336 + c++/mvnormal.cpp:18-47 of the reference),
// re-designed for MI355X:
//
//   k_sample1<K>     (K <= 32, the default) one single-wave workgroup per work item = column or
//                    chunk of a heavy column, cost-sorted, balanced by the hardware dispatcher.
//                    gram_chunk44: the K-vectors of the rated rows are gathered straight into the
//                    operand layout of v_mfma_f64_4x4x4_4b_f64 (16 ratings per instruction, one
//                    accumulator register per upper 4x4 block of sum_j u_j u_j^T), one group of 16
//                    ratings ahead of the MFMAs; sum_j w_j u_j rides along on the VALU.  Chunks of a
//                    heavy column park their accumulators (write-through stores); the wave drawing
//                    the last ticket sums them in chunk order and finishes the column.
//   finish_single<K> Lambda* = LambdaF + alpha*G through LDS into registers (S lanes per row),
//                    right-looking Cholesky two columns per step with the pivot block through
//                    v_readlane and the scaled columns broadcast through LDS, fused forward
//                    solve, Philox/polar normal draw, backward solve, coalesced 8*K-byte store.
//   deposit_column / finish_slots: C = 64/K columns factorised side by side by one wave, Gram on
//                    v_mfma_f64_16x16x4_f64 tiles (gram_chunk): the BPMF_REDUCE formulation (kernels_reduce.h).
//   k_colstats<K>    sum x, sum x x^T of the fresh columns (again an MFMA Gram); the last waves to
//                    arrive add the partials in a fixed order (run-to-run identical) and publish.
//   k_predict<K>     test-set dot products, running mean / M2, squared errors; last block publishes.
//   k_gate_stage     polls the host's gate word, then stages the parameter blob (asynchronous path).
// (kernels_q4.h: k_sample4, four columns per wave for sides of >= 20 000 columns; kernels_slab.h: K = 64;
//  kernels_lr.h: K = 64 product form for columns with <= 16 ratings; kernels_wg2.h: K = 128, fp64 and fp32.)
//
// Everything is fp64 like the reference (c++/bpmf.h:55-58).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"
#include "args.h"

namespace bpmf {

typedef double d4 __attribute__((ext_vector_type(4)));

// v_mfma_f64_16x16x4_f64 operand / result layout (lane l, kq = l>>4, li = l&15):
//   A[i=li][k=kq], B[k=kq][j=li]  one double each;  D[i = kq + 4*reg][j = li], reg 0..3.
__device__ __forceinline__ d4 mfma16(double a, double b, d4 c)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// v_mfma_f64_4x4x4_4b_f64: four independent 4x4x4 products per instruction.  Lane l = 16 k + 4 b + x:
//   A[b][i=x][k], B[b][k][j=x] one double each;  D[b][i][j] sits in lane 16 i + 4 b + j.
// (Found by brute force on gfx950: tools/probes/layout44_probe.hip.)  On MI355X it sustains
// ~18 cycles per instruction and SIMD (28 flop/cycle) against ~105 cycles for the 16x16x4 shape
// (19.5 flop/cycle) -- tools/probes/mfma44_probe.hip -- and its 4x4 granularity wastes nothing on
// the diagonal of a symmetric Gram.
__device__ __forceinline__ double mfma44(double a, double b, double c)
{
    return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------
// The Gram of four K-vectors on the 4x4x4 shape with ROTATED-BLOCK accumulators (K = 64): shared by the sampler's
// gram_slab (kernels_slab.h, which documents the scheme) and the column statistics (colstats_accumulate below).
// Operand register t holds x_k[16 t + c] in lane (k, c), c = 4 b + j -- the operand layout of the 16x16x4 shape too.
// ---------------------------------------------------------------------------
template <int K>
struct Rot44 {
    static constexpr int NT = K / 16;
    // tile (TI, TJ), TI <= TJ, keeps one accumulator per quad rotation d of the B operand -- d = 0 .. 3 off the
    // diagonal, d = 0 .. 2 on it (the blocks d = 3 would give are transposes of d = 1's)
    __host__ __device__ static constexpr int nrot(int TI, int TJ) { return TI == TJ ? 3 : 4; }
    __host__ __device__ static constexpr int aoff(int TI, int TJ)
    {
        int n = 0;
        for (int a = 0; a < NT; ++a)
            for (int b = a; b < NT; ++b) {
                if (a == TI && b == TJ) return n;
                n += nrot(a, b);
            }
        return n;
    }
    static constexpr int NACC = aoff(NT - 1, NT - 1) + 3;  // 36 at K = 64
};

// x rotated by 4 * D lanes inside each row of 16 lanes (quad b reads quad (b + D) % 4): one DPP move per half, no LDS
template <int D>
__device__ __forceinline__ double quad_rot(double x)
{
    constexpr int CTRL = 0x120 + (16 - 4 * D);                       // row_ror:(16 - 4 D): lane l reads lane (l + 4 D) % 16 of its row
    const long long v = __builtin_bit_cast(long long, x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// C += the Gram of the four vectors in yy.  A = register TI as it is (block b = rows 16 TI + 4 b ..), B = register TJ rotated by
// d quads (block b = columns 16 TJ + 4 ((b + d) % 4) ..): one instruction accumulates the blocks (4 TI + b, 4 TJ + (b + d) % 4).
// Rotations by one and by two quads of every register are what the diagonal tiles need; the off-diagonal tiles' d = 3 takes the
// A operand rotated by ONE quad against the natural B operand instead -- block b of that product is (4 TI + (b + 1) % 4, 4 TJ + b),
// the same four blocks {(r, r + 3)} in other slots (rot44_images knows) -- so that no rotation by three is made: 8 rotated
// registers (16 DPP moves) and NT (NT + 1) / 2 * 4 - NT MFMAs per call
template <int K>
__device__ __forceinline__ void rot44_contract(const double (&yy)[K / 16], double (&C)[Rot44<K>::NACC])
{
    using G = Rot44<K>;
    constexpr int NT = K / 16;
    double rot[NT][3];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        rot[t][0] = yy[t];
        rot[t][1] = quad_rot<1>(yy[t]);
        rot[t][2] = quad_rot<2>(yy[t]);
    }
#pragma unroll
    for (int TI = 0; TI < NT; ++TI)
#pragma unroll
        for (int TJ = TI; TJ < NT; ++TJ)
#pragma unroll
            for (int d = 0; d < G::nrot(TI, TJ); ++d) {
                if (d < 3) C[G::aoff(TI, TJ) + d] = mfma44(yy[TI], rot[TJ][d], C[G::aoff(TI, TJ) + d]);
                else C[G::aoff(TI, TJ) + d] = mfma44(rot[TI][1], yy[TJ], C[G::aoff(TI, TJ) + d]);
            }
}

// The accumulators of rot44_contract() -> 16 x 16 tiles in the accumulator layout of the 16x16x4 shape (register m of tile
// (TI, TJ), lane (i, c) = element [16 TI + 4 m + i][16 TJ + c]), handed to sink(tile index, TI, TJ, m, value).  The map is a
// permutation, so it commutes with sums of accumulators.  Tile by tile through two 2 KB LDS images taken in turn: lane
// (i, b, j) of rotation d holds G[16 TI + 4 b + i][16 TJ + 4 ((b + d) % 4) + j] and stores it at [4 b + i][4 ((b + d) % 4) + j]
// of the image.  A diagonal tile stores every element at its mirror position too, so that the image is the full symmetric
// tile (an element written twice is written with the same bits: same products, same order).  The images belong to ONE wave
// (LDS operations of a wave complete in order); the barriers pin the compiler's order and every wave of the workgroup has to
// come through here.
template <int K, typename Sink>
__device__ __forceinline__ void rot44_images(const double (&C)[Rot44<K>::NACC], double *buf0, double *buf1, int lane, Sink &&sink)
{
    using G = Rot44<K>;
    constexpr int NT = G::NT;
    const int i = lane >> 4, b = (lane >> 2) & 3, j = lane & 3;
    int tix = 0;
#pragma unroll
    for (int TI = 0; TI < NT; ++TI)
#pragma unroll
        for (int TJ = TI; TJ < NT; ++TJ, ++tix) {
            double *img = (tix & 1) ? buf1 : buf0;
#pragma unroll
            for (int d = 0; d < G::nrot(TI, TJ); ++d) {
                // (d = 3, off the diagonal only: made with the A operand rotated by one quad -- slot b is block ((b + 1) % 4, b))
                const int row = d < 3 ? 4 * b + i : 4 * ((b + 1) & 3) + i, col = d < 3 ? 4 * ((b + d) & 3) + j : 4 * b + j;
                const double v = C[G::aoff(TI, TJ) + d];
                img[row * 16 + col] = v;
                if (TI == TJ && d > 0) img[col * 16 + row] = v;
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 4; ++m) sink(tix, TI, TJ, m, img[(4 * m + i) * 16 + (lane & 15)]);
            __syncthreads();
        }
}

// 1/sqrt(d) to ~1 ulp: v_rsq_f64 (2^-23 relative) + one third-order (Halley) correction,
// y = y0 (1 + e/2 + 3e^2/8) with e = 1 - d y0^2, error ~ e^3: 6 dependent instructions
// instead of the ~25 of sqrt followed by a divide.  d <= 0 or NaN gives NaN/inf, which
// propagates into the sample and flags the column as "Cholesky failed".
__device__ __forceinline__ double rsqrt_nr(double d)
{
    const double y0 = __builtin_amdgcn_rsq(d);
    const double e = fma(-d, y0 * y0, 1.0);
    const double q = e * fma(0.375, e, 0.5);
    return fma(y0, q, y0);
}

// value of `v` in lane `base + off` of the wave, base per lane (LDS crossbar, no VALU work
// beyond the two moves): used for broadcasts inside one K-lane group of the factorisation
__device__ __forceinline__ double gbcast(double v, int base_bytes, int off)
{
    const int lo = __builtin_amdgcn_ds_bpermute(base_bytes + 4 * off, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(base_bytes + 4 * off, __double2hiint(v));
    return __hiloint2double(hi, lo);
}

// value of `v` in lane `src` (wave-uniform src) through v_readlane_b32: no LDS traffic
__device__ __forceinline__ double bcast(double v, int src)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}


// ---------------------------------------------------------------------------
// K normals of the reference's per-column stream, in stream order.
// The reference draws them one after another with the polar method; every
// attempt eats exactly one Philox block, so attempt n <-> block n, and the
// j-th normal is the j-th ACCEPTED attempt.  64 lanes try blocks base..base+63
// at once, a ballot ranks the accepted ones.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double polar_r2(double x, double y)
{
#pragma clang fp contract(off)
    return x * x + y * y;      // two roundings + add, as the un-fused x86 reference build evaluates it
}

// stream id of a column: (idx+1)*K*(iter+1) truncated to 32 bits (c++/sample.cpp:266, c++/bpmf.h:67).  K is the
// reference's num_latent -- the caller's (`ktrue` of the argument blocks), not the K the kernel is instantiated for:
// a num_latent between two instantiated sizes runs on the next one with zero factor rows / identity precision in the
// extra dimensions, and takes its stream id and its number of normals from the true K (c++/sample.cpp:266,322)
__device__ __forceinline__ uint32_t sample_counter(int64_t idx, int ktrue, uint32_t iter_plus_1)
{
    return (uint32_t)((uint64_t)(idx + 1) * (uint64_t)ktrue * (uint64_t)iter_plus_1);
}

// The hyper-parameters of this half-iteration may still be on their way (the host's Normal-Wishart
// draw -> pinned memory -> k_gate_stage -> device memory) when the launch starts: a workgroup only
// needs them after its Gram, so it waits HERE, not the launch at the queue (a cross-queue barrier
// packet ahead of the dispatch costs ~5 us of command-processor time per launch even when it has
// long been satisfied: tools/probes/boundary2.hip).  k_gate_stage writes the blob through to
// memory (device-scope relaxed atomic stores + s_waitcnt) before it sets the word; nothing in this
// launch has touched the blob before it sees the word, and the caches were invalidated when the
// launch began, so plain loads behind the wait read the new values.  Bounded: the gate workgroup
// itself gives up on the host after `wait_ticks` (and then still sets the word), so a workgroup here
// only runs into ITS limit (1.5 x that) when the gate workgroup never ran; either way the side's
// sticky time-out word is set and the host reports BPMF_HIP_ENODEV instead of using the results.
#define BPMF_RLX_SYSTEM_ __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM
enum { BPMF_TMO_GATE = 1, BPMF_TMO_PARAMS = 2, BPMF_TMO_STATS = 3 };
__device__ __forceinline__ void flag_timeout(unsigned long long *tmo, unsigned long long what)
{
    if (tmo) __hip_atomic_store(tmo, what, BPMF_RLX_SYSTEM_);
}

__device__ __forceinline__ void wait_params(const SampleArgs &a)
{
    if (a.gate_flag == nullptr) return;
    const unsigned long long t0 = wall_clock64();
    const unsigned long long limit = a.wait_ticks + (a.wait_ticks >> 1);
    while ((unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(a.gate_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != a.gate_want) {
        __builtin_amdgcn_s_sleep(8);
        if (wall_clock64() - t0 > limit) {
            if (threadIdx.x == 0) flag_timeout(a.tmo, BPMF_TMO_PARAMS);
            break;
        }
    }
    asm volatile("" ::: "memory");
}

// Profiling hooks -- phase ablation (BPMF_HIP_ABLATE), gathers confined to 64 hot rows, phase time stamps (BPMF_HIP_STAMPS) --
// exist only in the PROFILING build of the library (`make prof` -> libbpmf_hip_prof.so, -DBPMF_PROFILING=1; tools/ select it
// with BPMF_HIP_LIBRARY).  In the product build kProfiling is false: ablate_bits() is the constant 0, stamp() is empty, the
// row mask of the gathers is the constant -1, and the compiler removes every branch and the v_and they would cost in the hot
// loops (VERDICT r5 "weak" 9: the instruction count of these kernels is their stated bound).
#ifndef BPMF_PROFILING
#define BPMF_PROFILING 0
#endif
constexpr bool kProfiling = BPMF_PROFILING != 0;
__device__ __forceinline__ uint32_t ablate_bits(const SampleArgs &a)
{
    if constexpr (kProfiling) return a.ablate;
    else return 0u;
}

// profiling (BPMF_HIP_STAMPS=1): work items 0 and nwork / 2 of a launch record the wall clock at phase boundaries
__device__ __forceinline__ void stamp(const SampleArgs &a, int w, int slot)
{
    if constexpr (!kProfiling) {
        // What is left of a stamp in the product build: a fence for the instruction SCHEDULER only (no instruction).  The
        // stamps' stores cut the kernels into scheduling regions at the phase boundaries; without them the compiler moved
        // code across the phases of k_sample_wg2<128, 4, double> and the launches took 3.5 % longer (round 6, interleaved:
        // 1.267 ms per iteration with the run-time stamps, 1.317 without, 1.271 with this fence: gpurun_out/r6_k128_fence.log).
        __builtin_amdgcn_sched_barrier(0);
        return;
    }
    if (a.stamps == nullptr || threadIdx.x != 0) return;
    const int probe = (w == 0) ? 0 : ((w == a.nwork / 2) ? 1 : -1);
    if (probe >= 0 && slot < 64) a.stamps[probe * 64 + slot] = wall_clock64();
}

// number of set bits of `m` below this lane (v_mbcnt_lo / v_mbcnt_hi: two instructions)
__device__ __forceinline__ int rank_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// pad_to > n: out_lds[n .. pad_to) = 0 (the extra dimensions of a padded num_latent draw nothing: x stays 0 there)
template <int NMAX>
__device__ __forceinline__ void draw_normals(uint32_t counter, int n, double *out_lds, int lane, int pad_to = 0)
{
    for (int i = n + lane; i < pad_to; i += 64) out_lds[i] = 0.0;
    int produced = 0;
    uint32_t base = 0;
    while (produced < n) {                                         // wave-uniform
        const Philox4 b = stream_block(counter, base + (uint32_t)lane);
        const double x = 2.0 * canonical53(b.w[3], b.w[2]) - 1.0;   // URNG order: w3, w2, w1, w0
        const double y = 2.0 * canonical53(b.w[1], b.w[0]) - 1.0;
        const double r2 = polar_r2(x, y);
        const bool acc = !(r2 > 1.0 || r2 == 0.0);
        const unsigned long long m = __ballot(acc);
        const int rank = produced + rank_below(m);
        if (acc && rank < n) {
            out_lds[rank] = y * polar_mult(r2);                        // sqrt(-2 log(r2) / r2), philox.h
        }
        produced += __popcll(m);
        base += 64u;
    }
}

// The same stream when more than one round of 64 attempts is certain (n = 64 needs ~82): the rounds
// only park (y, r2) of the accepted attempts by rank; log / sqrt / divide -- a third of a round --
// run once at the end, one lane per normal.  Same expression on the same inputs: bit-identical.
template <int NMAX>
__device__ __forceinline__ void draw_normals_deferred(uint32_t counter, int n, double *out_lds, double *r2_lds, int lane, int pad_to = 0)
{
    for (int i = n + lane; i < pad_to; i += 64) out_lds[i] = 0.0;
    int produced = 0;
    uint32_t base = 0;
    while (produced < n) {                                         // wave-uniform
        const Philox4 b = stream_block(counter, base + (uint32_t)lane);
        const double x = 2.0 * canonical53(b.w[3], b.w[2]) - 1.0;   // URNG order: w3, w2, w1, w0
        const double y = 2.0 * canonical53(b.w[1], b.w[0]) - 1.0;
        const double r2 = polar_r2(x, y);
        const bool acc = !(r2 > 1.0 || r2 == 0.0);
        const unsigned long long m = __ballot(acc);
        const int rank = produced + rank_below(m);
        if (acc && rank < n) { out_lds[rank] = y; r2_lds[rank] = r2; }
        produced += __popcll(m);
        base += 64u;
    }
    for (int i = lane; i < n; i += 64) {
        const double r2 = r2_lds[i];
        out_lds[i] = out_lds[i] * polar_mult(r2);
    }
}

// The same streams for TWO columns at once.  n = 64 normals need ~82 attempts: a second round of 64 attempts uses a
// fifth of its lanes.  Here every column gets its first 64 attempts in a round of its own and the later rounds are
// SHARED: lanes 0..31 try the next 32 blocks of column A, lanes 32..63 the next 32 of column B (96 attempts are enough in
// 99.8 % of the cases: three Philox rounds per pair instead of four).  Attempt n is still block n of its column's stream
// and the j-th normal its j-th accepted attempt, so every normal is the one draw_normals_deferred produces.
template <int NMAX>
__device__ __forceinline__ void draw_normals_pair(uint32_t counterA, uint32_t counterB, int n, double *outA, double *outB,
                                                  double *r2A, double *r2B, int lane, int pad_to = 0)
{
    for (int i = n + lane; i < pad_to; i += 64) { outA[i] = 0.0; outB[i] = 0.0; }
    auto attempt = [&](uint32_t counter, uint32_t block, double &y, double &r2) -> bool {
        const Philox4 b = stream_block(counter, block);
        const double x = 2.0 * canonical53(b.w[3], b.w[2]) - 1.0;   // URNG order: w3, w2, w1, w0
        y = 2.0 * canonical53(b.w[1], b.w[0]) - 1.0;
        r2 = polar_r2(x, y);
        return !(r2 > 1.0 || r2 == 0.0);
    };
    int prodA, prodB;
    {   // first 64 attempts of A, then of B
        double y, r2;
        bool acc = attempt(counterA, (uint32_t)lane, y, r2);
        unsigned long long m = __ballot(acc);
        int rank = rank_below(m);
        if (acc && rank < n) { outA[rank] = y; r2A[rank] = r2; }
        prodA = __popcll(m);
        acc = attempt(counterB, (uint32_t)lane, y, r2);
        m = __ballot(acc);
        rank = rank_below(m);
        if (acc && rank < n) { outB[rank] = y; r2B[rank] = r2; }
        prodB = __popcll(m);
    }
    const bool hi = lane >= 32;
    const int l32 = lane & 31;
    uint32_t base = 64u;                                              // next unused block (the same for both columns)
    while (prodA < n || prodB < n) {                                  // wave-uniform
        double y, r2;
        const bool acc = attempt(hi ? counterB : counterA, base + (uint32_t)l32, y, r2);
        const unsigned long long m = __ballot(acc);
        const unsigned mA = (unsigned)m, mB = (unsigned)(m >> 32);
        const int rank = hi ? prodB + (int)__builtin_amdgcn_mbcnt_hi(mB, 0u) : prodA + (int)__builtin_amdgcn_mbcnt_lo(mA, 0u);   // accepted attempts of the same column below this lane
        if (acc && rank < n) { (hi ? outB : outA)[rank] = y; (hi ? r2B : r2A)[rank] = r2; }
        prodA += __popc(mA); prodB += __popc(mB);                     // (a column that is complete just drops its extra attempts)
        base += 32u;
    }
    for (int i = lane; i < n; i += 64) {
        const double ra = r2A[i], rb = r2B[i];
        outA[i] = outA[i] * polar_mult(ra);
        outB[i] = outB[i] * polar_mult(rb);
    }
}

// ---------------------------------------------------------------------------
// Gram accumulation over one chunk of a column's ratings.
// ---------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void gram_chunk(const int32_t *__restrict__ rowidx, const double *__restrict__ vals, int len,
                                           const double *__restrict__ other, const double *__restrict__ zero_row, double mean, double alpha,
                                           d4 (&acc)[Geo<K>::NTRI], double (&r)[Geo<K>::NT], int lane, int rowmask = -1)
{
    constexpr int NT = Geo<K>::NT;
    const int kq = lane >> 4, li = lane & 15;
    // The ratings are consumed in blocks of 64: one coalesced load brings 64 row ids and 64
    // values (lane l holds rating b+l), the 16 MFMA k-steps of the block then fetch their 4
    // row ids with a cross-lane permute instead of a dependent memory round trip.  Gathers of
    // the next 16 ratings are in flight while the MFMAs of the current 16 issue.
    int ri_n = (0 + lane < len) ? rowidx[lane] : -1;
    double wv_n = (0 + lane < len) ? (vals[lane] - mean) * alpha : 0.0;        // c++/sample.cpp:256
    for (int b = 0; b < len; b += 64) {
        const int ri = ri_n;
        const double wv = wv_n;
        if (b + 64 < len) {                                                      // wave-uniform
            const int q = b + 64 + lane;
            ri_n = (q < len) ? rowidx[q] : -1;
            wv_n = (q < len) ? (vals[q] - mean) * alpha : 0.0;
        }
        const int nsteps = (len - b >= 64) ? 16 : (len - b + 3) >> 2;           // k-steps in this block
        double y[4][NT], w[4];
        auto gather = [&](int g, double (&yy)[4][NT], double (&ww)[4]) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int src = (g * 4 + s) * 4 + kq;
                const int row = __shfl(ri, src);
                ww[s] = __shfl(wv, src);
                // No select around the loads (the compiler would branch around each one and wait for it on the spot):
                // padding slots gather a row of zeros; K = 8: the lanes li >= 8 read entry 0 and feed only the rows /
                // columns >= 8 of the padded 16 x 16 tile, which nobody reads.
                const double *col = (row >= 0) ? other + (size_t)(row & rowmask) * K : zero_row;   // rowmask: profiling only (ablate 4)
#pragma unroll
                for (int t = 0; t < NT; ++t) yy[s][t] = col[(t * 16 + li < K) ? t * 16 + li : 0];
            }
        };
        gather(0, y, w);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g * 4 >= nsteps) break;                                          // wave-uniform
            double yn[4][NT], wn[4];
            const bool more = (g + 1) * 4 < nsteps;
            if (g < 3 && more) gather(g + 1, yn, wn);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int t = 0; t < NT; ++t) r[t] = fma(y[s][t], w[s], r[t]);
                int tri = 0;
#pragma unroll
                for (int I = 0; I < NT; ++I)
#pragma unroll
                    for (int J = I; J < NT; ++J, ++tri) acc[tri] = mfma16(y[s][I], y[s][J], acc[tri]);
            }
            if (g < 3 && more) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    w[s] = wn[s];
#pragma unroll
                    for (int t = 0; t < NT; ++t) y[s][t] = yn[s][t];
                }
            }
        }
    }
    // the 4 k-groups of lanes hold partial rhs sums for the same latent index
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        r[t] += __shfl_xor(r[t], 16);
        r[t] += __shfl_xor(r[t], 32);
    }
}

// x + (x rotated by n lanes inside each row of 16 lanes), through DPP moves of the two halves
template <int CTRL>
__device__ __forceinline__ double row_ror_add(double x)
{
    const long long v = __builtin_bit_cast(long long, x);
    const int lo = (int)v, hi = (int)(v >> 32);
    // (bound_ctrl set: every lane of a rotate has a source, and with all rows / banks enabled the compiler then
    // knows the old value of the destination is dead -- otherwise it zeroes both halves ahead of every move)
    const int rlo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    const int rhi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    const long long rv = ((long long)rhi << 32) | (unsigned int)rlo;
    return x + __builtin_bit_cast(double, rv);
}

// first two 64-rating index blocks of a chunk: issued by the caller ahead of the normal draw, whose
// Philox / log / sqrt arithmetic then runs in the shadow of these loads
// The block keeps what was LOADED (row id and rating of slot base + lane; slots beyond the chunk read `safe`, K zeros):
// nothing is computed from the loads here, so the wave does not wait for them before their first use in gather().
// (With `(q < len) ? (vals[q] - mean) * alpha : 0` the compiler put each load in a branch of its own and waited for it
// on the spot: the normal draw that was meant to run in the shadow of these loads started after them.)
// WT (the weighted forms): the block also keeps sqrt(w) of its slot, loaded from `sw` the same way (slots beyond
// the chunk: the 0.0 of `safe`); gather() hands it on, contract() multiplies the gathered row by it.
template <bool WT> struct IdxBlockT { int ri; double v; int base; };
template <> struct IdxBlockT<true> { int ri; double v; int base; double s; };
typedef IdxBlockT<false> IdxBlock;
template <bool WT = false>
__device__ __forceinline__ IdxBlockT<WT> load_idx_block(const int32_t *__restrict__ rowidx, const double *__restrict__ vals, int base, int lane, int len,
                                                        const double *__restrict__ safe, const double *__restrict__ sw = nullptr)
{
    IdxBlockT<WT> r;
    const int q = base + lane;
    const int32_t *pr = (q < len) ? rowidx + q : reinterpret_cast<const int32_t *>(safe);
    const double *pv = (q < len) ? vals + q : safe;
    r.ri = *pr;
    r.v = *pv;
    if constexpr (WT) {
        const double *ps = (q < len) ? sw + q : safe;
        r.s = *ps;
    }
    r.base = base;
    return r;
}

template <int K, bool WT = false>
__device__ __forceinline__ void gram_chunk44(const int32_t *__restrict__ rowidx, const double *__restrict__ vals, int len,
                                             const double *__restrict__ other, const double *__restrict__ zero_row,
                                             double mean, double alpha, IdxBlockT<WT> cur, IdxBlockT<WT> nxt,
                                             double (&acc)[Geo44<K>::NB], double (&rr)[Geo44<K>::NG], int lane, int rowmask = -1,
                                             const double *__restrict__ sw = nullptr)
{
    using G = Geo44<K>;
    constexpr int NG = G::NG, NL = G::NL;
    typedef double dd2 __attribute__((ext_vector_type(2)));
    const int slot = lane >> 2, x = lane & 3;
    // 64 ratings per coalesced index block (lane l holds rating b0 + l, loaded two blocks ahead);
    // the four 16-rating groups of a block fetch their row ids with a cross-lane permute.  The
    // gathers run one group ahead of the MFMAs in two alternating operand sets, across block
    // boundaries too; padding slots of a ragged last group gather a row of zeros.
    auto gather = [&](const IdxBlockT<WT> &ib, int gg, dd2 (&yy)[NL], double &ww, double &ss) {
        const int src = gg * 16 + slot;
        const int row = __shfl(ib.ri, src);
        ww = (__shfl(ib.v, src) - mean) * alpha;                                  // c++/sample.cpp:256 (padding slots: times a row of zeros)
        if constexpr (WT) ss = __shfl(ib.s, src);
        const double *base = (ib.base + src < len) ? other + (size_t)(row & rowmask) * K : zero_row;
        const dd2 *p = reinterpret_cast<const dd2 *>(base + 2 * x);
#pragma unroll
        for (int h = 0; h < NL; ++h) yy[h] = p[4 * h];
    };
    // (weighted: the row enters the rhs update and the MFMAs as sqrt(w) u -- scaled here, where the gathered row is first used, so
    //  that nothing waits for a gather where it is issued)
    auto contract = [&](const dd2 (&yy)[NL], double ww, double ss) {
        double R[NG];
#pragma unroll
        for (int h = 0; h < NL; ++h) { R[2 * h] = yy[h].x; R[2 * h + 1] = yy[h].y; }
        if constexpr (WT) {
#pragma unroll
            for (int g = 0; g < NG; ++g) R[g] *= ss;
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) rr[g] = fma(R[g], ww, rr[g]);
        int blk = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int g2 = g; g2 < NG; ++g2, ++blk) acc[blk] = mfma44(R[g], R[g2], acc[blk]);
    };
    if (len <= 0) return;
    dd2 yA[NL], yB[NL];
    double wA, wB = 0.0, sA = 0.0, sB = 0.0;
    gather(cur, 0, yA, wA, sA);
    int b0 = 0;
    // full blocks that have a successor: straight-line code, the operand sets simply alternate
    for (; b0 + 64 < len; b0 += 64) {
        // the index block after the next one: requested here, a whole block ahead of its first use -- except by the weighted form, whose
        // blocks are two registers wider: three of them in flight spill at K = 32 (140 bytes per lane, 0.137 ms per ML-1M iteration
        // against 0.098 with the request at the end of the trip, which is still three groups of MFMAs ahead of the block's first gather)
        IdxBlockT<WT> nn{};
        if constexpr (!WT) nn = load_idx_block<WT>(rowidx, vals, b0 + 128, lane, len, zero_row, sw);
        gather(cur, 1, yB, wB, sB);
        contract(yA, wA, sA);
        gather(cur, 2, yA, wA, sA);
        contract(yB, wB, sB);
        gather(cur, 3, yB, wB, sB);
        contract(yA, wA, sA);
        gather(nxt, 0, yA, wA, sA);                                                  // first group of the next block
        contract(yB, wB, sB);
        cur = nxt;
        if constexpr (WT) nxt = load_idx_block<WT>(rowidx, vals, b0 + 128, lane, len, zero_row, sw);
        else nxt = nn;
    }
    // last block: 1..4 groups
    const int ng = (len - b0 + 15) >> 4;
    if (ng > 1) gather(cur, 1, yB, wB, sB);
    contract(yA, wA, sA);
    if (ng > 1) {
        if (ng > 2) gather(cur, 2, yA, wA, sA);
        contract(yB, wB, sB);
        if (ng > 2) {
            if (ng > 3) gather(cur, 3, yB, wB, sB);
            contract(yA, wA, sA);
            if (ng > 3) contract(yB, wB, sB);
        }
    }
}

// The same Gram from the side's gather stream (args.h: GatherRec, built once per side by build_schedule): lane (slot, x)
// reads the record of ITS slot of every group with one 16-byte load (the four x lanes share the address) -- no index
// blocks, no cross-lane permutes, no row * K, no r - mean; a padding record (off < 0, d = 0) gathers the row of zeros.
// One loop over the item's groups of 16 ratings, unrolled by two over the two operand sets: the records run two groups
// ahead of the MFMAs, the gathers one group ahead.  The record loads are unconditional (they run into the next item's
// records, or the kGatherTailGroups padding groups behind the last item); a gather is only issued for a group the item
// has.  Slot-to-block mapping, order of the groups and every floating-point operation are gram_chunk44's: the two forms
// give the same bits (d * alpha is the (v - mean) * alpha of the other form with the subtraction done on the host).
// r0, r1: the records of groups 0 and 1, requested by the caller ahead of the normal draw.
typedef double gs_raw __attribute__((ext_vector_type(2)));        // a record as loaded: .x = off | unused, .y = d
// rec: the item's first record (wave-uniform); slot_bytes: 16 * the lane's slot -- a scalar base the loop advances on the
// scalar unit plus a fixed 32-bit lane offset: no vector address arithmetic per load
__device__ __forceinline__ gs_raw load_gs_rec(const GatherRec *__restrict__ rec, int g, unsigned slot_bytes)
{
    return *reinterpret_cast<const gs_raw *>(reinterpret_cast<const char *>(rec + 16 * g) + slot_bytes);
}

template <int K>
__device__ __forceinline__ void gram_stream44(const GatherRec *__restrict__ rec, int ng, const double *__restrict__ other,
                                              const double *__restrict__ zero_row, double alpha, gs_raw r0, gs_raw r1, unsigned slot_bytes,
                                              double (&acc)[Geo44<K>::NB], double (&rr)[Geo44<K>::NG], int lane)
{
    using G = Geo44<K>;
    constexpr int NG = G::NG, NL = G::NL;
    typedef double dd2 __attribute__((ext_vector_type(2)));
    const int x = lane & 3;
    const dd2 *ox = reinterpret_cast<const dd2 *>(other + 2 * x), *zx = reinterpret_cast<const dd2 *>(zero_row + 2 * x);
    auto gather = [&](const gs_raw &rc, dd2 (&yy)[NL], double &ww) {
        const int off = (int)__builtin_bit_cast(long long, rc.x);
        ww = rc.y * alpha;                                                        // c++/sample.cpp:256
        const dd2 *p = (off >= 0) ? ox + off : zx;
#pragma unroll
        for (int h = 0; h < NL; ++h) yy[h] = p[4 * h];
    };
    auto contract = [&](const dd2 (&yy)[NL], double ww) {
        double R[NG];
#pragma unroll
        for (int h = 0; h < NL; ++h) { R[2 * h] = yy[h].x; R[2 * h + 1] = yy[h].y; }
#pragma unroll
        for (int g = 0; g < NG; ++g) rr[g] = fma(R[g], ww, rr[g]);
        int blk = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int g2 = g; g2 < NG; ++g2, ++blk) acc[blk] = mfma44(R[g], R[g2], acc[blk]);
    };
    if (ng <= 0) return;
    dd2 yA[NL], yB[NL];
    double wA, wB = 0.0;
    gather(r0, yA, wA);
    r0 = load_gs_rec(rec, 2, slot_bytes);
    if (ng > 1) gather(r1, yB, wB);                                              // group 1
    r1 = load_gs_rec(rec, 3, slot_bytes);
    // group 0 on its own: the accumulators are known to be zero here (the caller cleared them), so its MFMAs take the
    // constant 0 as their C operand and 44 register clears per item go away
    contract(yA, wA);
    int g = 1;
    // two groups per trip while the second of them has a successor; yB holds group g at the top
    for (; g + 2 < ng; g += 2) {
        gather(r0, yA, wA);                                                      // group g + 1
        r0 = load_gs_rec(rec, g + 3, slot_bytes);
        contract(yB, wB);
        gather(r1, yB, wB);                                                      // group g + 2
        r1 = load_gs_rec(rec, g + 4, slot_bytes);
        contract(yA, wA);
    }
    // the last one or two groups
    if (g < ng) {
        if (g + 1 < ng) gather(r0, yA, wA);
        contract(yB, wB);
        if (g + 1 < ng) contract(yA, wA);
    }
}

// DPP move of the lanes whose bank (the b of lane = 16 i + 4 b + j) is in BANKS; the other lanes keep `old`
template <int CTRL, int BANKS>
__device__ __forceinline__ double dpp_merge(double old, double src)
{
    const long long o = __builtin_bit_cast(long long, old), v = __builtin_bit_cast(long long, src);
    const int lo = __builtin_amdgcn_update_dpp((int)o, (int)v, CTRL, 0xF, BANKS, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(v >> 32), CTRL, 0xF, BANKS, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// The bank totals of four registers in one: bank 0 of the result holds the total of x0, bank 1 of x1, bank 2 of y0, bank 3 of
// y1 -- a reduce-scatter over the four b.  Level 1 (row_ror:8, bank b reads bank b ^ 2) merges (x, y) into one register with
// x_b + x_{b+2} in the banks 0, 1 and y_{b-2} + y_b in the banks 2, 3; level 2 merges two of those (row_ror:12: bank b reads
// bank b + 1, row_ror:4: bank b - 1).  Every addition pairs the two operands the all-lanes form pairs, (v_b + v_{b^2}) +
// (v_{b^1} + v_{b^3}): the totals have the same bits.  12 DPP moves, 3 additions and 3 register copies (a merge overwrites
// its `old`, which the partner merge still reads) where summing the four registers in every lane takes 16 moves and 8
// additions, and each total exists once.
__device__ __forceinline__ double bank_totals4(double x0, double x1, double y0, double y1)
{
    const double u0 = dpp_merge<0x128, 0x3>(y0, x0), v0 = dpp_merge<0x128, 0xC>(x0, y0);
    const double z0 = v0 + u0;
    const double u1 = dpp_merge<0x128, 0x3>(y1, x1), v1 = dpp_merge<0x128, 0xC>(x1, y1);
    const double z1 = v1 + u1;
    const double p = dpp_merge<0x12C, 0x5>(z1, z0), q = dpp_merge<0x124, 0xA>(z0, z1);
    return q + p;
}

// a + b of the two registers the row swap leaves: the rows (16 lanes) 1, 3 of x change places with the rows 0, 2 of y
// (WIDE: the rows 2, 3 of x with the rows 0, 1 of y)
template <bool WIDE>
__device__ __forceinline__ double row_swap_add(double x, double y)
{
    const unsigned long long a = __builtin_bit_cast(unsigned long long, x), b = __builtin_bit_cast(unsigned long long, y);
    unsigned alo, blo, ahi, bhi;
    if constexpr (WIDE) {
        const auto l = __builtin_amdgcn_permlane32_swap((unsigned)a, (unsigned)b, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap((unsigned)(a >> 32), (unsigned)(b >> 32), false, false);
        alo = l[0]; blo = l[1]; ahi = h[0]; bhi = h[1];
    } else {
        const auto l = __builtin_amdgcn_permlane16_swap((unsigned)a, (unsigned)b, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap((unsigned)(a >> 32), (unsigned)(b >> 32), false, false);
        alo = l[0]; blo = l[1]; ahi = h[0]; bhi = h[1];
    }
    return __builtin_bit_cast(double, ((unsigned long long)ahi << 32) | alo) + __builtin_bit_cast(double, ((unsigned long long)bhi << 32) | blo);
}

// K = 32: the four b of every accumulator are added ONCE (bank_totals4: four registers become one that holds each total in
// one bank), so every store below is a full-wave 8-byte store of 64 different entries -- no exec regions.  Which block goes
// to which bank is chosen so that a lane's store address is a per-lane term (computed once from b) plus a compile-time
// constant per register, and so that a register is mirrored as a whole or not at all:
//   2 registers  diagonal blocks (b, b) and (4 + b, 4 + b)
//   4 registers  block row g = 0..3 against the columns 4 + b
//   3 registers  the blocks inside the block quads 0..3 and 4..7: (g, g2), (g', g2') in the banks 0, 1 and the same + (4, 4) in 2, 3
//   2 registers  rhs sums b and 4 + b: their rows i are then added by two row swaps (the operand pairs of xor 16, xor 32);
//                after the first the two registers are one
// 9 + 7 stores of G and one of the rhs sums; a group of four accumulators is dead once it is merged.
template <int K>
__device__ __forceinline__ void assemble44_packed(double (&acc)[Geo44<K>::NB], double (&rr)[Geo44<K>::NG], double *sA, double *sb,
                                                  int LD, int lane)
{
    using G = Geo44<K>;
    constexpr int NG = G::NG;
    static_assert(NG == 8, "the packing is the one of K = 32");
    const int i = lane >> 4, b = (lane >> 2) & 3, j = lane & 3;
    auto blk = [](int g, int g2) constexpr { return g * NG - (g * (g - 1)) / 2 + (g2 - g); };
    const int ib = G::idx(b, 0), b1 = b & 1;
    const int quad = (b >> 1) * (G::idx(4, 0) * LD + G::idx(4, 0));              // banks 2, 3: the block + (4, 4)
    double *up = sA + (2 * i) * LD + 2 * j;      // entry (idx(g, i), idx(g2, j)) of block (g, g2): lane base + block offset
    double *lo = sA + (2 * j) * LD + 2 * i;      // its mirror image (idx(g2, j), idx(g, i))
    // inside the two quads: (0, 2) | (0, 3), (1, 2) | (1, 3) -- neighbours in a row -- and (0, 1) | (2, 3)
    {
        double *pu = up + quad + b1, *pl = lo + quad + b1 * LD;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const double v = bank_totals4(acc[blk(g, 2)], acc[blk(g, 3)], acc[blk(g + 4, 6)], acc[blk(g + 4, 7)]);
            pu[G::idx(g, 0) * LD + G::idx(2, 0)] = v;
            pl[G::idx(2, 0) * LD + G::idx(g, 0)] = v;
        }
        const int d = b1 * (G::idx(2, 0) * LD + G::idx(2, 0));                    // (0, 1) -> (2, 3)
        const double v = bank_totals4(acc[blk(0, 1)], acc[blk(2, 3)], acc[blk(4, 5)], acc[blk(6, 7)]);
        up[quad + d + G::idx(0, 0) * LD + G::idx(1, 0)] = v;
        lo[quad + d + G::idx(1, 0) * LD + G::idx(0, 0)] = v;
    }
    // block rows 0..3 x block columns 4..7
    {
        double *pu = up + ib, *pl = lo + ib * LD;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const double v = bank_totals4(acc[blk(g, 4)], acc[blk(g, 5)], acc[blk(g, 6)], acc[blk(g, 7)]);
            pu[G::idx(g, 0) * LD + G::idx(4, 0)] = v;
            pl[G::idx(4, 0) * LD + G::idx(g, 0)] = v;
        }
    }
    // diagonal blocks
    {
        double *p = up + ib * (LD + 1);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            p[G::idx(4 * h, 0) * (LD + 1)] = bank_totals4(acc[blk(4 * h, 4 * h)], acc[blk(4 * h + 1, 4 * h + 1)],
                                                          acc[blk(4 * h + 2, 4 * h + 2)], acc[blk(4 * h + 3, 4 * h + 3)]);
    }
    // rhs sums: row i & 1 ends up with the totals of the groups 4 (i & 1) + b
    {
        const double w0 = bank_totals4(rr[0], rr[1], rr[2], rr[3]), w1 = bank_totals4(rr[4], rr[5], rr[6], rr[7]);
        const double s = row_swap_add<false>(w0, w1);                             // rows 0, 2: w0 of i + i ^ 1; rows 1, 3: w1
        const double t = row_swap_add<true>(s, s);                                // + the same of i ^ 2
        sb[G::idx(4 * (i & 1), 0) + G::idx(b, j)] = t;
    }
}

// The four b of every accumulator are added (fixed order: (b + b^2) + the same of b^1; every lane ends up with the
// total), then the full symmetric G goes into the K x LD LDS matrix finish_single reads: the lanes b = 0 write the
// upper blocks, the lanes b = 1 their mirror images, two block rows (g, g + 1) at a time -- two exec regions per row
// pair instead of one per block, 16-byte stores wherever two blocks are neighbours in a row (idx(g, x) and
// idx(g + 1, x) are adjacent for even g).  The rhs sums (also over the four k) go into sb.
// K = 32 takes the packed form above (the same bits in LDS); this one serves K = 8 and 16, whose 5 and 14 registers
// do not fill groups of four.
template <int K>
__device__ __forceinline__ void assemble44(double (&acc)[Geo44<K>::NB], double (&rr)[Geo44<K>::NG], double *sA, double *sb,
                                           int LD, int lane)
{
    if constexpr (K == 32) {
        assemble44_packed<K>(acc, rr, sA, sb, LD, lane);
        return;
    }
    using G = Geo44<K>;
    constexpr int NG = G::NG;
    static_assert(NG % 2 == 0, "block rows are written in pairs");
    const int i = lane >> 4, b = (lane >> 2) & 3, j = lane & 3;
    auto blk = [](int g, int g2) constexpr { return g * NG - (g * (g - 1)) / 2 + (g2 - g); };
    double *up = sA + (2 * i) * LD + 2 * j;      // entry (idx(g, i), idx(g2, j)) of block (g, g2): lane base + compile-time offset
    double *lo = sA + (2 * j) * LD + 2 * i;      // its mirror image (idx(g2, j), idx(g, i))
#pragma unroll
    for (int g = 0; g < NG; g += 2) {
#pragma unroll
        for (int t = blk(g, g); t < blk(g + 1, NG - 1) + 1; ++t) {
            const double v = row_ror_add<0x128>(acc[t]);                          // row_ror:8
            acc[t] = row_ror_add<0x124>(v);                                       // row_ror:4
        }
        if (b == 0) {
            up[G::idx(g + 1, 0) * LD + G::idx(g + 1, 0)] = acc[blk(g + 1, g + 1)];
#pragma unroll
            for (int g2 = g; g2 < NG; g2 += 2) {
                double2 v; v.x = acc[blk(g, g2)]; v.y = acc[blk(g, g2 + 1)];
                *reinterpret_cast<double2 *>(&up[G::idx(g, 0) * LD + G::idx(g2, 0)]) = v;
                if (g2 > g) {
                    double2 w; w.x = acc[blk(g + 1, g2)]; w.y = acc[blk(g + 1, g2 + 1)];
                    *reinterpret_cast<double2 *>(&up[G::idx(g + 1, 0) * LD + G::idx(g2, 0)]) = w;
                }
            }
        } else if (b == 1) {
            lo[G::idx(g + 1, 0) * LD + G::idx(g, 0)] = acc[blk(g, g + 1)];
#pragma unroll
            for (int g2 = g + 2; g2 < NG; ++g2) {
                double2 v; v.x = acc[blk(g, g2)]; v.y = acc[blk(g + 1, g2)];
                *reinterpret_cast<double2 *>(&lo[G::idx(g2, 0) * LD + G::idx(g, 0)]) = v;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        double v = row_ror_add<0x128>(rr[g]);
        v = row_ror_add<0x124>(v);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lane < 4) sb[G::idx(g, lane)] = v;
    }
}

// ---------------------------------------------------------------------------
// Everything after the Gram (c++/sample.cpp:285,297-324), in two parts.
//
// deposit_column: the wave that holds a column's complete Gram parks
//     Lambda* = LambdaF + alpha G   (lower triangle, packed, :297-298),
//     b = LambdaF mu + rr           (:285,:256)   and   z ~ N(0,I)   (:322, stream :266)
// in one of its C = 64/K LDS slots.
//
// finish_slots: the wave factorises all filled slots side by side, lane (c, i) = (lane / K,
// lane % K) owning row i of slot c in registers.  Right-looking Cholesky, two columns per step:
// the 2x2 pivot block is factored redundantly by every lane of the group (its entries arrive
// through the LDS crossbar), each lane scales its two entries of columns k, k+1 and stores them
// (row-major packed L, one 16-byte store), then applies the rank-2 update to the rest of its
// row with L(j,k), L(j,k+1) read as one broadcast 16-byte LDS load per row j.  The forward
// solve L y = b is the same update applied to one more column (the rhs).  Backward solve and
// the coalesced 8K-byte store of the sample follow.  Per-step work that is identical for all
// lanes of a group (two 1/sqrt, the pivot algebra) is thus shared by C columns.
// ---------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void deposit_column(const SampleArgs &a, int64_t idx, const d4 (&acc)[Geo<K>::NTRI],
                                               const double (&r)[Geo<K>::NT], double *lds, int slot, int lane)
{
    using G = Geo<K>;
    constexpr int NT = G::NT;
    const int kq = lane >> 4, li = lane & 15;
    double *sL = lds + slot * G::SLOT, *sY = sL + G::PLEN, *sZ = sY + K;

    draw_normals<K>(sample_counter(idx, a.ktrue, a.iter_plus_1), a.ktrue, sZ, lane, K);
    const double *LF = a.prop_lambda ? a.prop_lambda + (size_t)(idx - a.col_from) * K * K : a.LambdaF;

    int tri = 0;
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = I; J < NT; ++J, ++tri)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int gi = I * 16 + kq + 4 * reg, gj = J * 16 + li;
                // G is symmetric and the upper tiles are what was accumulated: element (gi, gj) of
                // an off-diagonal tile is entry (row gj, col gi) of the lower triangle
                const int row = (I == J) ? gi : gj, col = (I == J) ? gj : gi;
                if (row < K && col <= row)
                    sL[tri_off(row) + col] = (a.diag_only && row != col) ? 0.0 : fma(a.alpha, acc[tri][reg], LF[row + col * K]);
            }
    if (kq == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t * 16 + li < K) {
                double lm = a.Lmu[t * 16 + li];
                if (a.prop_lambda) {                               // rr = Lambda_i * hp.mu (:285)
                    lm = 0.0;
                    for (int j = 0; j < K; ++j) lm = fma(LF[t * 16 + li + j * K], a.mu[j], lm);
                }
                sY[t * 16 + li] = lm + r[t];
            }
    }
    if (lane == 0) reinterpret_cast<long long *>(lds + G::C * G::SLOT)[slot] = idx;
}

template <int K>
struct Pivot { double dinv0, dinv1, l10; };

// Factors the 2x2 pivot block [a b; b c].  The two reciprocal square roots are independent --
// the second goes through the determinant, 1/sqrt(c - b^2/a) = sqrt(a)/sqrt(a c - b^2).
template <int K>
__device__ __forceinline__ Pivot<K> factor_block(double pa, double pb, double pc)
{
    Pivot<K> v;
    v.dinv0 = rsqrt_nr(pa);
    const double rdet = rsqrt_nr(fma(pa, pc, -(pb * pb)));
    v.dinv1 = rdet * (pa * v.dinv0);
    v.l10 = pb * v.dinv0;
    return v;
}

template <int K>
__device__ __forceinline__ void finish_slots(const SampleArgs &a, double *lds, int nfilled, int lane_in)
{
    using G = Geo<K>;
    constexpr int NP = G::NP;
    int lane = lane_in;
    // The caller runs this inside its persistent work loop: make the lane id opaque here so that
    // LLVM does not hoist every per-step address and lane mask out of that loop (and spill them).
    asm volatile("" : "+v"(lane));
    const int c = lane / K, i = lane % K;
    double *sL = lds + c * G::SLOT, *sY = sL + G::PLEN, *sZ = sY + K;
    double *myrow = sL + tri_off(i);
    const int gbase = 4 * (c * K);                                 // byte index of lane (c, 0) for ds_bpermute
    __syncthreads();                                               // the deposits are complete

    // this lane's row of Lambda* (entries right of the diagonal are never used), rhs, normal
    double row[K + 1];
#pragma unroll
    for (int j = 0; j < K; j += 2) {
        const double2 g = *reinterpret_cast<const double2 *>(&myrow[j]);
        row[j] = g.x;
        row[j + 1] = g.y;
    }
    row[K] = sY[i];
    const double zi = sZ[i];
    Pivot<K> pv = factor_block<K>(sL[0], sL[tri_off(1)], sL[tri_off(1) + 1]);
    __syncthreads();

#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int k = 2 * p;
        // scale this row's entries of columns k, k+1 and publish them; finished rows (i < k)
        // have nothing to store (their slot in the packed triangle does not exist)
        double2 lp;
        lp.x = row[k] * pv.dinv0;
        lp.y = fma(-lp.x, pv.l10, row[k + 1]) * pv.dinv1;
        if (i >= k) *reinterpret_cast<double2 *>(&myrow[k]) = lp;

        // Next pivot block [a b; b c] = entries (k+2..k+3, k+2..k+3) after this step's update.  Its
        // three entries and the rhs entries of rows k, k+1 come from their owner lanes through
        // the LDS crossbar, the four L values that update it from LDS after the barrier.
        double na = 0.0, nb = 0.0, nc = 0.0;
        if (p + 1 < NP) {
            na = gbcast(row[k + 2], gbase, k + 2);
            nb = gbcast(row[k + 2], gbase, k + 3);
            nc = gbcast(row[k + 3], gbase, k + 3);
        }
        const double rb0 = gbcast(row[K], gbase, k), rb1 = gbcast(row[K], gbase, k + 1);
        __syncthreads();
        const double2 L = *reinterpret_cast<const double2 *>(&myrow[k]);            // L(i,k), L(i,k+1)
        Pivot<K> pn = pv;
        if (p + 1 < NP) {
            const double2 l0 = *reinterpret_cast<const double2 *>(&sL[tri_off(k + 2) + k]);   // L(k+2,k), L(k+2,k+1)
            const double2 l1 = *reinterpret_cast<const double2 *>(&sL[tri_off(k + 3) + k]);   // L(k+3,k), L(k+3,k+1)
            const double pa = fma(-l0.y, l0.y, fma(-l0.x, l0.x, na));
            const double pb = fma(-l1.y, l0.y, fma(-l1.x, l0.x, nb));
            const double pc = fma(-l1.y, l1.y, fma(-l1.x, l1.x, nc));
            pn = factor_block<K>(pa, pb, pc);
        }
        // forward solve (:321) as one more column: y_k, y_k+1, then b_i -= L(i,k) y_k + L(i,k+1) y_k+1
        const double yk = rb0 * pv.dinv0;
        const double yk1 = fma(-pv.l10, yk, rb1) * pv.dinv1;
        if (i == 0) *reinterpret_cast<double2 *>(&sY[k]) = double2{yk, yk1};
        row[K] = fma(-L.y, yk1, fma(-L.x, yk, row[K]));
        // rank-2 update of the rest of the row: (i,j) -= L(i,k) L(j,k) + L(i,k+1) L(j,k+1), j > k+1
#pragma unroll
        for (int j = k + 2; j < K; ++j) {
            const double2 A = *reinterpret_cast<const double2 *>(&sL[tri_off(j) + k]);
            row[j] = fma(-L.y, A.y, fma(-L.x, A.x, row[j]));
        }
        // Pin this step's results: otherwise instruction selection defers every FMA chain to
        // the step that finally needs the entry and keeps (spills) all the L(j,k) it loaded meanwhile.
#pragma unroll
        for (int m = k + 2; m < K + 1; ++m) asm volatile("" : "+v"(row[m]));
        pv = pn;
    }
    __syncthreads();

    // rr += nrandn(K) (:322); backward solve L^T x = rr (:323):
    //   u_i = rr_i - sum_{k>i} L(k,i) x_k,  x_i = u_i / L(i,i)
    // the L(k,i) a lane needs are fetched eight steps at a time (LDS latency once per batch)
    double bi = sY[i] + zi;
    const double my_dinv = 1.0 / myrow[i];
    constexpr int BB = K < 8 ? K : 8;
#pragma unroll
    for (int kb = K - BB; kb >= 0; kb -= BB) {
        double lv[BB];
#pragma unroll
        for (int t = 0; t < BB; ++t) lv[t] = sL[tri_off(kb + t) + i];               // garbage for i > k: masked below
#pragma unroll
        for (int t = BB - 1; t >= 0; --t) {
            const int k = kb + t;
            if (k == 0) continue;
            const double xk = gbcast(bi * my_dinv, gbase, k);
            bi = (i < k) ? fma(-lv[t], xk, bi) : bi;
        }
    }
    const double xi = bi * my_dinv;

    if (c < nfilled) {
        const long long idx = reinterpret_cast<const long long *>(lds + G::C * G::SLOT)[c];
        a.items[(size_t)idx * K + i] = xi;                         // items().col(idx) = rr (:324)
        // a non-positive (or NaN) pivot makes its 1/sqrt NaN or inf, which reaches every later entry
        // and the sample itself: Eigen LLT's info() != Success -> THROWERROR("Cholesky failed") (:308)
        if (!(fabs(xi) <= 1.79769313486231570815e+308)) atomicMin(a.fail, (unsigned long long)idx);
    }
    __syncthreads();                                               // the slots are free again
}

#define BPMF_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// geometry of the one-column-per-wave factorisation (finish_single): S lanes per row
template <int K>
struct Geo1 {
    static constexpr int S = (64 / K < K / 2) ? 64 / K : K / 2;
    static constexpr int NP = K / 2;
    static constexpr int QN = NP / S;
    static constexpr int M = 2 * QN;
    static constexpr int FLD = K + 2;
    // K = 64: a full K x (K + 2) matrix is 34 KB of LDS per single-wave workgroup, i.e. ONE wave per SIMD.
    // Only the lower triangle is kept there (row j: entries 0 .. j, padded to an even count so that the
    // 16-byte accesses of the factorisation stay aligned): 19 KB, two waves per SIMD.
    static constexpr bool PACKED = K == 64;
    __host__ __device__ static constexpr int roff_c(int j) { return (j & 1) ? ((j + 1) * (j + 1)) / 2 : (j * (j + 2)) / 2; }
    static constexpr int AWORDS = PACKED ? roff_c(K) : K * FLD;
    static constexpr int LANES = K * S;
    static constexpr int LDS_WORDS = AWORDS + 4 * K + 2;
    // waves per SIMD k_sample1 is compiled for: the 4x4x4 Gram of K = 32 keeps 36 + 8 accumulators
    // and two operand sets in registers (<= 168 VGPRs)
    static constexpr int WPS = K == 32 ? 3 : (K < 32 ? 4 : 2);
};

// ---------------------------------------------------------------------------
// Everything after the Gram for one column (c++/sample.cpp:285,297-324).
//
// The wave holds Lambda* in registers, S lanes per row: lane (h, i) = (l / K, l % K) owns the
// entries (i, j) of the column pairs p = q*S + h (j = 2p, 2p+1), q = 0..QN-1, plus (lanes h = 0)
// the rhs b_i as one more column.  Right-looking Cholesky, TWO columns per step: the 2x2 pivot
// block comes through v_readlane, every lane factors it redundantly (two 1/sqrt), the owners
// scale their pair of column entries and publish them to LDS (row-major L, one 16-byte store),
// then each lane applies the rank-2 update to its remaining pairs, reading L(j,k),L(j,k+1) with
// one broadcast 16-byte LDS load per row.  The forward solve L y = b is the same update applied
// to the rhs column with the two y values (wave-uniform) in registers.  Backward solve, normal
// draw and the coalesced 8K-byte store follow.
// ---------------------------------------------------------------------------
// `assemble(sA, sb, LD, lane)` writes the full symmetric G (K x LD, row-major) and the rhs sums
// into LDS from the 4x4x4 blocks (assemble44).
template <int K, typename Assemble>
__device__ __forceinline__ void finish_single(const SampleArgs &a, int col_local, double *lds, int lane_in, bool have_z,
                                              Assemble &&assemble)
{
    int lane = lane_in;
    using G = Geo1<K>;
    constexpr int LD = G::FLD, S = G::S, NP = G::NP, QN = G::QN, M = G::M;
    // The caller runs this inside its persistent work loop: make the lane id opaque here so that
    // LLVM does not hoist every per-step address and lane mask out of that loop (and spill them).
    asm volatile("" : "+v"(lane));
    double *sA = lds, *sb = lds + G::AWORDS, *sz = sb + K, *sdummy = sz + K, *szero = sdummy + 2 * K;
    // start of row j of the LDS matrix (full rows of LD words, or the packed lower triangle)
    auto roff = [](int j) -> int {
        if constexpr (G::PACKED) return (j & 1) ? ((j + 1) * (j + 1)) >> 1 : (j * (j + 2)) >> 1;
        else return j * G::FLD;
    };
    const int64_t idx = a.col_from + col_local;

    // z ~ N(0, I) from stream (idx+1)*K*(iter+1) truncated to 32 bits (c++/sample.cpp:266, c++/bpmf.h:67)
    if (!have_z) draw_normals<K>(sample_counter(idx, a.ktrue, a.iter_plus_1), a.ktrue, sz, lane, K);

    const int l = lane & (G::LANES - 1);                           // K=8: the upper half-wave mirrors the lower
    const int h = l / K, i = l % K;
    // this lane's entries of LambdaF and LambdaF*mu: issued before the LDS round trip below
    const double *LF = a.prop_lambda ? a.prop_lambda + (size_t)col_local * K * K : a.LambdaF;
    // (K = 64: a row is 128 registers already; its LambdaF entries are read when they are used instead)
    constexpr bool PRELOAD = K <= 32;
    double lf[PRELOAD ? M : 2];
    if constexpr (PRELOAD) {
#pragma unroll
        for (int q = 0; q < QN; ++q) {
            const int j = 2 * (q * S + h);
            lf[2 * q] = LF[i + j * K];
            lf[2 * q + 1] = LF[i + (j + 1) * K];
        }
    }
    double lmu = a.Lmu[i];
    if (a.prop_lambda) {                                           // wave-uniform: rr = Lambda_i * hp.mu (:285)
        lmu = 0.0;
        for (int j = 0; j < K; ++j) lmu = fma(LF[i + j * K], a.mu[j], lmu);
    }

    // G -> LDS, mirrored (c++/sample.cpp:297); rhs sums -> LDS
    assemble(sA, sb, LD, lane);
    if (lane < 2) szero[lane] = 0.0;
    __syncthreads();

    // Lambda* = LambdaF + alpha * G (:298); b = LambdaF*mu + rr (:285,:256)
    double row[M + 2];
#pragma unroll
    for (int q = 0; q < QN; ++q) {
        double2 g;
        if constexpr (G::PACKED) {                                 // G(i, j): row max(i, j), column min(i, j)
            const int j = 2 * (q * S + h);
            g.x = sA[(j <= i) ? roff(i) + j : roff(j) + i];
            g.y = sA[(j + 1 <= i) ? roff(i) + j + 1 : roff(j + 1) + i];
        } else {
            g = *reinterpret_cast<const double2 *>(&sA[i * LD + 2 * (q * S + h)]);
        }
        if constexpr (PRELOAD) {
            row[2 * q] = fma(a.alpha, g.x, lf[2 * q]);
            row[2 * q + 1] = fma(a.alpha, g.y, lf[2 * q + 1]);
        } else {
            const int j = 2 * (q * S + h);
            row[2 * q] = fma(a.alpha, g.x, LF[i + j * K]);
            row[2 * q + 1] = fma(a.alpha, g.y, LF[i + (j + 1) * K]);
        }
    }
    if (a.diag_only) {                                             // wave-uniform
#pragma unroll
        for (int q = 0; q < QN; ++q) {
            const int j = 2 * (q * S + h);
            row[2 * q] = (j == i) ? row[2 * q] : 0.0;
            row[2 * q + 1] = (j + 1 == i) ? row[2 * q + 1] : 0.0;
        }
    }
    row[M] = (h == 0) ? lmu + sb[i] : 0.0;
    row[M + 1] = 0.0;
    const double zi = sz[i];
    double yi = 0.0;
    __syncthreads();

#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int hk = p % S, qk = p / S, k = 2 * p;
        const int src0 = hk * K + k, src1 = src0 + 1;
        // 2x2 pivot block [a b; b c] and the two rhs entries, wave-uniform
        const double pa = bcast(row[2 * qk], src0);
        const double pb = bcast(row[2 * qk], src1);
        const double pc = bcast(row[2 * qk + 1], src1);
        const double bk = bcast(row[M], k), bk1 = bcast(row[M], k + 1);
        // the two reciprocal square roots are independent (the second through the determinant:
        // 1/sqrt(c - b^2/a) = sqrt(a)/sqrt(a c - b^2)), so their latencies overlap
        const double dinv0 = rsqrt_nr(pa);
        const double rdet = rsqrt_nr(fma(pa, pc, -(pb * pb)));
        const double dinv1 = rdet * (pa * dinv0);
        const double l10 = pb * dinv0;
        // forward solve (:321) for these two rows: y_k, y_k+1
        const double yk = bk * dinv0;
        const double yk1 = fma(-l10, yk, bk1) * dinv1;
        yi = (i == k) ? yk : yi;
        yi = (i == k + 1) ? yk1 : yi;
        // owners scale their entries of columns k, k+1 and publish them; the other lanes hit a
        // dummy slot so that the step stays branch-free
        double2 lp;
        lp.x = row[2 * qk] * dinv0;
        lp.y = fma(-lp.x, l10, row[2 * qk + 1]) * dinv1;
        double *dst = (h == hk && (!G::PACKED || i >= k)) ? &sA[roff(i) + k] : &sdummy[2 * i];   // (packed: rows above k have no such entries)
        *reinterpret_cast<double2 *>(dst) = lp;
        __syncthreads();
        const double2 L = *reinterpret_cast<const double2 *>((!G::PACKED || i >= k) ? &sA[roff(i) + k] : szero);   // L(i,k), L(i,k+1)
        row[M] = fma(-L.y, yk1, fma(-L.x, yk, row[M]));            // rhs column: b_i -= L(i,k) y_k + L(i,k+1) y_k+1
        if constexpr (S > 1) {                                     // pairs of this slot owned by higher h are still to come
            const int j0 = 2 * (qk * S + h);
            const double2 A0 = *reinterpret_cast<const double2 *>(&sA[roff(j0) + k]);
            const double2 A1 = *reinterpret_cast<const double2 *>(&sA[roff(j0 + 1) + k]);
            const double u0 = fma(-L.y, A0.y, fma(-L.x, A0.x, row[2 * qk]));
            const double u1 = fma(-L.y, A1.y, fma(-L.x, A1.x, row[2 * qk + 1]));
            row[2 * qk] = (h > hk) ? u0 : row[2 * qk];
            row[2 * qk + 1] = (h > hk) ? u1 : row[2 * qk + 1];
        }
#pragma unroll
        for (int q = qk + 1; q < QN; ++q) {
            const int j0 = 2 * (q * S + h);
            const double2 A0 = *reinterpret_cast<const double2 *>(&sA[roff(j0) + k]);
            const double2 A1 = *reinterpret_cast<const double2 *>(&sA[roff(j0 + 1) + k]);
            row[2 * q] = fma(-L.y, A0.y, fma(-L.x, A0.x, row[2 * q]));
            row[2 * q + 1] = fma(-L.y, A1.y, fma(-L.x, A1.x, row[2 * q + 1]));
        }
        // Pin this step's results: otherwise instruction selection defers every FMA chain to
        // the step that finally needs the entry and keeps (spills) all the L(j,k) it loaded meanwhile.
#pragma unroll
        for (int m = 2 * qk; m < M + 1; ++m) asm volatile("" : "+v"(row[m]));
    }

    // rr += nrandn(K) (:322); backward solve L^T x = rr (:323):
    //   u_i = rr_i - sum_{k>i} L(k,i) x_k,  x_i = u_i / L(i,i)
    // the L(k,i) a lane needs are fetched eight steps at a time (LDS latency once per batch)
    double bi = yi + zi;
    const double my_dinv = 1.0 / sA[roff(i) + i];
    constexpr int BB = K < 8 ? K : 8;
#pragma unroll
    for (int kb = K - BB; kb >= 0; kb -= BB) {
        double lv[BB];
#pragma unroll
        for (int t = 0; t < BB; ++t) lv[t] = *((i < kb + t) ? &sA[roff(kb + t) + i] : szero);
#pragma unroll
        for (int t = BB - 1; t >= 0; --t) {
            const int k = kb + t;
            if (k == 0) continue;
            const double xk = bcast(bi * my_dinv, k);
            bi = fma(-lv[t], xk, bi);
        }
    }
    const double xi = bi * my_dinv;

    if (lane < K) a.items[(size_t)idx * K + lane] = xi;            // items().col(idx) = rr (:324)
    // a non-positive (or NaN) pivot makes its 1/sqrt NaN or inf, which reaches every later entry
    // and the sample itself: Eigen LLT's info() != Success -> THROWERROR("Cholesky failed") (:308)
    const bool bad = !(fabs(xi) <= 1.79769313486231570815e+308);
    if (__any(bad) && lane == 0) atomicMin(a.fail, (unsigned long long)idx);
}

// ---------------------------------------------------------------------------
// One-item-per-workgroup form of the sampler (BPMF_HIP_MODE=1): the hardware dispatcher hands
// the cost-sorted items to whatever wave slot frees up (dynamic balance without a software
// queue); the last chunk of a heavy column sums the partials; every column is factorised by
// one wave alone (finish_single: S lanes per row, lowest latency per column), which is what a
// matrix with only a few thousand columns per side needs.
// ---------------------------------------------------------------------------
// What else one k_sample1 launch carries besides its work items (the stateful single-GPU path):
// one workgroup per half-iteration that is not on any queue but this one.
//   * workgroup 0, if gate_host: the gate + staging of THIS launch's parameters (k_gate_stage's
//     job): polls the word the host sets when the Normal-Wishart draw is in pinned memory, copies
//     the blob to device memory, sets dflag; the item workgroups wait for dflag after their Gram
//     (wait_params).  Being the first workgroup of the launch it is always resident: no other
//     queue has to get a kernel scheduled beside a launch that fills the chip.
//   * the next nstat workgroups: the column statistics of the PREVIOUS launch's side (k_colstats'
//     job: that side's sampler is the previous kernel on this queue, so its columns are complete);
//     the host thread of that side spins on their result while this launch samples.
// A cross-queue dependency costs ~6.5 us of command-processor latency per hop even when it is
// satisfied long before (tools/probes/boundary2.hip): with both jobs inside the launch, two
// samplers follow each other on one queue in ~2 us instead of 8-11.
template <int K>
__device__ __forceinline__ void colstats_body(int w, const double *__restrict__ items, int64_t c0, int64_t c1, int nwaves,
                                              double *partials, const unsigned long long *__restrict__ fail_in,
                                              double *__restrict__ out, unsigned *ticket, unsigned *flag, unsigned seq,
                                              unsigned long long *tmo, unsigned long long wait_ticks, double *img);
__device__ __forceinline__ void gate_stage_body(int block, int nblocks, const unsigned *gate_host, unsigned want, const double *src_host,
                                                double *__restrict__ dst, int n, unsigned *dflag, unsigned dval,
                                                unsigned long long *tmo, unsigned long long wait_ticks);

// GS: the Gram reads the side's gather stream (gram_stream44: k_sample1) / the row ids and a value array through index
// blocks (gram_chunk44: k_sample1i, the launches that read other values than the side's own ratings and BPMF_HIP_GATHER_STREAM=0)
// WT: the weighted form (k_sample1w; never with GS): a.vals = sqrt(w) (r - mean), a.mean_rating = 0, a.sw = sqrt(w)
template <int K, bool GS, bool WT = false>
__device__ __forceinline__ void sample1_body(const SampleArgs &a, const FusedArgs &f, double *lds)
{
    const int lane = threadIdx.x;
    int bid = blockIdx.x;
    if (f.gate_host) {
        if (bid == 0) { gate_stage_body(0, 1, f.gate_host, f.gate_want, f.src_host, f.dst, f.n, f.dflag, f.dval, a.tmo, a.wait_ticks); return; }
        --bid;
    }
    if (bid < f.nstat) {
        colstats_body<K>(bid, f.st_items, f.st_c0, f.st_c1, f.nstat, f.st_partials, f.st_fail, f.st_out, f.st_ticket, f.st_flag, f.st_seq,
                         f.st_tmo, a.wait_ticks, lds);
        return;
    }
    const int w = bid - f.nstat;
    const int col = a.wi_col[w];
    const int64_t p0 = a.wi_p0[w];
    const int len = a.wi_len[w];
    const int mc = a.wi_mc[w];

    // the first index blocks (records of the first two groups) of the chunk are requested before anything else
    const int glen = (ablate_bits(a) & 2u) ? 0 : len;
    static_assert(!(GS && WT), "the gather stream carries no weights");
    IdxBlockT<WT> ib0{}, ib1{};
    gs_raw gr0{}, gr1{};
    const GatherRec *rec = nullptr;
    const unsigned slot_bytes = 16u * ((unsigned)lane >> 2);
    int ng = 0;
    if constexpr (GS) {
        rec = a.gs_rec + (size_t)a.gs_g0[w] * 16;
        ng = (ablate_bits(a) & 2u) ? 0 : a.gs_ng[w];
        gr0 = load_gs_rec(rec, 0, slot_bytes);
        gr1 = load_gs_rec(rec, 1, slot_bytes);
    } else {
        ib0 = load_idx_block<WT>(a.rowidx + p0, a.vals + p0, 0, lane, glen, a.zero_row, WT ? a.sw + p0 : nullptr);
        ib1 = load_idx_block<WT>(a.rowidx + p0, a.vals + p0, 64, lane, glen, a.zero_row, WT ? a.sw + p0 : nullptr);
    }

    // whole column in one item: its normals do not depend on the Gram -- draw them first so that
    // the Philox / log / sqrt chain is off the critical path between the last MFMA and the factorisation
    if (mc < 0 && !(ablate_bits(a) & 1u))
        draw_normals<K>(sample_counter(a.col_from + col, a.ktrue, a.iter_plus_1), a.ktrue, lds + Geo1<K>::AWORDS + K, lane, K);

    static_assert(K <= 32, "k_sample1: K <= 32 (K = 64 runs the slab form, K = 128 the workgroup form)");
    {
        // Gram on the 4x4x4 MFMA shape: NB block accumulators + NG rhs sums per lane
        using G4 = Geo44<K>;
        constexpr int NB = G4::NB, NG = G4::NG, PART = G4::PART;
        double acc[NB], rr[NG];
#pragma unroll
        for (int t = 0; t < NB; ++t) acc[t] = 0.0;
#pragma unroll
        for (int t = 0; t < NG; ++t) rr[t] = 0.0;
        if constexpr (GS)
            gram_stream44<K>(rec, ng, a.other_items, a.zero_row, a.alpha, gr0, gr1, slot_bytes, acc, rr, lane);
        else
            gram_chunk44<K, WT>(a.rowidx + p0, a.vals + p0, glen, a.other_items, a.zero_row, a.mean_rating, a.alpha, ib0, ib1, acc, rr, lane,
                                (ablate_bits(a) & 4u) ? 63 : -1, WT ? a.sw + p0 : nullptr);
        if (ablate_bits(a) & 1u) {
            double v = rr[0];
#pragma unroll
            for (int t = 0; t < NB; ++t) v += acc[t];
            if (mc < 0 && lane < K) a.items[(size_t)(a.col_from + col) * K + lane] = v;
            return;
        }
        if (mc >= 0) {
            // chunk of a heavy column: park the accumulators; whichever chunk arrives last adds them up
            const int nch = a.mc_nchunks[mc];
            double *pbase = a.partials + (size_t)a.mc_slot0[mc] * PART;
            double *p = pbase + (size_t)a.wi_chunk[w] * PART;
#pragma unroll
            for (int t = 0; t < NB; ++t) __hip_atomic_store(&p[t * 64 + lane], acc[t], BPMF_RLX_AGENT);
#pragma unroll
            for (int t = 0; t < NG; ++t) __hip_atomic_store(&p[(NB + t) * 64 + lane], rr[t], BPMF_RLX_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            unsigned t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add(&a.mc_count[mc], 1u, BPMF_RLX_AGENT);
            t = __builtin_amdgcn_readfirstlane(t);
            if ((int)t != nch - 1) return;
            if (lane == 0) __hip_atomic_store(&a.mc_count[mc], 0u, BPMF_RLX_AGENT);
#pragma unroll
            for (int t2 = 0; t2 < NB; ++t2) acc[t2] = 0.0;
#pragma unroll
            for (int t2 = 0; t2 < NG; ++t2) rr[t2] = 0.0;
            for (int ch = 0; ch < nch; ++ch) {
                const double *pc = pbase + (size_t)ch * PART;
                double tmp[NB + NG];                                  // all loads of a chunk in flight, then the adds (chunk order)
#pragma unroll
                for (int t2 = 0; t2 < NB + NG; ++t2) tmp[t2] = __hip_atomic_load(&pc[t2 * 64 + lane], BPMF_RLX_AGENT);
#pragma unroll
                for (int t2 = 0; t2 < NB; ++t2) acc[t2] += tmp[t2];
#pragma unroll
                for (int t2 = 0; t2 < NG; ++t2) rr[t2] += tmp[NB + t2];
            }
        }
        wait_params(a);
        finish_single<K>(a, col, lds, lane, mc < 0,
                         [&](double *sA, double *sb, int LD, int ln) { assemble44<K>(acc, rr, sA, sb, LD, ln); });
    }
}

template <int K>
__global__ __launch_bounds__(64, Geo1<K>::WPS) void k_sample1(SampleArgs a, FusedArgs f)
{
    __shared__ __attribute__((aligned(16))) double lds[Geo1<K>::LDS_WORDS];
    sample1_body<K, true>(a, f, lds);
}

// the index-block form
template <int K>
__global__ __launch_bounds__(64, Geo1<K>::WPS) void k_sample1i(SampleArgs a, FusedArgs f)
{
    __shared__ __attribute__((aligned(16))) double lds[Geo1<K>::LDS_WORDS];
    sample1_body<K, false>(a, f, lds);
}

// the index-block form with per-rating weights
template <int K>
__global__ __launch_bounds__(64, Geo1<K>::WPS) void k_sample1w(SampleArgs a, FusedArgs f)
{
    __shared__ __attribute__((aligned(16))) double lds[Geo1<K>::LDS_WORDS];
    sample1_body<K, false, true>(a, f, lds);
}

// ---------------------------------------------------------------------------
// sum x, sum x x^T over the columns [c0, c1) of `items` (thread_vector reducers,
// c++/sample.cpp:345-347,359-362,379-381).  Wave w takes a contiguous slice and
// writes a partial in accumulator layout; the last waves to arrive add the partials
// in wave order and unpacks to column-major prod | sum | norm.
// ---------------------------------------------------------------------------
// After its partial a wave takes a ticket; the last NFIN arrivers wait until every partial is
// written and then each adds up slices of 16 outputs over all partials (4 lane groups split the
// partials, combined in a fixed order), straight into `out`:
//     prod[K*K] col-major | sum[K] | (unused) | fail word
// and the last of those publishes `seq` to `flag` (the word a host thread spins on).  One kernel
// instead of two: the whole statistics pass is dispatched in the few microseconds before the next
// sampler floods the chip with workgroups, and its result is independent of the arrival order.
// Hand-off idiom of this file (see k_sample): data another workgroup will read is written with
// relaxed device-scope atomic stores (write-through, no cache flush), the writer waits for them
// (s_waitcnt vmcnt(0)) and only then bumps a relaxed device-scope counter; readers use relaxed
// device-scope atomic loads.  A release / acquire FENCE instead would write back and invalidate
// the whole L2 once per workgroup.  Results for the host go out as system-scope relaxed stores to
// pinned memory, the sequence number last.
#define BPMF_RLX_SYSTEM __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM
__device__ __forceinline__ void publish_when_last(unsigned *ticket, unsigned nblocks, unsigned *flag_host, unsigned seq,
                                                  unsigned *rearm = nullptr, unsigned *rearm2 = nullptr)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // this wave's result stores have landed
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, BPMF_RLX_AGENT);
        if (t == nblocks - 1) {
            __hip_atomic_store(ticket, 0u, BPMF_RLX_AGENT);          // re-arm
            if (rearm) __hip_atomic_store(rearm, 0u, BPMF_RLX_AGENT);
            if (rearm2) __hip_atomic_store(rearm2, 0u, BPMF_RLX_AGENT);
            __hip_atomic_store(flag_host, seq, BPMF_RLX_SYSTEM);
        }
    }
}

// sum x x^T (upper 16 x 16 tiles, accumulator layout of the f64 16x16x4 MFMA) and sum x of the columns [b, e): one wave
// (list != NULL: positions [b, e) of a list of LOCAL column ids, column = c0 + list[position]; the ids of a trip are
//  requested two trips ahead, its columns one trip ahead)
// K = 64 (kColstatsRot): the products run on the 4x4x4 shape in rotated-block accumulators (rot44_contract: 36 instructions of
// ~18 cycles per four columns instead of 10 of ~104) and are brought into the tile layout once at the end, through `img`:
// 512 doubles of LDS that belong to this wave (every wave of the workgroup has to make the call: rot44_images has barriers).
template <int K>
constexpr bool kColstatsRot = (K == 64);

template <int K>
__device__ __forceinline__ void colstats_accumulate(const double *__restrict__ items, int64_t b, int64_t e,
                                                    d4 (&acc)[Geo<K>::NTRI], double (&r)[Geo<K>::NT], int lane, double *img,
                                                    const int32_t *__restrict__ list = nullptr, int64_t c0 = 0)
{
    constexpr int NT = Geo<K>::NT;
    constexpr bool ROT = kColstatsRot<K>;
    const int kq = lane >> 4, li = lane & 15;
    double C[ROT ? Rot44<K>::NACC : 1];
#pragma unroll
    for (int t = 0; t < (ROT ? Rot44<K>::NACC : 1); ++t) C[t] = 0.0;
#pragma unroll
    for (int t = 0; t < Geo<K>::NTRI; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < NT; ++t) r[t] = 0.0;
    // Eight columns per trip; the loads of the NEXT trip are issued before the MFMAs of the current one, and no load
    // sits inside a select (slots beyond the slice read a valid column and are zeroed afterwards): with
    // `ok ? items[..] : 0.0` every load got a branch and a wait of its own, and the pass over the 483 k columns of
    // the ChEMBL-shaped compounds side took 0.32-0.38 ms instead of the ~60 us its 247 MB need.
    double yn[2][NT];
    int64_t idn[2];                                                   // columns of the trip after the next one
    auto ids = [&](int64_t c, int64_t (&id)[2]) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int64_t pos = (c + s * 4 + kq < e) ? c + s * 4 + kq : b;
            id[s] = list ? c0 + (int64_t)list[pos] : pos;
        }
    };
    auto fetch = [&](const int64_t (&id)[2], double (&yy)[2][NT]) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double *x = items + (size_t)id[s] * K;
#pragma unroll
            for (int t = 0; t < NT; ++t) yy[s][t] = x[(t * 16 + li < K) ? t * 16 + li : 0];
        }
    };
    if (b < e) {
        int64_t id0[2];
        ids(b, id0);
        fetch(id0, yn);
        ids((b + 8 < e) ? b + 8 : b, idn);
    }
    for (int64_t c = b; c < e; c += 8) {
        double y[2][NT];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bool ok = c + s * 4 + kq < e;
#pragma unroll
            for (int t = 0; t < NT; ++t) y[s][t] = (ok && (t * 16 + li < K)) ? yn[s][t] : 0.0;
        }
        fetch(idn, yn);                                               // (beyond the end: position b again, dropped by `ok`)
        ids((c + 16 < e) ? c + 16 : b, idn);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int t = 0; t < NT; ++t) r[t] += y[s][t];
            if constexpr (ROT) {
                rot44_contract<K>(y[s], C);
            } else {
                int tri = 0;
#pragma unroll
                for (int I = 0; I < NT; ++I)
#pragma unroll
                    for (int J = I; J < NT; ++J, ++tri) acc[tri] = mfma16(y[s][I], y[s][J], acc[tri]);
            }
        }
    }
    if constexpr (ROT) rot44_images<K>(C, img, img + 256, lane, [&](int tix, int, int, int m, double v) { acc[tix][m] = v; });
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        r[t] += __shfl_xor(r[t], 16);
        r[t] += __shfl_xor(r[t], 32);
    }
}

template <int K>
__device__ __forceinline__ void colstats_body(int w, const double *__restrict__ items, int64_t c0, int64_t c1, int nwaves,
                                              double *partials, const unsigned long long *__restrict__ fail_in,
                                              double *__restrict__ out, unsigned *ticket, unsigned *flag, unsigned seq,
                                              unsigned long long *tmo, unsigned long long wait_ticks, double *img)
{
    // img: kColstatsRot<K> ? 512 doubles of the (single-wave) workgroup's LDS : unused
    constexpr int NT = Geo<K>::NT, NTRI = Geo<K>::NTRI, PART = Geo<K>::PART;
    constexpr int NSUMS = blob::res_sums(K), NSLICE = (NSUMS + 15) / 16, FAILD = blob::res_failD(K), FAIL = blob::res_fail(K);
    const int lane = threadIdx.x;
    const int64_t n = c1 - c0;
    const int64_t per = (((n + nwaves - 1) / nwaves) + 3) & ~(int64_t)3;
    const int64_t b = c0 + w * per;
    const int64_t e = (b + per < c1) ? b + per : c1;

    {
        d4 acc[NTRI];
        double r[NT];
        colstats_accumulate<K>(items, b, e, acc, r, lane, img);
        double *p = partials + (size_t)w * PART;
#pragma unroll
        for (int t = 0; t < NTRI; ++t)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) __hip_atomic_store(&p[(t * 4 + reg) * 64 + lane], acc[t][reg], BPMF_RLX_AGENT);
        if (lane < 16) {
#pragma unroll
            for (int t = 0; t < NT; ++t) __hip_atomic_store(&p[NTRI * 256 + t * 16 + lane], r[t], BPMF_RLX_AGENT);
        }
    }

    // arrival: the partial has landed before the ticket is taken
    const int nfin = nwaves < NSLICE ? nwaves : NSLICE;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned tk = 0;
    if (lane == 0) tk = __hip_atomic_fetch_add(ticket, 1u, BPMF_RLX_AGENT);
    tk = __builtin_amdgcn_readfirstlane(tk);
    if ((int)tk < nwaves - nfin) return;
    const int f = (int)tk - (nwaves - nfin);                          // finisher 0 .. nfin-1
    // every wave takes its ticket before it waits, so the count reaches nwaves as soon as all
    // waves have run (those not yet resident get the slots the samplers' workgroups free): at most
    // NSLICE <= 66 (K = 32) / 260 (K = 64) waves ever wait, fewer than the wave slots of a single XCD.
    // Bounded all the same (a co-tenant holding every other slot): the sums published after a
    // time-out are incomplete, the sticky word says so and the host discards them.
    if (lane == 0) {
        const unsigned long long t0 = wall_clock64();
        while (__hip_atomic_load(ticket, BPMF_RLX_AGENT) < (unsigned)nwaves) {
            __builtin_amdgcn_s_sleep(1);
            if (wait_ticks && wall_clock64() - t0 > wait_ticks) { flag_timeout(tmo, BPMF_TMO_STATS); break; }
        }
    }
    __syncthreads();

    const int o = lane & 15, grp = lane >> 4;
    for (int slice = f; slice < NSLICE; slice += nfin) {
        const int eo = slice * 16 + o;
        double s = 0.0;
        if (eo < NSUMS) {
            int off;
            if (eo < K * K) {
                int i = eo % K, j = eo / K;
                if (i > j) { const int t = i; i = j; j = t; }      // symmetric: read the upper tile
                const int I = i >> 4, J = j >> 4;
                const int tri = I * NT - (I * (I - 1)) / 2 + (J - I);
                const int ii = i & 15, jj = j & 15;
                off = (tri * 4 + (ii >> 2)) * 64 + (ii & 3) * 16 + jj;
            } else {
                off = NTRI * 256 + (eo - K * K);
            }
            const int pw = (nwaves + 3) >> 2;
            const int w0 = grp * pw, w1 = (w0 + pw < nwaves) ? w0 + pw : nwaves;
            double acc[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) acc[u] = 0.0;
            for (int ww = w0; ww < w1; ww += 16) {
                // (sixteen loads in flight: none of them inside a select -- beyond the end they re-read partial w0 and are
                //  dropped afterwards; with `(ww + u < w1) ? load : 0` every load got a branch and a wait of its own and the
                //  finishers of a 2 048-wave pass took 0.6 ms)
                double v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u)
                    v[u] = __hip_atomic_load(&partials[(size_t)((ww + u < w1) ? ww + u : w0) * PART + off], BPMF_RLX_AGENT);
#pragma unroll
                for (int u = 0; u < 16; ++u) acc[u] += (ww + u < w1) ? v[u] : 0.0;
            }
#pragma unroll
            for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
                for (int u = 0; u < h; ++u) acc[u] += acc[u + h];
            s = acc[0];
        }
        s += __shfl_xor(s, 16);                                      // (g0 + g1), (g2 + g3)
        s += __shfl_xor(s, 32);                                      // fixed order: ((g0 + g1) + (g2 + g3))
        if (grp == 0 && eo < NSUMS) __hip_atomic_store(&out[eo], s, BPMF_RLX_SYSTEM);
    }
    if (f == 0 && lane == 0) {
        // failed column: as the u64 word of the blob, and as a double (0 = none, id + 1 otherwise)
        // that survives a SUM all-reduce of the blob over the ranks
        // (device-scope load: as riders of a fused launch the pass runs beside items that may lower the word on another XCD)
        const unsigned long long fw = __hip_atomic_load(fail_in, BPMF_RLX_AGENT);
        __hip_atomic_store(&out[FAILD], (fw == ~0ull) ? 0.0 : (double)(fw + 1ull), BPMF_RLX_SYSTEM);
        __hip_atomic_store(&reinterpret_cast<unsigned long long *>(out)[FAIL], fw, BPMF_RLX_SYSTEM);
    }
    publish_when_last(ticket + 1, (unsigned)nfin, flag, seq, ticket);
}

template <int K>
__global__ __launch_bounds__(64) void k_colstats(const double *__restrict__ items, int64_t c0, int64_t c1, int nwaves,
                                                 double *partials, const unsigned long long *__restrict__ fail_in,
                                                 double *__restrict__ out, unsigned *ticket, unsigned *flag, unsigned seq,
                                                 unsigned long long *tmo, unsigned long long wait_ticks)
{
    __shared__ double img[kColstatsRot<K> ? 512 : 1];
    colstats_body<K>((int)blockIdx.x, items, c0, c1, nwaves, partials, fail_in, out, ticket, flag, seq, tmo, wait_ticks, img);
}

// ---------------------------------------------------------------------------
// Sys::predict (c++/sample.cpp:48-96): one lane per test rating; each lane walks its two
// K-vectors with 16-byte loads (a 128-B line is consumed by one lane in 8 consecutive loads).
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// Column statistics of a BIG side (hundreds of thousands of columns; stand-alone launches only).  k_colstats' 2 048
// single-wave workgroups each leave a partial of PART doubles and 260 finisher waves then read those partials in
// 128-byte pieces 21 KB apart: 68 MB of page-missing reads -- 0.65 ms for the 483 k compounds of the ChEMBL shape,
// whatever ran beside it.  Here: workgroups of four waves that add their accumulators through LDS (a quarter of the
// partials), and finishers that walk the partials in THEIR order -- 512 contiguous bytes per partial and wave, sixteen
// loads in flight, four waves splitting the partials -- and scatter the few sums into the result.
// Order of every sum fixed: waves 0..3 of a workgroup, then the workgroups in quarters, ascending.
// ---------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void k_colstats_wg(const double *__restrict__ items, int64_t c0, int64_t c1, int nwg,
                                                    double *partials, const unsigned long long *__restrict__ fail_in,
                                                    double *__restrict__ out, unsigned *ticket, unsigned *flag, unsigned seq,
                                                    unsigned long long *tmo, unsigned long long wait_ticks,
                                                    const int32_t *__restrict__ list, int part0, int ntot, int finish)
{
    // list == NULL: the columns [c0, c1).  Else: positions [c0 .. c1) of `list` (local column ids; the side's first column is
    // items' column `from` = part of the pointer: `items` already points at local column 0).  This launch's workgroups write
    // the partials part0 .. part0 + nwg - 1; with `finish` its last arrivals add all `ntot` partials (those of earlier
    // launches on the same stream included) and publish, without it the launch only leaves its partials.
    constexpr int NT = Geo<K>::NT, NTRI = Geo<K>::NTRI, PART = Geo<K>::PART, NBLK = (PART + 63) / 64, FAILD = blob::res_failD(K), FAIL = blob::res_fail(K);
    __shared__ double red[PART];
    __shared__ double fin[4][64];
    __shared__ unsigned stk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t n = c1 - c0;
    const int nvw = nwg * 4, vw = (int)blockIdx.x * 4 + wave;
    const int64_t per = (((n + nvw - 1) / nvw) + 3) & ~(int64_t)3;
    const int64_t b = c0 + vw * per;
    const int64_t e = (b + per < c1) ? b + per : c1;
    {
        d4 acc[NTRI];
        double r[NT];
        static_assert(!kColstatsRot<K> || 4 * 512 <= PART, "the four waves' images fit the reduction buffer");
        colstats_accumulate<K>(items, b, e, acc, r, lane, red + 512 * wave, list, 0);   // (list mode: `items` points at local column 0)
        if (kColstatsRot<K>) __syncthreads();                         // (the images are read before `red` takes the sums)
        // waves 1, 2, 3 hand their sums to wave 0 through LDS, one after the other
        for (int src = 1; src < 4; ++src) {
            if (wave == src) {
#pragma unroll
                for (int t = 0; t < NTRI; ++t)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) red[(t * 4 + reg) * 64 + lane] = acc[t][reg];
                if (lane < 16) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) red[NTRI * 256 + t * 16 + lane] = r[t];
                }
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int t = 0; t < NTRI; ++t)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) acc[t][reg] += red[(t * 4 + reg) * 64 + lane];
#pragma unroll
                for (int t = 0; t < NT; ++t) r[t] += red[NTRI * 256 + t * 16 + (lane & 15)];
            }
            __syncthreads();
        }
        if (wave == 0) {
            double *p = partials + (size_t)(part0 + (int)blockIdx.x) * PART;
#pragma unroll
            for (int t = 0; t < NTRI; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) __hip_atomic_store(&p[(t * 4 + reg) * 64 + lane], acc[t][reg], BPMF_RLX_AGENT);
            if (lane < 16) {
#pragma unroll
                for (int t = 0; t < NT; ++t) __hip_atomic_store(&p[NTRI * 256 + t * 16 + lane], r[t], BPMF_RLX_AGENT);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the partial has landed before the ticket is taken
        }
    }
    if (!finish) return;
    const int nfin = nwg < NBLK ? nwg : NBLK;
    if (tid == 0) stk = __hip_atomic_fetch_add(ticket, 1u, BPMF_RLX_AGENT);
    __syncthreads();
    const unsigned tk = stk;
    if ((int)tk < nwg - nfin) return;                                 // (the whole workgroup)
    const int f = (int)tk - (nwg - nfin);                             // finisher 0 .. nfin-1
    if (tid == 0) {                                                   // bounded like every in-kernel wait (see colstats_body)
        const unsigned long long t0 = wall_clock64();
        while (__hip_atomic_load(ticket, BPMF_RLX_AGENT) < (unsigned)nwg) {
            __builtin_amdgcn_s_sleep(1);
            if (wait_ticks && wall_clock64() - t0 > wait_ticks) { flag_timeout(tmo, BPMF_TMO_STATS); break; }
        }
    }
    __syncthreads();
    const int pw = (ntot + 3) >> 2;
    const int w0 = wave * pw, w1 = (w0 + pw < ntot) ? w0 + pw : ntot;
    for (int blk = f; blk < NBLK; blk += nfin) {
        const int po = blk * 64 + lane;                               // position in the partial
        const int pc = po < PART ? po : 0;
        double acc[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u] = 0.0;
        for (int ww = w0; ww < w1; ww += 16) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                v[u] = __hip_atomic_load(&partials[(size_t)((ww + u < w1) ? ww + u : w0) * PART + pc], BPMF_RLX_AGENT);
#pragma unroll
            for (int u = 0; u < 16; ++u) acc[u] += (ww + u < w1) ? v[u] : 0.0;
        }
#pragma unroll
        for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
            for (int u = 0; u < h; ++u) acc[u] += acc[u + h];
        fin[wave][lane] = acc[0];
        __syncthreads();
        if (wave == 0 && po < PART) {
            const double sum = ((fin[0][lane] + fin[1][lane]) + fin[2][lane]) + fin[3][lane];
            if (po < NTRI * 256) {                                    // tile `tri`, register reg, lane ln of the accumulator layout
                const int tri = po >> 8, reg = (po >> 6) & 3, ln = po & 63;
                int I = 0, t = tri;
                while (t >= NT - I) { t -= NT - I; ++I; }
                const int J = I + t;
                const int gi = 16 * I + (ln >> 4) + 4 * reg, gj = 16 * J + (ln & 15);
                if (gi < K && gj < K) {
                    __hip_atomic_store(&out[gi + (size_t)gj * K], sum, BPMF_RLX_SYSTEM);
                    if (I != J) __hip_atomic_store(&out[gj + (size_t)gi * K], sum, BPMF_RLX_SYSTEM);
                }
            } else {
                const int el = po - NTRI * 256;
                if (el < K) __hip_atomic_store(&out[K * K + el], sum, BPMF_RLX_SYSTEM);
            }
        }
        __syncthreads();
    }
    if (f == 0 && tid == 0) {
        const unsigned long long fw = *fail_in;
        __hip_atomic_store(&out[FAILD], (fw == ~0ull) ? 0.0 : (double)(fw + 1ull), BPMF_RLX_SYSTEM);
        __hip_atomic_store(&reinterpret_cast<unsigned long long *>(out)[FAIL], fw, BPMF_RLX_SYSTEM);
    }
    publish_when_last(ticket + 1, (unsigned)nfin, flag, seq, ticket);
}

// NT: threads per workgroup.  256 by default; 64 (single-wave workgroups) for small test sets: beside a sampler launch that
// keeps refilling every wave slot with single-wave workgroups a four-wave workgroup only gets in when the launch drains.
template <int K, int NT = 256, typename T = double>
__global__ __launch_bounds__(NT) void k_predict(const int32_t *__restrict__ tcol, const int32_t *__restrict__ trow,
                                                 const double *__restrict__ tval, int64_t nnz,
                                                 const T *__restrict__ items, const T *__restrict__ other,
                                                 int64_t col_from, double mean, int n, double *__restrict__ pavg,
                                                 double *__restrict__ pm2, double *partial, double *__restrict__ out,
                                                 unsigned *ticket, unsigned *flag, unsigned seq, TwinArgs tw)
{
    __shared__ double red[4][NT / 64];
    __shared__ double fin[4][NT];
    __shared__ unsigned last;
    auto wsum = [](const double (&r)[NT / 64]) { if constexpr (NT == 256) return (r[0] + r[1]) + (r[2] + r[3]); else return r[0]; };
    const int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x;
    double se = 0.0, se_avg = 0.0, se_t = 0.0, se_avg_t = 0.0;
    if (q < nnz) {
        double d0 = 0.0, d1 = 0.0;
        if constexpr (sizeof(T) == 4) {                             // fp32 factors (K = 128 opt-in): fp64 accumulation, the order of k_predict_f32
            const float4 *m = reinterpret_cast<const float4 *>(items + (size_t)(col_from + tcol[q]) * K);
            const float4 *u = reinterpret_cast<const float4 *>(other + (size_t)trow[q] * K);
#pragma unroll 8
            for (int t = 0; t < K / 4; ++t) {
                const float4 x = m[t], y = u[t];
                d0 = fma((double)x.x, (double)y.x, d0);
                d1 = fma((double)x.y, (double)y.y, d1);
                d0 = fma((double)x.z, (double)y.z, d0);
                d1 = fma((double)x.w, (double)y.w, d1);
            }
        } else {
            const double2 *m = reinterpret_cast<const double2 *>(items + (size_t)(col_from + tcol[q]) * K);
            const double2 *u = reinterpret_cast<const double2 *>(other + (size_t)trow[q] * K);
#pragma unroll
            for (int t = 0; t < K / 2; ++t) {
                const double2 a = m[t], b = u[t];
                d0 = fma(a.x, b.x, d0);
                d1 = fma(a.y, b.y, d1);
            }
        }
        const double pred = (d0 + d1) + mean;                       // :78
        const double v = tval[q];
        se = (v - pred) * (v - pred);
        double avg = pavg[q];
        const double delta = pred - avg;
        avg = (n == 0) ? pred : (avg + delta / n);                  // :84 (n, not n+1: reference quirk)
        pavg[q] = avg;
        pm2[q] = (n == 0) ? 0.0 : pm2[q] + delta * (pred - avg);    // :86
        se_avg = (v - avg) * (v - avg);
        if (tw.perm) {
            // users.predict(movies), c++/bpmf.cpp:190: the same dot product (the two sides' roles swapped), plus THAT
            // side's mean, into ITS copy of the entry (Pavg / Pm2 of the second Sys, c++/sample.cpp:132-137)
            const int qt = tw.perm[q];
            const double pred_t = (d0 + d1) + tw.mean;
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
        // the last block to arrive adds the block partials up (fixed-shape tree: the result does
        // not depend on which block that is) and publishes the two sums
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, BPMF_RLX_AGENT);
        last = (t == gridDim.x - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    {
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
            __hip_atomic_store(ticket, 0u, BPMF_RLX_AGENT);          // re-arm
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(flag, seq, BPMF_RLX_SYSTEM);
            if (tw.perm) __hip_atomic_store(tw.flag, tw.seq, BPMF_RLX_SYSTEM);
        }
    }
}

// Connectivity-aware exchange: the columns a peer reads are packed into one contiguous buffer
// (and scattered back on the receiving side), one 16-byte piece per thread -- a column is K / 2
// consecutive pieces, so a wave moves whole 128-byte lines on both sides.
template <int K>
__global__ __launch_bounds__(256) void k_pack_cols(const double *__restrict__ items, const int32_t *__restrict__ cols, int64_t n,
                                                   double *__restrict__ buf)
{
    typedef double dd2 __attribute__((ext_vector_type(2)));
    constexpr int P = K / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * P) return;
    const int64_t c = i / P;
    const int piece = (int)(i % P);
    reinterpret_cast<dd2 *>(buf)[i] = reinterpret_cast<const dd2 *>(items + (size_t)cols[c] * K)[piece];
}

template <int K>
__global__ __launch_bounds__(256) void k_unpack_cols(const double *__restrict__ buf, const int32_t *__restrict__ cols, int64_t n,
                                                     double *__restrict__ items)
{
    typedef double dd2 __attribute__((ext_vector_type(2)));
    constexpr int P = K / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * P) return;
    const int64_t c = i / P;
    const int piece = (int)(i % P);
    reinterpret_cast<dd2 *>(items + (size_t)cols[c] * K)[piece] = reinterpret_cast<const dd2 *>(buf)[i];
}


// Gate + staging of the stateful path.  The kernel is queued ahead of a sampler whose
// hyper-parameters the host may still be computing: one lane polls a word in pinned host memory
// until the host has stored `want` there (release; after it wrote the parameter blob), then the
// block copies the blob into device memory.  The poll gives up after `wait_ticks` of wall clock
// (default 20 s; host gone or descheduled): it then sets the side's sticky time-out word, the sampler
// behind it runs on whatever the blob holds, and the host side discards that half-iteration with
// BPMF_HIP_ENODEV "device wait timed out" (collect() in capi_sample.hip).
__device__ __forceinline__ void gate_stage_body(int block, int nblocks, const unsigned *gate_host, unsigned want, const double *src_host,
                                                double *__restrict__ dst, int n, unsigned *dflag, unsigned dval,
                                                unsigned long long *tmo, unsigned long long wait_ticks)
{
    const int lane = threadIdx.x;
    if (lane == 0) {
        const unsigned long long t0 = wall_clock64();                 // 100 MHz
        // Relaxed polls, ONE acquire once the word is there; the first sixteen polls back to back (a gate that opens just after
        // the launch started: the fused forms), then ~ 3.4 us apart (s_sleep 127).  A gate kernel polls beside the partner's
        // sampler for hundreds of microseconds (K = 128: ~ 300 us per half-iteration, 16 waves): at one uncached system-scope read
        // per ~ 0.3 us and wave those launches ran 1.2 % longer (FINDINGS section 25; the `buffer_inv sc0 sc1` an acquiring load
        // drags along made no difference of its own).
        int polls = 0;
        while (__hip_atomic_load(gate_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != want) {
            if (polls < 16) { __builtin_amdgcn_s_sleep(4); ++polls; }
            else __builtin_amdgcn_s_sleep(127);
            if (wall_clock64() - t0 > wait_ticks) { flag_timeout(tmo, BPMF_TMO_GATE); break; }
        }
        (void)__hip_atomic_load(gate_host, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
    // uncached host memory, read after the acquire: 16-byte PCIe reads, four in flight per lane
    // (one wave only: it is launched beside a sampler that fills the chip with single-wave workgroups).  n is even.
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2 *src = reinterpret_cast<const d2 *>(src_host);
    d2 *out = reinterpret_cast<d2 *>(dst);
    const int n2 = n >> 1;
    // (big blobs, K = 128: several blocks, each polls the gate and copies every gridDim.x-th slab)
    for (int base = block * 256; base < n2; base += 256 * nblocks) {
        d2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * 64 + lane;
            v[u] = (i < n2) ? __builtin_nontemporal_load(src + i) : d2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * 64 + lane;
            if (i < n2) {
                if (dflag) {                                          // readers poll dflag inside a running launch: write through
                    __hip_atomic_store(dst + 2 * i, v[u].x, BPMF_RLX_AGENT);
                    __hip_atomic_store(dst + 2 * i + 1, v[u].y, BPMF_RLX_AGENT);
                } else {
                    out[i] = v[u];
                }
            }
        }
    }
    if (dflag) {                                                      // (one block in this form)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (lane == 0) __hip_atomic_store(dflag, dval, BPMF_RLX_AGENT);
    }
}



}  // namespace bpmf
