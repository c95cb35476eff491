// blob.h -- the three small blobs of doubles a half-iteration talks to the device through, defined once: offsets and sizes
// as functions of the instantiated num_latent K (constexpr: the template parameter in the kernels -- bind them to constexpr
// locals there, so that no call is left for the optimiser to fold -- and the run-time c->K on the
// host; constexpr functions are host + device functions to hipcc), typed accessors for the words that are not doubles.  No state.
#pragma once

namespace bpmf {
namespace blob {

// Parameter blob (host -> device, staged as 16-byte words by k_stage / k_gate_stage, hence the pad word: mu starts even)
//     LambdaF [K*K] | Lmu = LambdaF mu [K] | fail (u64) | pad | mu [K]
// fail: the smallest global column id whose factorisation failed, lowered by the samplers (~0: none); mu itself is what the
// propagated-posterior columns need.  K = 64, fp64 only, behind it the tail of the product form (k_sample_pf):
//     R0 = chol(LambdaF).matrixU() row-major [K*K] | S0t = (R0^-1)^T [K*K] | y0 = R0^-T Lmu [K]
// The slab form of K = 64 stages the blob without that tail.  fp32 context: LambdaF once more as fp32 tiles (k_lf32_tiles),
// par_lf32_words doubles behind the device copy of the whole blob (at the context's in_words).
constexpr int par_LambdaF(int) { return 0; }
constexpr int par_Lmu(int K) { return K * K; }
constexpr int par_fail(int K) { return K * K + K; }
constexpr int par_mu(int K) { return K * K + K + 2; }
constexpr int par_words(int K) { return par_mu(K) + K; }              // without the tail of the product form
constexpr int par_R0(int K) { return par_words(K); }
constexpr int par_S0t(int K) { return par_R0(K) + K * K; }
constexpr int par_y0(int K) { return par_S0t(K) + K * K; }
constexpr int par_words_pf(int K) { return par_y0(K) + K; }           // with it
constexpr int par_lf32_words(int K) { return (K / 16) * (K / 16 + 1) / 2 * 256 / 2; }

// Result blob (device -> pinned host memory, written by the statistics pass of a side)
//     prod = sum x x^T [K*K] | sum = sum x [K] | failD | fail (u64) | tmo (u64) | - | flag (u32)
// failD: the fail word as a double, 0 = none, column id + 1 otherwise -- the form that survives the SUM all-reduce of
// prod | sum | failD over the ranks (res_reduced_words).  tmo: sticky, non-zero once a bounded in-kernel wait gave up
// (kTimeoutWhat in state.h).  flag: the sequence number of the pass, published behind everything else: the last word.
constexpr int res_prod(int) { return 0; }
constexpr int res_sum(int K) { return K * K; }
constexpr int res_sums(int K) { return K * K + K; }                   // number of sums: prod | sum
constexpr int res_failD(int K) { return res_sums(K); }
constexpr int res_fail(int K) { return res_sums(K) + 1; }
constexpr int res_tmo(int K) { return res_sums(K) + 2; }
constexpr int res_flag(int K) { return res_sums(K) + 4; }
constexpr int res_words(int K) { return res_flag(K) + 1; }
constexpr int res_reduced_words(int K) { return res_failD(K) + 1; }

// Reduction blob (device: d_red of the context, a_d_red of a side): what is all-reduced in place before it is published
//     result blob | se | se_avg of an evaluation | the same of its twin | number of test entries (i64) | 3 spare words
constexpr int red_eval(int K) { return res_words(K); }
constexpr int red_twin(int K) { return res_words(K) + 2; }
constexpr int red_count(int K) { return res_words(K) + 4; }
constexpr int red_words(int K) { return res_words(K) + 8; }

// one partial (tiles | sum) of the K = 128 statistics pass is allocated as this many doubles (k_colstats_f32 uses fewer)
constexpr int stat_partial_words(int K) { return K * K + K; }

// the words that are not doubles (host or device pointer: address arithmetic only)
inline unsigned long long *par_fail_word(double *par, int K) { return reinterpret_cast<unsigned long long *>(par + par_fail(K)); }
inline const unsigned long long *par_fail_word(const double *par, int K) { return reinterpret_cast<const unsigned long long *>(par + par_fail(K)); }
inline unsigned long long *res_fail_word(double *res, int K) { return reinterpret_cast<unsigned long long *>(res + res_fail(K)); }
inline unsigned long long *tmo_word(double *res, int K) { return reinterpret_cast<unsigned long long *>(res + res_tmo(K)); }
inline unsigned *res_flag_word(double *res, int K) { return reinterpret_cast<unsigned *>(res + res_flag(K)); }

static_assert(par_fail(32) == 1056 && par_mu(32) == 1058 && par_words(32) == 1090, "parameter blob moved");
static_assert(par_words(64) % 2 == 0 && par_words_pf(64) % 2 == 0, "the parameter blob is staged as 16-byte words");
static_assert(par_R0(64) == 4226 && par_S0t(64) == 8322 && par_y0(64) == 12418 && par_words_pf(64) == 12482, "product-form tail moved");
static_assert(par_lf32_words(128) == 4608, "fp32 tiles of LambdaF");
static_assert(res_sum(32) == 1024 && res_failD(32) == 1056 && res_fail(32) == 1057 && res_tmo(32) == 1058, "result blob moved");
static_assert(res_flag(32) == 1060 && res_words(32) == 32 * 32 + 32 + 5 && res_reduced_words(32) == 1057, "result blob moved");
static_assert(red_eval(32) == 1061 && red_twin(32) == 1063 && red_count(32) == 1065 && red_words(32) == 1069, "reduction blob moved");

}  // namespace blob
}  // namespace bpmf
