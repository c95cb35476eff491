// ext_state.h -- what the add-ons of a side own on the device (included by state.h): bpmf_hip_side holds one owning pointer per
// add-on, NULL while the side has none; everything below is released when that pointer is reset.  The five add-ons with a latent
// step (probit, ordinal, censored, robust, bias) derive from bpmf_latent; state.h tells which of them a side is.
#pragma once
#include <limits>
#include <memory>
#include <vector>

#include "devbuf.h"

namespace bpmf { struct CgState; }

namespace bpmf_launch {

// A matrix compressed by rows on the device (F by rows, or F^T by rows = F by columns).  Rows of more than kSpChunk nonzeros are
// "long": cut into chunks whose partial sums are added in chunk order.  (link_sparse.h: sp_upload, sp_product)
struct SpMat {
    int64_t nrows = 0, nnz = 0;
    DevBuf<int64_t> ptr;
    DevBuf<int32_t> idx;
    DevBuf<double> vals;                                    // empty: every stored value is 1
    int nlong = 0; int64_t nchunks = 0;
    DevBuf<int32_t> lrow; DevBuf<int64_t> lfirst, cbeg, cend;
    DevBuf<double> part; int part_n = 0;                    // nchunks x part_n doubles
};

// the work arrays of K conjugate-gradient solves in lockstep on D x ld arrays (link_sparse.h: cg_alloc, cg_solve)
struct CgWork {
    DevBuf<double> p, q, t;                                 // D x ld, D x ld, N x ld
    DevBuf<double> partial;                                 // cg_blocks(D) x 128
    DevBuf<bpmf::CgState> state;
    Pinned<int> word;                                       // the number of active columns, written by the device
};

}  // namespace bpmf_launch

// The latent step of a side: the kernel that a probit, an ordinal, a censored or a robust side or a side with biases runs ahead of every
// one of its sampler launches (a side is at most one of the five: state.h has the kind and check_latent).  What they share: the word the kernel raises
// to a rating position it could not draw (~0: none; the kind says why), and the tag of the side's Philox streams.
struct bpmf_latent { Pinned<unsigned long long> fail; uint32_t tag = 0; };

// probit likelihood (capi_probit.hip): the latent scores (layout of d_vals; the samplers read them in its
// place) and the sign of every rating; the word is raised when a draw runs into its attempt cap
struct bpmf_probit : bpmf_latent { DevBuf<double> z; DevBuf<int8_t> sign; };

// ordinal probit likelihood (capi_ordinal.hip): the latent scores (layout of d_vals; the samplers read them in
// its place), the level 0 .. C - 1 of every rating, the C level values, the cutpoint table -inf, g_1 .. g_{C-1}, +inf on the host and
// two tables on the device (the current one and a proposal), the partials of the log-likelihood pass (2 x blocks, then the two sums);
// the word is raised at a rating whose dot product is not finite
struct bpmf_ordinal : bpmf_latent {
    DevBuf<double> z; DevBuf<uint8_t> level; DevBuf<double> g, g_prop, part;
    int nlev = 0;
    std::vector<double> levels, cut;                        // C values; C + 1 table entries
    int64_t loglik_launches = 0;                            // log-likelihood passes enqueued so far (bpmf_hip_side_ordinal_info)
};

// censored ratings (capi_censor.hip): the censored entries of the side as compact lists (position in the CSC,
// column, row, +1 = the rating is a lower bound / -1 = an upper bound) and the latent values (layout of d_vals: a copy of the ratings
// of which only the censored positions are ever rewritten; the samplers read it in place of d_vals); the word is raised when a draw
// runs into its attempt cap
struct bpmf_censor : bpmf_latent {
    DevBuf<int64_t> pos; DevBuf<int32_t> col, row; DevBuf<int8_t> sign;
    DevBuf<double> z;
    int64_t n = 0, nright = 0, nleft = 0;
};

// per-rating precision weights (capi_weights.hip): sw = sqrt(w) and zw = sqrt(w) (r - mean_rating) of every rating
// (layout of d_vals).  The weighted forms of the samplers read zw in place of d_vals with mean 0 and multiply every gathered row by sw.
struct bpmf_weights { DevBuf<double> sw, zw; int64_t nweighted = 0; double wmin = 1.0, wmax = 1.0; };

// implicit feedback (capi_implicit.hip): every cell of the matrix is observed, an unobserved one as r = 0 with
// weight w0.  The side's bpmf_weights hold sw = sqrt(w - w0) and zw = w r / sqrt(w - w0); gram: G = sum over ALL columns of the other
// side of u u^T (Kt x Kt), formed on the device ahead of every half-iteration, part: the chunk partials of that product; prior: alpha
// w0 G on the host, added to the LambdaF of the parameter blob behind Lmu.  in_call: bpmf_hip_implicit_sample is driving the
// stateless half-iteration of this side.
struct bpmf_implicit { double w0 = 0.0; bool in_call = false; DevBuf<double> gram, part; std::vector<double> prior; };

// Student-t noise (capi_robust.hip): the side's bpmf_weights are redrawn on the device ahead of every sampler
// launch.  nu: the degrees of freedom; wsum: the running sum of w over the kept samples (layout of d_vals), `kept` of them; the word
// is raised when a draw runs into its attempt cap or meets a residual that is not finite
struct bpmf_robust : bpmf_latent { double nu = 0.0; DevBuf<double> wsum; int kept = 0; };

// row and column bias terms (capi_bias.hip): one offset per column of the side, b_a ~ N(0, 1 / lambda).  b: the
// current biases; bsum: their running sum over the kept samples, `kept` of them; z: (r - b[col]) - c[row] (layout of d_vals; the
// samplers read it in place of d_vals); e, part: the residuals and the piece partials of the newest step; pieceptr: the first piece of
// every column (ncols + 1; npieces in all); lambda: the device word the draw reads its precision from (lambda_host: its value);
// role: which of the two extra ring rows carries b (0: (b, 1), 1: (1, b)).  The word is raised at a rating whose residual is not finite
struct bpmf_bias : bpmf_latent {
    DevBuf<double> b, bsum, z, e, part, lambda;
    DevBuf<int64_t> pieceptr; int64_t npieces = 0;
    double lambda_host = 1.0; int role = 0, kept = 0;
    int64_t steps = 0;                                      // bias steps enqueued so far
    // a sampled precision (bpmf_hip_side_bias_prior): lambda ~ Gamma(a0 + N / 2, b0 + sum b^2 / 2) by k_bias_lambda at the start of every
    // half-iteration of the side but its first; trace[iter] = the draw of that half-iteration (NaN where none was made), draws of them
    bool sample_lambda = false; double a0 = 0.0, b0 = 0.0;
    DevBuf<double> trace; int trace_cap = 0; int64_t draws = 0;
};

// dense features (capi_link.hip): F (ncols x D, row-major), W = [G^-1 | L_G^-T] (D x 2 D), the stacked right-hand side [P ; E] (2 D x ld)
struct bpmf_link_dense {
    DevBuf<double> F, W, PE;
    // device-factor mode (capi_link_lambda.hip; W is released): F^T F (D x D), the padded factor of
    // F^T F + fact_lambda I with its inverted diagonal blocks, the padded right-hand sides, the pivot flag
    bool devfac = false; double fact_lambda = 0.0;
    DevBuf<double> FtF, Lp, Linv, LinvT, Xp, Ep;
    DevBuf<int> flag;
};

// sparse features (capi_link_sparse.hip): F compressed both ways, the work arrays of the CG draw of beta, its
// right-hand side / residual (D x K) and R^-1 (Kt x Kt), the settings and the statistics of the solves
struct bpmf_link_sparse {
    bpmf_launch::SpMat F, Ft;
    bpmf_launch::CgWork cg;
    DevBuf<double> rhs, rinv;
    double tol = 1e-6; int max_iter = 1000;
    int iters_last = 0; int64_t iters_total = 0; double relres_max_last = 0.0; int hit_max_iter = 0;
};

// side information: beta (D x ld) and its running sum, the offsets M = F beta in the factors' layout, the
// residual ratings the samplers read in place of d_vals, staging arrays, and the features as exactly one of dense / sparse.
// in_call: bpmf_hip_link_sample is driving the stateless half-iteration of this side.
// sample_lambda: lambda is drawn at the start of every half-iteration but the side's first from Gamma(a0 + D K / 2, b0 + trace / 2)
// (DESIGN.md section 15); trace_last: the trace of the newest draw (NaN before it).
struct bpmf_link {
    int D = 0; double lambda = 0.0; uint32_t tag = 0; int nsum = 0; bool in_call = false;
    bool sample_lambda = false; double a0 = 0.0, b0 = 0.0, trace_last = std::numeric_limits<double>::quiet_NaN();
    DevBuf<double> beta, beta_sum, m, r, part, mu, btb, norm;
    std::unique_ptr<bpmf_link_dense> dense;
    std::unique_ptr<bpmf_link_sparse> sparse;
};

// posterior top-N (capi_topn.hip): ring of kept samples, fp64, column c / sample s / row k at c * max * kp + s * kp + k, and the
// sorted rated-candidate lists of every column (built on the first bpmf_hip_topn that excludes them)
struct bpmf_ring {
    DevBuf<double> samples; int max = 0, count = 0, kp = 0; DevBuf<int64_t> ex_ptr; DevBuf<int32_t> ex_rows;
    Timed cells;                             // around the newest launch of k_predict_cells with the side as the queries (bpmf_hip_predict_cells_last_ms)
    Timed sim;                               // around the newest bpmf_hip_similar of the side (bpmf_hip_similar_last_ms)
    Timed diag;                              // around the kernels of the newest bpmf_hip_diag_cells with the side as the queries (bpmf_hip_diag_last_ms)
    Timed score;                             // around the kernels of the newest bpmf_hip_score_cells with the side as the queries (bpmf_hip_score_last_ms)
    Timed interval;                          // around the kernels of the newest bpmf_hip_interval_cells with the side as the queries (bpmf_hip_interval_last_ms)
    Timed loo;                               // around the kernels of the newest bpmf_hip_loo_cells with the side as the queries (bpmf_hip_loo_last_ms)
};

// rows unseen in training (capi_newrows.hip): the features of n new entities of a side with features, as
// exactly one of dense (n x D, row-major) / sparse; the ring of their projected factors E[i, s, :] = mu_s + beta_s^T f_i (layout
// of bpmf_ring); w[c] = sum_s v_s(c)^T Lambda_s^-1 v_s(c) over the columns of the other side (nw of them; divided by the count
// when read); Y = V R^-1 of the newest sample (nw x kp), R^-1 and mu of it, and two pinned halves (R^-1 | mu) the copies to them
// are made from in turn, each with the event that says its last copy is done
struct bpmf_newrows {
    int64_t n = 0, nw = 0; int D = 0, max = 0, count = 0, kp = 0;
    DevBuf<double> F; std::unique_ptr<bpmf_launch::SpMat> sp;
    DevBuf<double> ring, w, y, rinv, mu;
    Pinned<double> stage; Event staged[2];
};

// fold-in (capi_foldin.hip): the hyper ring of the side -- alpha_s, mu_s (kt), Lambda_s (kt x kt) and Lambda_s mu_s
// (kt) of every kept sample, held on the host (kilobytes per sample) and uploaded by the fold-in that reads it -- and the newest
// set of folded-in rows: their ratings by rows (the exclusion lists of their ranking), the ring of their draws (n x S x kp, layout of
// bpmf_ring), the word the kernel raises to a row whose pivot was not positive and finite, and two events around the launch
struct bpmf_foldin {
    int hmax = 0, hcount = 0;
    std::vector<double> alpha, mu, lam, lmu;
    int64_t n = 0; int S = 0, kp = 0;
    DevBuf<int64_t> rowptr; DevBuf<int32_t> colidx; DevBuf<double> ring;
    Pinned<unsigned long long> fail;
    Timed timed;                            // around the newest launch of k_foldin (bpmf_hip_foldin_last_ms)
};

// adaptive noise (capi_noise.hip): the block partials | sum of bpmf_hip_train_sse
struct bpmf_sse { DevBuf<double> part; int nblk = 0; };
