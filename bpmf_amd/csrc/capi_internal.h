// capi_internal.h -- what the translation units of the C ABI (capi_*.hip) share: the host-side helpers that cross the files.
// Round 6 cut the former capi.hip (2 400 lines) into
//   capi_context.hip   errors, RCCL entry points, host trace, bounded waits, context create / destroy / sync, normal stream
//   capi_side.hip      static work schedule, side create / destroy, factor storage, priors, launch reports; what the add-ons share: the
//                      table of their mutual refusals (refuse) and the wait-check-copy of a latent step's read-back (latent_read_back)
//   capi_sample.hip    sampler launches, stateless half-iteration, posterior aggregation, the stateful pipeline (bpmf_hip_sys_sample)
//   capi_comm.hip      communicator, ranges, parts, staleness, packed connectivity exchange, BPMF_REDUCE between ranks
//   capi_eval.hip      test sets and Sys::predict
//   capi_topn.hip      sample rings and the posterior top-N ranking (bpmf_hip_topn, bpmf_hip_topn_scored, bpmf_hip_rank_eval); what every query
//                      over two rings shares: the prologue (pair_check_sides, pair_open_rings), the refusals of n and of a range, the
//                      lists of a ranking (TopnLists), the read-back (copy_back) and the *_last_ms entry points (last_ms)
//   capi_similar.hip   similar columns of one side by posterior cosine / distance over its ring (bpmf_hip_similar, bpmf_hip_similar_block)
//   capi_newrows.hip   dense blocks of predictions from two rings (bpmf_hip_predict_block); rows unseen in training (bpmf_hip_newrows_*)
//   capi_foldin.hip    the per-sample hyper-parameters of a side (hyper ring) and the fold-in of new rows from their ratings (bpmf_hip_foldin*)
//   capi_model.hip     saved models: read-back and load of a sample ring (bpmf_hip_side_samples_get / _set), predictions for a list of cells
//                      (bpmf_hip_predict_cells); what the cell lists share: their checks, their sort and their batches (CellsPlan)
//   capi_diag.hip      convergence diagnostics: split-Rhat and ESS of host traces (bpmf_hip_diag_traces) and of the predictions of a list of cells (bpmf_hip_diag_cells);
//                      the rank-normalised multi-chain forms (bpmf_hip_diag_traces_mc, bpmf_hip_diag_cells_mc)
//   capi_score.hip     model comparison: log pointwise predictive density and WAIC of a list of observed cells (bpmf_hip_score_cells); what it
//                      shares with capi_loo.hip: the refusals of a likelihood's arguments and its per-sample constants (logdens_check_args, logdens_constants)
//   capi_interval.hip  predictive intervals: the probability integral transform and quantiles of the posterior predictive mixture of a list of cells
//                      (bpmf_hip_interval_cells) and of host traces (bpmf_hip_interval_traces)
//   capi_loo.hip       PSIS-LOO cross-validation: Pareto-smoothed importance sampling of the log densities of a list of observed cells
//                      (bpmf_hip_loo_cells) and of host traces (bpmf_hip_loo_traces)
//   capi_noise.hip     training residuals and the draw of the noise precision (adaptive noise)
//   capi_probit.hip    probit likelihood: latent scores ahead of every sampler launch, predictive probabilities, AUC
//   capi_ordinal.hip   ordinal probit likelihood: latent scores between the cutpoints of their level, the Metropolis-Hastings step of the cutpoints, level probabilities
//   capi_censor.hip    censored ratings: the bounded latent values ahead of every sampler launch of a side with censored entries
//   capi_weights.hip   per-rating precision weights: sqrt(w) and sqrt(w) (r - mean) of a side, which the weighted forms of the samplers read
//   capi_implicit.hip  implicit feedback: unobserved cells as zeros of weight w0 behind the weighted samplers, the blocking half-iteration bpmf_hip_implicit_sample
//   capi_robust.hip    Student-t noise: the weights of a side redrawn on the device ahead of every sampler launch, their posterior mean
//   capi_bias.hip      row and column bias terms: the draw of a side's offsets ahead of every sampler launch, the values its samplers read, their posterior mean
//   capi_tensor.hip    sparse tensor factorisation (CP, order 3): a side per mode behind the Khatri-Rao rows of the other two, test entries
//   capi_link.hip      side information: features of a side, the link matrix beta, the blocking half-iteration bpmf_hip_link_sample
//   capi_link_sparse.hip  side information with a sparse feature matrix: beta by conjugate gradients on the device (link_sparse.h)
//   capi_link_lambda.hip  the sampled link precision lambda_beta; G(lambda_beta) factored and solved against on the device (link_lambda.h)
// Five of the add-ons (probit, ordinal, censored, robust, bias) run a latent kernel ahead of every sampler launch of their side: state.h names
// the kind of a side (likelihood), checks its fail word (check_latent) and picks the values its samplers read (sampler_values); the launch
// structs of launch.h share FactorPair / SideCsc, filled by factor_pair / side_csc below; their launchers share dispatch_k / dispatch_kt.
// The device memory of the last ten (probit, censoring, weights, Student-t noise, features, sample ring, new rows, fold-in, residual partials) is owned by the structs of ext_state.h
// and counted by bpmf_hip_live_device_bytes; the core state of a context, a side and a test set (state.h) is owned the same way -- DevBuf / Pinned / Event / Stream members
// (devbuf.h), released by `delete` -- and counted by bpmf_hip_live_core_bytes.  No file but devbuf.h allocates or releases device memory, pinned memory, events or streams.
// Everything here lives in namespace bpmf_capi with hidden visibility (-fvisibility=hidden): not part of the ABI.
#pragma once
#include <dlfcn.h>

#include <initializer_list>

#include "launch.h"

namespace bpmf_capi {

extern thread_local std::string g_err;                                 // the calling thread's last error (bpmf_hip_last_error)
extern const bool g_trace_on;                                          // BPMF_HIP_TRACE=1: host-side timeline, printed when a context dies
void trace(const char *tag, const bpmf_hip_side *s, int iter);
void trace_dump();

// bounded host-side waits (capi_context.hip): a stream / event that may carry a collective is polled with a deadline
double comm_timeout_s();
int comm_abort(bpmf_hip_ctx *c, const std::string &what);
int bounded_stream_sync(bpmf_hip_ctx *c, hipStream_t st, const char *what);
int bounded_event_sync(bpmf_hip_ctx *c, hipEvent_t ev, const char *what);
int wait_host(bpmf_hip_ctx *c);

// static work schedule of a side (capi_side.hip)
int build_schedule(bpmf_hip_side *s, const int64_t *colptr);
void free_schedule(bpmf_hip_side *s);
void pad_square(int Kt, int K, const double *src, double *dst, double diag);
void unpad_square(int Kt, int K, const double *src, double *dst);
// the index that keys the random numbers of the side's half-iteration `iter` (bpmf_hip_side_set_chain; bookkeeping keeps `iter`)
inline int key_iter(const bpmf_hip_side *s, int iter) { return iter + s->chain * BPMF_HIP_CHAIN_STRIDE; }
inline bool sharded(const bpmf_hip_side *s) { return s->from != 0 || s->to != s->ncols || !s->bounds.empty(); }
// refuses with "<who>: needs the side (both sides) whole on one GPU<tail>" when the context has a communicator or a side is a shard
int require_single_gpu(const char *who, const bpmf_hip_ctx *c, const bpmf_hip_side *a, const bpmf_hip_side *b = nullptr,
                       const char *tail = ", on a context without a communicator");
int ensure_colptr(bpmf_hip_side *s);                                   // s->d_colptr, uploaded on first use (the device is set)

// the stateful pipeline (capi_sample.hip)
int settle_async(bpmf_hip_side *s);                                    // waits until the worker is done with `s`; returns its deferred error
void predraw_stop(bpmf_hip_side *s);                                   // joins the side's pre-draw helper threads
int flush_pending_stats(bpmf_hip_ctx *c, bool on_main = false);        // statistics without a launch to ride in: a kernel of their own

// The latent step of a side (probit, ordinal, censored, robust, bias: state.h has the kind): the kernel of the half-iteration being enqueued, on
// the stream `st` its sampler goes on, ahead of it.  Each kind fills its launch struct and keeps its own refusals (capi_probit.hip,
// capi_ordinal.hip, capi_censor.hip, capi_robust.hip); latent_enqueue picks the one `self` is and does nothing on a Gaussian side.
int probit_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st);
int ordinal_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st);
int censor_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st);
int robust_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st);
int bias_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st);
int bias_pair_check(const bpmf_hip_side *self, const bpmf_hip_side *other);   // both sides of a pair carry biases, or neither does (capi_bias.hip)
inline int latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st)
{
    switch (likelihood(self)) {
    case Likelihood::probit: return probit_latent_enqueue(self, other, iter, alpha, st);
    case Likelihood::ordinal: return ordinal_latent_enqueue(self, other, iter, alpha, st);
    case Likelihood::censored: return censor_latent_enqueue(self, other, iter, alpha, st);
    case Likelihood::robust: return robust_latent_enqueue(self, other, iter, alpha, st);
    case Likelihood::bias: return bias_latent_enqueue(self, other, iter, alpha, st);
    case Likelihood::gaussian: break;
    }
    return other->bias ? bias_pair_check(self, other) : 0;
}
// the members the launch structs of the add-ons share (launch.h): the factors of the side being stepped and of its partner as the
// newest launch on S0 left them, and the side's ratings by columns (ensure_colptr has run)
inline bpmf_launch::FactorPair factor_pair(const bpmf_hip_side *self, const bpmf_hip_side *other)
{
    const bpmf_hip_ctx *c = self->ctx;
    return {self->d_items, other->d_items, c->dtype == BPMF_HIP_F32, c->K, c->Kt};
}
inline bpmf_launch::SideCsc side_csc(const bpmf_hip_side *self) { return {self->d_colptr.get(), self->ncols, self->d_rowidx, self->nnz}; }
// (capi_side.hip) waits for the side's work in flight -- its worker, then S0, reported as `func` -- and reports a raised latent word
// (check_latent: bpmf_hip_side_weights_get of a robust side); latent_read_back then copies the nnz doubles `z` to the host (the three
// *_latent entry points, bpmf_hip_side_robust_get)
int latent_settle(const char *func, bpmf_hip_side *s);
int latent_read_back(const char *func, bpmf_hip_side *s, const double *z, double *z_host);

// The refusals the setters of the add-ons give each other, in the standard wording "<who>: not on a probit side
// (bpmf_hip_side_set_probit)" etc. (the table is in capi_side.hip): the first of `order` that holds for `s` is reported as
// BPMF_HIP_EINVAL, 0 if none does.  The order decides what a side with two of the properties is told (a robust side has weights
// too); a caller whose wording differs writes that line out at its place between two calls.
enum class Not { probit, ordinal, censored, robust, weights, features, prop_posterior, reduce, bias, chain };
int refuse(const char *who, const bpmf_hip_side *s, std::initializer_list<Not> order);

// ---- Ring queries: what the entry points that reduce mean + u_s . v_s over two rings share (defined in capi_topn.hip) ----
// One ring as a launch reads it.  These three are the only places a ring stride is computed.
struct RingView { const double *ring; int64_t stride; int kp, count; };   // doubles per column, rows per sample, samples held
inline RingView ring_view(const bpmf_ring *r) { return {r->samples.get(), (int64_t)r->max * r->kp, r->kp, r->count}; }
inline RingView ring_view(const bpmf_newrows *nr) { return {nr->ring.get(), (int64_t)nr->max * nr->kp, nr->kp, nr->count}; }
inline RingView ring_view(const bpmf_foldin *f) { return {f->ring.get(), (int64_t)f->S * f->kp, f->kp, f->S}; }
// queries of `q` against candidates of `c` (a sample ring, new rows or folded-in rows each: either order); the queries' count is S
template <typename Q, typename Cn>
inline bpmf_launch::RingPair ring_pair(const Q *q, const Cn *c)
{
    const RingView a = ring_view(q), b = ring_view(c);
    return {a.ring, b.ring, a.stride, b.stride, a.kp, a.count};
}
// The prologue of a query over the sample rings of two sides, in two steps with the caller's own argument checks between them.
// pair_check_sides, on the host alone: NULL sides, two contexts and, if asked, a communicator or a shard (require_single_gpu).
// pair_open_rings: sets the device, waits for the sides' work in flight, then refuses a missing ring, rings that do not meet in one
// dot product (rows per sample, bias roles) and counts that differ or are 0; *out: the pair.
int pair_check_sides(const std::string &who, const bpmf_hip_side *query, const bpmf_hip_side *cand, bool single_gpu);
int pair_open_rings(const std::string &who, bpmf_hip_side *query, bpmf_hip_side *cand, bpmf_launch::RingPair *out);
int refuse_topn_n(const char *who, int n);                             // "<who>: n = .. (1 .. topn_max_n)"
int refuse_range(const char *who, const char *what, int64_t from, int64_t to, int64_t ncols);   // "<who>: <what> range out of bounds"
// device -> host copies of results, skipping a NULL destination or an empty array: "<who>: copying the results back failed"
struct CopyBack {
    void *dst; const void *src; size_t bytes;
    template <typename T>
    CopyBack(T *d, const typename std::common_type<T>::type *s, size_t count) : dst(d), src(s), bytes(count * sizeof(T)) {}   // (T from d alone)
};
int copy_back(const std::string &who, std::initializer_list<CopyBack> list);
// a *_last_ms entry point: NULL arguments, then `none_msg` while `t` (NULL: no state yet) has timed nothing
int last_ms(const char *who, const bpmf_hip_side *s, const Timed *t, float *ms, const char *none_msg);

// The lists of a ranking of nq queries x n places over nsplit candidate splits: what the score + select kernel leaves per split
// (part_*), what the merge leaves (out_*), and their read-back.  scored: the rankings by a score of their own keep score | mean | std
// per split; the plain one keeps the mean per split and gets its std after the merge.
struct TopnLists {
    size_t pn = 0, nsplit = 0; bool scored = false;
    DevBuf<double> part, out; DevBuf<int32_t> pidx, oidx;
    int alloc(const char *who, int64_t nsplit_, int64_t nq, int n, bool scored_);
    double *part_score() const { return part.get(); }
    double *part_mean() const { return part.get() + (scored ? nsplit * pn : 0); }
    double *part_std() const { return part.get() + 2 * nsplit * pn; }
    int32_t *part_idx() const { return pidx.get(); }
    double *out_score() const { return out.get(); }
    double *out_mean() const { return out.get() + (scored ? pn : 0); }
    double *out_std() const { return out_mean() + pn; }
    int32_t *out_idx() const { return oidx.get(); }
    int read_back(const char *who, int32_t *idx, double *score, double *mean, double *std) const;   // score NULL: not scored
};

// A list of (query, candidate) cells over two rings (capi_model.hip): what bpmf_hip_predict_cells, bpmf_hip_diag_cells,
// bpmf_hip_score_cells and bpmf_hip_interval_cells share.  cells_check_list refuses, as `who` and on the host alone, what pair_check_sides does (single GPU), then
// n, mean_rating, a NULL list and a cell out of range; pair_open_rings follows the caller's own checks.  cells_sort groups the list by
// query (stable counting sort).
struct CellsSorted { std::vector<int32_t> query, cand, orig; };       // per sorted cell: its query, its candidate, its place in the caller's list
int cells_check_list(const std::string &who, bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q, const int32_t *cc);
CellsSorted cells_sort(int64_t nq, int64_t n, const int32_t *q, const int32_t *cc);
// The launches of a sorted list: batches of `step` sorted cells (the last one shorter), every query's run within a batch cut into the
// segments of at most `seg` cells a workgroup takes.  Segments do not cross a batch; seg_beg counts from the start of the sorted
// list, so a cell's results do not depend on where the batches are cut.
struct CellsPlan {
    const CellsSorted &sorted; int64_t n, step;
    std::vector<int32_t> seg_q, seg_beg, seg_cnt;
    std::vector<size_t> first;                                         // per batch: its first segment; then their number
    DevBuf<int32_t> d_segq, d_segb, d_segc, d_cand, d_orig;
    CellsPlan(const CellsSorted &s, int64_t n_, int64_t step_, int seg);
    int upload();
    size_t nbatches() const { return first.size() - 1; }
    int64_t begin(size_t b) const { return (int64_t)b * step; }        // the first sorted cell of batch b
    int64_t cells(size_t b) const { return std::min<int64_t>(step, n - begin(b)); }
    const int32_t *orig() const { return d_orig.get(); }
    void bind(bpmf_launch::PredCellsLaunch &p, size_t b) const;        // nseg, seg_q, seg_beg, seg_cnt of batch b; cand, orig
};

// cells of a batch whose traces (S doubles per cell) fill the trace buffer of 256 MiB, or `forced` if > 0 (capi_diag.hip): what
// bpmf_hip_diag_cells / _traces and bpmf_hip_interval_cells / _traces cut their lists by
int64_t trace_batch_cells(int S, int forced);

// The likelihood of a list of observed cells (capi_score.hip): what bpmf_hip_score_cells and bpmf_hip_loo_cells share.  logdens_check_args
// refuses, as `who` and on the host alone, an unknown kind, a NULL alpha, a NULL y or output (null_output) with n > 0, flags or weights
// beside a kind that is not Gaussian, nu, nalpha < 1, an alpha, y, w or flag out of range.  logdens_constants: c0 | as | sa of
// kernels_score.h, S doubles each.
int logdens_check_args(const std::string &who, int64_t n, const int32_t *q, const int32_t *cc, const double *y, const double *w, const int8_t *flag,
                       int kind, double nu, int nalpha, const double *alpha, bool null_output);
std::vector<double> logdens_constants(int kind, double nu, int nalpha, const double *alpha, int S);

// Phi^-1(p), 0 < p < 1: Newton on Phi(x) - p from 0 in the variable that keeps the tail resolved (p <= 1/2 by symmetry), each
// step limited to 1; the start of the default cutpoints (capi_ordinal.hip) and the z of a quantile's bracket (capi_interval.hip)
inline double normal_quantile(double p)
{
    const bool upper = p > 0.5;
    const double q = upper ? 1.0 - p : p;                              // q = Phi(x), x <= 0
    double x = 0.0;
    for (int it = 0; it < 200; ++it) {
        const double f = 0.5 * std::erfc(-x * 0.70710678118654752440) - q;
        const double d = std::exp(-0.5 * x * x) * 0.3989422804014326779;
        double step = f / d;
        step = step > 1.0 ? 1.0 : step < -1.0 ? -1.0 : step;
        x -= step;
        if (std::fabs(step) <= 1e-16 * (1.0 + std::fabs(x))) break;
    }
    return upper ? -x : x;
}

// side information (capi_link.hip): what bpmf_hip_side_set_features and _set_features_sparse share -- the refusals (reported as `who`),
// then the arrays both kinds of features need, zeroed, with the ratings as the first residuals.  *out is not attached to `s` yet.
int link_attach_common(const char *who, bpmf_hip_side *s, int D, double lambda, unsigned tag, size_t part_words, std::unique_ptr<bpmf_link> *out);
int ensure_state(bpmf_hip_side *s);                                    // (capi_sample.hip) the Sys state of a side: cov, hyper-parameters

// C (N x ncw, leading dimension ldc) = A B on k_link_gemm_nn, columns n .. ncw - 1 zero (capi_link.hip)
int link_nn_product(const double *A, int64_t lda, const double *B, int64_t ldb, int64_t N, int Dr, int n, double *C, int64_t ldc, int ncw, hipStream_t st);
// canonical CSR or a refusal reported as `who` (capi_link_sparse.hip)
int link_check_csr(const char *who, int64_t N, int64_t D, const int64_t *rowptr, const int32_t *colidx, const double *vals);

// posterior top-N over two rings of S samples (capi_topn.hip): what bpmf_hip_topn and bpmf_hip_newrows_topn share.  Queries
// [q_from, q_from + nq) of qring against the candidates [0, nc) of cring; ex_ptr / ex_rows: the exclusion lists or NULL.  Waits.
int topn_rings(bpmf_hip_ctx *c, const bpmf_launch::RingPair &r, double mean_rating, int n, int64_t q_from, int64_t nq, int64_t nc, const int64_t *ex_ptr,
               const int32_t *ex_rows, int32_t *idx_out, double *mean_out, double *std_out);
// the candidate splits both rankings use: a split is a multiple of 64 candidates; they are used when the query blocks alone do not
// fill the device
void topn_splits(const bpmf_hip_ctx *c, int64_t nq, int64_t nc, int64_t *nsplit, int64_t *cspan);

// mean / std (nq x nc each) of queries [q_from, q_to) against candidates [c_from, c_to) of two rings of S samples (capi_newrows.hip):
// what bpmf_hip_predict_block, bpmf_hip_newrows_predict and bpmf_hip_foldin_predict share.  w: added to the variance as w[candidate] / S,
// or NULL.  device_out: the outputs are device memory of the context's device and written in place, else host arrays.  Waits.
int predict_rings(const char *who, bpmf_hip_ctx *c, const bpmf_launch::RingPair &r, int64_t nqcols, int64_t nccols, const double *w, double mean_rating,
                  int64_t q_from, int64_t q_to, int64_t c_from, int64_t c_to, double *mean_out, double *std_out, bool device_out = false);

// evaluation (capi_eval.hip)
void flush_deferred(bpmf_hip_test *t, bool on_main = false);           // enqueues an evaluation whose launch was put off

}  // namespace bpmf_capi

// KK: the instantiated num_latent; FF: the fp32 context (K = 128 only).  Uses the context `c` of the caller.
#define BPMF_DISPATCH_K(K_, ...)                                                     \
    [&]() -> int {                                                                   \
        switch (K_) {                                                                \
        case 8: { constexpr int KK = 8; constexpr bool FF = false; return __VA_ARGS__; }    \
        case 16: { constexpr int KK = 16; constexpr bool FF = false; return __VA_ARGS__; }  \
        case 32: { constexpr int KK = 32; constexpr bool FF = false; return __VA_ARGS__; }  \
        case 64: { constexpr int KK = 64; constexpr bool FF = false; return __VA_ARGS__; }  \
        case 128:                                                                    \
            if (c->dtype == BPMF_HIP_F32) { constexpr int KK = 128; constexpr bool FF = true; return __VA_ARGS__; } \
            else { constexpr int KK = 128; constexpr bool FF = false; return __VA_ARGS__; } \
        default: return fail(BPMF_HIP_EINVAL, "unsupported K");                     \
        }                                                                            \
    }()
