// launch.h -- what the C ABI (capi_*.hip) needs from the translation units that hold the kernels.  The templates
// are defined in launch_impl.h and explicitly instantiated one K per file (k8.hip ... k128.hip), so
// that the five instantiations of the sampler compile side by side (make -j).  The launch structs of the kernels that read two sample
// rings lead with one RingPair; those of the add-ons share FactorPair / SideCsc.
#pragma once
#include "state.h"

#include <type_traits>

// one kernel launch of a sampler sequence: events ride on the dispatch packet when given, the pending launch flags are consumed
// (EVERY kernel of a sampler sequence must be launched through this macro: bpmf_hip_side_kernel_resources runs the dispatch
//  logic over live factor pointers with a probe installed, and only this macro knows not to launch then)
#define BPMF_LAUNCH(kernel, grid, block, st, e0, e1, ...)                                                         \
    do {                                                                                                          \
        if (bpmf_launch::probe()) { bpmf_launch::probe()->record(reinterpret_cast<const void *>(kernel), #kernel, block); break; }   \
        const unsigned fl_ = bpmf_launch::take_flags();                                                           \
        hipEvent_t e0_ = (e0), e1_ = (e1);                                                                        \
        if (e0_ || e1_ || fl_) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, e0_, e1_, fl_, __VA_ARGS__);    \
        else hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);                                         \
    } while (0)

namespace bpmf_launch {

// "What would this side's sampler launch?" (bpmf_hip_side_kernel_resources): with a probe installed on the calling thread,
// BPMF_LAUNCH records the kernel's LDS / register budget and residency instead of launching it -- the dispatch logic of
// sampler_into answers for itself, no second copy of it to keep in step.
struct Probe {
    static constexpr int MAXK = 8;
    int n = 0;
    int64_t v[MAXK][4];          // LDS bytes per workgroup (static) | threads per workgroup | workgroups resident per CU | VGPRs (arch + acc)
    char name[MAXK][128];
    void record(const void *kernel, const char *text, dim3 block)
    {
        if (n >= MAXK) return;
        hipFuncAttributes a;
        int nb = 0;
        const int threads = (int)(block.x * block.y * block.z);
        if (hipFuncGetAttributes(&a, kernel) != hipSuccess) { (void)hipGetLastError(); return; }
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, 0) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
        v[n][0] = (int64_t)a.sharedSizeBytes; v[n][1] = threads; v[n][2] = nb; v[n][3] = a.numRegs;
        snprintf(name[n], sizeof name[n], "%s", text);
        ++n;
    }
};
inline Probe *&probe() { static thread_local Probe *p = nullptr; return p; }

// hipExtAnyOrderLaunch for the NEXT sampler launch of this thread, consumed by the first kernel of its sequence: that
// launch may start while the packet ahead of it in the queue -- the statistics pass of the other side -- is still
// running (see bpmf_hip_sys_sample: "in-order head start").
inline unsigned &next_flags() { static thread_local unsigned f = 0; return f; }
inline unsigned take_flags() { unsigned &f = next_flags(); const unsigned v = f; f = 0; return v; }

// A sampler's arguments pointed at the parameter blob `d_in` (blob.h) and at the side: the per-call members every form of
// the sampler reads.  Value-initialised: the schedule, gate and profiling members are left to the caller.
inline bpmf::SampleArgs blob_args(const bpmf_hip_side *self, double *out_items, double *d_in, int iter, double alpha)
{
    const bpmf_hip_ctx *c = self->ctx;
    const int K = c->K;
    bpmf::SampleArgs a{};
    a.items = out_items; a.col_from = self->from;
    a.LambdaF = d_in + blob::par_LambdaF(K); a.Lmu = d_in + blob::par_Lmu(K); a.fail = blob::par_fail_word(d_in, K);
    a.mu = d_in + blob::par_mu(K); a.prop_lambda = self->d_prop.get(); a.diag_only = c->diag_only;
    a.mean_rating = self->mean_rating; a.alpha = alpha; a.iter_plus_1 = (uint32_t)(iter + 1); a.ktrue = c->Kt;
    return a;
}

// The statistics pass of side P with sequence number `seq`: what it reads (P's current factors, the fail word of the
// parameter blob `d_in` its sampler ran with) and where its sums, flag and time-out word go (the result blob `out`).
// The stand-alone kernels (stats below) and the riders of a sampler launch (FusedArgs::st_*, StatRiders) are filled from it.
struct StatPass {
    const void *items; int64_t c0, c1; int nwaves; double *partials;
    const unsigned long long *fail_in; double *out; unsigned *ticket, *flag; unsigned seq; unsigned long long *tmo;
};
inline StatPass stat_pass(const bpmf_hip_side *P, const double *d_in, double *out_host_dev, unsigned *ticket, unsigned seq)
{
    const int K = P->ctx->K;
    return {P->d_items, P->from, P->to, P->nstat_waves, P->d_stat_partials.get(), blob::par_fail_word(d_in, K),
            out_host_dev, ticket, blob::res_flag_word(out_host_dev, K), seq, blob::tmo_word(out_host_dev, K)};
}

// the per-column update of `self` into `out_items`, reading the parameter blob `d_in`
template <int K, bool F32>
int sampler_into(bpmf_hip_side *self, double *out_items, const bpmf_hip_side *other, int iter, double alpha, double *d_in, hipStream_t st,
                 hipEvent_t ev_start, hipEvent_t ev_stop);
// multi-GPU: every rank's fresh columns travel to the others, in place in the replicated factor matrix.
// sub < 0: the whole range of every rank; sub >= 0: sub-range `sub` of every rank (bpmf_hip_side_set_overlap:
// the exchange of one part of a side's columns runs on a stream of its own beside the sampling of the next part)
template <int K, bool F32>
int exchange(bpmf_hip_side *self, hipStream_t st, int sub);
// sum x / sum x x^T of this rank's columns (+ all-reduce), published to the result blob of `p`
template <int K, bool F32>
int stats(bpmf_hip_side *self, hipStream_t st, const StatPass &p,
          hipEvent_t ev_done = nullptr);     // ev_done: rides on the dispatch packet of the pass's last kernel (single GPU; no marker packet behind it)
template <int K, bool F32>
void predict(bpmf_hip_test *t, const bpmf_hip_side *self, const void *self_items, const void *other_items, int n, hipStream_t ps, bool beside);

// K = 64: every kernel family sits in a unit of its own (k64_*.hip) -- the instantiations
// of this size take minutes to compile.  e0 / e1: events riding on the dispatch packet, or NULL.
void k64_pf(int cls, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::LrArgs &a);       // class 0..2: <= 3 | 6 | 16 ratings
void k64_pf_prepare(int grid, hipStream_t st, hipEvent_t e0, const double *S0t, const double *other_items, int64_t nrows, double *Q);

// slab form (kernels_slab.h): K = 64 fp64, one wave per work item
void k64_slab(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a);
// the weighted forms (a.sw) sit in units of their own: k64_slabw.hip, k128_f64w.hip, kw8.hip .. kw32.hip (launch_w.h)
void k64_slabw(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a);
void k64_1sw(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a, const bpmf::FusedArgs &f);   // k_sample1sw<64>: gate + riders + items
template <int K>
void sample1w(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a, const bpmf::FusedArgs &f);  // K <= 32: k_sample1w<K>
template <int K>
void sample4w(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a);                             // K <= 32: k_sample4w<K>
// K = 128 fp32: workgroup of two waves per item (kernels_wg2.h)
// (r: column statistics of another side as rider workgroups at the head of the grid, or r.nblocks == 0)
void k128_wg2(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a, const bpmf::StatRiders &r);
// K = 128 fp64 (num_latent 65 .. 128 in the reference's arithmetic): the same form with fp64 factors, four waves per item (k128_f64.hip)
void k128_wg2_f64(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a, const bpmf::StatRiders &r);
void k128_wg2w_f64(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a, const bpmf::StatRiders &r);

// BPMF_REDUCE formulation (kernels_reduce.h, kreduce.hip): fp64, K = 8 .. 64
int reduce_part_words(int K);                  // doubles per column of a side's `prec` array (0: K not supported)
int reduce_waves_per_simd(int K);
void reduce_precompute(int K, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::PrecArgs &p);
void reduce_sample(int K, int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a, const double *prec);

// kernels that do not depend on K (kcommon.hip)
void stage(const double *src_host_dev, double *dst, int n, hipStream_t st);
void gate_stage(int nblocks, const unsigned *gate_host_dev, unsigned want, const double *src_host_dev, double *dst, int n,
                unsigned long long *tmo, unsigned long long ticks, hipStream_t st);
void lf32_tiles(const double *LambdaF_dev, float *out, int K, hipStream_t st);    // fp32 path: LambdaF in tile layout behind the blob
void publish(const double *src, double *dst_host_dev, int n, unsigned *flag_host_dev, unsigned seq, int fail_at, hipStream_t st);
void randn_probe(uint32_t counter, int n, double *out_dev, hipStream_t st);
void aggr_add(const void *items, bool f32, int ld, int K, int64_t c0, int64_t ncols, double *mu, double *lambda, hipStream_t st);   // ld: device leading dimension, K: the caller's num_latent
void aggr_finalize(int K, int nsamples, int64_t ncols, double *mu, double *lambda, hipStream_t st);

// Two sample rings that meet in one dot product, as a kernel reads them: S samples of Kp rows per column, a column of the queries'
// ring every qstride doubles, of the candidates' every cstride.  Every launch struct of a ring query below leads with one (filled by
// ring_pair, capi_internal.h); its launcher tests the shape with ring_pair_ok and copies the members into its kernel's arguments.
struct RingPair { const double *qring, *cring; int64_t qstride, cstride; int Kp, S; };
inline bool ring_pair_ok(const RingPair &r)
{
    return r.Kp >= 4 && r.Kp <= 128 && r.Kp % 4 == 0 && r.S >= 1 && r.qstride >= (int64_t)r.S * r.Kp && r.cstride >= (int64_t)r.S * r.Kp;
}

// posterior top-N (kernels_topn.h, ktopn.hip)
void samples_add(const void *items, bool f32, int ld, int Kt, int Kp, int64_t ncols, double *ring, int64_t stride, int slot, hipStream_t st);
int topn_max_n();
struct TopnLaunch {
    RingPair r;
    int n; double mean_rating;
    int64_t q_from, nq, nc, cspan; int nsplit;
    const int64_t *ex_ptr; const int32_t *ex_rows;         // NULL: no exclusion
    double *part_mean; int32_t *part_idx;                  // nsplit x nq x n
    double *out_mean, *out_std; int32_t *out_idx;          // nq x n
};
void topn(const TopnLaunch &p, hipStream_t st);             // score + select, merge of the splits, std of the selected pairs

// ranks of held-out candidates among the candidates a query has not rated (kernels_rank.h, krank.hip)
struct RankLaunch {
    RingPair r;
    double mean_rating;
    int64_t q_from, nq, nc, cspan; int nsplit;
    const int64_t *ex_ptr; const int32_t *ex_rows;         // NULL: no exclusion
    const int64_t *tptr; const int32_t *tcand; int64_t nt; // held-out entries of query q: tcand[tptr[q] .. tptr[q + 1]), ascending; nt = tptr[nq]
    double *tscore;                                        // nt
    int32_t *part_cnt, *part_ncand;                        // nsplit x nt, nsplit x nq
    int32_t *rank, *ncand;                                 // nt, nq
};
void rank_eval(const RankLaunch &p, hipStream_t st);        // the scores of the entries, the counts, the sum of the splits

// posterior top-N by an acquisition score (kernels_topn_score.h, ktopnscore.hip)
struct TopnScoredLaunch {
    RingPair r;
    int n; double mean_rating;
    int kind; double param, sigma;                         // BPMF_HIP_SCORE_*; kappa or the threshold; sigma = 0: the noise-free forms
    int64_t q_from, nq, nc, cspan; int nsplit;
    const int64_t *ex_ptr; const int32_t *ex_rows;         // NULL: no exclusion
    double *part_score, *part_mean, *part_std; int32_t *part_idx;   // nsplit x nq x n
    double *out_score, *out_mean, *out_std; int32_t *out_idx;       // nq x n
};
int topn_scored(const TopnScoredLaunch &p, hipStream_t st);    // score + select, merge of the splits.  -1: shape not supported, -2: the LDS of the lists was refused (nothing launched)

// similar columns of one side by posterior cosine / distance (kernels_similar.h, ksimilar.hip).  -1: shape not supported (nothing launched)
int ring_norms(const double *ring, int64_t stride, int Kp, int S, int64_t ncols, double *tab, hipStream_t st);   // tab: 2 S doubles per column
struct SimilarLaunch {
    const double *ring; int64_t stride; const double *tab;
    int Kp, S, n; int kind; double kappa;                  // BPMF_HIP_SIM_*
    int64_t q_from, nq, nc, cspan; int nsplit;             // nc: the side's columns, all of them candidates
    const uint8_t *cand_ok;                                // device bytes, one per candidate, or NULL
    double *part_score, *part_mean, *part_std; int32_t *part_idx;   // nsplit x nq x n
    double *out_score, *out_mean, *out_std; int32_t *out_idx;       // nq x n
};
int similar_topn(const SimilarLaunch &p, hipStream_t st);  // score + select, merge of the splits.  -2: the LDS of the lists was refused
struct SimilarBlockLaunch {
    const double *ring; int64_t stride; const double *tab;
    int Kp, S; int kind;
    int64_t ncols, q_from, nq, c_from, nc;
    double *mean, *std;                                    // nq x nc, row-major
};
int similar_block(const SimilarBlockLaunch &p, hipStream_t st);

// dense blocks of predictions from two sample rings; rows unseen in training (kernels_predblock.h, kpredblock.hip)
struct PredBlockLaunch {
    RingPair r;
    double mean_rating;
    int64_t q_from, nq, c_from, nc;                        // queries [q_from, q_from + nq), candidates [c_from, c_from + nc)
    const double *w;                                       // added to the variance as w[candidate id] / S, or NULL
    double *mean, *std;                                    // nq x nc, row-major
};
int predict_block(const PredBlockLaunch &p, hipStream_t st);   // -1: shape not supported (nothing launched)
void rowsq_add(const double *Y, int64_t ldy, int n, int64_t ncols, double *w, hipStream_t st);      // w[c] += |Y[c][0 .. n)|^2
void ring_add_mu(double *ring, int64_t stride, int slot, int Kp, int Kt, int64_t nrows, const double *mu, hipStream_t st);

// fold-in of new rows from their ratings (kernels_foldin.h, kfoldin.hip)
struct FoldinLaunch {
    const int64_t *rowptr; const int32_t *colidx; const double *vals; int64_t n_new;   // the new rows by rows, on the device
    const double *cring; int64_t cstride;                  // the candidate side's ring, doubles per column
    const double *alpha, *lam, *lmu; int S;                // the hyper ring: S | S x kt x kt | S x kt
    int K, kt, kp;                                         // the context's device num_latent, the caller's, the ring's
    double mean_rating; uint32_t tag; int draw;
    double *out;                                           // n_new x S x kp
    unsigned long long *fail;                              // raised to a row whose pivot was not positive and finite
};
int foldin_chunk();                                        // ratings staged per pass (kFoldinChunk)
int foldin(const FoldinLaunch &p, hipStream_t st);         // -1: shape not supported (nothing launched)

// predictions for a list of cells from two sample rings; the repacking of a ring for its read-back and load (kernels_predcells.h, kpredcells.hip)
struct PredCellsLaunch {
    RingPair r;
    double mean_rating;
    int want_prob; double t, sigma;                        // prob = (1/S) sum Phi((p_s - t) / sigma); sigma < DBL_MIN: the counting form
    int64_t nseg;                                          // workgroups: runs of cells of one query, at most predict_cells_segment(Kp) each
    const int32_t *seg_q, *seg_beg, *seg_cnt;              // per segment: the query, its first cell in the sorted list, its cells
    const int32_t *cand, *orig;                            // per sorted cell: the candidate, the place in the caller's list
    double *mean, *std, *prob;                             // caller's order, on the device; prob NULL without want_prob
};
int predict_cells_segment(int Kp);
int predict_cells(const PredCellsLaunch &p, hipStream_t st);   // -1: shape not supported (nothing launched)
// packed (nc x n x Kt doubles) <- slots [s_from, s_from + n) of columns [c_from, c_from + nc) of a ring; and packed -> slots [0, n), pad rows zero
void samples_pack(const double *ring, int64_t stride, int Kp, int Kt, int64_t c_from, int64_t nc, int s_from, int n, double *packed, hipStream_t st);
void samples_unpack(const double *packed, int64_t stride, int Kp, int Kt, int64_t c_from, int64_t nc, int n, double *ring, hipStream_t st);

// convergence diagnostics (kernels_diag.h, kdiag.hip).  cell_traces: predict_cells without the probability, which also stores every
// cell's d_s at trace[(place among the sorted cells - tbase) * S + s]; the segments are those of one batch of sorted cells.
// trace_diag: split-Rhat and ESS of ntr traces of S samples (row-major, on the device) to rhat / ess[orig[t]] (orig NULL: [t]).
int diag_min_samples();
int diag_max_samples();
int cell_traces_segment(int Kp);                            // cells of a segment at most
int cell_traces(const PredCellsLaunch &p, double *trace, int64_t tbase, hipStream_t st);          // -1: shape not supported (nothing launched)
int trace_diag(const double *traces, int64_t ntr, int S, const int32_t *orig, double *rhat, double *ess, hipStream_t st);   // -1 likewise
// over several chains (kernels_diag_mc.h, kdiagmc.hip): the rank-normalised split-Rhat, bulk and tail ESS of ntr traces of C chains of S
// samples (chain-major rows of C S doubles, on the device) to rhat / ess_bulk / ess_tail[orig[t]] (orig NULL: [t])
int diag_mc_max_chains();
int diag_mc_min_samples();
int diag_mc_max_values();                                   // C * S at most
int trace_diag_mc(const double *traces, int64_t ntr, int C, int S, const int32_t *orig, double *rhat, double *ess_bulk, double *ess_tail,
                  hipStream_t st);                          // -1 likewise

// predictive intervals (kernels_interval.h, kinterval.hip): the probability integral transform of y (NULL: none) and nq quantiles of the
// mixture of S normals around ntr traces of S samples (row-major, on the device; what cell_traces stores), to pit[orig[t]] and
// quant[orig[t] * nq + j] (orig NULL: [t]).  y and w (NULL: 1) are read at the same places; sa: sqrt(alpha_s), S doubles on the device,
// or NULL: sa0 for every sample; tau increasing, z = Phi^-1(tau).
struct TraceQuantLaunch {
    const double *traces; int64_t ntr; int S; const int32_t *orig;
    double mean_rating;
    const double *y, *w, *sa; double sa0;
    int nq; double tau[8], z[8];
    double *pit, *quant;
};
int interval_max_samples();
int interval_max_quantiles();
int trace_quantiles(const TraceQuantLaunch &p, hipStream_t st);   // -1: shape not supported (nothing launched)

// PSIS-LOO (kernels_loo.h, kloo.hip): Pareto-smoothed importance sampling of ntr traces of S samples (row-major, on the device), to
// elpd[orig[t]], khat[orig[t]] and lpd[orig[t]] (orig NULL: [t]).  kind -1: the traces hold the log densities l_s.  Else BPMF_HIP_LOGDENS_*:
// they hold what cell_traces stores, and l_s is formed from it as score_cells forms it -- y, w (NULL: 1) and flag (NULL: none; probit:
// the sign of the label, never NULL) are read at the same places, c0 / as / sa are the per-sample constants of kernels_score.h.
struct TracePsisLaunch {
    const double *traces; int64_t ntr; int S; const int32_t *orig;
    int kind; double nu, mean_rating;
    const double *y, *w; const int8_t *flag;
    const double *c0, *as, *sa;
    double *elpd, *khat, *lpd;
};
int loo_max_samples();
int trace_psis(const TracePsisLaunch &p, hipStream_t st);   // -1: shape or kind not supported (nothing launched)

// model comparison (kernels_score.h, kscore.hip): predict_cells' walk of one batch of sorted cells (`cells`; want_prob, t, sigma and
// prob are not read), which also turns every cell's S predictions into the log pointwise predictive density and the variance of the
// log density.  kind: BPMF_HIP_LOGDENS_*; y, w (NULL: 1) and flag (NULL: none; probit: the sign of the label, never NULL) are in the
// caller's order, c0 / as / sa are the per-sample constants of kernels_score.h (S doubles each; sa NULL without flags), on the device.
struct ScoreCellsLaunch {
    PredCellsLaunch cells;
    int kind; double nu;
    const double *y, *w; const int8_t *flag;
    const double *c0, *as, *sa;
    double *lpd, *pw;                                      // caller's order, on the device
};
int score_cells_segment(int Kp);                           // cells of a segment at most
int score_cells(const ScoreCellsLaunch &p, hipStream_t st);   // -1: shape or kind not supported (nothing launched)

// What the launch structs of the add-ons below share, filled by factor_pair / side_csc (capi_internal.h):
struct FactorPair { const void *items, *other; bool f32; int K, kt; };   // both factor matrices (leading dimension K; floats if f32), the caller's num_latent kt
struct SideCsc { const int64_t *colptr; int64_t ncols; const int32_t *rowidx; int64_t nnz; };   // a side's ratings: column pointers (ncols + 1) and row ids, on the device

// The instantiated num_latent as a compile-time constant: fn(std::integral_constant<int, K>) for K = 8, 16, 32, 64, 128 -- the
// launcher units with fp64 kernels only.  -1 for any other K: fn is not called, nothing is launched.
template <typename Fn>
inline int dispatch_k(int K, Fn &&fn)
{
    switch (K) {
    case 8: fn(std::integral_constant<int, 8>{}); return 0;
    case 16: fn(std::integral_constant<int, 16>{}); return 0;
    case 32: fn(std::integral_constant<int, 32>{}); return 0;
    case 64: fn(std::integral_constant<int, 64>{}); return 0;
    case 128: fn(std::integral_constant<int, 128>{}); return 0;
    }
    return -1;
}
// ... and with the element type of the factors as a second argument (a value of it): double at every size, float at K = 128 alone
template <typename Fn>
inline int dispatch_kt(int K, bool f32, Fn &&fn)
{
    if (f32) {
        if (K != 128) return -1;
        fn(std::integral_constant<int, 128>{}, float{});
        return 0;
    }
    return dispatch_k(K, [&](auto k) { fn(k, double{}); });
}

// training residuals for the adaptive noise precision (kernels_noise.h, knoise.hip)
struct SseLaunch {
    SideCsc m; const double *vals;
    FactorPair f;
    double mean;
    double *partial; int nblk;                             // nblk partials, then the sum
};
int train_sse_blocks(int64_t nnz, int num_cu);
int train_sse(const SseLaunch &p, hipStream_t st);         // -1: unsupported K (nothing launched)


// probit likelihood (kernels_probit.h, kprobit.hip)
struct ProbitLatentLaunch {
    SideCsc m; const int8_t *sign;
    FactorPair f;
    uint32_t iter, tag;
    double *z;                                             // the latent scores, layout of the side's ratings
    unsigned long long *fail;                              // raised (rating position) when a draw runs into the attempt cap
};
struct ProbitProbLaunch {
    const int32_t *tcol, *trow; int64_t nnz;               // column and row of every test entry
    FactorPair f;
    double *sum;                                           // running sums of Phi(x . y) per test entry
};
void probit_sign(const double *vals, int64_t nnz, double threshold, int8_t *sign, hipStream_t st);
int probit_latent(const ProbitLatentLaunch &p, hipStream_t st);  // -1: unsupported K (nothing launched)
int probit_prob(const ProbitProbLaunch &p, hipStream_t st);

// ordinal probit likelihood (kernels_ordinal.h, kordinal.hip)
struct OrdinalLatentLaunch {
    SideCsc m; const uint8_t *level;                       // level: 0 .. nlev - 1 per rating
    FactorPair f;
    uint32_t iter, tag;
    const double *g; int nlev;                             // the cutpoint table on the device: -inf, g_1 .. g_{C-1}, +inf (nlev + 1 doubles)
    double *z;                                             // the latent scores, layout of the side's ratings
    unsigned long long *fail;                              // raised (rating position) when a dot product is not finite
};
struct OrdinalLoglikLaunch {
    SideCsc m; const uint8_t *level;
    FactorPair f;
    const double *g0, *g1; int nlev;                       // two cutpoint tables
    double *partial;                                       // 2 x ordinal_blocks(nnz) partials, then the two sums
};
struct OrdinalProbLaunch {
    const int32_t *tcol, *trow; int64_t nnz;               // column and row of every test entry
    FactorPair f;
    const double *g; int nlev;
    double *sum;                                           // nlev x nnz running sums of the level probabilities
};
int64_t ordinal_blocks(int64_t nnz);                       // workgroups of the three kernels: one tile of ratings each
int ordinal_latent(const OrdinalLatentLaunch &p, hipStream_t st);   // -1: unsupported K (nothing launched)
int ordinal_loglik(const OrdinalLoglikLaunch &p, hipStream_t st);   // nnz = 0: the final kernel alone (two zeros)
int ordinal_prob(const OrdinalProbLaunch &p, hipStream_t st);

// censored ratings (kernels_censor.h, kcensor.hip)
struct CensorLatentLaunch {
    const int64_t *pos; const int32_t *col, *row; const int8_t *sign; int64_t n;   // the censored entries: position in the CSC, column, row, +-1
    const double *vals;                                    // the side's ratings: vals[pos] is the bound
    FactorPair f;
    uint32_t iter, tag;
    double mean, sqrt_alpha, inv_sqrt_alpha;               // the side's mean rating; sqrt(alpha) and 1 / sqrt(alpha), formed on the host
    double *z;                                             // the latent values, layout of the side's ratings: z[pos] is written
    unsigned long long *fail;                              // raised (rating position) when a draw runs into the attempt cap
};
int censor_latent(const CensorLatentLaunch &p, hipStream_t st);  // -1: unsupported K (nothing launched); n = 0: nothing launched

// Student-t noise (kernels_robust.h, krobust.hip): fp64 factors only
struct RobustWeightsLaunch {
    SideCsc m; const double *vals;
    FactorPair f;                                          // (fp64 factors: f.f32 is not read)
    uint32_t iter, tag;
    double mean, sqrt_alpha, nu;                           // the side's mean rating; sqrt(alpha), formed on the host; the degrees of freedom
    double dd, c;                                          // a - 1 / 3 and 1 / sqrt(9 dd) of the shape a = (nu + 1) / 2, formed on the host
    double *sw, *zw;                                       // sqrt(w) and sqrt(w) (r - mean), layout of the side's ratings
    unsigned long long *fail;                              // raised (rating position) when a draw runs into the attempt cap
};
int robust_weights(const RobustWeightsLaunch &p, hipStream_t st);        // -1: unsupported K (nothing launched)
void robust_accumulate(const double *sw, int64_t nnz, double *wsum, hipStream_t st);   // wsum[p] += sw[p]^2

// row and column bias terms (kernels_bias.h, kbias.hip): fp64 factors only
struct BiasStepLaunch {
    SideCsc m; const double *vals;
    FactorPair f;                                          // (fp64 factors: f.f32 is not read)
    const int64_t *pieceptr; int64_t npieces;              // the first piece of every column (ncols + 1), the pieces of the side
    uint32_t iter, tag;
    double mean, alpha;                                    // the side's mean rating; the noise precision
    const double *lambda;                                  // the device word that holds the side's bias precision
    const double *cbias;                                   // the other side's biases, one per row of this side
    double *e, *part;                                      // work: nnz residuals, npieces piece partials
    double *b, *z;                                         // the side's biases (ncols); the values its samplers read (layout of vals)
    unsigned long long *fail;                              // raised (rating position) when a residual is not finite
};
struct BiasLambdaLaunch {
    const double *b; int64_t ncols;                        // the side's current biases
    double dd, c, b0;                                      // a - 1 / 3 and 1 / sqrt(9 dd) of the shape a = a0 + ncols / 2, formed on the host; the prior's rate
    uint32_t iter, tag;
    double *lambda; double *trace; int cap;                // the side's lambda word; trace[iter] gets the draw (iter < cap)
    unsigned long long *fail;
};
void bias_lambda(const BiasLambdaLaunch &p, hipStream_t st);   // one workgroup
// rows Kt, Kt + 1 of ring slot `slot` of every column: (b, 1) for role 0, (1, b) for role 1
void samples_add_bias(const double *b, int64_t ncols, int role, int Kt, double *ring, int64_t stride, int Kp, int slot, hipStream_t st);
int bias_light();                                          // ratings up to which a column has no piece (kBiasLight)
int bias_piece();                                          // ratings of a column per piece (kBiasPiece)
int bias_step(const BiasStepLaunch &p, hipStream_t st);    // residuals, piece sums, draw, values.  -1: unsupported K (nothing launched)
void bias_accumulate(const double *b, int64_t ncols, double *bsum, hipStream_t st);   // bsum[a] += b[a]
// k_predict_bias for the test matrix `t` of the biased side `self` against `other`, on `ps`, in order; the twin as bpmf_launch::predict
// treats it (one kernel for both copies when the entries match, else a launch of its own ahead).  -1: unsupported K
int bias_predict(bpmf_hip_test *t, const bpmf_hip_side *self, const bpmf_hip_side *other, const void *self_items, const void *other_items,
                 int n, hipStream_t ps);

// sparse tensor factorisation (kernels_tensor.h, ktensor.hip): fp64 factors only
struct KhatriRaoLaunch {                                   // P[:, e] = A[:, ia[e]] o B[:, ib[e]], e < n; rows kt .. ld - 1 of P zero
    const double *A, *B;                                   // the two other modes' factor matrices (leading dimension ld)
    const int32_t *ia, *ib; int64_t n;                     // per entry its column of A and of B
    int ld, kt;                                            // the context's leading dimension and the caller's num_latent
    double *P;                                             // ld x n
    hipEvent_t ev_start, ev_stop;                          // optional: recorded by the dispatch packet itself (bpmf_hip_tensor_last_ms)
};
int khatri_rao(const KhatriRaoLaunch &p, hipStream_t st);  // -1: unsupported ld (nothing launched); n = 0: nothing launched

// side information (kernels_link.h, klink.hip): fp64, row-major operands
struct LinkTnLaunch {                                      // C (D x n, leading dimension ldc) = A^T (B - 1 bvec^T)
    const double *A; int64_t lda;                          // N x D
    const double *B; int64_t ldb; const double *bvec;      // N x n (n <= 128), bvec: n doubles or NULL
    int64_t N; int D, n;
    double *C; int64_t ldc;
    double *part;                                          // link_tn_part_words(N, D, n) doubles: the partial of every chunk of N
};
struct LinkNnLaunch {                                      // C (N x ncw, leading dimension ldc) = A B, columns n .. ncw - 1 zero
    const double *A; int64_t lda;                          // N x Dr
    const double *B; int64_t ldb;                          // Dr x n
    int64_t N; int Dr, n;
    double *C; int64_t ldc; int ncw;                       // n <= ncw <= 128
};
struct LinkResidualLaunch {
    SideCsc m; const double *vals;
    const double *offs, *other; int K, kt;                 // the side's offsets and the other side's factors (leading dimension K)
    double *out;                                           // vals - offs_c . other_r, layout of vals
};
int64_t link_chunks(int64_t N);
size_t link_tn_part_words(int64_t N, int D, int n);
int link_gemm_tn(const LinkTnLaunch &p, hipStream_t st);    // -1: shape not supported (nothing launched)
int link_gemm_nn(const LinkNnLaunch &p, hipStream_t st);
int link_residual(const LinkResidualLaunch &p, hipStream_t st);
int link_shift_blocks(int64_t total);
void link_shift(double *items, const double *offs, int64_t total, double *partial, hipStream_t st);   // partial: link_shift_blocks(total) doubles

// the device factorisation of G(lambda) = F^T F + lambda I and the draw of beta against it (kernels_link_chol.h, klinkchol.hip).
// Work arrays: Lp (dp x dp doubles, dp = link_chol_dp(D)), Linv and LinvT (dp x 64 each), Xp and Ep (dp x 128 each), flag (one int,
// raised by a pivot that is not positive and finite; the caller zeroes and collects it).
struct LinkCholLaunch {                                    // Lp = the factor of [FtF + lambda I, 0; 0, I]
    const double *FtF; int D; double lambda;               // D x D, row-major
    double *Lp, *Linv, *LinvT; int *flag;
};
struct LinkCholSolveLaunch {                               // out (D x ncw, leading dimension ldo) = L^-T (L^-1 P + E), columns n .. ncw - 1 zero
    const double *Lp, *Linv, *LinvT; int D;
    const double *P; int64_t ldp; const double *E; int64_t lde; int n;   // D x n (n <= 128); E may be NULL
    double *Xp, *Ep;
    double *out; int64_t ldo; int ncw;                     // n <= ncw <= 128
};
int link_chol_dp(int D);
int link_chol_factor(const LinkCholLaunch &p, hipStream_t st);         // -1: shape not supported (nothing launched)
int link_chol_solve(const LinkCholSolveLaunch &p, hipStream_t st);

}  // namespace bpmf_launch
