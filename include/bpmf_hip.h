/*
 * bpmf_hip.h -- C ABI of the MI355X-native BPMF Gibbs hot path (libbpmf_hip.so).
 *
 * This is the drop-in boundary for the per-column sampler of ExaScience/bpmf.
 * The reference has no FFI: its boundary is the C++ class `struct Sys`
 * (c++/bpmf.h:112-239) selected at compile time through `#define SYS <Backend>_Sys`
 * (c++/nocomm.h:6, c++/bpmf.cpp:19-39,131-132).  A new back-end header
 * (INTEGRATION.md shows `hip_sys.h`) subclasses Sys and forwards the virtuals
 * below to these entry points; each prototype cites the reference member it
 * replaces.
 *
 * Conventions
 *   - every function returns 0 on success or a negative BPMF_HIP_E* code and
 *     leaves a message for bpmf_hip_last_error() (thread-local);
 *   - matrices are column-major doubles exactly like Eigen's MatrixNNd / the
 *     `items()` map (c++/bpmf.h:56,193-194): a factor matrix is K x N with one
 *     contiguous K-vector per user / item, so `.ddm` dumps stay byte-compatible;
 *   - sparse matrices are CSC with ascending row indices per column (what
 *     Eigen::SparseMatrix<double> holds after setFromTriplets, c++/io.cpp:521),
 *     int64 column pointers (2e9 nnz configs overflow Eigen's int), int32 rows;
 *   - host pointers unless a name ends in `_dev`; the caller keeps ownership of
 *     everything it passes in; handles own their device memory;
 *   - one context per process per GPU, used from one host thread at a time
 *     (the reference calls Sys::sample from the main thread, c++/bpmf.cpp:184-185).
 *   - there is NO CPU fallback: without a usable HIP device every entry point
 *     that touches the device fails with BPMF_HIP_ENODEV.
 */
#ifndef BPMF_HIP_H
#define BPMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPMF_HIP_ABI_VERSION 1

#if defined(__GNUC__)
#define BPMF_API __attribute__((visibility("default")))
#else
#define BPMF_API
#endif

enum {
    BPMF_HIP_OK = 0,
    BPMF_HIP_EINVAL = -1,   /* bad argument (unsupported K, NULL, range)            */
    BPMF_HIP_ENODEV = -2,   /* no HIP device / HIP runtime error                     */
    BPMF_HIP_ENOMEM = -3,   /* device or host allocation failed                      */
    BPMF_HIP_ECHOL = -4,    /* "Cholesky failed" (c++/sample.cpp:308); see _failed_column */
    BPMF_HIP_ENUM = -5      /* host-side numerical failure in the hyper-parameter draw */
};

typedef struct bpmf_hip_ctx bpmf_hip_ctx;     /* one GPU + stream + scratch            */
typedef struct bpmf_hip_side bpmf_hip_side;   /* one `Sys`: ratings CSC + factor matrix */
typedef struct bpmf_hip_test bpmf_hip_test;   /* test matrix T with Pavg / Pm2           */

/* message of the last failing call on this thread */
BPMF_API const char *bpmf_hip_last_error(void);
BPMF_API int bpmf_hip_abi_version(void);
/* diagnostic: device bytes the add-ons of all sides of this process own right now (probit, features, sample rings, residual partials,
 * the temporaries of their calls): hipMemGetInfo counts the whole card, other processes included */
BPMF_API int64_t bpmf_hip_live_device_bytes(void);
/* diagnostic: the same for the core state of all contexts, sides and test sets of this process -- blobs, ratings, factors, schedules,
 * posterior aggregates, per-column priors, test entries.  (Memory a caller lent -- bpmf_hip_side_create_dev, bpmf_hip_side_bind_items
 * -- is the caller's and not counted.)  A side's first bpmf_hip_sys_sample allocates here, never in the add-ons' counter. */
BPMF_API int64_t bpmf_hip_live_core_bytes(void);
/* diagnostic: how often this process has waited on the host for the main stream of a context (the waits of the entry points that say
 * "waits": bpmf_hip_train_sse, bpmf_hip_ordinal_cut_step, the _get calls ...).  A loop that does not drain leaves it unchanged. */
BPMF_API int64_t bpmf_hip_stream_drains(void);
/* 1 if a context of num_latent K (BPMF_NUMLATENT, c++/bpmf.h:22-24,53: the reference ships bpmf-8 ... bpmf-128 incl. 10, 20 ... 100,
 * ci/multilatent.sh:5) can be created in fp64: 1 <= K <= 128.  The kernels are instantiated for 8, 16, 32, 64, 128; any other K
 * runs on the next instantiated size (bpmf_hip_kernel_k) with zero factor rows and an identity block of the prior precision in
 * the extra dimensions, which draw no normals and stay exactly zero: the per-column RNG stream id (idx+1)*K*(iter+1) and the
 * number of normals per column are taken from the caller's K (c++/sample.cpp:266,322), the hyper-parameter draw runs at K, and
 * everything that crosses this interface (items, sums, cov, priors, outputs) has the caller's K x ... sizes. */
BPMF_API int bpmf_hip_supports_k(int K);
/* arithmetic of the column loop / storage type of the factors on the device.  The reference is
 * fp64 throughout (c++/bpmf.h:55-58); BPMF_HIP_F32 is the large-K mixed-precision path (K = 128:
 * fp32 factors, Gram, factorisation and solves; fp64 hyper-parameters, statistics, RMSE sums and
 * normal draws).  The host-side interface (items, sums) stays double in both cases. */
#define BPMF_HIP_F64 0
#define BPMF_HIP_F32 1
BPMF_API int bpmf_hip_supports(int K, int dtype);    /* fp64: 1 .. 128; fp32: 65 .. 128 (opt-in, never chosen silently) */
/* the instantiated size a context of (K, dtype) runs on (8, 16, 32, 64 or 128; 0: unsupported) */
BPMF_API int bpmf_hip_kernel_k(int K, int dtype);

/* ---- context --------------------------------------------------------------
 * Replaces Sys::Init / Sys::Finalize (c++/nocomm.h:19-27).  `stream` is a
 * hipStream_t to launch on (e.g. torch's current stream) or NULL to let the
 * context create its own non-blocking stream. */
BPMF_API int bpmf_hip_ctx_create(int device, int K, void *stream, bpmf_hip_ctx **out);      /* fp64 */
BPMF_API int bpmf_hip_ctx_create_ex(int device, int K, int dtype, void *stream, bpmf_hip_ctx **out);
/* run-time form of the reference's BPMF_NO_COVARIANCE build (c++/sample.cpp:300-304): only the
 * diagonal of Lambda* = LambdaF + alpha G enters the factorisation of every column */
BPMF_API int bpmf_hip_ctx_set_no_covariance(bpmf_hip_ctx *ctx, int on);
/* what the context was created with, and the leading dimension of its DEVICE arrays (= bpmf_hip_kernel_k): a factor matrix
 * handed out / bound as a raw device pointer (bpmf_hip_side_items_dev, _bind_items) is ld x N column-major with rows
 * num_latent .. ld-1 zero.  ld == num_latent for 8, 16, 32, 64, 128: byte-compatible with the reference's items(). */
BPMF_API int bpmf_hip_ctx_num_latent(const bpmf_hip_ctx *ctx);
BPMF_API int bpmf_hip_ctx_dtype(const bpmf_hip_ctx *ctx);
BPMF_API int bpmf_hip_ctx_ld(const bpmf_hip_ctx *ctx);
BPMF_API int bpmf_hip_ctx_destroy(bpmf_hip_ctx *ctx);
BPMF_API int bpmf_hip_ctx_sync(bpmf_hip_ctx *ctx);
BPMF_API void *bpmf_hip_ctx_stream(bpmf_hip_ctx *ctx);

/* ---- multi-GPU -----------------------------------------------------------------
 * One process per GPU.  Replaces the reference's MPI/GASPI/ArgoDSM back-ends (send_item of every
 * fresh column + reduce_sum_cov_norm, c++/mpi_common.h:44-50, c++/mpi_bcast.h:21-30) by RCCL:
 * rank 0 calls _comm_unique_id and ships the 128 bytes to the other ranks (torch.distributed,
 * MPI, a file ...); every rank calls _ctx_comm_init.  A side that holds a shard is then given the
 * column range of EVERY rank (_side_set_ranges, nranks+1 bounds, contiguous, tiling [0, ncols));
 * from then on bpmf_hip_sample_side / bpmf_hip_sys_sample additionally broadcast each rank's fresh
 * range in place (all-gather-v over xGMI) and all-reduce sum | prod | norm on the device, so that
 * the values returned (and the cov formed from them) are the GLOBAL ones on every rank, and
 * bpmf_hip_predict returns the all-reduced se / se_avg / count.  The all-gather-v is a mesh of grouped ncclSend /
 * ncclRecv pairs, one pair per peer and xGMI link (BPMF_HIP_EXCHANGE=bcast: one ncclBroadcast per owner instead).  RCCL is loaded on first use
 * (dlopen of librccl.so.1), single-GPU use never touches it. */
BPMF_API int bpmf_hip_comm_unique_id(void *id128);
BPMF_API int bpmf_hip_ctx_comm_init(bpmf_hip_ctx *ctx, int nranks, int rank, const void *id128);
/* ranks of the context's communicator as the communication library itself counts them (ncclCommCount); 1 without one.
 * What `nprocs` is to the reference (Sys::nprocs, c++/mpi_common.h:14-22): reports print it next to the numbers. */
BPMF_API int bpmf_hip_ctx_comm_nranks(const bpmf_hip_ctx *ctx);
/* communicators the context holds: 0 = none (single GPU), 1 = one (exchange and statistics on the main stream), 2 = a second one
 * was split off with ncclCommSplit for the statistics / evaluation streams (the default where the library offers it;
 * BPMF_HIP_COMM_STREAMS=1 keeps one).  The reference's back-ends have one MPI_COMM_WORLD (c++/mpi_common.h:44-50); what
 * the second communicator stands for is their second thread of progress (c++/mpi_isendirecv.h:222-260).  A run reports it
 * so that a silent fall-back to one communicator (ncclCommSplit refused) shows. */
BPMF_API int bpmf_hip_ctx_comm_streams(const bpmf_hip_ctx *ctx);
BPMF_API int bpmf_hip_side_set_ranges(bpmf_hip_side *side, const int64_t *bounds);
/* Overlap of exchange and sampling, the job of the reference's MPI_ISEND back-end (chunks of 100 fresh items are sent
 * while the next ones are sampled, c++/mpi_isendirecv.h:13-14,222-260): every rank's column range is cut into `nparts`
 * (1..8) parts of equal work; part c of all ranks is exchanged on a stream of its own while part c + 1 is being sampled.
 * Collective: every rank calls it with the same nparts after _side_set_ranges (which already picks 4 parts when a
 * half-iteration brings >= 64 MB of fresh columns to the rank with the narrowest range -- a quantity every rank computes
 * from the same bounds; not for K = 64 fp64, whose low-rank column forms need the uncut item list; BPMF_HIP_OVERLAP=n
 * overrides, 1 = off).  Same
 * samples as without parts. */
BPMF_API int bpmf_hip_side_set_overlap(bpmf_hip_side *side, int nparts);

/* Bounded-staleness exchange (third variant; the reference's relaxations: random send throttling of the
 * GASPI back-end, `send_prob`, c++/bpmf_gaspi.h:91-104, and the blocks up to `slack` iterations old of
 * c++/mpi_allreduce.h:134-175).  Part p of the side (the whole range if uncut) travels only in the half-iterations with
 * (p + iter) % (k + 1) == 0 and in iteration 0; in between the peers sample from the copy they have: at most k
 * half-iterations old, 1 / (k + 1) of the traffic.  Own columns and the all-reduced statistics stay exact.  k = 0
 * (default): the exact chain.  Every rank sets the same k (or BPMF_HIP_STALE=k in the environment of all ranks).
 * bpmf_hip_side_exchange brings the replicas up to date.  A relaxation: results differ from the reference's. */
BPMF_API int bpmf_hip_side_set_staleness(bpmf_hip_side *side, int k);

/* The BPMF_REDUCE formulation of the reference (`Sys::preComputeMuLambda`, c++/sample.cpp:234-246; the
 * sampler reading precMu / precLambda, :289-291; `other.preComputeMuLambda(*this)` after a side's columns, :375-377; the
 * per-owner MPI_Reduce of c++/mpi_reduce.h:24-47).  For a pair of sides: after side S has been sampled, the Gram and rhs
 * parts of EVERY column of the other side that come from this rank's columns of S are computed and kept
 * (ncols x ~(K^2/2 + K) doubles per side and rank: the K^2 N memory the reference pays); before a side is sampled the
 * parts of all ranks are summed onto the owners (ncclReduce per owner range) and the column update adds the prior to the
 * sums instead of gathering the other side's factors.  Both sides start from zero parts, as Sys::init leaves them
 * (c++/sample.cpp:192-195) -- the chain is the reference's BPMF_REDUCE chain, which differs from the default one only in
 * the order of the floating-point sums.  fp64, K = 8 .. 64; not together with _side_set_conn.  The fresh columns are
 * still exchanged afterwards for _predict over the whole test set and for the outputs (the reference's predict covers
 * local rows only in this mode and says so: c++/sample.cpp:59-61).  on = 0: back to the gather formulation.
 * `bpmf`: BPMF_REDUCE=1 in the environment. */
BPMF_API int bpmf_hip_sys_set_reduce(bpmf_hip_side *a, bpmf_hip_side *b, int on);

/* Connectivity-aware exchange.  Replaces Sys::update_conn's conn_map and the
 * per-item sends it steers (c++/assign.cpp:204-241; send_item at c++/sample.cpp:370,
 * c++/mpi_isendirecv.h:222-250, c++/bpmf_gaspi.h:140-172: `if (!conn(i, k)) continue`): a fresh column travels only to the ranks whose stored
 * ratings or test entries reference it, instead of to everyone.  After _side_set_ranges, give the
 * side, per peer rank r (offsets *_ptr[nranks+1], CSR style; global column ids, int32):
 *   send_cols[send_ptr[r] .. send_ptr[r+1])  columns of THIS rank's range that rank r reads,
 *   recv_cols[recv_ptr[r] .. recv_ptr[r+1])  columns of rank r's range that THIS rank reads
 * (the two must mirror each other across ranks: r's receive list from q == q's send list to r, same
 * order).  The exchange then packs, does one grouped ncclSend / ncclRecv per peer, and scatters;
 * columns nobody asked for stay stale in the replica (they are never read on this rank).  Both
 * pointers NULL: back to the all-gather form.  bpmf_hip_side_exchange runs the side's exchange on
 * its own (blocking), e.g. to replicate factors written with _side_set_items. */
BPMF_API int bpmf_hip_side_set_conn(bpmf_hip_side *side, const int64_t *send_ptr, const int32_t *send_cols,
                                    const int64_t *recv_ptr, const int32_t *recv_cols);
BPMF_API int bpmf_hip_side_exchange(bpmf_hip_side *side);

/* ---- one side (= one Sys) ---------------------------------------------------
 * Replaces Sys::Sys + alloc_and_init + Sys::init (c++/sample.cpp:112-137,179-226,
 * c++/nocomm.h:29-33).  The factor matrix has `ncols` columns (all of them,
 * replicated on every GPU) and is zero-initialised (items().setZero(), :185).
 * This rank samples columns [col_from, col_to) -- Sys::from()/to(),
 * c++/bpmf.h:170-172 -- and passes the CSC slice of exactly those columns:
 * colptr has col_to-col_from+1 entries starting at 0, rowidx are row ids of the
 * ratings = column ids of the OTHER side (must be < nrows).  mean_rating is
 * M.sum()/M.nonZeros() over the whole matrix (c++/sample.cpp:183).
 * The arrays are copied to the device; the `_dev` variant adopts device arrays
 * the caller keeps alive (e.g. a synthetic matrix generated on the GPU). */
BPMF_API int bpmf_hip_side_create(bpmf_hip_ctx *ctx, int64_t ncols, int64_t nrows, int64_t col_from, int64_t col_to,
                         const int64_t *colptr, const int32_t *rowidx, const double *vals,
                         double mean_rating, bpmf_hip_side **out);
BPMF_API int bpmf_hip_side_create_dev(bpmf_hip_ctx *ctx, int64_t ncols, int64_t nrows, int64_t col_from, int64_t col_to,
                             const int64_t *colptr_host, const int32_t *rowidx_dev, const double *vals_dev,
                             double mean_rating, bpmf_hip_side **out);
/* Propagated-posterior priors (-m / -l of the reference: Sys::add_prop_posterior,
 * c++/sample.cpp:157-174, used at :272-277).  Lambda: K*K doubles per column of the side's slice
 * [from, to) (each a column-major K x K precision, the layout of U-Lambda.ddm / V-Lambda.ddm); it
 * replaces hp.LambdaF in those columns' updates.  mu (K per column) is accepted and, like in the
 * reference, not used (rr = hp_LambdaF * hp.mu, c++/sample.cpp:285).  Lambda = NULL removes them. */
BPMF_API int bpmf_hip_side_set_prop_posterior(bpmf_hip_side *side, const double *mu, const double *Lambda);
BPMF_API int bpmf_hip_side_destroy(bpmf_hip_side *side);

/* items(): device address of the K x ncols factor matrix (c++/bpmf.h:193-194);
 * bind_items makes the side use caller-owned device storage instead (so a
 * torch tensor / RCCL buffer can be exchanged in place; replaces the
 * backend's malloc in alloc_and_init, c++/nocomm.h:31).  Either call pins the
 * factors to ONE address: the side gives up its second copy (see
 * bpmf_hip_predict_launch) and its samplers write in place from then on.
 * The caller states what it allocated: `ld` (rows per column of its storage) must equal
 * bpmf_hip_ctx_ld -- NOT num_latent when that is not one of 8 / 16 / 32 / 64 / 128 -- and `bytes`
 * must cover ld x ncols doubles; otherwise BPMF_HIP_EINVAL and nothing is bound. */
BPMF_API double *bpmf_hip_side_items_dev(bpmf_hip_side *side);
BPMF_API int bpmf_hip_side_bind_items(bpmf_hip_side *side, double *items_dev, int ld, size_t bytes);
/* host <-> device copies of the whole K x ncols matrix (the -v / -o dumps,
 * c++/bpmf.cpp:206-207,234-239) */
BPMF_API int bpmf_hip_side_get_items(bpmf_hip_side *side, double *items_host);
BPMF_API int bpmf_hip_side_set_items(bpmf_hip_side *side, const double *items_host);

/* ---- the hot path ----------------------------------------------------------
 * Replaces the column loop of Sys::sample(Sys&) (c++/sample.cpp:352-384) with
 * Sys::sample(long,Sys&) + computeMuLambda (:248-336) and the Philox/polar
 * draw (c++/mvnormal.cpp:18-47) inside: for every column idx in
 * [col_from,col_to) of `self`, from the current factor of `other`,
 *     Lambda* = LambdaF + alpha * sum_j u_j u_j^T,  b = LambdaF*mu + alpha * sum_j (r_ij - mean) u_j,
 *     x = L^-T (L^-1 b + z),  z ~ N(0,I) from stream (idx+1)*K*(iter+1) mod 2^32,
 * and writes x into self.items[:, idx].  `iter` is the value of Sys::iter after
 * the `iter++` at :344 (0 for the first call).  mu / LambdaF are the output of
 * bpmf_hyper_sample (hp.mu / hp.LambdaF).  On return the three reductions
 * over this rank's columns are on the host (thread_vector combine, :379-381):
 *     sum_out[K] = sum x,  prod_out[K*K] = sum x x^T (col-major),  *norm_out = sum |x|^2.
 * The call blocks until they have arrived.  BPMF_HIP_ECHOL if a pivot is not
 * positive (THROWERROR("Cholesky failed"), :308). */
BPMF_API int bpmf_hip_sample_side(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha,
                         const double *mu, const double *LambdaF,
                         double *sum_out, double *prod_out, double *norm_out);
/* the same split in two so that an exchange of the fresh columns can overlap
 * the reductions: _launch enqueues the kernels, _finish waits for the partials */
BPMF_API int bpmf_hip_sample_side_launch(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha,
                                const double *mu, const double *LambdaF);
BPMF_API int bpmf_hip_sample_side_finish(bpmf_hip_side *self, double *sum_out, double *prod_out, double *norm_out);
/* Stateful form, the virtual every reference back-end overrides: Sys::sample(Sys&)
 * (c++/sample.cpp:341-385; e.g. c++/mpi_bcast.h:21-30 wraps it).  Does iter++ (:344),
 * rng_set_pos(iter) + hp.sample(num(), sum = 0, cov) on the host (:349-350), the column loop
 * on the device, and cov = (prod - sum sum^T/N)/(N-1), norm (:379-384).  iter starts at -1
 * (:113), cov at 0 (:188).  Only for a side that owns all its columns (NO_COMM); a shard uses
 * bpmf_hip_sample_side and all-reduces the sums (or gives the context a communicator, see above).
 * The call is asynchronous inside: it enqueues the sampler and the column statistics and returns;
 * a host worker thread of the context collects the sums when they land, forms cov, draws this
 * side's NEXT hyper-parameters (they depend only on that cov and on iter+1) and stages them on the
 * device, while the caller samples the other side.  The only observable differences from a blocking
 * call: bpmf_hip_sys_state / the side's next bpmf_hip_sys_sample wait for that collection, and an
 * error of the half-iteration (BPMF_HIP_ECHOL) is reported by whichever of them comes first. */
BPMF_API int bpmf_hip_sys_sample(bpmf_hip_side *self, bpmf_hip_side *other, double alpha);
/* Independent chains.  Chain c of a side is the chain restarted from the initial state with its random numbers
 * taken at the half-iteration indices c * BPMF_HIP_CHAIN_STRIDE, c * BPMF_HIP_CHAIN_STRIDE + 1, ..: wherever bpmf_hip_sys_sample keys
 * random numbers of the side by the half-iteration index i -- the samplers' streams, the Normal-Wishart draw of the hyper-parameters,
 * the latent steps of a probit, censored or Student-t side -- it uses i + c * BPMF_HIP_CHAIN_STRIDE.  Everything that counts
 * half-iterations (bpmf_hip_sys_state, bpmf_hip_sys_norm) keeps the chain's own index 0, 1, ..; the entry points that take `iter`
 * from the caller (bpmf_hip_sample_side*, bpmf_hip_noise_sample) use what they are given: the caller passes the offset index.
 * Chain 0, or no call, is the run as it was, bit for bit.  BPMF_HIP_EINVAL with a one-line reason: a chain outside
 * 0 .. BPMF_HIP_CHAIN_MAX; a side that has taken a half-iteration; a context with a communicator or a shard; a side with features,
 * ordinal cutpoints, biases, implicit feedback, a tensor mode, propagated priors or BPMF_REDUCE -- whose setters in turn refuse a
 * side whose chain is not 0.  bpmf_hip_sys_sample refuses two sides of different chains. */
#define BPMF_HIP_CHAIN_STRIDE (1 << 20)
#define BPMF_HIP_CHAIN_MAX 63
BPMF_API int bpmf_hip_side_set_chain(bpmf_hip_side *side, int chain);
BPMF_API int bpmf_hip_side_chain(const bpmf_hip_side *side);
/* Sys::iter, Sys::norm, Sys::cov, hp.mu, hp.LambdaF, hp.LambdaU (c++/bpmf.h:86-89,139,222-223);
 * any output pointer may be NULL */
BPMF_API int bpmf_hip_sys_state(const bpmf_hip_side *side, int *iter, double *norm, double *cov, double *mu,
                                double *LambdaF, double *LambdaU);
/* norm (c++/sample.cpp:381: sum of the squared samples) of half-iteration `iter` of the side -- one of its last 8 -- waiting only
 * until that half-iteration's sums have landed; later half-iterations may be in flight (bpmf_hip_sys_state would wait for them).
 * What Sys::print of iteration i - 1 needs (c++/sample.cpp:101-107) when iteration i is already enqueued. */
BPMF_API int bpmf_hip_sys_norm(bpmf_hip_side *side, int iter, double *norm);
/* Posterior aggregation for the -o outputs.  _aggr_add replaces `aggrMu.col(i) += r; aggrLambda.col(i) += r r^T` of
 * Sys::sample(Sys&) (c++/sample.cpp:364-368): call it after a post-burn-in bpmf_hip_sys_sample; the K + K*K doubles
 * per LOCAL column live on the device.  _aggr_finalize replaces Sys::finalize_mu_lambda (c++/bpmf.cpp:281-295):
 * cov = (prod - sum sum^T / n) / (n - 1), Lambda = cov^-1 (batched, one workgroup per column), mu = sum / n; it
 * copies this rank's K x nloc means and K*K x nloc precisions (column-major per column, the layout of U-mu.ddm /
 * U-Lambda.ddm) to the host and frees the device buffers.  1 <= n <= K samples do not determine a K x K covariance (its rank
 * is at most n - 1): every entry of every Lambda is then NaN and no inverse is attempted, mu is still sum / n.  With n > K a
 * covariance with a pivot that is exactly zero gives NaN for that column. */
BPMF_API int bpmf_hip_side_aggr_add(bpmf_hip_side *side);
BPMF_API int bpmf_hip_side_aggr_finalize(bpmf_hip_side *side, int nsamples, double *mu_host, double *lambda_host);
/* global id of the first column whose factorisation failed, or -1 */
BPMF_API int64_t bpmf_hip_failed_column(const bpmf_hip_side *side);

/* ---- posterior top-N ranking --------------------------------------------------
 * Sample ring of a side: room for max_samples copies of the factor matrix in fp64 (fp32 factors are widened), one column's
 * samples contiguous: column c, sample s, row k at [c * max_samples * Kp + s * Kp + k], Kp = num_latent rounded up to 4, the
 * pad rows zero.  _reserve(side, 0) frees it (side_destroy does too); reserving again starts an empty ring.  _add copies the
 * current factors (every column of the matrix this rank holds) into the next slot: call it where _aggr_add sits, after a
 * post-burn-in bpmf_hip_sys_sample of both sides; BPMF_HIP_EINVAL once the ring is full. */
BPMF_API int bpmf_hip_side_samples_reserve(bpmf_hip_side *side, int max_samples);
BPMF_API int bpmf_hip_side_samples_add(bpmf_hip_side *side);
BPMF_API int bpmf_hip_side_samples_count(const bpmf_hip_side *side);
/* For every query column q in [q_from, q_to) of `query` and every column c of `cand`, with both rings holding the same S >= 1
 * samples: mean = mean_rating + (1/S) sum_s u_s(q) . v_s(c), std = sqrt(sum_s (p_s - mean)^2 / (S - 1)) (0 for S = 1),
 * p_s = mean_rating + u_s(q) . v_s(c).  Writes the n best candidates by mean (descending; equal means: lower candidate index
 * first) to the host arrays idx_out / mean_out / std_out, (q_to - q_from) x n row-major; exclude_rated != 0 skips the
 * candidates q rated in training (its column of the query side's ratings; the query side must hold all its columns).  Slots
 * beyond the eligible candidates: idx -1, mean 0, std 0.  1 <= n <= 64.  Waits for the half-iterations in flight on both sides.
 * The mean is the plain mean over the samples added (not the running Pavg of the test-set evaluation). */
BPMF_API int bpmf_hip_topn(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int n, int64_t q_from, int64_t q_to,
                           int exclude_rated, int32_t *idx_out, double *mean_out, double *std_out);

/* Ranks of held-out candidates.  Query q_from + q (q = 0 .. q_to - q_from - 1) has the held-out candidates
 * tcand[tptr[q] .. tptr[q + 1]), ascending and distinct.  With the score and the order of bpmf_hip_topn -- the same device code, the
 * same bits --
 *   rank_out[p]  = 1 + the number of candidates c' != tcand[p] in [0, cand's columns) that the query has not rated (exclude_rated != 0)
 *                  and that come before tcand[p] (higher score, or the same score and a lower index)
 *   ncand_out[q] = the number of candidates the query has not rated.
 * Other held-out candidates of the query count as ordinary candidates.  Two sweeps over the products of bpmf_hip_topn: the scores of
 * the held-out entries, then the counts; integer partials per candidate split, no atomics, no nq x nc buffer, no cap on the entries
 * of a query.  Waits.  BPMF_HIP_EINVAL: no or unequal sample rings, a query range or candidate out of bounds, candidates of a query
 * not ascending and distinct, and -- with exclude_rated -- a held-out entry that is a rated cell of the query (named). */
BPMF_API int bpmf_hip_rank_eval(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to,
                                int exclude_rated, const int64_t *tptr, const int32_t *tcand, int32_t *rank_out, int32_t *ncand_out);

/* The n best candidates by an ACQUISITION SCORE of the per-sample predictions p_s instead of their mean.
 * With mean and std as bpmf_hip_predict_block computes them (w = NULL), Phi / phi the standard normal cdf / pdf and
 * z_s = (p_s - t) / sigma:
 *   BPMF_HIP_SCORE_UCB   mean + param std                                   param = kappa, any finite value (negative: a lower bound)
 *   BPMF_HIP_SCORE_PROB  (1/S) sum_s Phi(z_s)                               param = t; sigma = 0: (1/S) #{s : p_s > t}
 *   BPMF_HIP_SCORE_EI    (1/S) sum_s [(p_s - t) Phi(z_s) + sigma phi(z_s)]  param = t; sigma = 0: (1/S) sum_s max(p_s - t, 0)
 * sigma >= 0 is an observation-noise standard deviation (1 / sqrt(alpha)); it is ignored for UCB, and a sigma below DBL_MIN
 * (a subnormal) takes the sigma = 0 forms.  Everything else is
 * bpmf_hip_topn's: the order (score descending, lower candidate index first), exclude_rated, the padding (idx -1, zeros), the
 * preconditions and the waits.  1 <= n <= 32.  BPMF_HIP_EINVAL also for an unknown kind, a non-finite param and a sigma that is
 * negative or not finite.  score_out / mean_out / std_out / idx_out: (q_to - q_from) x n row-major host arrays; mean and std of
 * a pick have the bits bpmf_hip_predict_block gives that pair. */
enum { BPMF_HIP_SCORE_UCB = 0, BPMF_HIP_SCORE_PROB = 1, BPMF_HIP_SCORE_EI = 2 };
BPMF_API int bpmf_hip_topn_scored(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int n, int64_t q_from, int64_t q_to,
                                  int exclude_rated, int kind, double param, double sigma, int32_t *idx_out, double *score_out,
                                  double *mean_out, double *std_out);

/* SIMILAR COLUMNS of one side: the n nearest neighbours of every column q_from .. q_to - 1 of `side` among
 * the side's own columns, by a similarity that no rotation of the latent space changes.  With v_s(c) column c of kept sample s
 * (S >= 1 samples in the side's ring), d_s = v_s(q) . v_s(c), n_s(c) = |v_s(c)|^2, r_s(c) = 1 / sqrt(n_s(c)) (0 where n_s(c) = 0):
 *   BPMF_HIP_SIM_COSINE  x_s = clamp(d_s * (r_s(q) * r_s(c)), -1, 1)      a column of norm zero has cosine 0 with everything
 *   BPMF_HIP_SIM_EUCLID  x_s = -max((n_s(q) + n_s(c)) - 2 d_s, 0)         the negative squared distance
 *   mean = (1/S) sum_s x_s,  std = sqrt(sum_s (x_s - mean)^2 / (S - 1)) (0 for S = 1),  score = mean - kappa std, kappa >= 0 finite
 * (kappa = 0: the plain posterior-mean similarity; kappa > 0: neighbours the posterior is sure about).  The order is
 * bpmf_hip_topn_scored's: score descending, lower column index first.  A query is never its own neighbour.  cand_ok: NULL, or one
 * host byte per column of the side, != 0 meaning the column may be listed (it does not restrict the queries).  Empty slots have
 * idx -1 and zeros.  1 <= n <= 32.  idx_out / score_out / mean_out / std_out: (q_to - q_from) x n row-major host arrays.
 * x_s(q, c) and x_s(c, q) have the same bits, and the bits of a pair depend on its two columns alone: not on the ranges, the
 * candidate splits, the mask or the call.  Supported range: every n_s(c) is 0 or within [2^-900, 2^900] (cosine) / [2^-500, 2^500] (euclid: its variance
 * squares a squared norm); outside it nothing
 * traps, and an element whose score is -inf or not a number is not listed.  Works on fp32 contexts (the ring is fp64).  Waits.
 * BPMF_HIP_EINVAL: no ring or an empty one, an unknown kind, kappa negative or not finite, n outside 1 .. 32, a range out of
 * bounds or with q_to < q_from, a side that does not hold all its columns or a context with a communicator.
 *
 * bpmf_hip_similar_block: mean_out / std_out ((q_to - q_from) x (c_to - c_from), row-major, host) of the dense block of pairs,
 * the diagonal included, bit for bit the values the lists carry.
 * bpmf_hip_similar_last_ms: device time between two events around the newest bpmf_hip_similar of the side (norm table, ranking, merge). */
enum { BPMF_HIP_SIM_COSINE = 0, BPMF_HIP_SIM_EUCLID = 1 };
BPMF_API int bpmf_hip_similar(bpmf_hip_side *side, int kind, double kappa, int n, int64_t q_from, int64_t q_to,
                              const uint8_t *cand_ok, int32_t *idx_out, double *score_out, double *mean_out, double *std_out);
BPMF_API int bpmf_hip_similar_block(bpmf_hip_side *side, int kind, int64_t q_from, int64_t q_to, int64_t c_from, int64_t c_to,
                                    double *mean_out, double *std_out);
BPMF_API int bpmf_hip_similar_last_ms(const bpmf_hip_side *side, float *ms);

/* ---- dense blocks of predictions; rows unseen in training ---------
 * bpmf_hip_predict_block: for every query column q in [q_from, q_to) of `query` and every candidate column c in [c_from, c_to)
 * of `cand`, from the sample rings of both sides (the same S >= 1 samples, bpmf_hip_side_samples_add): mean and std as
 * bpmf_hip_topn defines them, to the host arrays mean_out / std_out, (q_to - q_from) x (c_to - c_from) row-major.  One kernel,
 * no intermediate of S blocks; an element's bits do not depend on the ranges or the call.  Works on fp32 contexts (the rings are
 * fp64).  Waits.  The observation noise 1 / alpha is NOT part of std.
 * bpmf_hip_predict_block_device: the same with mean_dev / std_dev in device memory of the context's device (anything else is
 * BPMF_HIP_EINVAL), which the kernel writes in place: for a consumer on the device, and for timing the kernel without the copies.
 *
 * New rows: a side with features draws u ~ N(mu_s + beta_s^T f, Lambda_s^-1) in kept sample s, so an entity that was not in the
 * training matrix is predicted from its features f alone: e_s = mu_s + beta_s^T f, p_s = mean_rating + e_s . v_s(c),
 *   mean = (1/S) sum_s p_s,   var = sum_s (p_s - mean)^2 / (S - 1) + (1/S) sum_s v_s(c)^T Lambda_s^-1 v_s(c),   std = sqrt(var)
 * (the law of total variance over the kept samples; the first term is 0 for S = 1; 1 / alpha is not included).
 *   _newrows_set / _set_sparse  n_new >= 1 feature rows (dense: n_new x D row-major, D that of the side's features; sparse:
 *       canonical CSR as bpmf_hip_side_set_features_sparse, vals NULL = ones) of the same kind as the side's features, finite, and
 *       room for max_samples projected samples.  Calling again replaces them; max_samples = 0 frees them (side_destroy does too).
 *       BPMF_HIP_ENOMEM names the size that did not fit.
 *   _newrows_add(side, other)   where bpmf_hip_side_link_add sits, after a post-burn-in iteration with both sides sampled:
 *       projects the new rows into the next slot with the side's current beta, mu, and adds v(c)^T Lambda^-1 v(c) of the current
 *       factors of `other` and the side's current Lambda to w[c].  Enqueue only.  BPMF_HIP_EINVAL once max_samples are held.
 *   _newrows_get                E (n_new x S x K, the projected factors) and w (one per column of `other`, divided by S); either
 *       may be NULL.  Waits.
 *   _newrows_get_padded         E as the ring stores it, n_new x S x Kp with Kp = K rounded up to a multiple of 4: the components
 *       k >= K of every sample are the zero padding the kernels rely on.  Waits.
 *   bpmf_hip_newrows_predict    bpmf_hip_predict_block with the new rows of `side` as the queries and the sample ring of `cand`
 *       (the side's partner; the same number >= 1 of samples, else BPMF_HIP_EINVAL) as the candidates, std with the second term.
 *   bpmf_hip_newrows_topn       bpmf_hip_topn without exclusion (new rows rated nothing) with the new rows as the queries
 *       (new_are_queries != 0: n_new x n) or as the candidates (0: for every column of `cand` the n best new rows, ncols x n);
 *       std is the total one.
 * Every entry point needs both sides whole on a context without a communicator. */
BPMF_API int bpmf_hip_predict_block(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to,
                                    int64_t c_from, int64_t c_to, double *mean_out, double *std_out);
BPMF_API int bpmf_hip_predict_block_device(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to,
                                           int64_t c_from, int64_t c_to, double *mean_dev, double *std_dev);
BPMF_API int bpmf_hip_side_newrows_set(bpmf_hip_side *side, int64_t n_new, const double *F_host, int max_samples);
BPMF_API int bpmf_hip_side_newrows_set_sparse(bpmf_hip_side *side, int64_t n_new, const int64_t *rowptr, const int32_t *colidx,
                                              const double *vals, int max_samples);
BPMF_API int bpmf_hip_side_newrows_add(bpmf_hip_side *side, bpmf_hip_side *other);
BPMF_API int bpmf_hip_side_newrows_count(const bpmf_hip_side *side);
BPMF_API int bpmf_hip_side_newrows_get(bpmf_hip_side *side, double *E_host, double *w_host);
BPMF_API int bpmf_hip_side_newrows_get_padded(bpmf_hip_side *side, double *E_host);
BPMF_API int bpmf_hip_newrows_predict(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to,
                                      int64_t c_from, int64_t c_to, double *mean_out, double *std_out);
BPMF_API int bpmf_hip_newrows_topn(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int n, int new_are_queries,
                                   int32_t *idx_out, double *mean_out, double *std_out);

/* ---- fold-in: new rows from their ratings against the kept samples ---------
 * A row i that arrives after training with ratings {(j, r_ij)} over the columns of `cand` and no features.  Given kept sample s of
 * `cand` (v_js, its sample ring) and the hyper-parameters (alpha_s, mu_s, Lambda_s) the side of the row ran with at that iteration,
 *   Lambda* = Lambda_s + alpha_s sum_j v_js v_js^T,   b = Lambda_s mu_s + alpha_s sum_j (r_ij - mean_rating) v_js,
 *   Lambda* = L L^T,   u_is = L^-T (L^-1 b + z),   z ~ N(0, I)
 * the conditional bpmf_hip_sample_side draws from; no rating: a draw from the prior N(mu_s, Lambda_s^-1).  The influence of the
 * row on `cand` and on the hyper-parameters is ignored.  fp64 on every context.
 *   _hyper_reserve(side, max)   room for the hyper-parameters of max kept samples of the side (host memory); again: an empty ring
 *       of the new size; 0 frees it.
 *   _hyper_add(side, alpha, mu, LambdaF)   the next slot: alpha finite >= 0, mu (K), LambdaF (K x K, symmetric), finite.  mu ==
 *       NULL && LambdaF == NULL: the hyper-parameters the side's newest bpmf_hip_sys_sample ran with (waits for its collection,
 *       as bpmf_hip_sys_state); call it where bpmf_hip_side_samples_add of the OTHER side sits.  BPMF_HIP_EINVAL once the ring
 *       is full.
 *   _hyper_get                  the held slots: alpha (S), mu (S x K), LambdaF (S x K x K, each as given); any may be NULL.
 *   bpmf_hip_foldin(side, cand, mean_rating, n_new, rowptr, colidx, vals, tag, draw)   n_new >= 1 rows by rows (rowptr n_new + 1
 *       entries from 0, monotone; colidx in [0, cand's columns), strictly ascending within a row -- a column listed twice is an
 *       error that names row and column; vals finite), checked on the host before the device is used.  The hyper ring of `side`
 *       and the sample ring of `cand` must hold the same number S >= 1 of samples.  tag >= 1 names the random streams: block n
 *       of (row i of the batch, slot s) is Philox (i lo, i hi, s, n; 42, tag) and gives the normals 2 n, 2 n + 1 by Box-Muller,
 *       so the factors of a row depend on its index in the batch, not on the other rows; draw == 0: z = 0, the conditional
 *       mean.  Replaces an earlier set; n_new = 0 frees it.  Waits.  BPMF_HIP_ECHOL names a row with a pivot that is not positive
 *       and finite: its factors are stored as zeros, the set is kept.  BPMF_HIP_ENOMEM names the size that did not fit.
 *   _foldin_get / _get_padded   the factors, n_new x S x K / as the ring stores them, n_new x S x Kp (Kp = K rounded up to a
 *       multiple of 4, pad components 0).
 *   _foldin_predict             bpmf_hip_predict_block with the folded-in rows as the queries: a folded-in row is predicted like a
 *       row that had been in the matrix (the draw carries its uncertainty; 1 / alpha is not part of std).
 *   _foldin_topn                bpmf_hip_topn with the folded-in rows as the queries (n_new x n); exclude_rated != 0: without the
 *       columns the row itself rated.
 * Refused (BPMF_HIP_EINVAL): a communicator or a sharded side, the BPMF_REDUCE formulation, propagated priors, a probit side, and
 * a `side` with features (bpmf_hip_side_newrows_set predicts such rows).  A censored training side is fine; the ratings of a
 * folded-in row are exact values.  bpmf_hip_foldin_chunk: the ratings the kernel stages per pass (tests). */
BPMF_API int bpmf_hip_side_hyper_reserve(bpmf_hip_side *side, int max_samples);
BPMF_API int bpmf_hip_side_hyper_add(bpmf_hip_side *side, double alpha, const double *mu, const double *LambdaF);
BPMF_API int bpmf_hip_side_hyper_count(const bpmf_hip_side *side);
BPMF_API int bpmf_hip_side_hyper_get(const bpmf_hip_side *side, double *alpha, double *mu, double *LambdaF);
BPMF_API int bpmf_hip_foldin(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int64_t n_new, const int64_t *rowptr,
                             const int32_t *colidx, const double *vals, unsigned tag, int draw);
BPMF_API int bpmf_hip_foldin_count(const bpmf_hip_side *side);      /* n_new of the held set (0: none) */
BPMF_API int bpmf_hip_foldin_samples(const bpmf_hip_side *side);    /* S of the held set */
BPMF_API int bpmf_hip_foldin_get(bpmf_hip_side *side, double *E_host);
BPMF_API int bpmf_hip_foldin_get_padded(bpmf_hip_side *side, double *E_host);
BPMF_API int bpmf_hip_foldin_predict(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to,
                                     int64_t c_from, int64_t c_to, double *mean_out, double *std_out);
BPMF_API int bpmf_hip_foldin_topn(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int n, int exclude_rated,
                                  int32_t *idx_out, double *mean_out, double *std_out);
BPMF_API int bpmf_hip_foldin_last_ms(const bpmf_hip_side *side, float *ms);   /* device time of the newest launch of the kernel, between two events */
BPMF_API int bpmf_hip_foldin_chunk(void);

/* ---- saved models: ring read-back and load, predictions for a list of cells ----
 *   bpmf_hip_side_samples_get reads slots [s_from, s_to) of the side's sample ring without the pad rows:
 * ncols x (s_to - s_from) x num_latent doubles, column c / sample s / row k at host[(c n + s) K + k], n = s_to - s_from.  It
 * waits.  BPMF_HIP_EINVAL without a ring or for a range beyond bpmf_hip_side_samples_count.
 * bpmf_hip_side_samples_set is the inverse: `nsamples` samples in the same layout (s_from = 0) into a ring reserved with
 * max_samples >= nsamples; the pad rows are written as zeros (the ranking kernels rely on them); afterwards the ring counts
 * nsamples.  A value that is not finite is refused with its column and sample, before the device is touched.
 * Together with bpmf_hip_side_hyper_get / _hyper_reserve / _hyper_add this is all a process needs to serve bpmf_hip_topn*,
 * _rank_eval, _predict_block and _foldin* from a model another process trained. */
BPMF_API int bpmf_hip_side_samples_get(bpmf_hip_side *side, int s_from, int s_to, double *host);
BPMF_API int bpmf_hip_side_samples_set(bpmf_hip_side *side, int nsamples, const double *host);
/* For the n cells (q[i], c[i]) -- column q[i] of `query`, column c[i] of `cand`; any order, repeats allowed, n = 0 allowed --
 * with p_s = mean_rating + u_s(q) . v_s(c) over the S >= 1 samples both rings hold: mean_out[i] and std_out[i] as bpmf_hip_topn
 * defines them (std: 0 for S = 1; 1 / alpha is NOT included), and with want_prob prob_out[i] = (1/S) sum_s Phi((p_s - t) / sigma),
 * the formula of BPMF_HIP_SCORE_PROB (sigma < DBL_MIN: the share of samples with p_s > t).  prob_out may be NULL without
 * want_prob.  An index out of range is BPMF_HIP_EINVAL naming the cell, before the device is used.  The bits of a cell depend on
 * the rings, (q, c), mean_rating, t and sigma alone: not on the other cells, its place in the list or the launch.  Works on
 * fp32 contexts (the rings are fp64); needs both sides whole and no communicator.  Waits. */
BPMF_API int bpmf_hip_predict_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q,
                                    const int32_t *c, int want_prob, double t, double sigma, double *mean_out, double *std_out,
                                    double *prob_out);
BPMF_API int bpmf_hip_predict_cells_last_ms(const bpmf_hip_side *query, float *ms);   /* device time of the newest launch with `query` as the queries */

/* ---- convergence diagnostics: split-Rhat and ESS ----
 *   For one trace x_0 .. x_{S-1} in chronological order, 8 <= S <= BPMF_HIP_DIAG_MAX_SAMPLES, with
 * n = floor(S / 2), the halves A = x[0, n) and B = x[S - n, S), per half the mean m_h, d = x - m_h and
 * c_h(t) = (1/n) sum_{i <= n-1-t} d_i d_{i+t}, c(t) = (c_A(t) + c_B(t)) / 2:
 *     W = c(0) n / (n - 1),  var+ = c(0) + (m_A - m_B)^2 / 2,  rhat = sqrt(var+ / W),  rho_t = 1 - (W - c(t)) / var+,
 *     P_0 = 1 + rho_1,  P_k = min(rho_2k + rho_2k+1, P_k-1) while 2k + 1 <= n - 3 and the pair sum is > 0,
 *     tau = max(-1 + 2 sum_k P_k, 1 / log10(2n)),  ess = 2n / tau
 * -- the split-chain estimator of Vehtari et al. (2021) without rank normalisation.  A trace with W not > 0 (constant, or holding
 * a value that is not finite) gives NaN for both.  All fp64, also on fp32 contexts; the bits of a trace depend on the trace
 * alone: not on its place, the batch or the launch.
 * bpmf_hip_diag_traces: n >= 0 traces of S samples, row-major on the host.  BPMF_HIP_EINVAL: S outside the range, a NULL argument.
 * bpmf_hip_diag_cells: the traces are p_s = mean_rating + u_s(q[i]) . v_s(c[i]) over the S samples both rings hold (mean_rating
 * drops out of both figures); mean_out and std_out are those of bpmf_hip_predict_cells, bit for bit.  Its checks and refusals are
 * those of bpmf_hip_predict_cells, and S outside the range.  The list is processed in batches of cells whose traces fit a fixed
 * buffer; bpmf_hip_diag_batch_cells sets the cells per batch (0: automatic) for tests: results do not depend on it.  Waits.
 * bpmf_hip_diag_last_ms: device time of the kernels of the newest bpmf_hip_diag_cells with `query` as the queries. */
#define BPMF_HIP_DIAG_MAX_SAMPLES 4096
BPMF_API int bpmf_hip_diag_traces(bpmf_hip_ctx *ctx, int64_t n, int S, const double *traces, double *rhat, double *ess);
BPMF_API int bpmf_hip_diag_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q,
                                 const int32_t *c, double *mean_out, double *std_out, double *rhat_out, double *ess_out);
BPMF_API int bpmf_hip_diag_batch_cells(int cells);
BPMF_API int bpmf_hip_diag_last_ms(const bpmf_hip_side *query, float *ms);

/* ---- convergence diagnostics over several chains: rank-normalised split-Rhat, bulk and tail ESS ----
 * (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021.)  A trace is C * S doubles, chain-major: chain c is
 * x[c S, (c + 1) S), chronological inside; 1 <= C <= 64, S >= 8, C S <= BPMF_HIP_DIAG_MAX_SAMPLES.  With n = floor(S / 2) every chain
 * gives the half-chains x_c[0, n) and x_c[S - n, S): M = 2C half-chains, N = M n kept values.  est(y) is the estimator of the section
 * above with the two halves generalised to M half-chains: c(t) = (1 / N) sum over the half-chains of sum_i d_i d_{i+t},
 * W = c(0) n / (n - 1), var+ = c(0) + sum_h (m_h - mbar)^2 / (M - 1), tau = max(-1 + 2 sum_k P_k, 1 / log10 N), ess = N / tau.
 * z(y) replaces every value by the normal score of its rank among the N (average ranks for values that compare equal):
 * z = -+ sqrt 2 erfcinv((2a - 0.75) / (N + 0.25)), a = min(r, N + 1 - r).
 *     rhat     = max(est(z(x)).rhat, est(z(|x - med|)).rhat), med the mean of the two middle order statistics
 *     ess_bulk = est(z(x)).ess
 *     ess_tail = min over p in {0.05, 0.95} of est(1[x <= x_(floor((N - 1) p) + 1)]).ess
 * An est with W not > 0 gives NaN for what depends on it (a constant trace, chains that are each constant, a tail indicator that is
 * constant in every half-chain); a value that is not finite anywhere in the trace gives NaN for all three, for that trace alone.
 * All fp64, also on fp32 contexts; the bits of a trace depend on the trace alone.
 * bpmf_hip_diag_traces_mc: n >= 0 traces, row-major on the host.  BPMF_HIP_EINVAL: C or S outside the ranges, a NULL argument.
 * bpmf_hip_diag_cells_mc: as bpmf_hip_diag_cells over two rings that hold exactly C S samples in chain-major order (what
 * bpmf_hip_samples_set of C chains one after the other leaves); its refusals, C and S outside the ranges, and a number of samples
 * that C does not divide.  mean_out and std_out are those of bpmf_hip_predict_cells, bit for bit.  bpmf_hip_diag_batch_cells and
 * bpmf_hip_diag_last_ms serve it as they serve bpmf_hip_diag_cells.  Waits. */
#define BPMF_HIP_DIAG_MAX_CHAINS 64
BPMF_API int bpmf_hip_diag_traces_mc(bpmf_hip_ctx *ctx, int64_t n, int C, int S, const double *traces, double *rhat, double *ess_bulk,
                                     double *ess_tail);
BPMF_API int bpmf_hip_diag_cells_mc(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q,
                                    const int32_t *c, int C, double *mean_out, double *std_out, double *rhat_out, double *ess_bulk_out,
                                    double *ess_tail_out);

/* ---- model comparison: log pointwise predictive density and WAIC ----
 *   For the observed cell i = (q[i], c[i]) with the value y[i], over the S samples both rings hold, with
 * p_s = mean_rating + u_s(q[i]) . v_s(c[i]) and l_s = log p(y[i] | sample s):
 *     lpd[i] = log((1/S) sum_s exp l_s),   pwaic[i] = sum_s (l_s - lbar)^2 / (S - 1)   (0 for S = 1)
 * so that sum_i lpd[i] is the log score of held-out cells and sum_i (lpd[i] - pwaic[i]) the WAIC estimate of the expected log
 * pointwise predictive density of training cells.  l_s by kind, with alpha_s the noise precision sample s ran with (alpha[0] for
 * nalpha = 1, else alpha[s] in ring-slot order, nalpha = S) and w[i] the weight of the cell (NULL: 1):
 *     BPMF_HIP_LOGDENS_GAUSSIAN   (1/2) log(alpha_s w_i / 2 pi) - (1/2) alpha_s w_i (y_i - p_s)^2
 *         a cell with flag[i] = +-1 (a censored value: y_i is a bound; flag NULL: none): log Phi(flag sqrt(alpha_s) (p_s - y_i))
 *     BPMF_HIP_LOGDENS_STUDENT    lgamma((nu+1)/2) - lgamma(nu/2) + (1/2) log(alpha_s / (nu pi)) - ((nu+1)/2) log1p(alpha_s (y_i - p_s)^2 / nu)
 *     BPMF_HIP_LOGDENS_PROBIT     log Phi(p_s) for y_i > 0 (a positive label), log Phi(-p_s) otherwise
 * All fp64, also on fp32 contexts.  The sum over s is a streaming log-sum-exp in s order and the variance a Welford recurrence; log Phi
 * stays finite in both tails.  mean and std are those of bpmf_hip_predict_cells, bit for bit.  The bits of a cell depend on the cell,
 * S and the kind alone: not on the other cells, its place in the list or the batches (bpmf_hip_score_batch_cells sets the cells per
 * launch, 0: automatic, for tests).  Checked on the host before any launch, BPMF_HIP_EINVAL with a line that names the first
 * offending cell: what bpmf_hip_predict_cells refuses, a NULL argument, nalpha that is neither 1 nor S, an alpha or w that is not
 * finite and > 0, a y that is not finite, w or flags with a kind other than gaussian, a flag outside {-1, 0, +1}, nu not finite or
 * < 1 for student.  n = 0 launches nothing.  Waits.
 * bpmf_hip_score_last_ms: device time of the kernels of the newest bpmf_hip_score_cells with `query` as the queries. */
#define BPMF_HIP_LOGDENS_GAUSSIAN 0
#define BPMF_HIP_LOGDENS_STUDENT 1
#define BPMF_HIP_LOGDENS_PROBIT 2
BPMF_API int bpmf_hip_score_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q,
                                  const int32_t *c, const double *y, const double *w, const int8_t *flag, int kind, double nu,
                                  int nalpha, const double *alpha, double *lpd, double *pwaic, double *mean, double *std);
BPMF_API int bpmf_hip_score_batch_cells(int cells);
BPMF_API int bpmf_hip_score_last_ms(const bpmf_hip_side *query, float *ms);

/* ---- predictive intervals: probability integral transform and quantiles of the posterior predictive ----
 *   For the cell i = (q[i], c[i]) with the weight w_i = w[i] (NULL: 1), over the S samples both rings hold,
 * with p_s = mean_rating + u_s(q[i]) . v_s(c[i]) and alpha_s the noise precision sample s ran with (alpha[0] for nalpha = 1, else
 * alpha[s] in ring-slot order, nalpha = S: the convention of bpmf_hip_score_cells), the posterior predictive of the cell is the mixture
 *     F_i(x) = (1/S) sum_s Phi((x - p_s) sqrt(alpha_s w_i)),   Phi(t) = erfc(-t / sqrt 2) / 2
 *     pit[i] = F_i(y[i])                 the probability integral transform of the observed value y[i] (y NULL: none)
 *     quant[i * nq + j] = F_i^-1(tau[j])  F_i increases strictly, so the root is unique
 * A central interval of level l is [F^-1((1 - l) / 2), F^-1((1 + l) / 2)], and y[i] lies inside it exactly when |pit[i] - 1/2| <= l / 2.
 * 0 <= nq <= BPMF_HIP_INTERVAL_MAX_QUANTILES, tau strictly increasing, every tau in [0.001, 0.999]; 1 <= S <= BPMF_HIP_INTERVAL_MAX_SAMPLES.
 * The root is found in x - mean_rating by a Newton iteration kept inside the bracket of the component quantiles, with at most 128
 * evaluations of F (kernels_interval.h); tau > 1/2 is solved on the survival function.  All fp64, also on fp32 contexts; quantiles never
 * decrease in tau.  mean and std (either may be NULL) are those of bpmf_hip_predict_cells, bit for bit.  The bits of a cell depend on
 * the cell, S, the alphas, its weight, its y and the taus alone: not on the other cells, its place in the list or the batches
 * (bpmf_hip_interval_batch_cells sets the cells per batch, 0: automatic, for tests).  A cell whose trace holds a value that is not
 * finite gets NaN, and no other cell does.  Checked on the host before any launch, BPMF_HIP_EINVAL with a line that names the first
 * offender: what bpmf_hip_predict_cells refuses, nq outside the range, nothing to do (y NULL and nq = 0), a tau outside the range or
 * not increasing, nalpha that is neither 1 nor S, an alpha or w that is not finite and > 0, a y that is not finite, S above the
 * range, pit NULL with y given or quant NULL with nq > 0.  n = 0 launches nothing.  Waits.
 * bpmf_hip_interval_traces: the same for n traces d_s = p_s - mean_rating of S samples given by the host, row-major (y, w per trace).
 * bpmf_hip_interval_last_ms: device time of the kernels of the newest bpmf_hip_interval_cells with `query` as the queries. */
#define BPMF_HIP_INTERVAL_MAX_SAMPLES 4096
#define BPMF_HIP_INTERVAL_MAX_QUANTILES 8
BPMF_API int bpmf_hip_interval_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q,
                                     const int32_t *c, const double *y, const double *w, int nalpha, const double *alpha, int nq,
                                     const double *tau, double *pit, double *quant, double *mean, double *std);
BPMF_API int bpmf_hip_interval_traces(bpmf_hip_ctx *ctx, int64_t n, int S, const double *traces, double mean_rating, const double *y,
                                      const double *w, int nalpha, const double *alpha, int nq, const double *tau, double *pit,
                                      double *quant);
BPMF_API int bpmf_hip_interval_batch_cells(int cells);
BPMF_API int bpmf_hip_interval_last_ms(const bpmf_hip_side *query, float *ms);

/* ---- PSIS-LOO: leave-one-out cross-validation of observed cells by Pareto-smoothed importance sampling ----
 * (Vehtari, Gelman & Gabry 2017; Vehtari et al. 2024.)  For one cell, l_s is its log density under kept sample s
 * (the likelihoods of bpmf_hip_score_cells), s = 0 .. S - 1, 1 <= S <= BPMF_HIP_LOO_MAX_SAMPLES.  Everything is fp64, also on fp32 contexts.
 *  1. r_s = -l_s, shifted so that max_s r_s = 0; r_(0) <= .. <= r_(S-1) are the sorted values.
 *  2. The tail length is M = min(floor(0.2 S), ceil(3 sqrt S)) (the relative efficiency is taken as 1; M <= 192).  M < 5 (S < 25): no
 *     smoothing, khat = +infinity.
 *  3. The cutoff is c = r_(S-M-1); the tail excesses are x_j = exp(r_(S-M-1+j)) - exp(c), j = 1 .. M, ascending.  x_M = x_1 (a constant
 *     tail), or x at the index floor(M/4 + 1/2) equal to 0: no smoothing, khat = +infinity.
 *  4. The generalised Pareto fit of Zhang & Stephens 2009: m = 30 + floor(sqrt M), x* = x at the index floor(M/4 + 1/2) (1-based),
 *     theta_j = 1 / x_M + (1 - sqrt(m / (j - 1/2))) / (3 x*), j = 1 .. m;  k_j = (1/M) sum_i log1p(-theta_j x_i);
 *     L_j = M (log(-theta_j / k_j) - k_j - 1);  w_j = exp(L_j - max L) / sum_j exp(L_j - max L);  theta^ = sum_j w_j theta_j;
 *     k = (1/M) sum_i log1p(-theta^ x_i);  sigma = -k / theta^;  khat = (k M + 5) / (M + 10).  An L_j, theta^, k, sigma or khat that is
 *     not finite: no smoothing, khat = +infinity.
 *  5. The smoothed tail: p_j = (j - 1/2) / M, t_j = -log1p(-p_j), q_j = sigma expm1(khat t_j) / khat (sigma t_j for |khat| < 1e-30),
 *     lw_(S-M-1+j) = min(log(q_j + exp(c)), 0); every other lw_s = r_s.
 *  6. elpd_loo = logsumexp_s(lw_s + l_s) - logsumexp_s(lw_s);  lpd = logsumexp_s(l_s) - log S;  khat as above.
 * On the host: p_loo = lpd - elpd_loo and looic = -2 sum elpd_loo.  khat <= 0.7 (for small S: min(1 - 1 / log10 S, 0.7)) says that the
 * estimate of the cell can be trusted.  Every sum runs over the positions of the sorted order -- a lane adds positions lane, lane + 64, ..
 * in increasing order, then the 64 lanes add by a butterfly (xor 32 .. 1); the M terms of a k_j are added in increasing i -- so the bits
 * of a cell depend on the cell, S, the kind and its parameters alone: not on the other cells, its place in the list or the batches
 * (bpmf_hip_loo_batch_cells sets the cells per batch, 0: automatic, for tests).  No atomics.  A trace holding a value that is not finite
 * gives NaN in its own three outputs and touches no other trace.
 * bpmf_hip_loo_cells: the arguments, checks and refusals of bpmf_hip_score_cells (y, w, flag, kind, nu, nalpha, alpha), and S above
 * BPMF_HIP_LOO_MAX_SAMPLES is refused; lpd, mean and std may be NULL; mean and std are those of bpmf_hip_predict_cells, bit for bit.
 * n = 0 launches nothing.  Waits.
 * bpmf_hip_loo_traces: the same rule for n traces of l_s given by the host, row-major (n x S); lpd may be NULL.
 * bpmf_hip_loo_last_ms: device time of the kernels of the newest bpmf_hip_loo_cells with `query` as the queries. */
#define BPMF_HIP_LOO_MAX_SAMPLES 4096
BPMF_API int bpmf_hip_loo_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q,
                                const int32_t *c, const double *y, const double *w, const int8_t *flag, int kind, double nu, int nalpha,
                                const double *alpha, double *elpd_loo, double *khat, double *lpd, double *mean, double *std);
BPMF_API int bpmf_hip_loo_traces(bpmf_hip_ctx *ctx, int64_t n, int S, const double *logdens, double *elpd_loo, double *khat, double *lpd);
BPMF_API int bpmf_hip_loo_batch_cells(int cells);
BPMF_API int bpmf_hip_loo_last_ms(const bpmf_hip_side *query, float *ms);

/* ---- adaptive noise precision -------------------------------------------------
 * SSE = sum over the ratings of `side` (row r, column c, value v) of (v - mean_rating - x_c . y_r)^2, x = side's current
 * factors, y = other's (other has one column per row of side's ratings); *n = the number of those ratings.  fp64 throughout
 * (fp32 factors are widened), a fixed order of summation: the same bits on every call.  Enqueued on the context stream behind
 * the newest sampler of both sides (bpmf_hip_sys_sample or bpmf_hip_sample_side), on the copy of the factors it writes; waits
 * for the sum.  Both sides whole on a context without a communicator, else BPMF_HIP_EINVAL. */
BPMF_API int bpmf_hip_train_sse(bpmf_hip_side *side, bpmf_hip_side *other, double *sse, int64_t *n);
/* Host only.  The noise precision of iteration iter + 1 after iteration iter left SSE `sse` over n training ratings, with a
 * Gamma(a0, b0) prior (shape, rate): *alpha = g / (b0 + sse / 2), g ~ Gamma(a0 + n / 2, 1) drawn with libstdc++'s
 * gamma_distribution on the Philox stream BPMF_NOISE_COUNTER(iter) (the top of the counter range, counting down: apart from
 * the hyper-parameter streams, which count up from 0).  alpha_max > 0 caps the result; <= 0: no cap.  BPMF_HIP_EINVAL for
 * a0 <= 0, b0 < 0, n <= 0, iter < 0, a negative or non-finite sse, or b0 = sse = 0. */
#define BPMF_NOISE_COUNTER(iter) (0xFFFFFFFFu - (uint32_t)(iter))
BPMF_API int bpmf_hip_noise_sample(double a0, double b0, double sse, int64_t n, int iter, double alpha_max, double *alpha);

/* ---- probit likelihood for binary matrices ---------------------------------------
 * A rating v is a label: positive (s = +1) if v > threshold, else negative (s = -1).  Every rating p of a probit side carries a
 * latent score z_p whose sign is s_p (Albert-Chib); the column samplers read the scores in place of the ratings, with mean 0
 * and alpha = 1.  DESIGN.md section 12 has the model and the draw.
 *
 * bpmf_hip_side_set_probit turns `side` into a probit side: it allocates the latent array (layout of the side's ratings, which
 * are never written), derives the signs once on the device, and from then on every sampler launch of the side
 * (bpmf_hip_sys_sample, bpmf_hip_sample_side[_launch]; iteration `iter`) is preceded on the same stream by the latent step
 *     m = x_c . y_r  (x: the side's factors before this update, y: the other side's newest; fp64),
 *     z_p ~ N(m, 1) truncated to (0, inf) if s_p = +1, to (-inf, 0) otherwise,
 * drawn from the Philox4x32-10 blocks (counter = p low, p high, iter, attempt; key = 42, tag).  tag >= 1 keeps the side's
 * streams apart from every other stream of the library (key word 1 = 0) and from the other side's (give the two sides different
 * tags).  Such a side must be sampled with alpha = 1.  No host wait is added to the sampling calls, and the
 * latent step is ahead of the wait for the hyper-parameters in the queue (it needs none).  A draw rejected 64 times
 * (probability < 2^-128 per rating with finite factors) stores s_p and makes the sampling call that collects the
 * half-iteration fail with BPMF_HIP_ENUM.
 * BPMF_HIP_EINVAL: mean_rating != 0, tag = 0, a non-finite threshold, a context with a communicator, a sharded side, the
 * BPMF_REDUCE formulation on, or a side that is a probit side already. */
BPMF_API int bpmf_hip_side_set_probit(bpmf_hip_side *side, double threshold, unsigned tag);
/* The side's latent scores as the newest sampler launch read them, nnz doubles in the order of the side's ratings (waits for
 * the work in flight). */
BPMF_API int bpmf_hip_side_probit_latent(bpmf_hip_side *side, double *z_host);
/* Adds Phi(x_c . y_r) of the current factors of `self` (the side of `test`) and `other` to the running sum of every entry of
 * the test matrix.  Enqueued on the context stream behind the newest sampler of both sides, on the copies of the factors they
 * wrote; does not wait.  Both sides whole on a context without a communicator, else BPMF_HIP_EINVAL. */
BPMF_API int bpmf_hip_test_probit_add(bpmf_hip_test *test, bpmf_hip_side *self, bpmf_hip_side *other);
/* The mean of the added probabilities per entry, in the order of the test matrix as given to bpmf_hip_test_create, and the
 * number of samples added (nsamples may be NULL).  Waits.  BPMF_HIP_EINVAL when nothing was added. */
BPMF_API int bpmf_hip_test_probit_get(bpmf_hip_test *test, double *prob_host, int *nsamples);
/* Host only.  Area under the ROC curve of `score` against the labels value[i] > threshold: the fraction of (positive, negative)
 * pairs that the score orders correctly, ties counted half (average ranks).  *auc = NaN when one class is empty (n = 0
 * included).  BPMF_HIP_EINVAL for NULL arguments, n < 0 or a NaN score. */
BPMF_API int bpmf_hip_auc(const double *score, const double *value, int64_t n, double threshold, double *auc);

/* ---- ordinal probit likelihood with sampled cutpoints -----------------------------
 * The ratings of an ordinal side take one of C levels l_1 < ... < l_C (2 <= C <= 16).  A rating at level c carries a latent
 * score z with g_{c-1} < z <= g_c, z ~ N(u . v, 1), g_0 = -inf, g_C = +inf: the probit model above with C - 1 cutpoints in
 * place of the threshold.  The column samplers read the scores in place of the ratings, with mean 0 and alpha = 1.  DESIGN.md
 * section 23 has the model, the draw and the keying.
 *
 * bpmf_hip_side_set_ordinal turns `side` into an ordinal side: `levels` are the nlevels level values, strictly increasing;
 * `cutpoints` the nlevels - 1 initial cutpoints, strictly increasing, or NULL for Phi^-1 of the cumulative frequencies of the
 * side's ratings (every level counted half a rating higher when one of them has no rating).  From then on every sampler launch of
 * the side is preceded on the same stream by the latent step
 *     m = x_c . y_r,   z_p ~ N(m, 1) truncated to the interval of the level of rating p at the side's current cutpoints,
 * by inversion from ONE Philox4x32-10 block per rating (counter = p low, p high, iter, 0; key = 42, tag): no rejection, no host
 * wait, ahead of the wait for the hyper-parameters in the queue.  tag >= 1 as for a probit side (bpmf_amd.gibbs uses 11 =
 * movies, 12 = users; 1 .. 10 are taken).  Give both sides of a model the same levels and cutpoints.  A score that is not finite
 * makes the sampling call that collects the half-iteration fail with BPMF_HIP_ENUM.
 * BPMF_HIP_EINVAL: NULL, nlevels outside 2 .. 16, levels or cutpoints not finite or not strictly increasing, a rating that is not
 * a level, tag = 0, mean_rating != 0 (and, at a launch, alpha != 1), a side that is ordinal already, a probit, censored, weighted
 * or robust side, features, propagated priors, the BPMF_REDUCE formulation, a communicator or a sharded side.  In turn
 * bpmf_hip_side_set_probit, _set_censored, _set_weights, _set_robust, _set_features[_sparse], _set_prop_posterior,
 * bpmf_hip_sys_set_reduce, bpmf_hip_train_sse, the fold-in and a tensor mode refuse an ordinal side. */
BPMF_API int bpmf_hip_side_set_ordinal(bpmf_hip_side *side, const double *levels, int nlevels, const double *cutpoints, unsigned tag);
/* The number of levels, the level values (16 doubles of room) and the log-likelihood passes enqueued so far; each may be NULL. */
BPMF_API int bpmf_hip_side_ordinal_info(bpmf_hip_side *side, int *nlevels, double *levels, int64_t *loglik_launches);
/* The side's latent scores as the newest sampler launch read them, nnz doubles in the order of the side's ratings (waits). */
BPMF_API int bpmf_hip_side_ordinal_latent(bpmf_hip_side *side, double *z_host);
/* The side's nlevels - 1 cutpoints.  _cut_set waits for the work in flight (a latent kernel reads the table), then replaces them. */
BPMF_API int bpmf_hip_side_ordinal_cut_get(bpmf_hip_side *side, double *cutpoints);
BPMF_API int bpmf_hip_side_ordinal_cut_set(bpmf_hip_side *side, const double *cutpoints);
/* out[0] = sum over the ratings of `self` of log[Phi(g_y - m) - Phi(g_{y-1} - m)] at the side's cutpoints, out[1] the same at
 * `cutpoints_prop`, m = x_c . y_r of the newest factors of both sides; one pass over the ratings, no atomics, the same bits for
 * the same inputs.  Enqueues behind the newest samplers on the context stream and waits. */
BPMF_API int bpmf_hip_ordinal_loglik(bpmf_hip_side *self, bpmf_hip_side *other, const double *cutpoints_prop, double *out);
/* One Metropolis-Hastings step of all cutpoints given the factors (Cowles 1996), the scores integrated out.  For c = 1 .. C - 1
 * in turn g'_c ~ N(g_c, step^2) truncated to (g'_{c-1}, g_{c+1}); accepted with log-ratio l(g') - l(g) + sum_c (log[Phi((g_{c+1}
 * - g_c) / step) - Phi((g'_{c-1} - g_c) / step)] - log[Phi((g'_{c+1} - g'_c) / step) - Phi((g_{c-1} - g'_c) / step)]), both l from
 * one bpmf_hip_ordinal_loglik pass over the ratings of `movies`.  Random numbers: the Philox4x32-10 blocks (counter =
 * BPMF_ORDINAL_COUNTER(iter), c, 0, attempt; key = 42, 0); an attempt is one Box-Muller pair (u1 = 1 - canonical53(w3, w2), u2 =
 * canonical53(w1, w0); g_c + step sqrt(-2 ln u1) cos(2 pi u2), then ... sin(2 pi u2): the first inside the bounds), after 64
 * attempts g'_c = g_c; the accept uniform is u1 of the block c = 0, attempt 0.  *accepted = 1: both sides hold g' now.  Waits. */
#define BPMF_ORDINAL_COUNTER(iter) (0x40000000u + (uint32_t)(iter))
BPMF_API int bpmf_hip_ordinal_cut_step(bpmf_hip_side *movies, bpmf_hip_side *users, int iter, double step, int *accepted);
/* Adds the C level probabilities Phi(g_c - m) - Phi(g_{c-1} - m) of the current factors and cutpoints of `self` (the side of
 * `test`) to the running sums of every entry of the test matrix.  Enqueue only, as bpmf_hip_test_probit_add. */
BPMF_API int bpmf_hip_test_ordinal_add(bpmf_hip_test *test, bpmf_hip_side *self, bpmf_hip_side *other);
/* The mean of the added probabilities, nnz x C row-major (entry-major) in the order of the test matrix, the number of levels and
 * of samples added (either may be NULL).  Waits.  BPMF_HIP_EINVAL when nothing was added. */
BPMF_API int bpmf_hip_test_ordinal_get(bpmf_hip_test *test, double *prob_host, int *nlevels, int *nsamples);

/* ---- censored ratings (Tobit) ----------------------------------------------------
 * A training rating may be a bound on the measurement instead of the measurement.  Every rating p of a side (position in the
 * side's CSC) has a flag c_p: 0 = the recorded value b_p is the measurement, +1 = the true value is at least b_p, -1 = at most
 * b_p.  With y_p ~ N(mean_rating + x_c . y_r, 1 / alpha) a censored cell carries a latent value z_p drawn from that normal
 * truncated to (b_p, inf) or (-inf, b_p); the column samplers read z in place of the ratings, with the side's own mean rating and
 * the caller's alpha (any alpha > 0).  DESIGN.md section 16 has the model and the draw.
 *
 * bpmf_hip_side_set_censored takes the flags (nnz of them, in the order of the side's ratings), builds the lists of the censored
 * entries on the device and the array z (layout of the side's ratings, a copy of them; the ratings are never written).  From then
 * on every sampler launch of the side (bpmf_hip_sys_sample, bpmf_hip_sample_side[_launch]; iteration `iter`) is preceded on the
 * same stream by the latent step over the censored entries only, with s = c_p:
 *     m = x_c . y_r  (x: the side's factors before this update, y: the other side's newest; fp64),
 *     e = (b_p - mean_rating) - m,  a = s (sqrt(alpha) e),  t ~ N(0, 1) | t > a,  z_p = b_p + s ((t - a) / sqrt(alpha)),
 * t drawn as for a probit side from the Philox4x32-10 blocks (counter = p low, p high, iter, attempt; key = 42, tag).  tag >= 1
 * names the side's streams: different for the two sides of a model, and different from the tags of every probit side and of
 * every side with features (bpmf_amd.gibbs and `bpmf` use 5 = movies, 6 = users here; 1 / 2 probit; 3 / 4 features).  No host
 * wait is added to the sampling calls; a side whose flags are all 0 launches no kernel and samples exactly as a side without
 * flags.  A draw rejected 64 times (non-finite factors) stores b_p + s / sqrt(alpha) and makes the call that collects the
 * half-iteration fail with BPMF_HIP_ENUM.  fp32 contexts are allowed: z and the bounds are fp64 as the ratings are.
 * BPMF_HIP_EINVAL: a NULL argument, a flag outside {-1, 0, +1}, tag = 0, a side that is censored already, a probit side, a side
 * with features, propagated priors, the BPMF_REDUCE formulation, a context with a communicator or a sharded side.  In turn
 * bpmf_hip_side_set_probit, bpmf_hip_side_set_features[_sparse], bpmf_hip_sys_set_reduce and bpmf_hip_train_sse refuse a
 * censored side (the residuals of the last would take the bounds for measurements). */
BPMF_API int bpmf_hip_side_set_censored(bpmf_hip_side *side, const int8_t *flags, unsigned tag);
/* The numbers of lower bounds (flag +1) and upper bounds (flag -1) of a censored side. */
BPMF_API int bpmf_hip_side_censored_count(bpmf_hip_side *side, int64_t *right, int64_t *left);
/* The array z as the side's newest sampler launch read it, nnz doubles in the order of the side's ratings: the ratings at the
 * exact positions, the newest draws at the censored ones (waits for the work in flight). */
BPMF_API int bpmf_hip_side_censored_latent(bpmf_hip_side *side, double *z_host);

/* ---- per-rating precision weights ---------------------------------------------------
 * Every rating p of a side may carry a weight w_p > 0: r_p ~ N(mean_rating + x_c . y_r, 1 / (alpha w_p)) -- assays of different
 * quality, a mean of w_p replicates, a confidence per cell.  The conditional of column c becomes
 *     Lambda* = Lambda + alpha sum_p w_p y_r y_r^T,   b = Lambda mu + alpha sum_p w_p (r_p - mean_rating) y_r,
 * and since w y y^T = (sqrt(w) y)(sqrt(w) y)^T the samplers need one change: the weighted form of a kernel reads
 * zw_p = sqrt(w_p) (r_p - mean_rating) as its values with mean 0 and multiplies every gathered factor row by sw_p = sqrt(w_p)
 * before it enters the right-hand side and the Gram.  DESIGN.md section 20 has the forms and what they cost.
 *
 * bpmf_hip_side_set_weights takes nnz weights in the order of the side's ratings, waits for the side's work in flight and stores sw
 * and zw on the device: bitwise the IEEE doubles sqrt(w) and sqrt(w) * (r - mean_rating) (formed on the host).  Every sampler launch
 * of the side (bpmf_hip_sys_sample, bpmf_hip_sample_side[_launch]) then runs the weighted form -- its kernel's name with a `w`
 * (bpmf_hip_side_kernel_name: k_sample1w<K>, k_sample4w<K>, k_sample_slabw<64>, k_sample1sw<64>, k_sample_wg2w<128,4,double>);
 * at K <= 32 never the gather stream, at K = 64 every column in the slab form (no product form).  Nothing is enqueued per
 * iteration and nothing waits on the host.  Weights that are all 1 give the unweighted side's factors and statistics bit for bit.
 * A second call replaces the weights (the hook for weights that are redrawn per iteration); the side's ratings are never written.
 * Evaluation, the sample rings, top-N, new rows and fold-in work on top unchanged (the test matrix and a folded-in row's own
 * ratings have weight 1).
 * BPMF_HIP_EINVAL: a NULL argument, a weight that is not finite and > 0 (the first one is named by its position), an fp32 context,
 * a probit side, a censored side, a side with features, propagated priors, the BPMF_REDUCE formulation, a context with a
 * communicator or a sharded side.  In turn bpmf_hip_side_set_probit, bpmf_hip_side_set_censored,
 * bpmf_hip_side_set_features[_sparse], bpmf_hip_side_set_prop_posterior, bpmf_hip_sys_set_reduce and bpmf_hip_train_sse refuse a
 * side with weights. */
BPMF_API int bpmf_hip_side_set_weights(bpmf_hip_side *side, const double *w_host);
/* sw and zw as the device holds them, nnz doubles each in the order of the side's ratings; either pointer may be NULL. */
BPMF_API int bpmf_hip_side_weights_get(bpmf_hip_side *side, double *sw_host, double *zw_host);
/* The number of ratings whose weight is not 1, the smallest and the largest weight of a side with weights. */
BPMF_API int bpmf_hip_side_weights_count(bpmf_hip_side *side, int64_t *nweighted, double *wmin, double *wmax);

/* ---- implicit feedback ----------------------------------------------------------------------------------
 * Every cell (i, j) of the matrix is observed with precision alpha w_ij: an unobserved cell as r = 0 with w = w0, a stored cell with
 * its value and a confidence w_ij > w0; the mean rating is 0 (Hu, Koren & Volinsky's confidence model as a Gibbs conditional).  The
 * conditional of column j is the weighted column update with sw = sqrt(w - w0), zw = w r / sqrt(w - w0) under the prior precision
 * Lambda + alpha w0 G, G = sum over ALL columns u of the other side of u u^T, with the right-hand side Lambda mu unchanged.
 *
 * bpmf_hip_side_set_implicit takes w0 and nnz confidences in the order of the side's ratings (NULL: every confidence is 1), forms sw
 * and zw on the host in IEEE arithmetic and installs them as the side's weights (bpmf_hip_side_weights_get returns them), so every
 * launch of the side runs the weighted form of its sampler -- at K = 64 the slab form only.
 * BPMF_HIP_EINVAL: w0 not finite and > 0; a confidence not finite and > w0 (the first one is named); a side whose mean_rating is not
 * exactly 0; an fp32 context; a communicator or a sharded side; a side with Student-t noise, weights, a probit, ordinal or censored
 * likelihood, features, propagated priors, the BPMF_REDUCE formulation or a hyper ring (fold-in).  In turn bpmf_hip_side_set_weights,
 * _set_robust, _set_probit, _set_ordinal, _set_censored, _set_features[_sparse], _set_prop_posterior, bpmf_hip_sys_set_reduce,
 * bpmf_hip_side_hyper_reserve and bpmf_hip_tensor_sample refuse an implicit side (it is a side with weights).
 *
 * bpmf_hip_implicit_sample is the blocking half-iteration of an implicit side, modelled on bpmf_hip_link_sample: iter++, the
 * hyper-parameters at counter iter from the side's own cov, G of `other`'s current factors on the device (every column, those without
 * ratings too; k_link_gemm_tn: fp64, fixed order, no floating-point atomics -- the same bits at every call), alpha w0 G added to the
 * LambdaF of the parameter blob after Lmu = Lambda mu was formed (padded num_latent: into the leading block), the stateless weighted
 * launch, cov from the sums.  Both sides of a model are implicit, with one w0, or neither: anything else is BPMF_HIP_EINVAL, and so
 * are bpmf_hip_sys_sample, bpmf_hip_link_sample and bpmf_hip_sample_side on an implicit side.  bpmf_hip_sys_state, the sample rings,
 * the -o aggregates, bpmf_hip_topn[_scored], bpmf_hip_rank_eval and the evaluation work on top as they do for a side with features. */
BPMF_API int bpmf_hip_side_set_implicit(bpmf_hip_side *side, double w0, const double *w_host);
/* w0 of an implicit side; 0 for any other side. */
BPMF_API double bpmf_hip_side_implicit_w0(const bpmf_hip_side *side);
/* G of the side's newest bpmf_hip_implicit_sample, Kt x Kt doubles (waits). */
BPMF_API int bpmf_hip_side_implicit_gram(bpmf_hip_side *side, double *G_host);
BPMF_API int bpmf_hip_implicit_sample(bpmf_hip_side *self, bpmf_hip_side *other, double alpha);

/* ---- Student-t noise: the weights redrawn on the device ------------------------------
 * r_p ~ Student-t with nu degrees of freedom, location mean_rating + x_c . y_r, scale 1 / sqrt(alpha), as a scale mixture:
 *     r_p | w_p ~ N(mean_rating + x_c . y_r, 1 / (alpha w_p)),   w_p ~ Gamma(nu / 2, rate nu / 2),
 *     w_p | rest ~ Gamma((nu + 1) / 2, rate (nu + alpha e^2) / 2),   e = (r_p - mean_rating) - x_c . y_r.
 * A gross outlier draws a small weight and stops dragging its factor columns.  nu >= 1 is fixed by the caller (1: Cauchy noise;
 * large: the Gaussian model), alpha by the sampling calls.  DESIGN.md section 21 has the draw and what it costs.
 *
 * bpmf_hip_side_set_robust makes `side` a side with per-rating weights (above) that start at 1 and are redrawn on the device ahead of
 * every sampler launch of the side (bpmf_hip_sys_sample, bpmf_hip_sample_side[_launch]) by k_robust_weights, from the factors that
 * launch reads, on the Philox blocks (rating lo, rating hi, iteration, 2 attempt [+ 1]; 42, tag): in the launch's queue, without a
 * host wait.  The launch itself is the weighted form of the side's sampler, as after bpmf_hip_side_set_weights;
 * bpmf_hip_side_weights_get then waits for the work in flight and returns the arrays the newest launch read.  Give the two sides of
 * a model different tags that no other add-on of the run uses.
 * A draw that is rejected 64 times (probability < 2^-270) or meets a residual that is not finite (NaN factors) stores w = 1 and
 * is reported by the next call that collects the side's results as BPMF_HIP_ENUM naming the rating.
 * BPMF_HIP_EINVAL: NULL, nu not finite or < 1, tag 0, an fp32 context, a side that has weights or is robust already, a probit side,
 * a censored side, a side with features, propagated priors, the BPMF_REDUCE formulation, a context with a communicator or a
 * sharded side; a launch with an alpha that is not finite and > 0.  In turn bpmf_hip_side_set_weights, bpmf_hip_side_set_probit,
 * bpmf_hip_side_set_censored, bpmf_hip_side_set_features[_sparse], bpmf_hip_side_set_prop_posterior, bpmf_hip_sys_set_reduce and
 * bpmf_hip_train_sse refuse a robust side. */
BPMF_API int bpmf_hip_side_set_robust(bpmf_hip_side *side, double nu, unsigned tag);
/* Adds the weights the side's newest launch read to their running sums (k_robust_accumulate behind that launch: enqueue only). */
BPMF_API int bpmf_hip_side_robust_add(bpmf_hip_side *side);
/* The posterior-mean weight of every rating (nnz doubles in the order of the side's ratings: the sums over the count of
 * bpmf_hip_side_robust_add calls; waits for the work in flight), that count and nu.  Any pointer may be NULL; wmean_host given and
 * nothing added: BPMF_HIP_EINVAL. */
BPMF_API int bpmf_hip_side_robust_get(bpmf_hip_side *side, double *wmean_host, int *count, double *nu);

/* ---- row and column bias terms --------------------------------------------------------
 * r_ij ~ N(mean_rating + b_i + c_j + u_i . v_j, 1 / alpha): one offset per column of either side, b_a ~ N(0, 1 / lambda), one
 * lambda per side, fixed or sampled (bpmf_hip_side_bias_prior).  DESIGN.md section 28 has the model, the summation order, the sampled
 * precision and the bias rows of the sample rings.
 *
 * bpmf_hip_side_set_bias gives a side its biases (all 0 at first).  Both sides of a pair carry them or neither does: a launch or an
 * evaluation of one kind against the other is BPMF_HIP_EINVAL.  From then on every sampler launch of the side (bpmf_hip_sys_sample,
 * bpmf_hip_sample_side[_launch]; iteration `iter`) is preceded on the same stream by the bias step over the factors x the side holds
 * now, the other side's factors y and biases c:
 *     S_a = sum_p ((r_p - mean_rating) - c[row p]) - x_a . y_row(p);   prec = lambda + alpha n_a;
 *     b_a = (alpha S_a) / prec + xi_a / sqrt(prec),   xi_a ~ N(0, 1) from the Philox block (a lo, a hi, iter, 0; 42, tag)
 * (a column without ratings draws from the prior), and the side's samplers read z_p = (r_p - b_a) - c[row p] in place of r_p, with
 * the side's own mean_rating.  The sums have a fixed order (kernels_bias.h): the biases do not depend on the grid, and two launches
 * of one iteration give the same bits.  A residual that is not finite (non-finite factors) makes the call that collects the
 * half-iteration fail with BPMF_HIP_ENUM, naming the rating.  bpmf_hip_predict[_launch] of such a pair adds both biases to every
 * prediction and always runs on the main stream, in order.  `role` (0 or 1; the two sides of a pair take different ones) lays out
 * the bias rows of the side's sample ring: a ring reserved AFTER this call keeps roundup4(num_latent + 2) rows per sample, and
 * bpmf_hip_side_samples_add writes (b, 1) (role 0) or (1, b) (role 1) behind the factor rows, so that the ring dot product of two
 * sides of opposite roles is u . v + b + c and bpmf_hip_topn, _topn_scored, _rank_eval, _predict_block and _predict_cells serve the
 * bias model unchanged.  Those five refuse two rings with different rows per sample, biases on one side only, and equal roles;
 * bpmf_hip_side_samples_reserve refuses a side with biases at num_latent > 126 (the ring kernels serve 128 rows).
 * BPMF_HIP_EINVAL: NULL, lambda not finite and > 0, tag 0, a role outside {0, 1}, an fp32 context, a side that has
 * biases already, a probit, ordinal, censored, weighted, implicit or robust side, a mode of a tensor, features, propagated priors, the
 * BPMF_REDUCE formulation, a sample ring reserved already or a hyper ring (fold-in), a context with a communicator or a sharded side.
 * In turn those setters, bpmf_hip_side_hyper_reserve, bpmf_hip_sys_set_reduce, bpmf_hip_train_sse, bpmf_hip_similar[_block],
 * bpmf_hip_side_samples_get / _set, and fold-in / new rows against such a candidate side refuse a side with biases. */
BPMF_API int bpmf_hip_side_set_bias(bpmf_hip_side *side, double lambda, unsigned tag, int role);
/* The current biases, ncols doubles (waits for the work in flight) / replaces them (every value finite). */
BPMF_API int bpmf_hip_side_bias_get(bpmf_hip_side *side, double *b_host);
BPMF_API int bpmf_hip_side_bias_set(bpmf_hip_side *side, const double *b_host);
/* The array z as the side's newest sampler launch read it, nnz doubles in the order of the side's ratings (waits). */
BPMF_API int bpmf_hip_side_bias_latent(bpmf_hip_side *side, double *z_host);
/* Adds the current biases to their running sums (k_bias_accumulate behind the newest step: enqueue only). */
BPMF_API int bpmf_hip_side_bias_add(bpmf_hip_side *side);
/* The posterior mean of the biases (ncols doubles: the sums over the count of bpmf_hip_side_bias_add calls; waits) and that count.
 * Either pointer may be NULL; mean_host given and nothing added: BPMF_HIP_EINVAL. */
BPMF_API int bpmf_hip_side_bias_mean(bpmf_hip_side *side, double *mean_host, int *count);
/* Samples the side's lambda instead of fixing it: prior Gamma(A0, rate B0), conditional Gamma(A0 + N / 2, B0 + sum_a b_a^2 / 2) with N
 * the side's columns, drawn on the device (k_bias_lambda: the sum of squares in chunks of 256 columns added in chunk order, the
 * Marsaglia-Tsang draw of the Student-t weights on the Philox blocks (~0, ~0, iter, attempt; 42, tag)) at the start of every
 * half-iteration of the side but its first, into the device word the bias draw reads: no host round trip.  A draw that runs into its
 * attempt cap, or biases that are not finite, make the call that collects the half-iteration fail with BPMF_HIP_ENUM.
 * BPMF_HIP_EINVAL: no bias terms, A0 not finite and > 0, B0 not finite and >= 0, A0 + N / 2 < 1. */
BPMF_API int bpmf_hip_side_bias_prior(bpmf_hip_side *side, double a0, double b0);
/* The side's current lambda (waits for the work in flight); trace_host[i], i < ntrace: the lambda the bias step of iteration i ran
 * with (the newest draw at or before i, the value of bpmf_hip_side_set_bias before the first; draws of the first 65 536 iterations are
 * kept); the bias steps and the lambda draws enqueued so far.  trace_host (with ntrace = 0), steps and draws may be NULL. */
BPMF_API int bpmf_hip_side_bias_lambda_get(bpmf_hip_side *side, double *lambda, double *trace_host, int ntrace, int64_t *steps, int64_t *draws);

/* ---- sparse tensor factorisation: Bayesian CP of order 3 -------------------------------
 * A tensor of ratings r(i, j, t) -- compound x target x assay type, user x movie x time -- is modelled as
 *     r(i, j, t) ~ N(mean_rating + sum_k a_ik b_jk c_tk, 1 / alpha),   a Normal-Wishart prior per mode.
 * The conditional of one factor row of a mode is the column update of the matrix model with the other side's row replaced by the
 * Hadamard product of the other two modes' rows, p_e = b_j o c_t: Lambda* = Lambda + alpha sum_e p_e p_e^T,
 * b = Lambda mu + alpha sum_e (r_e - mean_rating) p_e.  So every mode is an ordinary side whose ratings are the tensor's entries in
 * the order of the mode's index, entry e rating row e of a matrix P (ld x nnz fp64, ld = bpmf_hip_ctx_ld) that k_khatri_rao rebuilds
 * ahead of every one of the mode's sampler launches; the samplers are the matrix model's.  DESIGN.md section 22 has the layout and
 * what it costs.
 *
 * bpmf_hip_tensor_create takes nnz entries as three 0-based index arrays and their values, in any order.  Per mode m it sorts the
 * entries stably by their mode-m index (ties keep the caller's order: that fixes the samplers' summation order) and creates a side
 * with dims[m] columns and nnz rows, schedule, chunks and gather stream as for any side.  Device memory: ld * nnz * 8 bytes for P
 * (one buffer, shared by the three modes), per mode 2 * 4 * nnz bytes of indices, 8 * nnz of values and 4 * nnz of row ids, the
 * mode's two factor copies and, at ld <= 32, its gather stream (16 bytes per entry).
 * BPMF_HIP_EINVAL, before anything is enqueued: nmodes != 3, a size outside 1 .. 2^31-1, nnz outside 0 .. 2^31-1 (the samplers' row
 * ids are 32-bit), an index out of range or a value that is not finite (the first such entry is named, 1-based), a cell listed twice
 * (named in 1-based indices, with the two entries), an fp32 context, a context with a communicator.
 * A mode's side (bpmf_hip_tensor_side) serves bpmf_hip_side_get_items / _set_items, the sample ring, _aggr_add / _aggr_finalize,
 * _kernel_name and _schedule_info; it belongs to the tensor and is not destroyed by the caller.  A mode that was given a probit
 * likelihood, censored ratings, weights, Student-t noise, features, propagated priors or the BPMF_REDUCE formulation is refused by
 * bpmf_hip_tensor_sample.  Destroy a tensor's test sets before the tensor. */
typedef struct bpmf_hip_tensor bpmf_hip_tensor;
typedef struct bpmf_hip_tensor_test bpmf_hip_tensor_test;
BPMF_API int bpmf_hip_tensor_create(bpmf_hip_ctx *ctx, int nmodes, const int64_t *dims, int64_t nnz, const int32_t *idx0, const int32_t *idx1,
                                    const int32_t *idx2, const double *vals, double mean_rating, bpmf_hip_tensor **out);
BPMF_API int bpmf_hip_tensor_destroy(bpmf_hip_tensor *tensor);
BPMF_API bpmf_hip_side *bpmf_hip_tensor_side(bpmf_hip_tensor *tensor, int mode);
/* One blocking half-iteration of mode `mode` (0 .. 2): k_khatri_rao writes the mode's rows of P from the current factors of the two
 * other modes, then the mode's sampler runs behind it in the same queue, as bpmf_hip_sample_side (same arguments, same sums, same
 * error codes: BPMF_HIP_ECHOL with bpmf_hip_failed_column of the mode's side).  `iter` is the iteration number, the same value for
 * every mode of an iteration, as the matrix loop passes it for both sides. */
BPMF_API int bpmf_hip_tensor_sample(bpmf_hip_tensor *tensor, int mode, int iter, double alpha, const double *mu, const double *LambdaF,
                                    double *sum_out, double *prod_out, double *norm_out);
/* The rows of P the next sampler launch of `mode` would read: runs k_khatri_rao and copies ld x nnz doubles (column e: the entry at
 * position e of the mode's order; rows num_latent .. ld - 1 zero) to the host; out_host = NULL: runs the kernel and waits, no copy.
 * For tests, debugging and measurements. */
BPMF_API int bpmf_hip_tensor_product(bpmf_hip_tensor *tensor, int mode, double *out_host);
/* Device time of the newest k_khatri_rao launch of a mode (bpmf_hip_tensor_sample, _product), from events on its dispatch packet;
 * waits for it.  0 before the first launch.  The sampler behind it: bpmf_hip_side_last_kernel_ms of the mode's side. */
BPMF_API int bpmf_hip_tensor_last_ms(bpmf_hip_tensor *tensor, float *khatri_rao_ms);
/* Test entries of a tensor: entry q is predicted as mean_rating + c_t . (a_i o b_j).  bpmf_hip_tensor_predict writes the entries'
 * Khatri-Rao rows over the first two modes with k_khatri_rao and evaluates them against the last mode with the evaluation kernel of
 * bpmf_hip_predict: Pavg / Pm2 / n and the returned sums are that call's.  bpmf_hip_tensor_test_get returns Pavg and Pm2 in the
 * order the entries were passed (either pointer may be NULL). */
BPMF_API int bpmf_hip_tensor_test_create(bpmf_hip_tensor *tensor, int64_t nnz, const int32_t *idx0, const int32_t *idx1, const int32_t *idx2,
                                         const double *vals, bpmf_hip_tensor_test **out);
BPMF_API int bpmf_hip_tensor_test_destroy(bpmf_hip_tensor_test *test);
BPMF_API int bpmf_hip_tensor_predict(bpmf_hip_tensor_test *test, int n, double *se, double *se_avg, int64_t *count);
BPMF_API int bpmf_hip_tensor_test_get(bpmf_hip_tensor_test *test, double *pavg, double *pm2);

/* ---- side information: row / column features linked to the factor priors -----------
 * A side with N columns may carry a dense feature matrix F (N x D, fp64), a link matrix beta (D x K) and a fixed
 * lambda_beta > 0:
 *     u_i | mu, Lambda, beta ~ N(mu + beta^T f_i, Lambda^-1),   rows of beta: beta_d ~ N(0, (lambda_beta Lambda)^-1).
 * With u~_i = u_i - m_i, m_i = beta^T f_i, the unchanged column samplers draw u~ from the residual ratings r - m_c . y_r.
 *
 * bpmf_hip_side_set_features uploads F (row_major != 0: F[i * D + d]; 0: column-major, F[d * N + i], the layout of a .ddm file),
 * forms G = F^T F + lambda_beta I on the device, factors and inverts it on the host (once), and allocates beta (0), the offsets
 * M = F beta (0) and the residual array.  tag >= 1 is key word 1 of the Philox stream the normals of the link draw come from:
 * different per side, and different from the probit tags in use.
 * BPMF_HIP_EINVAL: D < 1 or > 1024, lambda_beta <= 0 or not finite, tag 0, a non-finite feature, an fp32 context, a sharded
 * side, a context with a communicator, the BPMF_REDUCE formulation on, a probit side, propagated priors, or features set
 * already.  BPMF_HIP_ENUM: G is not positive definite. */
BPMF_API int bpmf_hip_side_set_features(bpmf_hip_side *side, const double *F_host, int D, int row_major, double lambda_beta, unsigned tag);
/* The stateful, BLOCKING half-iteration of `self` against `other` (iter++):
 *   1. hyper-parameters as bpmf_hyper_sample_ex at counter iter with the scatter lambda_beta beta^T beta and D extra degrees of freedom
 *   2. beta = G^-1 F^T (U - 1 mu^T) + L_G^-T Z R^-T, Z: D x K normals of bpmf_randn_stream_tag(iter, tag), Lambda = R^T R
 *   3. M = F beta      4. r~ = r - m_c . y_r      5. the column samplers on r~ write U~; cov from their sums      6. U = U~ + M
 * A side without features takes steps 1 (plain) and 5 only.  A model with side information steps BOTH sides through this call;
 * bpmf_hip_sys_sample and bpmf_hip_sample_side refuse a side with features.  bpmf_hip_sys_state reports iter, norm (of U), cov
 * (of U~), mu, Lambda of a side stepped this way. */
BPMF_API int bpmf_hip_link_sample(bpmf_hip_side *self, bpmf_hip_side *other, double alpha);
/* beta (D x K, row-major) and the offsets M (N x K, one row per column of the side); either may be NULL.  Waits. */
BPMF_API int bpmf_hip_side_link_get(bpmf_hip_side *side, double *beta_host, double *offsets_host);
/* Sets beta (D x K, row-major) and recomputes M = F beta on the device (a chain continued from stored state; the tests). */
BPMF_API int bpmf_hip_side_link_set(bpmf_hip_side *side, const double *beta_host);
/* The running mean of beta: _add adds the current beta (where bpmf_hip_side_aggr_add sits), _mean returns sum / nsamples. */
BPMF_API int bpmf_hip_side_link_add(bpmf_hip_side *side);
BPMF_API int bpmf_hip_side_link_mean(bpmf_hip_side *side, double *beta_host, int *nsamples);
/* Steps 4 and 6 alone, for tests and tools: the residuals of the side's ratings for its current offsets and the current factors
 * of `other` (nnz doubles, order of the ratings), and U += M on the side's current factors (norm: sum |u|^2 afterwards). */
BPMF_API int bpmf_hip_side_link_residual(bpmf_hip_side *side, const bpmf_hip_side *other, double *r_host);
BPMF_API int bpmf_hip_side_link_shift(bpmf_hip_side *side, double *norm);
/* The two dense products of the link on host arrays (row-major fp64), for tests and tools; no handle needed.
 *   tn: C (D x n) = A^T (B - 1 bvec^T), A: N x D, B: N x n, bvec: n doubles or NULL; n <= 128, or B = A (n = D: pass B = NULL)
 *   nn: C (N x n) = A B, A: N x D, B: D x n, n <= 128
 * Both are bit-identical from call to call; tn adds the partials of fixed chunks of N in chunk order, whatever the grid. */
BPMF_API int bpmf_hip_link_gemm_tn(int device, const double *A, int64_t N, int D, const double *B, int n, const double *bvec, double *C);
BPMF_API int bpmf_hip_link_gemm_nn(int device, const double *A, int64_t N, int D, const double *B, int n, double *C);

/* ---- side information with a SPARSE feature matrix ------------
 * F (N x D) is given in canonical CSR: rowptr (N + 1, rowptr[0] = 0), colidx (strictly increasing within a row, inside [0, D)),
 * vals (fp64, or NULL: every stored entry is 1, a fingerprint).  Any D >= 1: G = F^T F + lambda_beta I is never formed.  The side
 * keeps F compressed by rows and by columns on the device, and step 2 of bpmf_hip_link_sample becomes
 *   2'. X = U - 1 mu^T + Z1 R^-T,  RHS = F^T X + sqrt(lambda_beta) Z2 R^-T,  (F^T F + lambda_beta I) beta = RHS by conjugate
 *       gradients, the K columns in lockstep from beta = 0 (the same conditional of beta as the dense path draws)
 * with M = F beta by the sparse product.  Row i of Z1 (Z2) is the first K normals of the polar method on the blocks
 * Philox4x32-10(counter = {i low, i high, iter, attempt}, key = {42, tag + 0x10000 (tag + 0x20000)}), generated on the device.
 * Column k of the solve is active in an iteration iff |r_k|^2 > tol^2 |rhs_k|^2 at its start; only active columns are updated;
 * the solve ends at the first iteration without an active column or at max_iter (defaults: tol 1e-6, max_iter 1000).  Reaching
 * max_iter is not an error: bpmf_hip_side_link_cg_stats reports it.
 * Everything else -- bpmf_hip_side_link_get / _set / _add / _mean / _residual / _shift, bpmf_hip_sys_state, prediction,
 * aggregation, top-N -- works as for a side with dense features.
 * BPMF_HIP_EINVAL: the refusals of bpmf_hip_side_set_features except the bound on D, and: rowptr not starting at 0 or decreasing,
 * a column index outside [0, D), unsorted or duplicate column indices within a row, a non-finite value, tag >= 0x10000. */
BPMF_API int bpmf_hip_side_set_features_sparse(bpmf_hip_side *side, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals,
                                               double lambda_beta, unsigned tag);
/* tol in (0, 1), max_iter >= 1, for the following draws.  BPMF_HIP_EINVAL on a side without sparse features. */
BPMF_API int bpmf_hip_side_link_cg_set(bpmf_hip_side *side, double tol, int max_iter);
/* Of the last draw: the iterations of the column that needed most, the largest |r_k| / |rhs_k| (recursion residual), whether a
 * column was still active at max_iter; iters_total adds iters_last over all draws.  Any pointer may be NULL. */
BPMF_API int bpmf_hip_side_link_cg_stats(bpmf_hip_side *side, int *iters_last, int64_t *iters_total, double *relres_max_last, int *hit_max_iter);
/* The pieces on host arrays (row-major fp64; F in CSR as above), for tests and tools; no handle needed.
 *   spmm_nn: Y (N x n) = F V, V: D x n            spmm_tn: C (D x n) = F^T X (+ lambda P), X: N x n, P: D x n or NULL
 *   cg_solve: (F^T F + lambda I) X = RHS (D x n) as above; iters: n ints (per column) or NULL
 *   noise_rows: out (nrows x K) = rows 0 .. nrows - 1 of the noise matrix of iteration `it` and key word `key_word`, times R^-T
 *               (Rinv: K x K row-major upper triangular) or the normals themselves (Rinv = NULL)
 * n, K <= 128.  All are bit-identical from call to call and whatever the grid (BPMF_LINK_WG_CHUNKS) or the host's look-ahead
 * (BPMF_LINK_CG_CHECK: CG iterations enqueued between two looks at the convergence word). */
BPMF_API int bpmf_hip_link_spmm_nn(int device, int64_t N, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals, const double *V,
                                   int n, double *Y);
BPMF_API int bpmf_hip_link_spmm_tn(int device, int64_t N, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals, const double *X,
                                   int n, double lambda, const double *P, double *C);
BPMF_API int bpmf_hip_link_cg_solve(int device, int64_t N, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals, double lambda,
                                    const double *RHS, int n, double tol, int max_iter, double *X, int *iters, int *hit_max_iter);
BPMF_API int bpmf_hip_link_noise_rows(int device, int64_t nrows, int K, uint32_t it, uint32_t key_word, const double *Rinv, double *out);

/* ---- a sampled link precision lambda_beta --------------------------
 * Opt-in per side, on a side with dense or sparse features.  Prior lambda_beta ~ Gamma(shape a0, rate b0); conditional
 *     lambda_beta | beta, Lambda ~ Gamma(a0 + D K / 2, b0 + t / 2),   t = tr(Lambda beta^T beta) = |beta R^T|_F^2,  Lambda = R^T R,
 * K = num_latent.  bpmf_hip_link_sample draws it at the START of a half-iteration `iter`, before step 1, from the beta of the
 * side's previous half-iteration and the Lambda that beta was drawn under; everything after it (the scatter, G(lambda_beta), the
 * sparse operator) uses the new value.  At the side's first half-iteration there is no draw: the lambda_beta given to
 * bpmf_hip_side_set_features* is used.
 *
 * Host only: *lambda = g / (b0 + trace / 2), g ~ Gamma(a0 + count / 2, 1) drawn with libstdc++'s gamma_distribution on the Philox
 * stream BPMF_LINK_LAMBDA_COUNTER(iter, tag), key word 1 = 0: the middle of the counter range, apart from the hyper-parameter
 * streams (counting up from 0) and the noise streams (counting down from 2^32 - 1) while iter < 2^27.  BPMF_HIP_EINVAL for
 * a0 <= 0, b0 < 0, non-finite values, count <= 0, a negative trace, tag outside 1 .. 15, iter outside [0, 2^27), or b0 = trace = 0. */
#define BPMF_LINK_LAMBDA_COUNTER(iter, tag) (0x80000000u + 16u * (uint32_t)(iter) + ((uint32_t)(tag) & 15u))
BPMF_API int bpmf_hip_link_lambda_sample(double a0, double b0, double trace, int64_t count, int iter, unsigned tag, double *lambda);
/* Switches the sampling of lambda_beta on, with the prior Gamma(a0, b0).  Only before the side's first half-iteration.  A side with
 * dense features enters DEVICE-FACTOR MODE: F^T F is formed once on the device and kept; every half-iteration forms
 * G = F^T F + lambda_beta I, factors it G = L L^T by a blocked Cholesky on the device and draws beta = L^-T (L^-1 P + E) by two
 * blocked triangular solves (P, E as in step 2 of bpmf_hip_link_sample); W = [G^-1 | L_G^-T] is released.  A non-positive or
 * non-finite pivot makes that bpmf_hip_link_sample fail with BPMF_HIP_ENUM.
 * BPMF_HIP_EINVAL: no features on the side, a0 <= 0, b0 < 0, non-finite values, a tag above 15 (given to set_features*), or a side
 * that has been stepped. */
BPMF_API int bpmf_hip_side_link_lambda_prior(bpmf_hip_side *side, double a0, double b0);
/* Sets lambda_beta (> 0, finite) for the following draws of beta: a chain continued from stored state; the tests.  A side with
 * dense features enters device-factor mode on first use.  Without a prior the value then stays fixed (G is factored once). */
BPMF_API int bpmf_hip_side_link_lambda_set(bpmf_hip_side *side, double lambda);
/* The current lambda_beta, the trace t of its newest draw (NaN before the first), whether it is sampled.  Any pointer may be NULL. */
BPMF_API int bpmf_hip_side_link_lambda_get(bpmf_hip_side *side, double *lambda, double *trace_last, int *sampled);
/* The factorisation and the two solves on host arrays (row-major fp64), for tests and tools; no handle needed.  A: D x D symmetric
 * positive definite (the lower triangle is read), 1 <= D <= 1024; P and E: D x n, 1 <= n <= 128, E may be NULL (zero);
 * X (D x n) = L^-T (L^-1 P + E) with A = L L^T; L_out (D x D, lower triangular, zeros above) if not NULL.  Bit-identical from call
 * to call.  BPMF_HIP_ENUM: A is not positive definite (a pivot was not positive and finite). */
BPMF_API int bpmf_hip_link_chol_solve(int device, const double *A, int D, const double *P, const double *E, int n, double *X, double *L_out);

/* ---- prediction / RMSE -------------------------------------------------------
 * Replaces Sys::predict (c++/sample.cpp:48-96).  The test matrix slice covers
 * the same columns [col_from,col_to) as `side`; Pavg = Pm2 = T initially
 * (c++/sample.cpp:123).  n = iter < burnin ? 0 : iter - burnin (:50).  Returns
 * the partial sums of this rank: se = sum (r-pred)^2, se_avg = sum (r-avg)^2,
 * count = number of predictions; rmse = sqrt(se/count) (:93-95). */
BPMF_API int bpmf_hip_test_create(bpmf_hip_side *side, const int64_t *tcolptr, const int32_t *trowidx,
                         const double *tvals, bpmf_hip_test **out);
BPMF_API int bpmf_hip_test_destroy(bpmf_hip_test *test);
BPMF_API int bpmf_hip_predict(bpmf_hip_test *test, const bpmf_hip_side *self, const bpmf_hip_side *other, int n,
                     double *se, double *se_avg, int64_t *count);
/* the same in two halves: _launch requests the evaluation of the factors as they are after the
 * samplers enqueued so far, _finish waits for the two sums.  A caller may enqueue the next
 * iteration in between (one evaluation per test matrix may be outstanding).  While both sides
 * keep two copies of their factors (library-owned storage, raw pointer never requested) those
 * samplers do not wait for the evaluation: they write the other copies, and the kernel is enqueued
 * beside them.  Otherwise it runs in order on the main stream.  Same results either way. */
BPMF_API int bpmf_hip_predict_launch(bpmf_hip_test *test, const bpmf_hip_side *self, const bpmf_hip_side *other, int n);
BPMF_API int bpmf_hip_predict_finish(bpmf_hip_test *test, double *se, double *se_avg, int64_t *count);
/* `users.predict(movies)` of the reference's loop (c++/bpmf.cpp:190; inside its timed region, its results never
 * printed): `twin` is a test matrix created on the OTHER side from the transposed test entries; it is evaluated with
 * the roles of the two factor matrices swapped whenever `test` is (same launch sequence, its own Pavg / Pm2 and sums).
 * Collect its sums with bpmf_hip_predict_finish(twin, ...) after those of `test`.  twin = NULL detaches. */
BPMF_API int bpmf_hip_test_set_twin(bpmf_hip_test *test, bpmf_hip_test *twin);
/* Pavg / Pm2 in the nnz order of the slice passed to _test_create (Pavg.sdm /
 * Pm2.sdm outputs, c++/bpmf.cpp:229-230) */
BPMF_API int bpmf_hip_test_get(bpmf_hip_test *test, double *pavg_host, double *pm2_host);

/* ---- hyper-parameters (host) --------------------------------------------------
 * Replaces rng_set_pos(iter) + HyperParams::sample (c++/sample.cpp:349-350,
 * c++/bpmf.h:98-103) = CondNormalWishart/NormalWishart/WishartChol/
 * WishartUnitChol/MvNormalChol_prec (c++/mvnormal.cpp:56-135) with the fixed
 * prior mu0=0, b0=2, WI=I, df=K.  Runs on the host with libstdc++'s
 * normal/gamma distributions on the Philox stream `counter` (= iter).
 * cov is K x K; Um is sum/N or NULL for the reference's behaviour (its member
 * `sum` is never updated, so it always passes 0).  Outputs: mu[K], LambdaU
 * (upper Cholesky factor, K x K), LambdaF = LambdaU^T LambdaU. */
BPMF_API int bpmf_hyper_sample(int K, int64_t N, const double *cov, const double *Um, uint32_t counter,
                      double *mu, double *LambdaU, double *LambdaF);
/* The same draw in two steps, so that the expensive, cov-independent part can be produced ahead of
 * time: _draws consumes the whole Philox stream `counter` (unit-Wishart factor au[K*K], upper, and
 * the K normals z of MvNormalChol_prec), _finish does the algebra once cov is known.
 * bpmf_hyper_sample(...) == _draws followed by _finish. */
BPMF_API int bpmf_hyper_draws(int K, int64_t N, uint32_t counter, double *au, double *z);
BPMF_API int bpmf_hyper_finish(int K, int64_t N, const double *cov, const double *Um, const double *au, const double *z,
                               double *mu, double *LambdaU, double *LambdaF);
/* The draw with an extra scatter matrix and extra degrees of freedom (side information: lambda_beta beta^T beta and the D rows
 * of the link matrix): posterior scale X = I + N cov + kappa_m (..) + extra_scatter, Wishart degrees of freedom K + N + extra_dof;
 * kappa_c = 2 + N is unchanged.  extra_scatter = NULL and extra_dof = 0: the bits of the functions above. */
BPMF_API int bpmf_hyper_sample_ex(int K, int64_t N, const double *cov, const double *Um, const double *extra_scatter, int64_t extra_dof,
                                  uint32_t counter, double *mu, double *LambdaU, double *LambdaF);
BPMF_API int bpmf_hyper_draws_ex(int K, int64_t N, int64_t extra_dof, uint32_t counter, double *au, double *z);
BPMF_API int bpmf_hyper_finish_ex(int K, int64_t N, const double *cov, const double *Um, const double *extra_scatter, const double *au,
                                  const double *z, double *mu, double *LambdaU, double *LambdaF);
/* cov = (prod - sum sum^T / N) / (N - 1)  (c++/sample.cpp:383-384) */
BPMF_API void bpmf_cov_from_sums(int K, int64_t N, const double *sum, const double *prod, double *cov);
/* the per-column normal stream, for tests: out[i] = i-th randn() after
 * rng_set_pos(counter) (c++/mvnormal.cpp:34-43) */
BPMF_API void bpmf_randn_stream(uint32_t counter, int n, double *out);
/* the same stream with key word 1 = tag (tag 0: bpmf_randn_stream) */
BPMF_API void bpmf_randn_stream_tag(uint32_t counter, uint32_t tag, int n, double *out);
/* the same n draws produced by the device sampler (n <= 128) */
BPMF_API int bpmf_hip_randn_stream(bpmf_hip_ctx *ctx, uint32_t counter, int n, double *out);

/* Reporting (the reference's counters.cpp / measure_perf hooks have no numeric equivalent; these serve bench.py):
 * the kernel(s) a sampler launch of this side consists of, by name, as a profile shows them; and the side's static
 * schedule in numbers (16 words, see capi_side.hip: form, work items, chunks, columns per product-form class ...). */
BPMF_API int bpmf_hip_side_kernel_name(const bpmf_hip_side *side, char *buf, int n);
/* LDS / register budget and residency of the kernel(s) of one sampler launch of the side (what `LDS occupancy on the Cholesky`
 * of the north star is computed from): per kernel 4 words in `out` -- static LDS bytes per workgroup, threads per workgroup,
 * workgroups resident per CU as the runtime's occupancy query reports it, VGPRs -- in launch order; `names`: the kernels as the
 * launch sites spell them, ';'-separated.  Returns the number of kernels (<= max_kernels) or a negative error.  Launches nothing. */
BPMF_API int bpmf_hip_side_kernel_resources(bpmf_hip_side *side, int64_t *out, int max_kernels, char *names, int names_len);
BPMF_API int bpmf_hip_side_schedule_info(const bpmf_hip_side *side, int64_t *out16, int n);
/* the side's column statistics pass in numbers (8 words, see capi_side.hip): form (0 waves, 1 four-wave workgroups, 2 tiles),
 * waves / workgroups / slices, columns per wave or slice, waves or slices with an empty range, passes enqueued so far as
 * riders of a sampler launch and as kernels of their own.  Launches nothing, waits for nothing. */
BPMF_API int bpmf_hip_side_stat_info(const bpmf_hip_side *side, int64_t *out8, int n);
/* the side's work items in launch order (what replaces the `#pragma omp parallel for schedule(guided)` over the columns,
 * c++/sample.cpp:353-356): local column, number of ratings, and the ordinal of the item's heavy column (-1: the item is
 * a whole column).  Copies min(n, work items) entries; returns the number of work items through *nitems. */
BPMF_API int bpmf_hip_side_schedule_items(const bpmf_hip_side *side, int32_t *col, int32_t *len, int32_t *heavy, int64_t n, int64_t *nitems);
/* sums of the sampler / statistics kernel times (ms, HIP events on their streams) over all
 * half-iterations of the stateful path collected so far, and their number */
BPMF_API int bpmf_hip_side_kernel_ms_sum(bpmf_hip_side *side, double *sample_ms, double *reduce_ms, int64_t *launches);
/* kernel timing of the last _sample_side on this side, in milliseconds, from
 * HIP events recorded on the context's stream (for bench.py's roofline line) */
BPMF_API int bpmf_hip_side_last_kernel_ms(bpmf_hip_side *side, float *sample_ms, float *reduce_ms);

#ifdef __cplusplus
}
#endif
#endif /* BPMF_HIP_H */
