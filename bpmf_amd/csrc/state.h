// state.h -- host-side state behind the opaque handles of include/bpmf_hip.h, shared by capi_*.hip
// (the C ABI) and the per-K launch units (k8.hip ... k128.hip, kcommon.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>      // types and prototypes only: the library is dlopen'ed on first use

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <deque>
#include <limits>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/bpmf_hip.h"
#include "args.h"

extern "C" void bpmf_hip_set_error_(const char *msg);

inline int fail(int code, const std::string &msg)
{
    bpmf_hip_set_error_(msg.c_str());
    return code;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? BPMF_HIP_ENOMEM : BPMF_HIP_ENODEV,                 \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                            \
    } while (0)

#include "ext_state.h"      // the owners (devbuf.h) and the owned state of the add-ons (uses fail / HIP_TRY above)

namespace blob = bpmf::blob;      // the layouts of the parameter / result / reduction blobs (blob.h)

inline int env_int(const char *name, int dflt)
{
    const char *s = getenv(name);
    return (s && *s) ? atoi(s) : dflt;
}

// how long a host thread spins on a result word before it falls back to a blocking wait on the
// event behind the kernels (BPMF_HIP_SPIN_MS, default 50; 0 = always block: used by the tests)
inline double spin_limit_s()
{
    static const double v = env_int("BPMF_HIP_SPIN_MS", 50) * 1e-3;
    return v;
}
// spins until the flag word of a result blob shows `seq`; false: the limit ran out first (the caller then blocks)
inline bool spin_for_seq(const unsigned *flag, unsigned seq)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return true;
        if (spin_limit_s() <= 0.0) return false;
        __builtin_ia32_pause();
        if ((spins & 0xFFFu) == 0xFFFu && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > spin_limit_s()) return false;
    }
}

// bound of every in-kernel wait (gate of the hyper-parameters, staged-parameter word, arrival count of
// the statistics waves), in ticks of the 100 MHz wall clock the kernels read: BPMF_HIP_WAIT_TIMEOUT_MS,
// default 20 s.  A wait that runs into it sets the sticky word `tmo` of the result blob (blob.h) and the
// host reports BPMF_HIP_ENODEV "device wait timed out" instead of using the results.
inline unsigned long long wait_ticks()
{
    static const unsigned long long v = (unsigned long long)std::max(1, env_int("BPMF_HIP_WAIT_TIMEOUT_MS", 20000)) * 100000ull;
    return v;
}
static const char *const kTimeoutWhat[5] = {"", "the gate of the hyper-parameters never opened (host worker stalled?)",
                                     "the staged parameters never arrived (gate workgroup not scheduled?)",
                                     "the column statistics never completed (waves not scheduled?)",
                                     "(unused)"};

// RCCL entry points, resolved at run time: single-GPU users never load the library, and inside a
// torch process the already-loaded librccl.so.1 is reused (one communicator runtime per process).
struct Rccl {
    void *handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;     // optional (bpmf_hip_side_set_overlap: the parts of every rank)
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommSplit) CommSplit = nullptr;       // optional (second communicator for the statistics streams)
    decltype(&ncclSend) Send = nullptr;                 // optional (connectivity-aware exchange)
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclReduce) Reduce = nullptr;             // optional (BPMF_REDUCE formulation: the parts of a side's Gram onto the owners)
    decltype(&ncclCommCount) CommCount = nullptr;       // optional (bpmf_hip_ctx_comm_nranks)
    decltype(&ncclCommAbort) CommAbort = nullptr;       // optional (a collective that never completes: comm_abort in capi_context.hip)
};

Rccl *rccl();      // capi_context.hip

// Every path that would enqueue a collective asks first: after a timed-out collective the communicators were aborted
// (capi_context.hip comm_abort) and their handles must not be used again -- the call fails with BPMF_HIP_ENODEV instead.
#define COMM_ALIVE_OR_FAIL(ctx_, who_)                                                                         \
    do {                                                                                                       \
        if ((ctx_)->comm_dead.load(std::memory_order_acquire))                                                 \
            return fail(BPMF_HIP_ENODEV, std::string(who_) + ": the communicator of this context was aborted (a collective timed out)"); \
    } while (0)

#define NCCL_TRY(expr)                                                                                 \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess)                                                                         \
            return fail(BPMF_HIP_ENODEV, std::string(#expr) + ": " +                                   \
                        (rccl() && rccl()->GetErrorString ? rccl()->GetErrorString(r_) : "RCCL error")); \
    } while (0)


// ncclGroupStart / ncclGroupEnd as a scope: an operation that fails inside a group must not leave the group open
// (every later collective of the thread would be queued instead of issued, and hang)
struct NcclGroup {
    Rccl *R;
    bool open = false;
    explicit NcclGroup(Rccl *r) : R(r) {}
    ncclResult_t start() { const ncclResult_t r = R->GroupStart(); open = r == ncclSuccess; return r; }
    ncclResult_t end() { open = false; return R->GroupEnd(); }
    ~NcclGroup() { if (open) (void)R->GroupEnd(); }
};

struct bpmf_hip_ctx {
    int device = 0;
    // K: the num_latent the kernels are instantiated for -- the leading dimension of EVERY device array and blob (factors,
    // LambdaF, sums).  Kt <= K: the caller's num_latent (c++/bpmf.h:22-24 BPMF_NUMLATENT), the size of everything that crosses
    // the C ABI.  Kt < K: the extra dimensions carry zero factor rows and an identity block of the prior precision, draw no
    // normals and stay exactly zero; RNG stream ids use Kt (c++/sample.cpp:266).
    int K = 0, Kt = 0;
    int dtype = BPMF_HIP_F64;            // arithmetic of the column loop and storage of the factors (BPMF_HIP_F32: K = 128)
    Stream stream;                       // S0: samplers, exchange, predict (its own, or the caller's: borrowed).  Declared first: released last
    hipEvent_t last_sampler_done = nullptr;   // stop event of the newest thing on S0 when that is a stateful sampler (+ exchange), else NULL
    // fused stateful path: the side whose newest half-iteration still has its statistics to run (they
    // ride in the next k_sample1 launch; flush_pending_stats launches them alone if none comes)
    struct bpmf_hip_side *pending_stats = nullptr; unsigned pending_seq = 0; int pending_evset = 0;
    // ... or, unfused sides with a stand-alone statistics pass (big sides, the fp32 path): the pass goes onto S0 itself just
    // ahead of the NEXT sampler launch, which is then launched "any order" (no barrier bit): see bpmf_hip_sys_sample
    // ... or, fp32 path: as rider workgroups at the head of the next k_sample_wg2 launch (StatRiders, args.h)
    bool pending_riders = false;
    std::vector<bpmf_hip_side *> sides;  // stateful sides with a statistics stream of their own (for ctx_sync)
    int num_cu = 256;
    unsigned ablate = 0;
    unsigned diag_only = 0;              // BPMF_NO_COVARIANCE variant (bpmf_hip_ctx_set_no_covariance)
    // per-call parameter blob (blob.h): pinned host copy + device copy
    Pinned<double> h_in; CoreBuf<double> d_in;
    // result blob (blob.h) in pinned host memory the kernels write directly (zero-copy)
    Pinned<double> h_out;
    size_t in_words = 0, out_words = 0;  // their sizes: blob::par_words / par_words_pf (K = 64 in fp64), blob::res_words
    std::mutex launch_mutex;             // kernel launches come from the caller's thread and from the sides' workers
    // multi-GPU: RCCL communicator (one rank per process / GPU) and the reduction blob (blob.h) for the all-reduced sums
    ncclComm_t comm = nullptr;
    // second communicator over the same ranks (ncclCommSplit): the all-reduce of a side's column
    // statistics runs on the side's own stream, beside the other side's sampler and exchange, which
    // two collectives on ONE communicator could not do.  NULL: everything on the main stream.
    ncclComm_t comm2 = nullptr;
    // A collective whose peer never shows up would hold this rank for ever: every host-side wait on a stream that may carry
    // one is bounded (BPMF_HIP_COMM_TIMEOUT_MS, default 60 s; bounded_stream_sync / bounded_event_sync in capi_context.hip); when it
    // runs out both communicators are aborted (ncclCommAbort), the context is dead for collectives and every later call that
    // needs them fails with BPMF_HIP_ENODEV -- the reference's MPI_ERRORS_ARE_FATAL / SUCCESS_OR_DIE (c++/mpi_common.h:16,
    // c++/bpmf_gaspi.h:26-64) as an error code instead of a hang.
    std::atomic<bool> comm_dead{false};
    std::mutex abort_mutex;
    int nranks = 1, rank = 0;
    CoreBuf<double> d_red;
    unsigned seq = 0;                    // value the next publishing kernel writes behind its results
    CoreBuf<unsigned> d_ticket;          // arrival counters of k_colstats' waves (stateless path)
    CoreBuf<unsigned long long> d_stamps;     // BPMF_HIP_STAMPS=1: phase time stamps of two probe work items (printed when the context dies)
    CoreBuf<double> d_zero;              // K zeros: the row padding slots of a ragged rating group gather from
    Event ev[3];
};

struct bpmf_hip_side {
    bpmf_hip_ctx *ctx = nullptr;
    int64_t ncols = 0, nrows = 0, from = 0, to = 0, nnz = 0;
    double mean_rating = 0.0;
    // the ratings and the factors as every launch reads them: views.  Their storage is in the owners below unless the caller
    // lent it (bpmf_hip_side_create_dev, bpmf_hip_side_bind_items, the tensor sides): an empty owner means borrowed
    int32_t *d_rowidx = nullptr; double *d_vals = nullptr;
    CoreBuf<int32_t> own_rowidx; CoreBuf<double> own_vals;
    double *d_items = nullptr;
    // Second copy of the factor matrix: a sampler writes the copy that is NOT current and the two swap
    // roles behind it, so that an evaluation of the previous iteration (k_predict on its own stream)
    // can still read the factors the sampler replaces.  Only while the library owns the storage, the
    // raw pointer was never handed out, and this rank's launches rewrite or receive every column.
    // The swap exchanges the views d_items / d_items_alt; the two owners (fp32 contexts: floats behind them, sized in doubles)
    // stay where they are.
    double *d_items_alt = nullptr; bool items_exposed = false; int cur_buf = 0;
    CoreBuf<double> items_buf[2];
    struct Reader { struct bpmf_hip_test *t = nullptr; unsigned seq = 0; } readers[2];   // last evaluation that read buffer 0 / 1
    struct bpmf_hip_test *deferred_eval = nullptr;      // evaluation waiting for this side's next gate kernel (flush_deferred)
    CoreBuf<double> d_aggr_mu, d_aggr_lambda;                // -o: aggrMu (K x nloc) / aggrLambda (K*K x nloc) of the local columns
    CoreBuf<double> d_prop;              // propagated posterior (-m / -l): K x K prior precision per local column, or NULL
    // the add-ons (ext_state.h), each NULL until its entry point attaches it; released with the side
    std::unique_ptr<bpmf_probit> probit;   // probit likelihood (bpmf_hip_side_set_probit)
    std::unique_ptr<bpmf_censor> censor;   // censored ratings (bpmf_hip_side_set_censored)
    std::unique_ptr<bpmf_ordinal> ordinal; // ordinal probit likelihood (bpmf_hip_side_set_ordinal)
    std::unique_ptr<bpmf_weights> weights; // per-rating precision weights (bpmf_hip_side_set_weights)
    std::unique_ptr<bpmf_implicit> implicit; // implicit feedback: unobserved cells are zeros of weight w0 (bpmf_hip_side_set_implicit)
    std::unique_ptr<bpmf_robust> robust;   // Student-t noise: the weights are redrawn per launch (bpmf_hip_side_set_robust)
    std::unique_ptr<bpmf_bias> bias;       // row / column bias terms: one offset per column, redrawn per launch (bpmf_hip_side_set_bias)
    std::unique_ptr<bpmf_link> link;       // side information, dense or sparse (bpmf_hip_side_set_features, _set_features_sparse)
    std::unique_ptr<bpmf_ring> ring;       // sample ring of the top-N ranking (bpmf_hip_side_samples_reserve)
    std::unique_ptr<bpmf_newrows> newrows; // rows unseen in training: their features and projected samples (bpmf_hip_side_newrows_set)
    std::unique_ptr<bpmf_foldin> foldin;   // fold-in: the per-sample hyper-parameters and the folded-in rows (bpmf_hip_side_hyper_reserve, bpmf_hip_foldin)
    std::unique_ptr<bpmf_sse> sse;         // partials of the training residuals (bpmf_hip_train_sse)
    DevBuf<int64_t> d_colptr;              // the column pointers on the device, uploaded when an add-on first needs them (ensure_colptr)
    bool tensor_mode = false;            // the side is a mode of a tensor (capi_tensor.hip): its "rows" are Khatri-Rao rows, not the other side's columns
    bool latent_queued = false;          // bpmf_hip_sys_sample has enqueued the latent kernel of the launch it is building (launch_sampler then does not)
    // schedule
    int nwork = 0, nmulti = 0, nslots = 0, mode = 0;
    int chunk = 0;                         // ratings per work item above which a column is cut (BPMF_HIP_CHUNK or the automatic value, rounded up to 16)
    // K = 64: columns with <= 16 ratings take the product form (k_sample_pf), the rest the slab form --
    // lr_n light items + hv_nwork others (the full list above stays for per-column priors etc.)
    int lr_n = 0, hv_nwork = 0;
    int64_t pf_ratings2 = 0;
    int64_t pf_ratings = 0;                // ratings of the product-form columns (bpmf_hip_side_schedule_info)
    int pf_class[4] = {0, 0, 0, 0};        // the light items by class: <= 3 ratings, 4..6, 7..16 -- class c is [pf_class[c], pf_class[c+1])
    CoreBuf<double> d_pf_q;                // product form: R0^-T u_row for every row of the other side (nrows x K), per half-iteration
    CoreBuf<int32_t> d_lr_col, d_lr_len; CoreBuf<int64_t> d_lr_p0;
    CoreBuf<int32_t> d_hv_col, d_hv_len, d_hv_mc, d_hv_chunk; CoreBuf<int64_t> d_hv_p0;
    CoreBuf<int32_t> d_wi_col, d_wi_len, d_wi_mc, d_wi_chunk;
    CoreBuf<int64_t> d_wi_p0;
    // gather stream (mode 1, K <= 32; build_schedule): one 16-byte record per rating in item order, per item its first
    // group of 16 records and its number of groups.  Empty: not built (BPMF_HIP_GATHER_STREAM=0, another form of the sampler)
    CoreBuf<bpmf::GatherRec> d_gs_rec;
    CoreBuf<int32_t> d_gs_g0, d_gs_ng;
    int64_t gs_groups = 0;                 // groups of 16 records in the stream, the padding groups behind the last item included
    CoreBuf<int32_t> d_mc_slot0, d_mc_nch;
    CoreBuf<unsigned> d_mc_count;
    CoreBuf<double> d_partials;
    int nstat_waves = 0;
    int nstat_wg = 0;                    // > 0: the side's stand-alone statistics pass runs as this many four-wave workgroups (k_colstats_wg: big sides)
    Event ev_stat_go;                    // big side: S0 continues only once S1 has reached the statistics kernel (head start for its workgroups)
    CoreBuf<double> d_stat_partials;
    int64_t stat_rider_passes = 0, stat_alone_passes = 0;   // statistics passes of this side enqueued as riders / as kernels of their own (bpmf_hip_side_stat_info)
    std::vector<int64_t> bounds;         // multi-GPU: column range of every rank (nranks + 1 entries)
    // overlap of exchange and sampling (bpmf_hip_side_set_overlap): every rank's range is cut into nsub parts of
    // equal work; part c of every rank is exchanged on the stream `sx` while part c + 1 is being sampled
    int nsub = 1;
    // bounded staleness (bpmf_hip_side_set_staleness): part p of this side travels only in the half-iterations with
    // (p + iter) % (stale_k + 1) == 0 (and in iteration 0); in between the peers sample from the copy they have
    int stale_k = 0;
    bool stale_explicit = false;         // k came through bpmf_hip_side_set_staleness (the environment then does not override it)
    bool stale_primed = false;           // every part has travelled once since k was set (the first half-iteration always exchanges everything)
    std::vector<int64_t> sub_bounds;     // nranks x (nsub + 1): global column bounds of the parts of every rank
    std::vector<int> sub_item_off;       // nsub + 1: the work items of part c are [off[c], off[c+1]) of the item arrays
    int item_off = 0, item_n = -1;       // item window of the launch being enqueued (-1: the whole list)
    Stream sx;                           // exchange stream
    Event sub_ev[8], sx_done;
    // BPMF_REDUCE formulation (bpmf_hip_sys_set_reduce, kernels_reduce.h): this side's precomputed Gram parts
    // (ncols x part words, every column -- not only the local ones) and the transpose of this rank's block of
    // ratings (for every column of the OTHER side: the local columns of this side that rate it), longest first
    bool reduce_on = false;
    CoreBuf<double> d_prec;
    CoreBuf<int64_t> d_t_colptr; CoreBuf<int32_t> d_t_rowidx; CoreBuf<double> d_t_vals; CoreBuf<int32_t> d_t_order;
    std::vector<int64_t> h_colptr;       // host copy of the local column pointers (schedules are rebuilt when the parts change)
    // connectivity-aware exchange (bpmf_hip_side_set_conn): per peer, the columns of this rank's range the
    // peer reads (send) and the columns of the peer's range this rank reads (recv), as global column ids
    std::vector<int64_t> conn_send_ptr, conn_recv_ptr;
    CoreBuf<int32_t> d_conn_send, d_conn_recv;
    CoreBuf<double> d_conn_sbuf, d_conn_rbuf;
    // asynchronous (stateful) path: own parameter / result blobs, gate word, events -- set once (ensure_state), then read by both threads
    Pinned<double> a_h_in; CoreBuf<double> a_d_in;
    Pinned<double> a_h_out;
    CoreBuf<unsigned> a_dflag;           // device word k_gate_stage sets when the parameters are staged (in-kernel gate of the sampler)
    Pinned<unsigned> a_gate;                             // pinned word the host sets to iter + 1 when a_h_in holds that iteration's parameters
    CoreBuf<unsigned> a_ticket;                          // arrival counters of this side's k_colstats waves
    CoreBuf<double> a_d_red;                             // multi-GPU: this side's device blob for the all-reduced sums
    Event evs[2][4];                     // (start, sampled, stats, staged) of the two half-iterations that may be in flight
    Stream saux;                         // this side's statistics stream (high priority: its few blocks must not queue behind the other side's sampler)
    // What the caller's thread writes with every launch, on cache lines of its own: the side's worker reads the members above
    // and writes the ones below while the caller enqueues, and a line the two threads share travels between their cores on
    // the path from "sums landed" to "gate open".  (ML-1M shape, K = 32, alternating processes against the layout before the
    // owning members: with those simply in declaration order the iteration took 0.35 % longer, seven pairs, every one slower;
    // grouped like this 0.1 % less, four pairs.)
    alignas(64) bpmf::FusedArgs cur_fused{};   // gate + statistics riders of the k_sample1 launch being enqueued (fused stateful path)
    bpmf::StatRiders cur_riders{};       // fp32 path: statistics riders of the k_sample_wg2 launch being enqueued
    const unsigned *cur_gate_flag = nullptr; unsigned cur_gate_want = 0;   // what the launch being enqueued polls (NULL: ordered by the queue)
    unsigned a_seq = 0;
    int chain = 0;                       // bpmf_hip_side_set_chain: the random numbers of half-iteration i are those keyed i + chain * BPMF_HIP_CHAIN_STRIDE
    int iter = -1;                       // state of the reference's Sys (c++/bpmf.h:139,221-226) for bpmf_hip_sys_sample
    bool pending = false;
    hipEvent_t last_stop = nullptr;      // stop event of this side's newest sampler (diagnostic: boundary to the next launch)
    // the event behind which this side's statistics of the job with event set 0 / 1 are complete, once they
    // have been enqueued (inside the next sampler launch, or as a kernel of their own): the collector's blocking wait
    std::atomic<hipEvent_t> stats_ev[2] = {{nullptr}, {nullptr}};
    // host worker of this side: collects its sums when they land, forms cov, draws its next
    // hyper-parameters and releases the gate of its next sampler, all while the GPU samples the other side.
    // From here on: what the worker writes (in the stateless path, the caller at collection).
    struct Job { int iter; unsigned seq; int evset; bool timed; hipEvent_t prev_stop; };
    alignas(64) int64_t failed_column = -1;
    float last_sample_ms = 0.f, last_reduce_ms = 0.f;
    bool timing_valid = true;
    double tot_gap_ms = 0.0; int64_t n_gap = 0;
    std::thread worker;
    std::mutex wm;
    std::condition_variable wcv;
    std::deque<Job> jobs;
    int in_flight = 0;                   // half-iterations enqueued and not collected yet (at most 2)
    bool wstop = false;
    int async_rc = 0;                    // deferred error of a half-iteration (e.g. Cholesky failed)
    std::string async_msg;
    int gate_iter = -2;                  // iteration whose parameters the gate has been opened for
    double tot_sample_ms = 0.0, tot_reduce_ms = 0.0;
    long long n_launches = 0;
    double norm = 0.0;
    // norm of the last few collected half-iterations (bpmf_hip_sys_norm: the line of iteration i - 1 is printed after iteration i
    // has been enqueued; asking bpmf_hip_sys_state for it would drain the side's pipeline first).  Guarded by `wm`.
    int collected_iter = -1;
    double norm_hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<double> cov, hp_mu, hp_LambdaU, hp_LambdaF;      // current
    std::vector<double> nx_mu, nx_LambdaU, nx_LambdaF;           // pre-drawn for iteration nx_iter
    int nx_iter = -2;
    std::vector<double> rd_au, rd_z;                             // cov-independent random part, drawn for iteration rd_iter
    int rd_iter = -2;
    // The random part of a hyper-parameter draw (Wishart gammas / normals, K (K - 1) + 2 K numbers from the Philox
    // stream `iter`) depends on nothing but the iteration number and costs more than a whole sampler launch at
    // K >= 64 (K = 128: ~1 ms on the host): helper threads draw a few iterations AHEAD into a ring, the collector
    // thread only picks the finished draw up.
    struct Predraw {
        static constexpr int DEPTH = 8;
        struct Slot { std::vector<double> au, z; int iter = -1; };
        Slot slot[DEPTH];
        std::vector<std::thread> threads;
        std::mutex m;
        std::condition_variable cv;
        int next = 0;                    // first iteration no helper has claimed
        int consumed = -1;               // last iteration handed out
        bool stop = false;
    } predraw;
};

// The likelihood of a side's ratings: the setters see to it that a side is at most one of the five that are not plain Gaussian
// (bias: Gaussian ratings around mean + b_col + c_row + x . y, a latent step all the same).
enum class Likelihood { gaussian, probit, ordinal, censored, robust, bias };
inline Likelihood likelihood(const bpmf_hip_side *s)
{
    return s->probit ? Likelihood::probit : s->ordinal ? Likelihood::ordinal : s->censor ? Likelihood::censored
           : s->robust ? Likelihood::robust : s->bias ? Likelihood::bias : Likelihood::gaussian;
}
// the latent step of the side (ext_state.h), NULL on a Gaussian side
inline bpmf_latent *latent_step(const bpmf_hip_side *s)
{
    switch (likelihood(s)) {
    case Likelihood::probit: return s->probit.get();
    case Likelihood::ordinal: return s->ordinal.get();
    case Likelihood::censored: return s->censor.get();
    case Likelihood::robust: return s->robust.get();
    case Likelihood::bias: return s->bias.get();
    case Likelihood::gaussian: break;
    }
    return nullptr;
}
// what the samplers of the side read as its values (layout of d_vals): the latent scores of a probit or an ordinal side, the ratings
// with a fresh draw at every censored position (capi_censor.hip), the residuals r - m_c . y_r of a side with features
// (capi_link.hip), the ratings less both bias terms of a side with biases (capi_bias.hip), else the ratings themselves
inline const double *sampler_values(const bpmf_hip_side *s)
{
    switch (likelihood(s)) {
    case Likelihood::probit: return s->probit->z.get();
    case Likelihood::ordinal: return s->ordinal->z.get();
    case Likelihood::censored: return s->censor->z.get();
    case Likelihood::bias: return s->bias->z.get();
    default: return s->link ? s->link->r.get() : s->d_vals;
    }
}
// ... and whether those are the side's own ratings
inline bool reads_own_ratings(const bpmf_hip_side *s)
{
    const Likelihood k = likelihood(s);
    return (k == Likelihood::gaussian || k == Likelihood::robust) && !s->link;
}

// Does a k_sample1 launch of the side read its gather stream?  The stream holds r - mean_rating of the side's OWN ratings:
// a probit, censored or side-information launch reads other values in their place and keeps the index-block form
// (k_sample1i), and so does the hot-row profiling switch (BPMF_HIP_ABLATE & 4), which rewrites the row ids.  A weighted side
// never reads it either: a record has no room for sqrt(w) (k_sample1w, the weighted index-block form).
inline bool uses_gather_stream(const bpmf_hip_side *s)
{
    return s->d_gs_rec && s->mode == 1 && reads_own_ratings(s) && !s->weights && !(s->ctx->ablate & 4u);
}

struct bpmf_hip_test {
    bpmf_hip_side *side = nullptr;
    int64_t nnz = 0;
    CoreBuf<int32_t> d_tcol, d_trow;
    CoreBuf<double> d_tval, d_pavg, d_pm2, d_partial;
    int64_t nblocks = 0;
    int wg = 256;                        // threads per workgroup of k_predict (64: single-wave workgroups, small test sets)
    int64_t global_nnz = -1;             // multi-GPU: test ratings over all ranks (all-reduced once)
    Pinned<double> h_res;                                // pinned: se | se_avg | flag
    CoreBuf<unsigned> d_ticket;                          // arrival counter of k_predict's blocks
    unsigned seq = 0, done_seq = 0;
    bool launched = false;
    Event ev_in, ev_done[2]; hipEvent_t in_ev = nullptr;
    hipStream_t pstream = nullptr;       // where the launch in flight was enqueued (the main stream, or the other side's)
    // requested, not yet enqueued (flush_deferred): the factor copies it reads, captured at the request
    bool deferred = false, cancelled = false; int def_n = 0; struct bpmf_hip_side *def_other = nullptr;
    const void *def_self_items = nullptr, *def_other_items = nullptr;
    // users.predict(movies) of c++/bpmf.cpp:190: the test matrix of the OTHER side (transposed entries), evaluated with
    // the roles swapped whenever this one is (bpmf_hip_test_set_twin); owner: the test matrix this one is the twin of
    struct bpmf_hip_test *twin = nullptr, *owner = nullptr;
    // single GPU, fp64: the twin's entries are this matrix's, transposed -- entry q here is entry twin_perm[q] there, and
    // ONE kernel writes both copies (k_predict's TwinArgs).  Empty: the twin runs as a kernel of its own (sharded, fp32).
    CoreBuf<int32_t> d_twin_perm;
    std::vector<int32_t> h_col, h_row;   // global column / row of every entry (kept for the matching)
    DevBuf<double> d_prob_sum; int prob_n = 0;       // probit: running sums of Phi(x . y) per entry and the samples added (capi_probit.hip)
    DevBuf<double> ord_sum; int ord_n = 0, ord_nlev = 0; // ordinal: running sums of the level probabilities, level-major (nlev x nnz), and the samples added (capi_ordinal.hip)
};

// did a device-side wait of the pass that wrote this result blob time out?  (the word is sticky: cleared here)
inline int check_timeout(double *h_blob, int K, std::string *msg)
{
    unsigned long long *w = blob::tmo_word(h_blob, K);
    const unsigned long long v = __atomic_load_n(w, __ATOMIC_ACQUIRE);
    if (!v) return 0;
    __atomic_store_n(w, 0ull, __ATOMIC_RELEASE);
    *msg = std::string("device wait timed out: ") + kTimeoutWhat[v < 5 ? v : 0];
    return BPMF_HIP_ENODEV;
}

// Did the latent kernel of this side (probit, ordinal, censored, robust, bias) raise its word -- a draw that ran into its attempt cap, a
// dot product or residual that is not finite?  Checked where a half-iteration's results are collected; the word is reset.
inline int check_latent(bpmf_hip_side *s, std::string *msg)
{
    static const char *const kBefore[] = {"", "probit: the truncated-normal draw of rating ", "ordinal: the score of rating ",
                                          "censored: the truncated-normal draw of rating ", "robust: the weight of rating ",
                                          "bias: the residual of rating "};
    static const char *const kAfter[] = {"", " was rejected 64 times (non-finite factors?)", " is not finite (non-finite factors?)",
                                         " was rejected 64 times (non-finite factors?)",
                                         " could not be drawn: 64 rejections, or a residual that is not finite (non-finite factors?)",
                                         " is not finite (non-finite factors?)"};
    bpmf_latent *l = latent_step(s);
    if (!l) return 0;
    unsigned long long *word = l->fail.host();
    const unsigned long long v = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    if (v == ~0ull) return 0;
    __atomic_store_n(word, ~0ull, __ATOMIC_RELEASE);
    const int k = (int)likelihood(s);
    if (k == (int)Likelihood::bias && v == ~0ull - 1ull) {            // (kernels_bias.h: kBiasLambdaFailed)
        *msg = "bias: the draw of lambda was rejected 64 times or met biases that are not finite";
        return BPMF_HIP_ENUM;
    }
    *msg = kBefore[k] + std::to_string(v) + kAfter[k];
    return BPMF_HIP_ENUM;
}

// doubles in the partial of one chunk of a heavy column: the larger of the two accumulator layouts
// (16x16x4 tiles of k_sample, 4x4x4 blocks of k_sample1 for K <= 32)
template <int K>
inline size_t part_words()
{
    size_t w = (size_t)bpmf::Geo<K>::PART;
    if constexpr (K <= 32) w = std::max(w, (size_t)bpmf::Geo44<K>::PART);
    return w;
}

inline size_t part_words_rt(int K, bool f32)
{
    switch (K) {
    case 8: return part_words<8>();
    case 16: return part_words<16>();
    case 32: return part_words<32>();
    case 64: return part_words<64>();
    case 128: return (size_t)(36 * 256 + 8 * 16) / (f32 ? 2 : 1);       // 36 tiles + rhs in the element type of the factors (GeoW2<128>::PART_FLOATS, GeoS<128>::PART)
    }
    return 0;
}


// doubles behind the parameter blob of a half-iteration that hold LambdaF as fp32 tiles (fp32 path only)
inline size_t lf32_words(const bpmf_hip_ctx *c) { return c->dtype == BPMF_HIP_F32 ? (size_t)blob::par_lf32_words(c->K) : 0; }

// may this side's samplers write the second copy of the factors?  Every column of the new copy must
// be produced by this launch or arrive through the exchange that follows it.
inline bool second_copy_usable(const bpmf_hip_side *s)
{
    if (!s->d_items_alt || !s->items_buf[s->cur_buf] || s->items_exposed || s->nwork <= 0) return false;
    // bounded staleness: a part that does not travel must keep the value the peer LAST RECEIVED, and that sits in the
    // current copy only -- with two copies a skipped part would fall back to what the other copy held two
    // half-iterations earlier: the samplers of such a side write in place
    if (s->stale_k > 0) return false;
    const bool dist = s->ctx->comm != nullptr && !s->bounds.empty();
    return dist || (s->from == 0 && s->to == s->ncols);
}
