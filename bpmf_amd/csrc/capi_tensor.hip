// capi_tensor.hip -- sparse tensor factorisation, Bayesian CP of order 3 (kernel in kernels_tensor.h):
//     r(i, j, t) ~ N(mean + sum_k a_ik b_jk c_tk, 1 / alpha),   a Normal-Wishart prior per mode.
// The conditional of one factor row of mode m is the column update of the matrix model with the other side's row replaced by the
// Hadamard product of the other two modes' rows.  So a mode is an ordinary side (capi_side.hip) whose ratings are the tensor's entries
// in the order of the mode's index, entry e rating row e of a matrix P (ld x nnz) that k_khatri_rao rebuilds ahead of every one of the
// mode's sampler launches; the samplers, their schedule, chunks and gather stream are the matrix model's, untouched.  The test entries
// get their Khatri-Rao rows over the first two modes from the same kernel and are evaluated against the last mode by k_predict.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

// What a sampler launch reads of its `other` side is its context, its number of columns and its factor pointer (launch_impl.h:
// sampler_into; capi_sample.hip: bpmf_hip_sample_side_launch), an evaluation also from / mean_rating / bounds of `self`: a
// default-constructed bpmf_hip_side with those members set carries a buffer it does not own -- no schedule, no second copy.
static bpmf_hip_side *carrier(bpmf_hip_ctx *c, int64_t ncols, int64_t nrows, double mean, double *items)
{
    bpmf_hip_side *s = new (std::nothrow) bpmf_hip_side();
    if (!s) return nullptr;
    s->ctx = c; s->ncols = ncols; s->nrows = nrows; s->from = 0; s->to = ncols; s->mean_rating = mean;
    s->d_items = items;                                             // (a view: the side's owners stay empty)
    return s;
}

struct bpmf_hip_tensor {
    bpmf_hip_ctx *ctx = nullptr;
    int64_t dims[3] = {0, 0, 0}, nnz = 0;
    double mean_rating = 0.0;
    bpmf_hip_side *side[3] = {nullptr, nullptr, nullptr};              // mode m as a side: dims[m] columns, nnz rows
    DevBuf<int32_t> ia[3], ib[3];                                      // per mode, in its order: the entries' indices in the two other modes
    DevBuf<double> P;                                                  // ld x nnz, shared by the three modes
    bpmf_hip_side *pcar = nullptr;                                     // P as "the other side"
    int ntests = 0;                                                    // live test sets (they read the sides)
    Event kr_ev[2];                                                    // start / stop of the newest k_khatri_rao of a mode (bpmf_hip_tensor_last_ms)
    bool kr_timed = false;
};

struct bpmf_hip_tensor_test {
    bpmf_hip_tensor *tensor = nullptr;
    int64_t nnz = 0;
    std::vector<int64_t> perm;                                         // position p of the last mode's order holds entry perm[p] of the caller
    DevBuf<int32_t> qa, qb;                                            // in that order: the entries' indices in modes 0 and 1
    DevBuf<double> Q;                                                  // ld x nnz: their Khatri-Rao rows
    bpmf_hip_side *tside = nullptr, *qcar = nullptr;                   // the last mode's factors as `self`, Q as `other` of the evaluation
    bpmf_hip_test *test = nullptr;
};

// the two other modes of mode m, ascending
static inline void others(int m, int *a, int *b) { *a = m == 0 ? 1 : 0; *b = m == 2 ? 1 : 2; }

// indices in range and values finite, or a refusal naming the first offender in 1-based ids
static int check_entries(const char *who, const int64_t *dims, int64_t n, const int32_t *const idx[3], const double *vals)
{
    for (int64_t e = 0; e < n; ++e) {
        for (int m = 0; m < 3; ++m)
            if (idx[m][e] < 0 || idx[m][e] >= dims[m])
                return fail(BPMF_HIP_EINVAL, std::string(who) + ": entry " + std::to_string(e + 1) + " has index " + std::to_string((long long)idx[m][e] + 1) +
                            " in mode " + std::to_string(m + 1) + " of size " + std::to_string(dims[m]));
        if (!std::isfinite(vals[e])) return fail(BPMF_HIP_EINVAL, std::string(who) + ": the value of entry " + std::to_string(e + 1) + " is not finite");
    }
    return 0;
}

// stable counting sort of the entries by key[e] in [0, nkeys): perm (position -> entry) and the column pointers
static void order_by(const int32_t *key, int64_t nkeys, int64_t n, std::vector<int64_t> *perm, std::vector<int64_t> *colptr)
{
    colptr->assign((size_t)nkeys + 1, 0);
    for (int64_t e = 0; e < n; ++e) (*colptr)[(size_t)key[e] + 1]++;
    for (int64_t c = 0; c < nkeys; ++c) (*colptr)[(size_t)c + 1] += (*colptr)[(size_t)c];
    std::vector<int64_t> at(colptr->begin(), colptr->end() - 1);
    perm->resize((size_t)n);
    for (int64_t e = 0; e < n; ++e) (*perm)[(size_t)at[(size_t)key[e]]++] = e;
}

static int enqueue_khatri_rao(bpmf_hip_ctx *c, const double *A, const double *B, const int32_t *ia, const int32_t *ib, int64_t n, double *P,
                              hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr)
{
    bpmf_launch::KhatriRaoLaunch p{};
    p.A = A; p.B = B; p.ia = ia; p.ib = ib; p.n = n; p.ld = c->K; p.kt = c->Kt; p.P = P; p.ev_start = ev_start; p.ev_stop = ev_stop;
    if (bpmf_launch::khatri_rao(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, "tensor: unsupported K " + std::to_string(c->K));
    HIP_TRY(hipGetLastError());
    c->last_sampler_done = nullptr;                                   // (the newest thing on S0 is no longer a sampler)
    return 0;
}

// mode m's rows of P from the current copies of the two other factor matrices, on S0.  No host wait.
static int build_product(bpmf_hip_tensor *t, int m)
{
    int a, b;
    others(m, &a, &b);
    t->kr_timed = t->nnz > 0;
    return enqueue_khatri_rao(t->ctx, t->side[a]->d_items, t->side[b]->d_items, t->ia[m].get(), t->ib[m].get(), t->nnz, t->P.get(), t->kr_ev[0].get(), t->kr_ev[1].get());
}

extern "C" int bpmf_hip_tensor_destroy(bpmf_hip_tensor *t)
{
    if (!t) return BPMF_HIP_OK;
    if (t->ntests > 0) return fail(BPMF_HIP_EINVAL, "tensor_destroy: destroy the tensor's test sets first (bpmf_hip_tensor_test_destroy)");
    if (t->ctx) (void)hipSetDevice(t->ctx->device);
    for (bpmf_hip_side *s : t->side) if (s) (void)bpmf_hip_side_destroy(s);      // (waits for S0: nothing reads P after this)
    delete t->pcar;
    delete t;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_tensor_create(bpmf_hip_ctx *ctx, int nmodes, const int64_t *dims, int64_t nnz, const int32_t *idx0, const int32_t *idx1,
                                      const int32_t *idx2, const double *vals, double mean_rating, bpmf_hip_tensor **out)
{
    if (!out) return fail(BPMF_HIP_EINVAL, "tensor_create: out is NULL");
    *out = nullptr;
    if (nmodes != 3) return fail(BPMF_HIP_EINVAL, "tensor_create: " + std::to_string(nmodes) + " modes given, tensors of order 3 only");
    if (!dims) return fail(BPMF_HIP_EINVAL, "tensor_create: dims is NULL");
    for (int m = 0; m < 3; ++m)
        if (dims[m] <= 0 || dims[m] > (int64_t)INT32_MAX)
            return fail(BPMF_HIP_EINVAL, "tensor_create: mode " + std::to_string(m + 1) + " has size " + std::to_string(dims[m]) + ", 1 .. 2^31-1 allowed");
    // entry e is row e of the samplers' other side: their row ids are 32-bit (the gather stream's 32-bit offsets are the side's own
    // affair: build_gather_stream falls back to the index-block form where ld / 2 x nnz passes 2^31-1)
    if (nnz < 0 || nnz > (int64_t)INT32_MAX)
        return fail(BPMF_HIP_EINVAL, "tensor_create: " + std::to_string(nnz) + " entries, 0 .. 2^31-1 allowed (32-bit row ids of the samplers)");
    if (nnz > 0 && (!idx0 || !idx1 || !idx2 || !vals)) return fail(BPMF_HIP_EINVAL, "tensor_create: NULL indices / values");
    if (!std::isfinite(mean_rating)) return fail(BPMF_HIP_EINVAL, "tensor_create: mean_rating is not finite");
    const int32_t *const idx[3] = {idx0, idx1, idx2};
    int rc = check_entries("tensor_create", dims, nnz, idx, vals);
    if (rc) return rc;
    // per mode: the stable order by the mode's index (ties in input order: that fixes the samplers' summation order)
    std::vector<int64_t> perm[3], colptr[3];
    for (int m = 0; m < 3; ++m) order_by(idx[m], dims[m], nnz, &perm[m], &colptr[m]);
    {   // no cell twice: inside a column of mode 0 (input order), sorted by (j, t, position)
        std::vector<int64_t> col;
        int64_t first = -1, other = -1;
        for (int64_t c = 0; c < dims[0]; ++c) {
            col.assign(perm[0].begin() + colptr[0][(size_t)c], perm[0].begin() + colptr[0][(size_t)c + 1]);
            std::sort(col.begin(), col.end(), [&](int64_t x, int64_t y) {
                if (idx1[x] != idx1[y]) return idx1[x] < idx1[y];
                if (idx2[x] != idx2[y]) return idx2[x] < idx2[y];
                return x < y;
            });
            for (size_t q = 1; q < col.size(); ++q)
                if (idx1[col[q]] == idx1[col[q - 1]] && idx2[col[q]] == idx2[col[q - 1]] && (first < 0 || col[q] < first)) { first = col[q]; other = col[q - 1]; }
        }
        if (first >= 0)
            return fail(BPMF_HIP_EINVAL, "tensor_create: cell (" + std::to_string((long long)idx0[first] + 1) + ", " + std::to_string((long long)idx1[first] + 1) + ", " +
                        std::to_string((long long)idx2[first] + 1) + ") is listed twice (entries " + std::to_string(other + 1) + " and " + std::to_string(first + 1) + ")");
    }
    if (!ctx) return fail(BPMF_HIP_EINVAL, "tensor_create: ctx is NULL");
    if (ctx->dtype != BPMF_HIP_F64) return fail(BPMF_HIP_EINVAL, "tensor_create: not on an fp32 context");
    if (ctx->comm) return fail(BPMF_HIP_EINVAL, "tensor_create: needs the tensor whole on one GPU, on a context without a communicator");
    HIP_TRY(hipSetDevice(ctx->device));
    bpmf_hip_tensor *t = new (std::nothrow) bpmf_hip_tensor();
    if (!t) return fail(BPMF_HIP_ENOMEM, "tensor_create: out of host memory");
    t->ctx = ctx; t->nnz = nnz; t->mean_rating = mean_rating;
    for (int m = 0; m < 3; ++m) t->dims[m] = dims[m];
    const size_t n1 = (size_t)std::max<int64_t>(nnz, 1);
    std::vector<int32_t> rowidx(n1, 0), ha(n1, 0), hb(n1, 0);
    std::vector<double> v(n1, 0.0);
    for (int64_t p = 0; p < nnz; ++p) rowidx[(size_t)p] = (int32_t)p;
    for (int m = 0; m < 3 && !rc; ++m) {
        int a, b;
        others(m, &a, &b);
        for (int64_t p = 0; p < nnz; ++p) {
            const int64_t e = perm[m][(size_t)p];
            ha[(size_t)p] = idx[a][e]; hb[(size_t)p] = idx[b][e]; v[(size_t)p] = vals[e];
        }
        if ((rc = t->ia[m].upload(ha.data(), (size_t)nnz)) || (rc = t->ib[m].upload(hb.data(), (size_t)nnz))) break;
        rc = bpmf_hip_side_create(ctx, dims[m], (int64_t)n1, 0, dims[m], colptr[m].data(), rowidx.data(), v.data(), mean_rating, &t->side[m]);
        if (!rc) t->side[m]->tensor_mode = true;
    }
    for (Event &e : t->kr_ev)
        if (!rc && e.create()) { (void)hipGetLastError(); rc = fail(BPMF_HIP_ENODEV, "tensor_create: hipEventCreate failed"); }
    if (!rc) rc = t->P.alloc((size_t)ctx->K * n1);
    if (!rc) rc = t->P.zero_async(ctx->stream.get());
    if (!rc && !(t->pcar = carrier(ctx, (int64_t)n1, 0, mean_rating, t->P.get()))) rc = fail(BPMF_HIP_ENOMEM, "tensor_create: out of host memory");
    if (rc) {
        const std::string keep = bpmf_hip_last_error();              // (the destructor's calls may not replace the reason)
        (void)bpmf_hip_tensor_destroy(t);
        return fail(rc, keep);
    }
    *out = t;
    return BPMF_HIP_OK;
}

extern "C" bpmf_hip_side *bpmf_hip_tensor_side(bpmf_hip_tensor *t, int m)
{
    if (!t || m < 0 || m > 2) { (void)fail(BPMF_HIP_EINVAL, "tensor_side: NULL tensor or a mode outside 0 .. 2"); return nullptr; }
    return t->side[m];
}

// a mode's side may carry the sample ring, the hyper ring and the -o aggregates; everything that changes what its sampler reads is refused
static int check_plain_mode(const char *who, const bpmf_hip_side *s)
{
    static const char *const kKind[] = {nullptr, "a probit likelihood", "an ordinal likelihood", "censored ratings", "Student-t noise", "bias terms"};
    const char *what = latent_step(s) ? kKind[(int)likelihood(s)] : s->weights ? "per-rating weights"
                       : s->link ? "features" : s->d_prop.get() ? "propagated priors" : s->reduce_on ? "the BPMF_REDUCE formulation" : nullptr;
    if (what) return fail(BPMF_HIP_EINVAL, std::string(who) + ": not together with " + what + " on a mode of a tensor");
    if (s->ctx->comm || sharded(s)) return fail(BPMF_HIP_EINVAL, std::string(who) + ": needs the tensor whole on one GPU, on a context without a communicator");
    return 0;
}

extern "C" int bpmf_hip_tensor_sample(bpmf_hip_tensor *t, int m, int iter, double alpha, const double *mu, const double *LambdaF,
                                      double *sum_out, double *prod_out, double *norm_out)
{
    if (!t || !mu || !LambdaF || !sum_out || !prod_out || !norm_out) return fail(BPMF_HIP_EINVAL, "tensor_sample: NULL argument");
    if (m < 0 || m > 2) return fail(BPMF_HIP_EINVAL, "tensor_sample: mode " + std::to_string(m) + " given, 0 .. 2 allowed");
    if (iter < 0) return fail(BPMF_HIP_EINVAL, "tensor_sample: iter < 0");
    int rc;
    for (int k = 0; k < 3; ++k)
        if ((rc = check_plain_mode("tensor_sample", t->side[k]))) return rc;
    if (t->side[m]->pending) return fail(BPMF_HIP_EINVAL, "tensor_sample: previous launch not finished");
    HIP_TRY(hipSetDevice(t->ctx->device));
    if ((rc = build_product(t, m))) return rc;
    return bpmf_hip_sample_side(t->side[m], t->pcar, iter, alpha, mu, LambdaF, sum_out, prod_out, norm_out);
}

extern "C" int bpmf_hip_tensor_product(bpmf_hip_tensor *t, int m, double *out_host)
{
    if (!t) return fail(BPMF_HIP_EINVAL, "tensor_product: NULL argument");
    if (m < 0 || m > 2) return fail(BPMF_HIP_EINVAL, "tensor_product: mode " + std::to_string(m) + " given, 0 .. 2 allowed");
    bpmf_hip_ctx *c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = build_product(t, m);
    if (rc) return rc;
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    if (t->nnz > 0 && out_host) HIP_TRY(hipMemcpy(out_host, t->P.get(), (size_t)c->K * (size_t)t->nnz * sizeof(double), hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_tensor_last_ms(bpmf_hip_tensor *t, float *khatri_rao_ms)
{
    if (!t || !khatri_rao_ms) return fail(BPMF_HIP_EINVAL, "tensor_last_ms: NULL argument");
    *khatri_rao_ms = 0.f;
    if (!t->kr_timed) return BPMF_HIP_OK;                            // (nothing launched yet, or a tensor without entries)
    HIP_TRY(hipSetDevice(t->ctx->device));
    { const int re_ = bounded_event_sync(t->ctx, t->kr_ev[1].get(), "tensor_last_ms"); if (re_) return re_; }
    HIP_TRY(hipEventElapsedTime(khatri_rao_ms, t->kr_ev[0].get(), t->kr_ev[1].get()));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_tensor_test_destroy(bpmf_hip_tensor_test *tt)
{
    if (!tt) return BPMF_HIP_OK;
    if (tt->tensor && tt->tensor->ctx) (void)hipSetDevice(tt->tensor->ctx->device);
    if (tt->test) (void)bpmf_hip_test_destroy(tt->test);              // (waits for S0; reads tside)
    delete tt->tside;
    delete tt->qcar;
    if (tt->tensor) --tt->tensor->ntests;
    delete tt;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_tensor_test_create(bpmf_hip_tensor *t, int64_t nnz, const int32_t *idx0, const int32_t *idx1, const int32_t *idx2,
                                           const double *vals, bpmf_hip_tensor_test **out)
{
    if (!out) return fail(BPMF_HIP_EINVAL, "tensor_test_create: out is NULL");
    *out = nullptr;
    if (!t) return fail(BPMF_HIP_EINVAL, "tensor_test_create: the tensor is NULL");
    if (nnz < 0 || nnz > (int64_t)INT32_MAX) return fail(BPMF_HIP_EINVAL, "tensor_test_create: " + std::to_string(nnz) + " entries, 0 .. 2^31-1 allowed");
    if (nnz > 0 && (!idx0 || !idx1 || !idx2 || !vals)) return fail(BPMF_HIP_EINVAL, "tensor_test_create: NULL indices / values");
    const int32_t *const idx[3] = {idx0, idx1, idx2};
    int rc = check_entries("tensor_test_create", t->dims, nnz, idx, vals);
    if (rc) return rc;
    bpmf_hip_ctx *c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    bpmf_hip_tensor_test *tt = new (std::nothrow) bpmf_hip_tensor_test();
    if (!tt) return fail(BPMF_HIP_ENOMEM, "tensor_test_create: out of host memory");
    tt->tensor = t; tt->nnz = nnz; ++t->ntests;
    // the test matrix of k_predict: one column per index of the last mode, entry p of that order in row p of Q
    std::vector<int64_t> tcolptr;
    order_by(idx2, t->dims[2], nnz, &tt->perm, &tcolptr);
    const size_t n1 = (size_t)std::max<int64_t>(nnz, 1);
    std::vector<int32_t> rowidx(n1, 0), ha(n1, 0), hb(n1, 0);
    std::vector<double> v(n1, 0.0);
    for (int64_t p = 0; p < nnz; ++p) {
        const int64_t e = tt->perm[(size_t)p];
        rowidx[(size_t)p] = (int32_t)p; ha[(size_t)p] = idx0[e]; hb[(size_t)p] = idx1[e]; v[(size_t)p] = vals[e];
    }
    if (!(rc = tt->qa.upload(ha.data(), (size_t)nnz)) && !(rc = tt->qb.upload(hb.data(), (size_t)nnz)) && !(rc = tt->Q.alloc((size_t)c->K * n1)) &&
        !(rc = tt->Q.zero_async(c->stream.get()))) {
        tt->tside = carrier(c, t->dims[2], (int64_t)n1, t->mean_rating, t->side[2]->d_items);
        tt->qcar = carrier(c, (int64_t)n1, 0, t->mean_rating, tt->Q.get());
        if (!tt->tside || !tt->qcar) rc = fail(BPMF_HIP_ENOMEM, "tensor_test_create: out of host memory");
        else rc = bpmf_hip_test_create(tt->tside, tcolptr.data(), rowidx.data(), v.data(), &tt->test);
    }
    if (rc) {
        const std::string keep = bpmf_hip_last_error();
        (void)bpmf_hip_tensor_test_destroy(tt);
        return fail(rc, keep);
    }
    *out = tt;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_tensor_predict(bpmf_hip_tensor_test *tt, int n, double *se, double *se_avg, int64_t *count)
{
    if (!tt || !se || !se_avg || !count) return fail(BPMF_HIP_EINVAL, "tensor_predict: NULL argument");
    if (n < 0) return fail(BPMF_HIP_EINVAL, "tensor_predict: n < 0");
    bpmf_hip_tensor *t = tt->tensor;
    bpmf_hip_ctx *c = t->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = enqueue_khatri_rao(c, t->side[0]->d_items, t->side[1]->d_items, tt->qa.get(), tt->qb.get(), tt->nnz, tt->Q.get());
    if (rc) return rc;
    tt->tside->d_items = t->side[2]->d_items;                         // (the copy that is current now: a sampler launch swaps the two)
    return bpmf_hip_predict(tt->test, tt->tside, tt->qcar, n, se, se_avg, count);
}

extern "C" int bpmf_hip_tensor_test_get(bpmf_hip_tensor_test *tt, double *pavg, double *pm2)
{
    if (!tt) return fail(BPMF_HIP_EINVAL, "tensor_test_get: NULL");
    if (tt->nnz == 0) return BPMF_HIP_OK;
    std::vector<double> a((size_t)tt->nnz), b((size_t)tt->nnz);
    const int rc = bpmf_hip_test_get(tt->test, pavg ? a.data() : nullptr, pm2 ? b.data() : nullptr);
    if (rc) return rc;
    for (int64_t p = 0; p < tt->nnz; ++p) {
        if (pavg) pavg[tt->perm[(size_t)p]] = a[(size_t)p];
        if (pm2) pm2[tt->perm[(size_t)p]] = b[(size_t)p];
    }
    return BPMF_HIP_OK;
}
