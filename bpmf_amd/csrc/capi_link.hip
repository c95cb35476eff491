// capi_link.hip -- side information (kernels in kernels_link.h): the features of a side, its link matrix beta
// and offsets M = F beta, and bpmf_hip_link_sample, the blocking half-iteration that feeds the unchanged column samplers the
// residual ratings r - m_c . y_r.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"
#include "link_sparse.h"
#include "link_lambda.h"

using namespace bpmf_capi;

namespace {

constexpr int kMaxD = 1024;

// G = L L^T (row-major, lower), T = L^-T (row-major, upper) and Ginv = T T^T, all D x D; every inner loop runs along two rows.
bool factor_and_invert(int D, const std::vector<double> &G, std::vector<double> &T, std::vector<double> &Ginv)
{
    const size_t n = (size_t)D;
    std::vector<double> L(n * n, 0.0);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j <= i; ++j) {
            double s = G[i * n + j];
            const double *li = &L[i * n], *lj = &L[j * n];
            for (size_t k = 0; k < j; ++k) s -= li[k] * lj[k];
            if (i == j) {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                L[i * n + i] = std::sqrt(s);
            } else
                L[i * n + j] = s / L[j * n + j];
        }
    T.assign(n * n, 0.0);
    for (size_t c = 0; c < n; ++c) {                       // row c of T = column c of L^-1: L x = e_c
        double *x = &T[c * n];
        x[c] = 1.0 / L[c * n + c];
        for (size_t i = c + 1; i < n; ++i) {
            const double *li = &L[i * n];
            double s = 0.0;
            for (size_t k = c; k < i; ++k) s -= li[k] * x[k];
            x[i] = s / li[i];
        }
    }
    Ginv.assign(n * n, 0.0);
    for (size_t a = 0; a < n; ++a)
        for (size_t b = 0; b <= a; ++b) {
            const double *ta = &T[a * n], *tb = &T[b * n];
            double s = 0.0;
            for (size_t k = a; k < n; ++k) s += ta[k] * tb[k];
            Ginv[a * n + b] = s; Ginv[b * n + a] = s;
        }
    return true;
}

// C = A^T (B - 1 bvec^T) for any n: column tiles of 128 through the one kernel (B = A, n = D for F^T F)
int tn_product(const double *A, int64_t lda, const double *B, int64_t ldb, const double *bvec, int64_t N, int D, int n, double *C, int64_t ldc,
               double *part, hipStream_t st)
{
    for (int c0 = 0; c0 < n; c0 += 128) {
        bpmf_launch::LinkTnLaunch p{};
        p.A = A; p.lda = lda; p.B = B + c0; p.ldb = ldb; p.bvec = bvec ? bvec + c0 : nullptr; p.N = N; p.D = D; p.n = std::min(128, n - c0);
        p.C = C + c0; p.ldc = ldc; p.part = part;
        if (bpmf_launch::link_gemm_tn(p, st)) return fail(BPMF_HIP_EINVAL, "link: unsupported shape of the long-dimension product");
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int nn_product(const double *A, int64_t lda, const double *B, int64_t ldb, int64_t N, int Dr, int n, double *C, int64_t ldc, int ncw, hipStream_t st)
{
    bpmf_launch::LinkNnLaunch p{};
    p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.N = N; p.Dr = Dr; p.n = n; p.C = C; p.ldc = ldc; p.ncw = ncw;
    if (bpmf_launch::link_gemm_nn(p, st)) return fail(BPMF_HIP_EINVAL, "link: unsupported shape of the short-dimension product");
    HIP_TRY(hipGetLastError());
    return 0;
}

// M = F beta in the factors' layout (pad slots zero)
int offsets_update(bpmf_hip_side *s)
{
    const bpmf_hip_ctx *c = s->ctx;
    const bpmf_link *L = s->link.get();
    if (L->sparse) return link_sparse_offsets(s);
    return nn_product(L->dense->F.get(), L->D, L->beta.get(), c->K, s->ncols, L->D, c->Kt, L->m.get(), c->K, c->K, c->stream.get());
}

int residual_enqueue(bpmf_hip_side *s, const bpmf_hip_side *other, double *out)
{
    const bpmf_hip_ctx *c = s->ctx;
    bpmf_launch::LinkResidualLaunch p{};
    p.m = side_csc(s); p.vals = s->d_vals;
    p.offs = s->link->m.get(); p.other = other->d_items; p.K = c->K; p.kt = c->Kt; p.out = out;
    if (bpmf_launch::link_residual(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, "link: unsupported K " + std::to_string(c->K));
    HIP_TRY(hipGetLastError());
    return 0;
}

// items += offs over `total` elements; *norm = sum of the new items^2, the block partials added in block order on the host
int shift_and_norm(bpmf_hip_side *s, double *items, const double *offs, int64_t total, double *norm)
{
    bpmf_hip_ctx *c = s->ctx;
    bpmf_launch::link_shift(items, offs, total, s->link->norm.get(), c->stream.get());
    HIP_TRY(hipGetLastError());
    const int nb = bpmf_launch::link_shift_blocks(total);
    std::vector<double> part((size_t)std::max(nb, 1), 0.0);
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    if (nb > 0) HIP_TRY(hipMemcpy(part.data(), s->link->norm.get(), (size_t)nb * sizeof(double), hipMemcpyDeviceToHost));
    double nn = 0.0;
    for (int b = 0; b < nb; ++b) nn += part[(size_t)b];
    if (norm) *norm = nn;
    return 0;
}

int check_pair(const char *who, const bpmf_hip_side *self, const bpmf_hip_side *other)
{
    if (!self || !other) return fail(BPMF_HIP_EINVAL, std::string(who) + ": NULL argument");
    if (other->ctx != self->ctx) return fail(BPMF_HIP_EINVAL, std::string(who) + ": sides belong to different contexts");
    if (other->ncols != self->nrows) return fail(BPMF_HIP_EINVAL, std::string(who) + ": other side has the wrong number of columns");
    return 0;
}

}  // namespace

namespace bpmf_capi {

int link_tn_product(const double *A, int64_t lda, const double *B, int64_t ldb, const double *bvec, int64_t N, int D, int n, double *C,
                    int64_t ldc, double *part, hipStream_t st)
{
    return tn_product(A, lda, B, ldb, bvec, N, D, n, C, ldc, part, st);
}

int link_nn_product(const double *A, int64_t lda, const double *B, int64_t ldb, int64_t N, int Dr, int n, double *C, int64_t ldc, int ncw, hipStream_t st)
{
    return nn_product(A, lda, B, ldb, N, Dr, n, C, ldc, ncw, st);
}

int link_attach_common(const char *who, bpmf_hip_side *s, int D, double lambda, unsigned tag, size_t part_words, std::unique_ptr<bpmf_link> *out)
{
    const std::string w(who);
    bpmf_hip_ctx *c = s->ctx;
    if (s->link) return fail(BPMF_HIP_EINVAL, w + ": the side has features already");
    if (!(lambda > 0.0) || !std::isfinite(lambda)) return fail(BPMF_HIP_EINVAL, w + ": lambda_beta must be positive and finite");
    if (tag == 0) return fail(BPMF_HIP_EINVAL, w + ": tag must be >= 1 (key word 0 belongs to the samplers' streams)");
    if (c->dtype != BPMF_HIP_F64) return fail(BPMF_HIP_EINVAL, w + ": not on an fp32 context");
    int rc = require_single_gpu(who, c, s);
    if (rc) return rc;
    if ((rc = refuse(who, s, {Not::reduce, Not::bias, Not::chain}))) return rc;
    if (s->probit) return fail(BPMF_HIP_EINVAL, w + ": not on a probit side");
    if (s->ordinal) return fail(BPMF_HIP_EINVAL, w + ": not on an ordinal side");
    if (s->censor) return fail(BPMF_HIP_EINVAL, w + ": not on a censored side (the residuals would have to be formed from the latent values)");
    if ((rc = refuse(who, s, {Not::robust, Not::weights, Not::prop_posterior}))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    const size_t N = (size_t)s->ncols, ld = (size_t)c->K, Kt = (size_t)c->Kt;
    const int nblk = std::max(bpmf_launch::link_shift_blocks((int64_t)(N * ld)), bpmf_launch::link_shift_blocks((int64_t)D * c->K));
    auto L = std::make_unique<bpmf_link>();
    L->D = D; L->lambda = lambda; L->tag = (uint32_t)tag;
    if ((rc = L->beta.alloc((size_t)D * ld)) || (rc = L->beta_sum.alloc((size_t)D * ld)) || (rc = L->m.alloc(N * ld)) ||
        (rc = L->r.alloc((size_t)s->nnz)) || (rc = L->part.alloc(part_words)) || (rc = L->mu.alloc(ld)) || (rc = L->btb.alloc(Kt * Kt)) ||
        (rc = L->norm.alloc((size_t)nblk)) || (rc = ensure_colptr(s)))
        return rc;
    if ((rc = L->beta.zero_async(c->stream.get())) || (rc = L->beta_sum.zero_async(c->stream.get())) || (rc = L->m.zero_async(c->stream.get()))) return rc;
    // (the residuals of M = 0 are the ratings: a sampler that ran before the first link_sample would still read ratings)
    if (s->nnz > 0) HIP_TRY(hipMemcpyAsync(L->r.get(), s->d_vals, (size_t)s->nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream.get()));
    *out = std::move(L);
    return 0;
}

}  // namespace bpmf_capi

extern "C" int bpmf_hip_side_set_features(bpmf_hip_side *s, const double *F_host, int D, int row_major, double lambda_beta, unsigned tag)
{
    if (!s || !F_host) return fail(BPMF_HIP_EINVAL, "side_set_features: NULL argument");
    bpmf_hip_ctx *c = s->ctx;
    if (D < 1 || D > kMaxD) return fail(BPMF_HIP_EINVAL, "side_set_features: D must be 1 .. " + std::to_string(kMaxD));
    const int64_t N = s->ncols;
    const size_t nD = (size_t)N * (size_t)D, DD = (size_t)D * D;
    for (size_t q = 0; q < nD; ++q)
        if (!std::isfinite(F_host[q])) return fail(BPMF_HIP_EINVAL, "side_set_features: feature " + std::to_string(q) + " is not finite");
    const int K = c->K, Kt = c->Kt;
    std::unique_ptr<bpmf_link> L;
    int rc = link_attach_common("side_set_features", s, D, lambda_beta, tag,
                                std::max(bpmf_launch::link_tn_part_words(N, D, Kt), bpmf_launch::link_tn_part_words(D, Kt, Kt)), &L);
    if (rc) return rc;
    std::vector<double> tmp;
    const double *Frm = F_host;
    if (!row_major) {                                                  // column-major (.ddm): F[d * N + i] -> F[i * D + d], in tiles
        tmp.resize(std::max<size_t>(nD, 1));
        constexpr int64_t TL = 32;
        for (int64_t i0 = 0; i0 < N; i0 += TL)
            for (int64_t d0 = 0; d0 < D; d0 += TL)
                for (int64_t i = i0; i < std::min(N, i0 + TL); ++i)
                    for (int64_t d = d0; d < std::min<int64_t>(D, d0 + TL); ++d) tmp[(size_t)i * D + d] = F_host[(size_t)d * N + i];
        Frm = tmp.data();
    }
    auto dn = std::make_unique<bpmf_link_dense>();
    if ((rc = dn->F.upload(Frm, nD))) return rc;
    tmp.clear(); tmp.shrink_to_fit();
    std::vector<double> G(DD), T, Ginv;
    {   // G = F^T F on the device, factored and inverted on the host
        DevBuf<double> d_G, d_part0;
        if ((rc = d_G.alloc(DD)) || (rc = d_part0.alloc(bpmf_launch::link_tn_part_words(N, D, std::min(D, 128))))) return rc;
        if ((rc = tn_product(dn->F.get(), D, dn->F.get(), D, nullptr, N, D, D, d_G.get(), D, d_part0.get(), c->stream.get()))) return rc;
        if ((rc = bounded_stream_sync(c, c->stream.get(), __func__))) return rc;
        if (hipMemcpy(G.data(), d_G.get(), DD * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(BPMF_HIP_ENODEV, "side_set_features: copy of G failed");
    }
    for (int d = 0; d < D; ++d) G[(size_t)d * D + d] += lambda_beta;
    if (!factor_and_invert(D, G, T, Ginv)) return fail(BPMF_HIP_ENUM, "side_set_features: F^T F + lambda_beta I is not positive definite");
    std::vector<double> W(2 * DD);                                     // [G^-1 | L_G^-T], D x 2 D
    for (int a = 0; a < D; ++a) {
        memcpy(&W[(size_t)a * 2 * D], &Ginv[(size_t)a * D], sizeof(double) * D);
        memcpy(&W[(size_t)a * 2 * D + D], &T[(size_t)a * D], sizeof(double) * D);
    }
    if ((rc = dn->W.upload(W.data(), 2 * DD)) || (rc = dn->PE.alloc(2 * (size_t)D * K)) || (rc = dn->PE.zero_async(c->stream.get()))) return rc;
    L->dense = std::move(dn);
    s->link = std::move(L);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_link_sample(bpmf_hip_side *self, bpmf_hip_side *other, double alpha)
{
    { const int rc = check_pair("link_sample", self, other); if (rc) return rc; }
    bpmf_hip_ctx *c = self->ctx;
    { const int rc = require_single_gpu("link_sample", c, self, other); if (rc) return rc; }
    bpmf_link *L = self->link.get();
    if (self->implicit || other->implicit)
        return fail(BPMF_HIP_EINVAL, "link_sample: the model is implicit: step BOTH sides with bpmf_hip_implicit_sample");
    if (L && (self->reduce_on || self->probit || self->d_prop))
        return fail(BPMF_HIP_EINVAL, "link_sample: features do not go together with BPMF_REDUCE, a probit side or propagated priors");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_state(self)) || (rc = ensure_state(other))) return rc;
    if ((rc = settle_async(self)) || (rc = settle_async(other))) return rc;
    if ((rc = flush_pending_stats(c, true))) return rc;
    const int K = c->K, Kt = c->Kt, D = L ? L->D : 0;
    const int64_t N = self->ncols;
    const int iter = self->iter + 1;
    const bool link = L != nullptr;
    hipStream_t st = c->stream.get();
    std::vector<double> mu((size_t)Kt), LU((size_t)Kt * Kt), LF((size_t)Kt * Kt), scatter;

    // 1. hyper-parameters: the link's scatter lambda_beta beta^T beta (K x K, formed on the device) and its D degrees of freedom.
    // 0. (a side that samples lambda_beta, section 15) lambda_beta | beta, Lambda first, from the same beta^T beta
    if (link) {
        scatter.assign((size_t)Kt * Kt, 0.0);
        if ((rc = tn_product(L->beta.get(), K, L->beta.get(), K, nullptr, D, Kt, Kt, L->btb.get(), Kt, L->part.get(), st))) return rc;
        if ((rc = bounded_stream_sync(c, st, __func__))) return rc;
        HIP_TRY(hipMemcpy(scatter.data(), L->btb.get(), scatter.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (L->sample_lambda && (rc = link_lambda_draw(self, scatter.data(), iter))) return rc;
        for (double &v : scatter) v *= L->lambda;
    }
    rc = bpmf_hyper_sample_ex(Kt, N, self->cov.data(), nullptr, link ? scatter.data() : nullptr, link ? D : 0, (uint32_t)iter, mu.data(), LU.data(),
                              LF.data());
    if (rc) return rc;

    if (link && L->sparse) {
        // 2'. beta by CG on a noise-injected right-hand side, 3'. M = F beta by the sparse product (capi_link_sparse.hip); 4. residuals
        if ((rc = link_sparse_draw(self, mu.data(), LU.data(), iter))) return rc;
        if ((rc = residual_enqueue(self, other, L->r.get()))) return rc;
    } else if (link) {
        // 2. beta = G^-1 P + L_G^-T E = [G^-1 | L_G^-T] [P ; E],  P = F^T (U - 1 mu^T),  E = Z R^-T with Lambda = R^T R
        std::vector<double> pad((size_t)K, 0.0);
        memcpy(pad.data(), mu.data(), sizeof(double) * Kt);
        HIP_TRY(hipMemcpyAsync(L->mu.get(), pad.data(), sizeof(double) * K, hipMemcpyHostToDevice, st));
        if ((rc = tn_product(L->dense->F.get(), D, self->d_items, K, L->mu.get(), N, D, Kt, L->dense->PE.get(), K, L->part.get(), st))) return rc;
        std::vector<double> Z((size_t)D * Kt), E((size_t)D * K, 0.0);
        bpmf_randn_stream_tag((uint32_t)iter, L->tag, D * Kt, Z.data());
        for (int d = 0; d < D; ++d) {                                   // row d: R e = z, R = LambdaU (upper, column-major)
            const double *z = &Z[(size_t)d * Kt];
            double *e = &E[(size_t)d * K];
            for (int i = Kt - 1; i >= 0; --i) {
                double v = z[i];
                for (int j = i + 1; j < Kt; ++j) v -= LU[(size_t)j * Kt + i] * e[j];
                e[i] = v / LU[(size_t)i * Kt + i];
            }
        }
        HIP_TRY(hipMemcpyAsync(L->dense->PE.get() + (size_t)D * K, E.data(), E.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));                              // (the host buffers above go out of use here)
        if (L->dense->devfac) {                                         // beta = L^-T (L^-1 P + E), G(lambda_beta) = L L^T factored on the device
            if ((rc = link_chol_draw(self))) return rc;
        } else if ((rc = nn_product(L->dense->W.get(), 2 * D, L->dense->PE.get(), K, D, 2 * D, Kt, L->beta.get(), K, K, st)))
            return rc;
        // 3. offsets, 4. residuals: from the copy of the other side's factors the sampler below reads
        if ((rc = offsets_update(self))) return rc;
        if ((rc = residual_enqueue(self, other, L->r.get()))) return rc;
    }

    // 5. the unchanged column samplers (on the residuals: launch_impl.h picks link->r), their sums, cov
    std::vector<double> sum((size_t)Kt), prod((size_t)Kt * Kt);
    double norm = 0.0;
    if (link) L->in_call = true;
    rc = bpmf_hip_sample_side(self, other, iter, alpha, mu.data(), LF.data(), sum.data(), prod.data(), &norm);
    if (link) L->in_call = false;
    if (rc) return rc;
    // 6. U = U~ + M on the copy the sampler wrote (d_items after its swap), and the norm of U
    if (link && (rc = shift_and_norm(self, self->d_items, L->m.get(), N * (int64_t)K, &norm))) return rc;
    c->last_sampler_done = nullptr;
    self->iter = iter;
    self->norm = norm;
    bpmf_cov_from_sums(Kt, N, sum.data(), prod.data(), self->cov.data());
    self->hp_mu = mu; self->hp_LambdaU = LU; self->hp_LambdaF = LF;
    { std::lock_guard<std::mutex> lk(self->wm); self->collected_iter = iter; self->norm_hist[iter & 7] = norm; }
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_get(bpmf_hip_side *s, double *beta_host, double *offsets_host)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_link_get: NULL");
    if (!s->link) return fail(BPMF_HIP_EINVAL, "side_link_get: the side has no features (bpmf_hip_side_set_features)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    const size_t K = (size_t)c->K, Kt = (size_t)c->Kt;
    if (beta_host) HIP_TRY(hipMemcpy2D(beta_host, Kt * sizeof(double), s->link->beta.get(), K * sizeof(double), Kt * sizeof(double), (size_t)s->link->D, hipMemcpyDeviceToHost));
    if (offsets_host && s->ncols > 0)
        HIP_TRY(hipMemcpy2D(offsets_host, Kt * sizeof(double), s->link->m.get(), K * sizeof(double), Kt * sizeof(double), (size_t)s->ncols, hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_set(bpmf_hip_side *s, const double *beta_host)
{
    if (!s || !beta_host) return fail(BPMF_HIP_EINVAL, "side_link_set: NULL argument");
    if (!s->link) return fail(BPMF_HIP_EINVAL, "side_link_set: the side has no features (bpmf_hip_side_set_features)");
    bpmf_hip_ctx *c = s->ctx;
    const size_t K = (size_t)c->K, Kt = (size_t)c->Kt;
    for (size_t q = 0; q < (size_t)s->link->D * Kt; ++q)
        if (!std::isfinite(beta_host[q])) return fail(BPMF_HIP_EINVAL, "side_link_set: beta is not finite");
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    HIP_TRY(hipMemcpy2D(s->link->beta.get(), K * sizeof(double), beta_host, Kt * sizeof(double), Kt * sizeof(double), (size_t)s->link->D, hipMemcpyHostToDevice));
    return offsets_update(s);
}

extern "C" int bpmf_hip_side_link_add(bpmf_hip_side *s)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_link_add: NULL");
    if (!s->link) return fail(BPMF_HIP_EINVAL, "side_link_add: the side has no features (bpmf_hip_side_set_features)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    bpmf_launch::link_shift(s->link->beta_sum.get(), s->link->beta.get(), (int64_t)s->link->D * c->K, s->link->norm.get(), c->stream.get());   // (sum += beta; the norm goes unused)
    HIP_TRY(hipGetLastError());
    c->last_sampler_done = nullptr;
    ++s->link->nsum;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_mean(bpmf_hip_side *s, double *beta_host, int *nsamples)
{
    if (!s || !beta_host) return fail(BPMF_HIP_EINVAL, "side_link_mean: NULL argument");
    if (!s->link) return fail(BPMF_HIP_EINVAL, "side_link_mean: the side has no features (bpmf_hip_side_set_features)");
    if (nsamples) *nsamples = s->link->nsum;
    if (s->link->nsum == 0) return fail(BPMF_HIP_EINVAL, "side_link_mean: nothing added (bpmf_hip_side_link_add)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    const size_t K = (size_t)c->K, Kt = (size_t)c->Kt;
    HIP_TRY(hipMemcpy2D(beta_host, Kt * sizeof(double), s->link->beta_sum.get(), K * sizeof(double), Kt * sizeof(double), (size_t)s->link->D, hipMemcpyDeviceToHost));
    const double n = (double)s->link->nsum;
    for (size_t q = 0; q < (size_t)s->link->D * Kt; ++q) beta_host[q] /= n;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_residual(bpmf_hip_side *s, const bpmf_hip_side *other, double *r_host)
{
    { const int rc = check_pair("side_link_residual", s, other); if (rc) return rc; }
    if (!r_host) return fail(BPMF_HIP_EINVAL, "side_link_residual: NULL argument");
    if (!s->link) return fail(BPMF_HIP_EINVAL, "side_link_residual: the side has no features (bpmf_hip_side_set_features)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    { const int rc = residual_enqueue(s, other, s->link->r.get()); if (rc) return rc; }
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    if (s->nnz > 0) HIP_TRY(hipMemcpy(r_host, s->link->r.get(), (size_t)s->nnz * sizeof(double), hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_shift(bpmf_hip_side *s, double *norm)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_link_shift: NULL");
    if (!s->link) return fail(BPMF_HIP_EINVAL, "side_link_shift: the side has no features (bpmf_hip_side_set_features)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    return shift_and_norm(s, s->d_items, s->link->m.get(), s->ncols * (int64_t)c->K, norm);
}

// ---- the two products on host arrays (tests, tools) ------------------------------------------------------------------------

extern "C" int bpmf_hip_link_gemm_tn(int device, const double *A, int64_t N, int D, const double *B, int n, const double *bvec, double *C)
{
    if (!A || !C || N < 1 || D < 1 || n < 1) return fail(BPMF_HIP_EINVAL, "link_gemm_tn: bad argument");
    if (!B && n != D) return fail(BPMF_HIP_EINVAL, "link_gemm_tn: B = NULL means B = A, n = D");
    if (B && n > 128) return fail(BPMF_HIP_EINVAL, "link_gemm_tn: n <= 128 (or B = NULL for A^T A)");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> dA, dB, dv, dC, dP;
    int rc;
    if ((rc = dA.upload(A, (size_t)N * D)) || (B && (rc = dB.upload(B, (size_t)N * n))) || (bvec && (rc = dv.upload(bvec, (size_t)n))) ||
        (rc = dC.alloc((size_t)D * n)) || (rc = dP.alloc(bpmf_launch::link_tn_part_words(N, D, std::min(n, 128)))))
        return rc;
    if ((rc = tn_product(dA.get(), D, B ? dB.get() : dA.get(), B ? n : D, dv.get(), N, D, n, dC.get(), n, dP.get(), nullptr))) return rc;
    if (hipDeviceSynchronize() != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_gemm_tn: kernel failed");
    if (hipMemcpy(C, dC.get(), (size_t)D * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_gemm_tn: copy failed");
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_link_gemm_nn(int device, const double *A, int64_t N, int D, const double *B, int n, double *C)
{
    if (!A || !B || !C || N < 1 || D < 1 || n < 1 || n > 128) return fail(BPMF_HIP_EINVAL, "link_gemm_nn: bad argument (n <= 128)");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> dA, dB, dC;
    int rc;
    if ((rc = dA.upload(A, (size_t)N * D)) || (rc = dB.upload(B, (size_t)D * n)) || (rc = dC.alloc((size_t)N * n))) return rc;
    if ((rc = nn_product(dA.get(), D, dB.get(), n, N, D, n, dC.get(), n, n, nullptr))) return rc;
    if (hipDeviceSynchronize() != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_gemm_nn: kernel failed");
    if (hipMemcpy(C, dC.get(), (size_t)N * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_gemm_nn: copy failed");
    return BPMF_HIP_OK;
}
