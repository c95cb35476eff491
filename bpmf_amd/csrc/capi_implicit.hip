// capi_implicit.hip -- implicit feedback: every cell of the matrix is observed with precision alpha w, an
// unobserved one as r = 0 with w = w0, an observed one with its value and a confidence w > w0, mean rating 0.  The conditional of
// column j,
//   Lambda* = Lambda + alpha w0 G + alpha sum_obs (w - w0) u u^T,  G = sum over ALL columns u of the other side of u u^T
//   b       = Lambda mu + alpha sum_obs w r u,
// is the weighted column update with sw = sqrt(w - w0), zw = w r / sqrt(w - w0) under the prior precision Lambda + alpha w0 G whose
// right-hand side stays Lambda mu.  bpmf_hip_side_set_implicit installs these arrays as the side's bpmf_weights, so the launch path
// picks the weighted form of the side's sampler family unchanged; bpmf_hip_implicit_sample forms G on the device (k_link_gemm_tn:
// fp64, fixed order, no atomics) and hands alpha w0 G to the stateless half-iteration, which adds it to the blob's LambdaF behind Lmu.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"
#include "link_lambda.h"

using namespace bpmf_capi;

extern "C" int bpmf_hip_side_set_implicit(bpmf_hip_side *s, double w0, const double *w)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_set_implicit: NULL argument");
    bpmf_hip_ctx *c = s->ctx;
    if (!(w0 > 0.0) || !std::isfinite(w0)) return fail(BPMF_HIP_EINVAL, "side_set_implicit: w0 must be finite and > 0");
    if (c->dtype != BPMF_HIP_F64) return fail(BPMF_HIP_EINVAL, "side_set_implicit: not on an fp32 context");
    if (s->implicit) return fail(BPMF_HIP_EINVAL, "side_set_implicit: the side is an implicit side already");
    int rc = refuse("side_set_implicit", s, {Not::bias, Not::robust, Not::chain});
    if (rc) return rc;
    if (s->weights) return fail(BPMF_HIP_EINVAL, "side_set_implicit: not on a side with per-rating weights (pass the confidences to this call)");
    if ((rc = refuse("side_set_implicit", s, {Not::probit, Not::censored, Not::ordinal, Not::features, Not::prop_posterior, Not::reduce}))) return rc;
    if (s->foldin) return fail(BPMF_HIP_EINVAL, "side_set_implicit: not together with fold-in on the side (the folded-in rows would need G)");
    if (s->mean_rating != 0.0) {
        char v[32];
        snprintf(v, sizeof v, "%g", s->mean_rating);
        return fail(BPMF_HIP_EINVAL, "side_set_implicit: the side's mean rating is " + std::string(v) + ", the implicit model needs exactly 0");
    }
    if ((rc = require_single_gpu("side_set_implicit", c, s))) return rc;
    for (int64_t p = 0; w && p < s->nnz; ++p)
        if (!(w[p] > w0) || !std::isfinite(w[p])) {
            char v[32], v0[32];
            snprintf(v, sizeof v, "%g", w[p]); snprintf(v0, sizeof v0, "%g", w0);
            return fail(BPMF_HIP_EINVAL, "side_set_implicit: the confidence " + std::string(v) + " of rating " + std::to_string((long long)p) +
                                             " is not finite and > w0 = " + v0);
        }
    if (!w && !(1.0 > w0)) return fail(BPMF_HIP_EINVAL, "side_set_implicit: without confidences every rating has w = 1, which needs w0 < 1");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    // sw = sqrt(w - w0) and zw = w r / sw are formed on the host in IEEE arithmetic, as side_set_weights forms its arrays (the
    // ratings come back from the device: a side keeps no host copy of them)
    const size_t n = (size_t)s->nnz;
    std::vector<double> sw(std::max<size_t>(n, 1)), zw(std::max<size_t>(n, 1));
    if (n > 0) HIP_TRY(hipMemcpy(zw.data(), s->d_vals, n * sizeof(double), hipMemcpyDeviceToHost));
    auto ws = std::make_unique<bpmf_weights>();
    double wmin = std::numeric_limits<double>::infinity(), wmax = 0.0;
    for (size_t p = 0; p < n; ++p) {
        const double wp = w ? w[p] : 1.0;
        sw[p] = std::sqrt(wp - w0);
        zw[p] = wp * zw[p] / sw[p];
        ws->nweighted += wp != 1.0;
        wmin = std::min(wmin, wp); wmax = std::max(wmax, wp);
    }
    if (n > 0) { ws->wmin = wmin; ws->wmax = wmax; }
    auto im = std::make_unique<bpmf_implicit>();
    im->w0 = w0;
    const int Kt = c->Kt;
    im->prior.assign((size_t)Kt * Kt, 0.0);
    if ((rc = ws->sw.upload(sw.data(), n)) || (rc = ws->zw.upload(zw.data(), n)) || (rc = im->gram.alloc((size_t)Kt * Kt)) ||
        (rc = im->part.alloc(bpmf_launch::link_tn_part_words(s->nrows, Kt, Kt))))
        return rc;
    s->weights = std::move(ws);
    s->implicit = std::move(im);
    return BPMF_HIP_OK;
}

// w0 of an implicit side (0: the side is not implicit)
extern "C" double bpmf_hip_side_implicit_w0(const bpmf_hip_side *s) { return s && s->implicit ? s->implicit->w0 : 0.0; }

// G of the side's newest half-iteration (Kt x Kt): what bpmf_hip_implicit_sample formed from the other side's factors
extern "C" int bpmf_hip_side_implicit_gram(bpmf_hip_side *s, double *G_host)
{
    if (!s || !G_host) return fail(BPMF_HIP_EINVAL, "side_implicit_gram: NULL argument");
    if (!s->implicit) return fail(BPMF_HIP_EINVAL, "side_implicit_gram: the side is not implicit (bpmf_hip_side_set_implicit)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    HIP_TRY(hipMemcpy(G_host, s->implicit->gram.get(), (size_t)c->Kt * c->Kt * sizeof(double), hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}

// The blocking half-iteration of an implicit side, modelled on bpmf_hip_link_sample: hyper-parameters at counter iter from the side's
// own cov, G of the other side's current factors (all its columns), the stateless weighted launch under Lambda + alpha w0 G, cov.
extern "C" int bpmf_hip_implicit_sample(bpmf_hip_side *self, bpmf_hip_side *other, double alpha)
{
    if (!self || !other) return fail(BPMF_HIP_EINVAL, "implicit_sample: NULL argument");
    bpmf_hip_ctx *c = self->ctx;
    if (other->ctx != c) return fail(BPMF_HIP_EINVAL, "implicit_sample: sides belong to different contexts");
    if (other->ncols != self->nrows) return fail(BPMF_HIP_EINVAL, "implicit_sample: other side has the wrong number of columns");
    if (!self->implicit) return fail(BPMF_HIP_EINVAL, "implicit_sample: the side is not implicit (bpmf_hip_side_set_implicit)");
    if (!other->implicit)
        return fail(BPMF_HIP_EINVAL, "implicit_sample: the other side is not implicit: both sides of a model are implicit, or neither");
    if (other->implicit->w0 != self->implicit->w0) return fail(BPMF_HIP_EINVAL, "implicit_sample: the two sides were given different w0");
    if (!(alpha > 0.0) || !std::isfinite(alpha)) return fail(BPMF_HIP_EINVAL, "implicit_sample: alpha must be finite and > 0");
    { const int rc = require_single_gpu("implicit_sample", c, self, other); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_state(self)) || (rc = ensure_state(other))) return rc;
    if ((rc = settle_async(self)) || (rc = settle_async(other))) return rc;
    if ((rc = flush_pending_stats(c, true))) return rc;
    const int K = c->K, Kt = c->Kt;
    const int64_t N = self->ncols;
    const int iter = self->iter + 1;
    hipStream_t st = c->stream.get();
    bpmf_implicit *im = self->implicit.get();
    std::vector<double> mu((size_t)Kt), LU((size_t)Kt * Kt), LF((size_t)Kt * Kt);

    // 1. hyper-parameters from the side's own cov
    if ((rc = bpmf_hyper_sample_ex(Kt, N, self->cov.data(), nullptr, nullptr, 0, (uint32_t)iter, mu.data(), LU.data(), LF.data()))) return rc;
    // 2. G = V^T V over every column of the other side (those without ratings too), leading Kt x Kt; alpha w0 G on the host
    if ((rc = link_tn_product((const double *)other->d_items, K, (const double *)other->d_items, K, nullptr, other->ncols, Kt, Kt, im->gram.get(),
                              Kt, im->part.get(), st)))
        return rc;
    if ((rc = bounded_stream_sync(c, st, __func__))) return rc;
    HIP_TRY(hipMemcpy(im->prior.data(), im->gram.get(), im->prior.size() * sizeof(double), hipMemcpyDeviceToHost));
    const double aw0 = alpha * im->w0;
    for (double &v : im->prior) v *= aw0;

    // 3. the unchanged weighted column samplers (launch_impl.h picks the side's weights), their sums, cov
    std::vector<double> sum((size_t)Kt), prod((size_t)Kt * Kt);
    double norm = 0.0;
    im->in_call = true;
    rc = bpmf_hip_sample_side(self, other, iter, alpha, mu.data(), LF.data(), sum.data(), prod.data(), &norm);
    im->in_call = false;
    if (rc) return rc;
    c->last_sampler_done = nullptr;
    self->iter = iter;
    self->norm = norm;
    bpmf_cov_from_sums(Kt, N, sum.data(), prod.data(), self->cov.data());
    self->hp_mu = mu; self->hp_LambdaU = LU; self->hp_LambdaF = LF;
    { std::lock_guard<std::mutex> lk(self->wm); self->collected_iter = iter; self->norm_hist[iter & 7] = norm; }
    return BPMF_HIP_OK;
}
