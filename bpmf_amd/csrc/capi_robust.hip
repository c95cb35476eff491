// capi_robust.hip -- Student-t noise (kernels in kernels_robust.h): r_ij ~ t_nu(mean + u_i . v_j, 1 / sqrt(alpha)) as
// the scale mixture r_ij | w_ij ~ N(mean + u_i . v_j, 1 / (alpha w_ij)), w_ij ~ Gamma(nu / 2, rate nu / 2).  A robust side is a side with
// per-rating weights (capi_weights.hip) whose sw / zw are redrawn on the device ahead of every one of its sampler launches, from the
// factors that launch reads: bpmf_hip_side_set_robust, the weight step, and the posterior mean of the weights.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

namespace bpmf_capi {

// The weight kernel of the half-iteration being enqueued, on the stream `st` its sampler goes on, ahead of it: the place, the factor
// copies and the "queued already" flag of probit_latent_enqueue (capi_probit.hip).  No host wait.
int robust_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st)
{
    bpmf_hip_ctx *c = self->ctx;
    if (!(alpha > 0.0) || !std::isfinite(alpha)) return fail(BPMF_HIP_EINVAL, "robust: a robust side is sampled with a finite alpha > 0");
    if (c->comm || sharded(self) || self->reduce_on || self->item_n >= 0 || self->d_prop || c->dtype != BPMF_HIP_F64 || !self->weights)
        return fail(BPMF_HIP_EINVAL, "robust: needs the side whole on one GPU in fp64, without a communicator, BPMF_REDUCE or propagated priors");
    const bpmf_robust *rb = self->robust.get();
    bpmf_launch::RobustWeightsLaunch p{};
    p.m = side_csc(self); p.vals = self->d_vals; p.f = factor_pair(self, other);
    p.iter = (uint32_t)iter; p.tag = rb->tag; p.mean = self->mean_rating; p.sqrt_alpha = std::sqrt(alpha); p.nu = rb->nu;
    const double a = 0.5 * (rb->nu + 1.0);
    p.dd = a - 1.0 / 3.0;
    const double nine_dd = 9.0 * p.dd;
    p.c = 1.0 / std::sqrt(nine_dd);
    p.sw = self->weights->sw.get(); p.zw = self->weights->zw.get(); p.fail = rb->fail.dev();
    if (bpmf_launch::robust_weights(p, st)) return fail(BPMF_HIP_EINVAL, "robust: unsupported K " + std::to_string(c->K));
    return 0;
}

}  // namespace bpmf_capi

extern "C" int bpmf_hip_side_set_robust(bpmf_hip_side *s, double nu, unsigned tag)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_set_robust: NULL");
    bpmf_hip_ctx *c = s->ctx;
    if (!std::isfinite(nu) || !(nu >= 1.0)) {
        char v[32];
        snprintf(v, sizeof v, "%g", nu);
        return fail(BPMF_HIP_EINVAL, "side_set_robust: nu = " + std::string(v) + " is not finite and >= 1");
    }
    if (tag == 0) return fail(BPMF_HIP_EINVAL, "side_set_robust: tag must be >= 1 (key word 0 belongs to the samplers' streams)");
    if (c->dtype != BPMF_HIP_F64) return fail(BPMF_HIP_EINVAL, "side_set_robust: not on an fp32 context");
    if (s->robust) return fail(BPMF_HIP_EINVAL, "side_set_robust: the side is a robust side already");
    int rc = refuse("side_set_robust", s, {Not::bias, Not::weights, Not::probit, Not::censored, Not::ordinal, Not::features, Not::prop_posterior, Not::reduce});
    if (rc || (rc = require_single_gpu("side_set_robust", c, s))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    // w = 1 until the first launch: sw = 1 and zw = r - mean, the fp64 subtraction bpmf_hip_side_set_weights does (the ratings come
    // back from the device: a side keeps no host copy of them)
    const size_t n = (size_t)s->nnz;
    std::vector<double> sw(std::max<size_t>(n, 1), 1.0), zw(std::max<size_t>(n, 1), 0.0);
    if (n > 0) HIP_TRY(hipMemcpy(zw.data(), s->d_vals, n * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < n; ++p) zw[p] = zw[p] - s->mean_rating;
    auto ws = std::make_unique<bpmf_weights>();                       // (both freed with everything they hold on every return below)
    auto rb = std::make_unique<bpmf_robust>();
    if ((rc = ws->sw.upload(sw.data(), n)) || (rc = ws->zw.upload(zw.data(), n)) || (rc = rb->wsum.alloc(n)) || (rc = rb->fail.alloc(1)) ||
        (rc = ensure_colptr(s)) || (rc = rb->wsum.zero_async(c->stream.get())))
        return rc;
    *rb->fail.host() = ~0ull;
    rb->nu = nu; rb->tag = (uint32_t)tag;
    s->weights = std::move(ws);
    s->robust = std::move(rb);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_robust_add(bpmf_hip_side *s)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_robust_add: NULL");
    if (!s->robust) return fail(BPMF_HIP_EINVAL, "side_robust_add: not a robust side (bpmf_hip_side_set_robust)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    // S0 holds the side's newest weight kernel and sampler; the next weight kernel is behind this one in the same queue.  Enqueue
    // only: nothing waits.
    bpmf_launch::robust_accumulate(s->weights->sw.get(), s->nnz, s->robust->wsum.get(), c->stream.get());
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "side_robust_add: kernel launch failed");
    c->last_sampler_done = nullptr;                                   // (the newest thing on S0 is no longer a sampler)
    ++s->robust->kept;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_robust_get(bpmf_hip_side *s, double *wmean_host, int *count, double *nu)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_robust_get: NULL argument");
    if (!s->robust) return fail(BPMF_HIP_EINVAL, "side_robust_get: not a robust side (bpmf_hip_side_set_robust)");
    bpmf_robust *rb = s->robust.get();
    if (count) *count = rb->kept;
    if (nu) *nu = rb->nu;
    if (!wmean_host) return BPMF_HIP_OK;
    if (rb->kept == 0) return fail(BPMF_HIP_EINVAL, "side_robust_get: nothing added (bpmf_hip_side_robust_add)");
    { const int rc = latent_read_back(__func__, s, rb->wsum.get(), wmean_host); if (rc) return rc; }
    const double k = (double)rb->kept;
    for (int64_t p = 0; p < s->nnz; ++p) wmean_host[p] /= k;
    return BPMF_HIP_OK;
}
