// capi_weights.hip -- per-rating precision weights: r_ij ~ N(mean + u_i . v_j, 1 / (alpha w_ij)).
// bpmf_hip_side_set_weights stores sw = sqrt(w) and zw = sqrt(w) (r - mean_rating) on the device; sampler_into (launch_impl.h) then
// launches the weighted form of the side's sampler family, which reads zw as its values with mean 0 and multiplies every gathered
// factor row by sw.  Nothing is enqueued per iteration.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

extern "C" int bpmf_hip_side_set_weights(bpmf_hip_side *s, const double *w)
{
    if (!s || !w) return fail(BPMF_HIP_EINVAL, "side_set_weights: NULL argument");
    bpmf_hip_ctx *c = s->ctx;
    if (c->dtype != BPMF_HIP_F64) return fail(BPMF_HIP_EINVAL, "side_set_weights: not on an fp32 context");
    if (s->implicit) return fail(BPMF_HIP_EINVAL, "side_set_weights: not on an implicit side (bpmf_hip_side_set_implicit takes the confidences itself)");
    if (s->robust) return fail(BPMF_HIP_EINVAL, "side_set_weights: not on a side with Student-t noise (bpmf_hip_side_set_robust redraws the weights itself)");
    int rc = refuse("side_set_weights", s, {Not::bias, Not::probit, Not::censored, Not::ordinal, Not::features, Not::prop_posterior, Not::reduce});
    if (rc || (rc = require_single_gpu("side_set_weights", c, s))) return rc;
    for (int64_t p = 0; p < s->nnz; ++p)
        if (!(w[p] > 0.0) || !std::isfinite(w[p])) {
            char v[32];
            snprintf(v, sizeof v, "%g", w[p]);
            return fail(BPMF_HIP_EINVAL, "side_set_weights: the weight " + std::string(v) + " of rating " + std::to_string((long long)p) +
                                             " is not finite and > 0");
        }
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    // (a launch of the side that still reads the arrays being replaced; an evaluation reads neither)
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    // sqrt(w) and sqrt(w) (r - mean) are formed on the host: the IEEE square root and product, correctly rounded, whatever the
    // device's sqrt sequence would give (the ratings come back from the device: a side keeps no host copy of them)
    const size_t n = (size_t)s->nnz;
    std::vector<double> sw(std::max<size_t>(n, 1)), zw(std::max<size_t>(n, 1));
    if (n > 0) HIP_TRY(hipMemcpy(zw.data(), s->d_vals, n * sizeof(double), hipMemcpyDeviceToHost));
    auto ws = std::make_unique<bpmf_weights>();
    double wmin = std::numeric_limits<double>::infinity(), wmax = 0.0;
    for (size_t p = 0; p < n; ++p) {
        const double d = zw[p] - s->mean_rating;
        sw[p] = std::sqrt(w[p]);
        zw[p] = sw[p] * d;
        ws->nweighted += w[p] != 1.0;
        wmin = std::min(wmin, w[p]); wmax = std::max(wmax, w[p]);
    }
    if (n > 0) { ws->wmin = wmin; ws->wmax = wmax; }
    if ((rc = ws->sw.upload(sw.data(), n)) || (rc = ws->zw.upload(zw.data(), n))) return rc;
    s->weights = std::move(ws);                                       // (a second call: the arrays held so far are freed here)
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_weights_get(bpmf_hip_side *s, double *sw_host, double *zw_host)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_weights_get: NULL argument");
    if (!s->weights) return fail(BPMF_HIP_EINVAL, "side_weights_get: the side has no weights (bpmf_hip_side_set_weights)");
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (s->robust) { const int rc = latent_settle(__func__, s); if (rc) return rc; }     // (redrawn per launch: the arrays the side's newest launch read)
    const size_t n = (size_t)s->nnz;
    if (sw_host && n > 0) HIP_TRY(hipMemcpy(sw_host, s->weights->sw.get(), n * sizeof(double), hipMemcpyDeviceToHost));
    if (zw_host && n > 0) HIP_TRY(hipMemcpy(zw_host, s->weights->zw.get(), n * sizeof(double), hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}

// (number of ratings whose weight is not 1, the smallest and the largest weight) of a side with weights
extern "C" int bpmf_hip_side_weights_count(bpmf_hip_side *s, int64_t *nweighted, double *wmin, double *wmax)
{
    if (!s || !nweighted || !wmin || !wmax) return fail(BPMF_HIP_EINVAL, "side_weights_count: NULL argument");
    if (!s->weights) return fail(BPMF_HIP_EINVAL, "side_weights_count: the side has no weights (bpmf_hip_side_set_weights)");
    *nweighted = s->weights->nweighted; *wmin = s->weights->wmin; *wmax = s->weights->wmax;
    return BPMF_HIP_OK;
}
