// capi_censor.hip -- censored ratings (kernel in kernels_censor.h): bpmf_hip_side_set_censored, the latent step
// ahead of every sampler launch of such a side, and the entry points that read the counts and the latent values back.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

namespace bpmf_capi {

// The latent kernel of the half-iteration being enqueued, on the stream `st` its sampler goes on, ahead of it: the place and the
// factor copies of probit_latent_enqueue (capi_probit.hip).  A side whose flags are all zero launches nothing.
int censor_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st)
{
    bpmf_hip_ctx *c = self->ctx;
    if (!(alpha > 0.0) || !std::isfinite(alpha)) return fail(BPMF_HIP_EINVAL, "censored: a censored side is sampled with a finite alpha > 0");
    if (c->comm || sharded(self) || self->reduce_on || self->item_n >= 0 || self->d_prop)
        return fail(BPMF_HIP_EINVAL, "censored: needs the side whole on one GPU, without a communicator, BPMF_REDUCE or propagated priors");
    const bpmf_censor *cs = self->censor.get();
    bpmf_launch::CensorLatentLaunch p{};
    p.pos = cs->pos.get(); p.col = cs->col.get(); p.row = cs->row.get(); p.sign = cs->sign.get(); p.n = cs->n; p.vals = self->d_vals;
    p.f = factor_pair(self, other);
    p.iter = (uint32_t)iter; p.tag = cs->tag; p.mean = self->mean_rating;
    p.sqrt_alpha = std::sqrt(alpha); p.inv_sqrt_alpha = 1.0 / p.sqrt_alpha;
    p.z = cs->z.get(); p.fail = cs->fail.dev();
    if (bpmf_launch::censor_latent(p, st)) return fail(BPMF_HIP_EINVAL, "censored: unsupported K " + std::to_string(c->K));
    return 0;
}

}  // namespace bpmf_capi

extern "C" int bpmf_hip_side_set_censored(bpmf_hip_side *s, const int8_t *flags, unsigned tag)
{
    if (!s || !flags) return fail(BPMF_HIP_EINVAL, "side_set_censored: NULL argument");
    bpmf_hip_ctx *c = s->ctx;
    if (s->censor) return fail(BPMF_HIP_EINVAL, "side_set_censored: the side is a censored side already");
    int rc = refuse("side_set_censored", s, {Not::bias, Not::probit, Not::features, Not::robust, Not::weights, Not::prop_posterior, Not::ordinal});
    if (rc) return rc;
    if (tag == 0) return fail(BPMF_HIP_EINVAL, "side_set_censored: tag must be >= 1 (key word 0 belongs to the samplers' streams)");
    if ((rc = require_single_gpu("side_set_censored", c, s)) || (rc = refuse("side_set_censored", s, {Not::reduce}))) return rc;
    if ((int64_t)s->h_colptr.size() != s->ncols + 1) return fail(BPMF_HIP_EINVAL, "side_set_censored: the side has no host column pointers");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    auto cs = std::make_unique<bpmf_censor>();                        // (freed with everything it holds on every return below)
    // z starts as the ratings; only the censored positions are ever rewritten
    if ((rc = cs->z.alloc((size_t)s->nnz)) || (rc = cs->fail.alloc(1))) return rc;
    if (s->nnz > 0) HIP_TRY(hipMemcpyAsync(cs->z.get(), s->d_vals, (size_t)s->nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream.get()));
    // the lists of the censored entries in the order of the CSC, in one pass over the flags: positions ascend, columns come from
    // the host column pointers, rows from the side's row indices (on the device since the side was created)
    std::vector<int32_t> rowidx((size_t)s->nnz);
    if (s->nnz > 0) HIP_TRY(hipMemcpy(rowidx.data(), s->d_rowidx, (size_t)s->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> pos;
    std::vector<int32_t> col, row;
    std::vector<int8_t> sign;
    int64_t nright = 0;
    for (int64_t cc = 0; cc < s->ncols; ++cc)
        for (int64_t p = s->h_colptr[(size_t)cc]; p < s->h_colptr[(size_t)cc + 1]; ++p) {
            if (flags[p] < -1 || flags[p] > 1)
                return fail(BPMF_HIP_EINVAL, "side_set_censored: flag " + std::to_string((int)flags[p]) + " of rating " + std::to_string((long long)p) +
                                                 " is not one of -1, 0, +1");
            if (!flags[p]) continue;
            pos.push_back(p); col.push_back((int32_t)cc); row.push_back(rowidx[(size_t)p]); sign.push_back(flags[p]);
            nright += flags[p] > 0;
        }
    const int64_t n = (int64_t)pos.size();
    if ((rc = cs->pos.upload(pos.data(), (size_t)n)) || (rc = cs->col.upload(col.data(), (size_t)n)) || (rc = cs->row.upload(row.data(), (size_t)n)) ||
        (rc = cs->sign.upload(sign.data(), (size_t)n)))
        return rc;
    *cs->fail.host() = ~0ull;
    cs->n = n; cs->nright = nright; cs->nleft = n - nright; cs->tag = (uint32_t)tag;
    s->censor = std::move(cs);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_censored_count(bpmf_hip_side *s, int64_t *right, int64_t *left)
{
    if (!s || !right || !left) return fail(BPMF_HIP_EINVAL, "side_censored_count: NULL argument");
    if (!s->censor) return fail(BPMF_HIP_EINVAL, "side_censored_count: not a censored side (bpmf_hip_side_set_censored)");
    *right = s->censor->nright; *left = s->censor->nleft;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_censored_latent(bpmf_hip_side *s, double *z_host)
{
    if (!s || !z_host) return fail(BPMF_HIP_EINVAL, "side_censored_latent: NULL argument");
    if (!s->censor) return fail(BPMF_HIP_EINVAL, "side_censored_latent: not a censored side (bpmf_hip_side_set_censored)");
    return latent_read_back(__func__, s, s->censor->z.get(), z_host);
}
