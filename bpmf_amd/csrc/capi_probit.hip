// capi_probit.hip -- probit likelihood for binary matrices (kernels in kernels_probit.h):
// bpmf_hip_side_set_probit, the latent step ahead of every sampler launch of such a side, the posterior predictive
// probabilities of a test matrix, and the host-only bpmf_hip_auc.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

namespace bpmf_capi {

// The latent kernel of the half-iteration being enqueued, on the stream `st` its sampler goes on, ahead of it: `self->d_items` is
// still the copy the side holds before this update (the sampler behind writes the other copy, or this one in place, later in
// the same queue), and `other->d_items` the copy that sampler reads.  Called by bpmf_hip_sys_sample BEFORE it makes that stream
// wait for the gate kernel of the hyper-parameters (unfused form: the kernel needs none and runs while the host still draws
// them), and by launch_sampler (capi_sample.hip) for every other path.
int probit_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st)
{
    bpmf_hip_ctx *c = self->ctx;
    if (alpha != 1.0) return fail(BPMF_HIP_EINVAL, "probit: a probit side is sampled with alpha = 1 (the latent scores have unit variance)");
    if (c->comm || sharded(self) || self->reduce_on || self->item_n >= 0)
        return fail(BPMF_HIP_EINVAL, "probit: needs the side whole on one GPU, without a communicator and without BPMF_REDUCE");
    bpmf_launch::ProbitLatentLaunch p{};
    const bpmf_probit *pb = self->probit.get();
    p.m = side_csc(self); p.f = factor_pair(self, other); p.sign = pb->sign.get();
    p.iter = (uint32_t)iter; p.tag = pb->tag; p.z = pb->z.get(); p.fail = pb->fail.dev();
    if (bpmf_launch::probit_latent(p, st)) return fail(BPMF_HIP_EINVAL, "probit: unsupported K " + std::to_string(c->K));
    return 0;
}

}  // namespace bpmf_capi

extern "C" int bpmf_hip_side_set_probit(bpmf_hip_side *s, double threshold, unsigned tag)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_set_probit: NULL");
    bpmf_hip_ctx *c = s->ctx;
    if (s->probit) return fail(BPMF_HIP_EINVAL, "side_set_probit: the side is a probit side already");
    int rc = refuse("side_set_probit", s, {Not::bias, Not::ordinal, Not::features, Not::censored, Not::robust, Not::weights});
    if (rc) return rc;
    if (s->mean_rating != 0.0) return fail(BPMF_HIP_EINVAL, "side_set_probit: the side must have been created with mean_rating = 0");
    if (tag == 0) return fail(BPMF_HIP_EINVAL, "side_set_probit: tag must be >= 1 (key word 0 belongs to the samplers' streams)");
    if (!std::isfinite(threshold)) return fail(BPMF_HIP_EINVAL, "side_set_probit: the threshold is not finite");
    if ((rc = require_single_gpu("side_set_probit", c, s)) || (rc = refuse("side_set_probit", s, {Not::reduce}))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    auto pb = std::make_unique<bpmf_probit>();
    if ((rc = pb->z.alloc((size_t)s->nnz)) || (rc = pb->sign.alloc((size_t)s->nnz)) || (rc = ensure_colptr(s)) || (rc = pb->fail.alloc(1)) ||
        (rc = pb->z.zero_async(c->stream.get())))
        return rc;
    *pb->fail.host() = ~0ull;
    pb->tag = (uint32_t)tag;
    bpmf_launch::probit_sign(s->d_vals, s->nnz, threshold, pb->sign.get(), c->stream.get());
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "side_set_probit: kernel launch failed");
    s->probit = std::move(pb);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_probit_latent(bpmf_hip_side *s, double *z_host)
{
    if (!s || !z_host) return fail(BPMF_HIP_EINVAL, "side_probit_latent: NULL argument");
    if (!s->probit) return fail(BPMF_HIP_EINVAL, "side_probit_latent: not a probit side (bpmf_hip_side_set_probit)");
    return latent_read_back(__func__, s, s->probit->z.get(), z_host);
}

extern "C" int bpmf_hip_test_probit_add(bpmf_hip_test *t, bpmf_hip_side *self, bpmf_hip_side *other)
{
    if (!t || !self || !other) return fail(BPMF_HIP_EINVAL, "test_probit_add: NULL argument");
    bpmf_hip_ctx *c = self->ctx;
    if (t->side != self) return fail(BPMF_HIP_EINVAL, "test_probit_add: the test matrix belongs to another side");
    if (other->ctx != c || other->ncols != self->nrows) return fail(BPMF_HIP_EINVAL, "test_probit_add: the two sides do not belong together");
    { const int rc = require_single_gpu("test_probit_add", c, self, other); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    if (!t->d_prob_sum) {
        int rc = t->d_prob_sum.alloc((size_t)t->nnz);
        if (!rc) rc = t->d_prob_sum.zero_async(c->stream.get());
        if (rc) return rc;
    }
    // S0 holds the newest sampler of both sides and d_items is the copy it writes (as in bpmf_hip_train_sse); whichever
    // sampler rewrites one of these copies later is behind this kernel in the same queue.  Enqueue only: nothing waits.
    bpmf_launch::ProbitProbLaunch p{};
    p.tcol = t->d_tcol.get(); p.trow = t->d_trow.get(); p.nnz = t->nnz; p.f = factor_pair(self, other);
    p.sum = t->d_prob_sum.get();
    if (bpmf_launch::probit_prob(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, "test_probit_add: unsupported K " + std::to_string(c->K));
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "test_probit_add: kernel launch failed");
    c->last_sampler_done = nullptr;                                   // (the newest thing on S0 is no longer a sampler)
    ++t->prob_n;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_test_probit_get(bpmf_hip_test *t, double *prob_host, int *nsamples)
{
    if (!t || !prob_host) return fail(BPMF_HIP_EINVAL, "test_probit_get: NULL argument");
    if (nsamples) *nsamples = t->prob_n;
    if (!t->d_prob_sum || t->prob_n == 0) return fail(BPMF_HIP_EINVAL, "test_probit_get: nothing added (bpmf_hip_test_probit_add)");
    bpmf_hip_ctx *c = t->side->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    if (t->nnz > 0) HIP_TRY(hipMemcpy(prob_host, t->d_prob_sum.get(), (size_t)t->nnz * sizeof(double), hipMemcpyDeviceToHost));
    const double inv = (double)t->prob_n;
    for (int64_t q = 0; q < t->nnz; ++q) prob_host[q] /= inv;
    return BPMF_HIP_OK;
}

// Host only.  AUC = (sum of the average ranks of the positives - P (P + 1) / 2) / (P N): the fraction of (positive, negative)
// pairs the score orders correctly, ties counted half.
extern "C" int bpmf_hip_auc(const double *score, const double *value, int64_t n, double threshold, double *auc)
{
    if (!auc || n < 0 || (n > 0 && (!score || !value))) return fail(BPMF_HIP_EINVAL, "auc: bad argument");
    for (int64_t i = 0; i < n; ++i) if (score[i] != score[i]) return fail(BPMF_HIP_EINVAL, "auc: score " + std::to_string((long long)i) + " is NaN");
    std::vector<int64_t> order((size_t)n);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [score](int64_t a, int64_t b) { return score[a] < score[b]; });
    // twice the rank sum of the positives, in integers (average ranks are half-integers): exact up to 2^63
    unsigned long long twice = 0, npos = 0;
    for (int64_t i = 0; i < n;) {
        int64_t j = i;
        unsigned long long pos = 0;
        while (j < n && score[order[(size_t)j]] == score[order[(size_t)i]]) { pos += value[order[(size_t)j]] > threshold; ++j; }
        twice += pos * (unsigned long long)(i + 1 + j);              // ranks i + 1 .. j: average (i + 1 + j) / 2
        npos += pos;
        i = j;
    }
    const unsigned long long nneg = (unsigned long long)n - npos;
    if (npos == 0 || nneg == 0) { *auc = std::numeric_limits<double>::quiet_NaN(); return BPMF_HIP_OK; }
    const unsigned long long num2 = twice - npos * (npos + 1);       // 2 x (pairs in order + half the ties)
    *auc = (double)num2 / (2.0 * (double)npos * (double)nneg);
    return BPMF_HIP_OK;
}
