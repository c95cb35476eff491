// capi_noise.hip -- training residuals for the adaptive noise precision (bpmf_hip_train_sse; kernels in kernels_noise.h).
// The draw of the precision itself, bpmf_hip_noise_sample, is host code beside the other Gamma draws in hyper.cpp.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

extern "C" int bpmf_hip_train_sse(bpmf_hip_side *self, bpmf_hip_side *other, double *sse, int64_t *n)
{
    if (!self || !other || !sse || !n) return fail(BPMF_HIP_EINVAL, "train_sse: NULL argument");
    bpmf_hip_ctx *c = self->ctx;
    if (other->ctx != c) return fail(BPMF_HIP_EINVAL, "train_sse: the two sides belong to different contexts");
    if (other->ncols != self->nrows) return fail(BPMF_HIP_EINVAL, "train_sse: the other side must have one column per row of this side's ratings");
    int rc = require_single_gpu("train_sse", c, self, other, " (a sharded side or a communicator would need an all-reduce of the sum, which adaptive noise does not do)");
    if (rc) return rc;
    // (alpha | y needs a fresh draw of every censored y from the newest factors of BOTH sides ahead of the sum: DESIGN.md section 16)
    if (self->bias || other->bias) return fail(BPMF_HIP_EINVAL, "train_sse: not with a side with bias terms (the residuals would leave the biases out)");
    if (self->censor || other->censor) return fail(BPMF_HIP_EINVAL, "train_sse: not with a censored side (the sum would take the bounds for measurements)");
    if (self->ordinal || other->ordinal) return fail(BPMF_HIP_EINVAL, "train_sse: not with an ordinal side (its ratings are levels and alpha is 1)");
    // (alpha | r of the weighted model takes sum w (r - mean - u . v)^2: not what this sums)
    if (self->weights || other->weights) return fail(BPMF_HIP_EINVAL, "train_sse: not with a side with per-rating weights (the sum would have to be weighted)");
    HIP_TRY(hipSetDevice(c->device));
    *sse = 0.0;
    *n = self->nnz;
    if (self->nnz == 0) return BPMF_HIP_OK;
    if (!self->sse) {                                                 // first call: the column pointers and the partials, once
        auto e = std::make_unique<bpmf_sse>();
        e->nblk = bpmf_launch::train_sse_blocks(self->nnz, c->num_cu);
        if ((rc = ensure_colptr(self)) || (rc = e->part.alloc((size_t)e->nblk + 1))) return rc;
        self->sse = std::move(e);
    }
    // S0 holds the newest sampler of both sides (bpmf_hip_sys_sample and bpmf_hip_sample_side enqueue there) and d_items is
    // the copy it writes: behind it in the queue, nothing else needed.  Nothing this waits for depends on a later enqueue:
    // statistics waiting for a rider and a deferred evaluation go to other launches, not to the samplers ahead of this one.
    bpmf_launch::SseLaunch p{};
    p.m = side_csc(self); p.vals = self->d_vals; p.f = factor_pair(self, other);
    p.mean = self->mean_rating; p.partial = self->sse->part.get(); p.nblk = self->sse->nblk;
    if (bpmf_launch::train_sse(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, "train_sse: unsupported K " + std::to_string(c->K));
    c->last_sampler_done = nullptr;                                   // (the newest thing on S0 is no longer a sampler)
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "train_sse: kernel launch failed");
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    HIP_TRY(hipMemcpy(sse, self->sse->part.get() + self->sse->nblk, sizeof(double), hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}
