// capi_bias.hip -- row and column bias terms (kernels in kernels_bias.h): r_ij ~ N(mean + b_i + c_j + u_i . v_j,
// 1 / alpha), b_a ~ N(0, 1 / lambda) with one lambda per side.  A side with biases is a Gaussian side with a latent step: ahead of
// every one of its sampler launches its biases are redrawn from the factors that launch reads and the other side's biases, and the
// samplers read z = (r - b[col]) - c[row] in place of the ratings.  bpmf_hip_side_set_bias, the step, the evaluation's partner
// check, and the entry points that read, set and average the biases.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

namespace bpmf_capi {

int bias_pair_check(const bpmf_hip_side *self, const bpmf_hip_side *other)
{
    if ((bool)self->bias == (bool)other->bias) return 0;
    return fail(BPMF_HIP_EINVAL, "bias: both sides of a pair carry bias terms or neither does (bpmf_hip_side_set_bias)");
}

// The bias step of the half-iteration being enqueued, on the stream `st` its sampler goes on, ahead of it: the place and the factor
// copies of probit_latent_enqueue (capi_probit.hip).  No host wait.
int bias_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st)
{
    bpmf_hip_ctx *c = self->ctx;
    int rc = bias_pair_check(self, other);
    if (rc) return rc;
    if (!(alpha > 0.0) || !std::isfinite(alpha)) return fail(BPMF_HIP_EINVAL, "bias: a side with bias terms is sampled with a finite alpha > 0");
    if (c->comm || sharded(self) || self->reduce_on || self->item_n >= 0 || self->d_prop || c->dtype != BPMF_HIP_F64)
        return fail(BPMF_HIP_EINVAL, "bias: needs the side whole on one GPU in fp64, without a communicator, BPMF_REDUCE or propagated priors");
    if (other->ncols != self->nrows) return fail(BPMF_HIP_EINVAL, "bias: the other side has not one column per row of this side");
    bpmf_bias *bs = self->bias.get();
    // a sampled precision: drawn from the biases the side holds now, at the start of every half-iteration of the side but its first
    // (the rule of the sampled link precision, capi_link_lambda.hip); the step below reads the word the draw wrote
    if (bs->sample_lambda && bs->steps > 0) {
        bpmf_launch::BiasLambdaLaunch q{};
        q.b = bs->b.get(); q.ncols = self->ncols;
        const double a = bs->a0 + 0.5 * (double)self->ncols;
        q.dd = a - 1.0 / 3.0;
        const double nine_dd = 9.0 * q.dd;
        q.c = 1.0 / std::sqrt(nine_dd);
        q.b0 = bs->b0; q.iter = (uint32_t)iter; q.tag = bs->tag;
        q.lambda = bs->lambda.get(); q.trace = bs->trace.get(); q.cap = bs->trace_cap; q.fail = bs->fail.dev();
        bpmf_launch::bias_lambda(q, st);
        ++bs->draws;
    }
    bpmf_launch::BiasStepLaunch p{};
    p.m = side_csc(self); p.vals = self->d_vals; p.f = factor_pair(self, other);
    p.pieceptr = bs->pieceptr.get(); p.npieces = bs->npieces;
    p.iter = (uint32_t)iter; p.tag = bs->tag; p.mean = self->mean_rating; p.alpha = alpha;
    p.lambda = bs->lambda.get(); p.cbias = other->bias->b.get();
    p.e = bs->e.get(); p.part = bs->part.get(); p.b = bs->b.get(); p.z = bs->z.get(); p.fail = bs->fail.dev();
    if (bpmf_launch::bias_step(p, st)) return fail(BPMF_HIP_EINVAL, "bias: unsupported K " + std::to_string(c->K));
    ++bs->steps;
    return 0;
}

}  // namespace bpmf_capi

extern "C" int bpmf_hip_side_set_bias(bpmf_hip_side *s, double lambda, unsigned tag, int role)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_set_bias: NULL");
    bpmf_hip_ctx *c = s->ctx;
    if (!std::isfinite(lambda) || !(lambda > 0.0)) {
        char v[32];
        snprintf(v, sizeof v, "%g", lambda);
        return fail(BPMF_HIP_EINVAL, "side_set_bias: lambda = " + std::string(v) + " is not finite and > 0");
    }
    if (tag == 0) return fail(BPMF_HIP_EINVAL, "side_set_bias: tag must be >= 1 (key word 0 belongs to the samplers' streams)");
    if (role != 0 && role != 1) return fail(BPMF_HIP_EINVAL, "side_set_bias: role must be 0 or 1");
    if (c->dtype != BPMF_HIP_F64) return fail(BPMF_HIP_EINVAL, "side_set_bias: not on an fp32 context");
    if (s->bias) return fail(BPMF_HIP_EINVAL, "side_set_bias: the side has bias terms already");
    if (s->tensor_mode) return fail(BPMF_HIP_EINVAL, "side_set_bias: not on a mode of a tensor (its rows are products of two other modes' rows)");
    if (s->implicit) return fail(BPMF_HIP_EINVAL, "side_set_bias: not on an implicit side (bpmf_hip_side_set_implicit)");
    int rc = refuse("side_set_bias", s, {Not::probit, Not::ordinal, Not::censored, Not::robust, Not::weights, Not::features, Not::prop_posterior, Not::reduce, Not::chain});
    if (rc || (rc = require_single_gpu("side_set_bias", c, s))) return rc;
    if (s->ring) return fail(BPMF_HIP_EINVAL, "side_set_bias: not on a side with a sample ring (bpmf_hip_side_samples_reserve)");
    if (s->foldin) return fail(BPMF_HIP_EINVAL, "side_set_bias: not together with fold-in (bpmf_hip_side_hyper_reserve)");
    if ((int64_t)s->h_colptr.size() != s->ncols + 1) return fail(BPMF_HIP_EINVAL, "side_set_bias: the side has no host column pointers");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    // the pieces of every column: ceil(n_a / piece), none for a column of at most `light` ratings
    const int64_t piece = bpmf_launch::bias_piece(), light = bpmf_launch::bias_light();
    std::vector<int64_t> pp((size_t)s->ncols + 1, 0);
    for (int64_t a = 0; a < s->ncols; ++a) {
        const int64_t n = s->h_colptr[(size_t)a + 1] - s->h_colptr[(size_t)a];
        pp[(size_t)a + 1] = pp[(size_t)a] + (n > light ? (n + piece - 1) / piece : 0);
    }
    auto bs = std::make_unique<bpmf_bias>();                          // (freed with everything it holds on every return below)
    const size_t n = (size_t)s->nnz, nc = (size_t)s->ncols;
    bs->npieces = pp.back();
    if ((rc = bs->b.alloc(nc)) || (rc = bs->bsum.alloc(nc)) || (rc = bs->z.alloc(n)) || (rc = bs->e.alloc(n)) ||
        (rc = bs->part.alloc((size_t)bs->npieces)) || (rc = bs->lambda.upload(&lambda, 1)) || (rc = bs->pieceptr.upload(pp.data(), pp.size())) ||
        (rc = bs->fail.alloc(1)) || (rc = ensure_colptr(s)) || (rc = bs->b.zero_async(c->stream.get())) || (rc = bs->bsum.zero_async(c->stream.get())))
        return rc;
    // b = 0 until the first step: z starts as the ratings
    if (n > 0) HIP_TRY(hipMemcpyAsync(bs->z.get(), s->d_vals, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream.get()));
    *bs->fail.host() = ~0ull;
    bs->lambda_host = lambda; bs->tag = (uint32_t)tag; bs->role = role;
    s->bias = std::move(bs);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_bias_get(bpmf_hip_side *s, double *b_host)
{
    if (!s || !b_host) return fail(BPMF_HIP_EINVAL, "side_bias_get: NULL argument");
    if (!s->bias) return fail(BPMF_HIP_EINVAL, "side_bias_get: not a side with bias terms (bpmf_hip_side_set_bias)");
    const int rc = latent_settle(__func__, s);
    if (rc) return rc;
    if (s->ncols > 0) HIP_TRY(hipMemcpy(b_host, s->bias->b.get(), (size_t)s->ncols * sizeof(double), hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_bias_set(bpmf_hip_side *s, const double *b_host)
{
    if (!s || !b_host) return fail(BPMF_HIP_EINVAL, "side_bias_set: NULL argument");
    if (!s->bias) return fail(BPMF_HIP_EINVAL, "side_bias_set: not a side with bias terms (bpmf_hip_side_set_bias)");
    for (int64_t a = 0; a < s->ncols; ++a)
        if (!std::isfinite(b_host[a])) return fail(BPMF_HIP_EINVAL, "side_bias_set: the bias of column " + std::to_string((long long)a) + " is not finite");
    const int rc = latent_settle(__func__, s);
    if (rc) return rc;
    if (s->ncols > 0) HIP_TRY(hipMemcpy(s->bias->b.get(), b_host, (size_t)s->ncols * sizeof(double), hipMemcpyHostToDevice));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_bias_latent(bpmf_hip_side *s, double *z_host)
{
    if (!s || !z_host) return fail(BPMF_HIP_EINVAL, "side_bias_latent: NULL argument");
    if (!s->bias) return fail(BPMF_HIP_EINVAL, "side_bias_latent: not a side with bias terms (bpmf_hip_side_set_bias)");
    return latent_read_back(__func__, s, s->bias->z.get(), z_host);
}

extern "C" int bpmf_hip_side_bias_add(bpmf_hip_side *s)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_bias_add: NULL");
    if (!s->bias) return fail(BPMF_HIP_EINVAL, "side_bias_add: not a side with bias terms (bpmf_hip_side_set_bias)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    // S0 holds the side's newest bias step; the next one is behind this kernel in the same queue.  Enqueue only: nothing waits.
    bpmf_launch::bias_accumulate(s->bias->b.get(), s->ncols, s->bias->bsum.get(), c->stream.get());
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "side_bias_add: kernel launch failed");
    c->last_sampler_done = nullptr;                                   // (the newest thing on S0 is no longer a sampler)
    ++s->bias->kept;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_bias_mean(bpmf_hip_side *s, double *mean_host, int *count)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_bias_mean: NULL argument");
    if (!s->bias) return fail(BPMF_HIP_EINVAL, "side_bias_mean: not a side with bias terms (bpmf_hip_side_set_bias)");
    bpmf_bias *bs = s->bias.get();
    if (count) *count = bs->kept;
    if (!mean_host) return BPMF_HIP_OK;
    if (bs->kept == 0) return fail(BPMF_HIP_EINVAL, "side_bias_mean: nothing added (bpmf_hip_side_bias_add)");
    const int rc = latent_settle(__func__, s);
    if (rc) return rc;
    if (s->ncols > 0) HIP_TRY(hipMemcpy(mean_host, bs->bsum.get(), (size_t)s->ncols * sizeof(double), hipMemcpyDeviceToHost));
    const double k = (double)bs->kept;
    for (int64_t a = 0; a < s->ncols; ++a) mean_host[a] /= k;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_bias_prior(bpmf_hip_side *s, double a0, double b0)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_bias_prior: NULL");
    if (!s->bias) return fail(BPMF_HIP_EINVAL, "side_bias_prior: not a side with bias terms (bpmf_hip_side_set_bias)");
    if (!(a0 > 0.0) || !std::isfinite(a0) || !(b0 >= 0.0) || !std::isfinite(b0))
        return fail(BPMF_HIP_EINVAL, "side_bias_prior: the prior Gamma(A0, B0) needs a finite A0 > 0 and a finite B0 >= 0");
    // (the device draw is Marsaglia-Tsang without the boost step of a shape below 1)
    if (a0 + 0.5 * (double)s->ncols < 1.0) return fail(BPMF_HIP_EINVAL, "side_bias_prior: the shape A0 + N / 2 of the conditional is below 1");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = latent_settle(__func__, s);
    if (rc) return rc;
    bpmf_bias *bs = s->bias.get();
    const int cap = 1 << 16;                                          // iterations whose draw is kept in the trace
    std::vector<double> nan((size_t)cap, std::numeric_limits<double>::quiet_NaN());
    if ((rc = bs->trace.upload(nan.data(), nan.size()))) return rc;
    bs->trace_cap = cap; bs->sample_lambda = true; bs->a0 = a0; bs->b0 = b0;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_bias_lambda_get(bpmf_hip_side *s, double *lambda, double *trace_host, int ntrace, int64_t *steps, int64_t *draws)
{
    if (!s || !lambda || ntrace < 0 || (ntrace > 0 && !trace_host)) return fail(BPMF_HIP_EINVAL, "side_bias_lambda_get: bad argument");
    if (!s->bias) return fail(BPMF_HIP_EINVAL, "side_bias_lambda_get: not a side with bias terms (bpmf_hip_side_set_bias)");
    bpmf_bias *bs = s->bias.get();
    const int rc = latent_settle(__func__, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(lambda, bs->lambda.get(), sizeof(double), hipMemcpyDeviceToHost));
    // slot i: the precision the step of iteration i ran with -- the newest draw at or before i, the initial value before the first
    const int have = std::min(ntrace, bs->trace_cap);
    if (have > 0) HIP_TRY(hipMemcpy(trace_host, bs->trace.get(), (size_t)have * sizeof(double), hipMemcpyDeviceToHost));
    double cur = bs->lambda_host;
    for (int i = 0; i < ntrace; ++i) {
        if (i < have && !std::isnan(trace_host[i])) cur = trace_host[i];
        trace_host[i] = cur;
    }
    if (steps) *steps = bs->steps;
    if (draws) *draws = bs->draws;
    return BPMF_HIP_OK;
}
