// capi_ordinal.hip -- ordinal probit likelihood with sampled cutpoints (kernels in kernels_ordinal.h):
// bpmf_hip_side_set_ordinal, the latent step ahead of every sampler launch of such a side, the log-likelihood of two cutpoint
// tables in one pass, the Metropolis-Hastings step of the cutpoints (host arithmetic around that pass) and the posterior
// predictive level probabilities of a test matrix.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"
#include "philox.h"

using namespace bpmf_capi;

namespace {

constexpr double kInf = std::numeric_limits<double>::infinity();
constexpr double kTail = 37.0, kRsqrt2 = 0.70710678118654752440, kHalfLog2Pi = 0.91893853320467274178;   // (kernels_ordinal.h)

double log_tail(double a)
{
    const double r = 1.0 / (a * a);
    const double s = std::fma(r, std::fma(r, std::fma(r, std::fma(r, 105.0, -15.0), 3.0), -1.0), 1.0);
    return -0.5 * a * a - std::log(a) - kHalfLog2Pi + std::log(s);
}

// log[Phi(b) - Phi(a)], the formulas of ordinal_logmass (kernels_ordinal.h) on the host: the proposal correction of the cutpoint step
double logmass(double a, double b)
{
    if (a + b < 0.0) { const double t = a; a = -b; b = -t; }
    if (a > kTail) {
        const double la = log_tail(a);
        if (!(b < kInf)) return la;
        return la + std::log1p(-std::exp(log_tail(b) - la));
    }
    return std::log(0.5 * (std::erfc(a * kRsqrt2) - std::erfc(b * kRsqrt2)));
}

int check_cutpoints(const char *who, const double *cut, int nlev)
{
    for (int i = 0; i + 1 < nlev; ++i) {
        if (!std::isfinite(cut[i])) return fail(BPMF_HIP_EINVAL, std::string(who) + ": cutpoint " + std::to_string(i + 1) + " is not finite");
        if (i > 0 && !(cut[i] > cut[i - 1])) return fail(BPMF_HIP_EINVAL, std::string(who) + ": the cutpoints are not strictly increasing");
    }
    return 0;
}

// the table -inf, cut, +inf on the host and on the device (the caller has waited for everything that reads the old table)
int store_cutpoints(bpmf_hip_side *s, const double *cut)
{
    bpmf_ordinal *o = s->ordinal.get();
    o->cut[0] = -kInf; o->cut[(size_t)o->nlev] = kInf;
    for (int i = 0; i + 1 < o->nlev; ++i) o->cut[(size_t)i + 1] = cut[i];
    HIP_TRY(hipMemcpy(o->g.get(), o->cut.data(), ((size_t)o->nlev + 1) * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

int check_pair(const char *who, const bpmf_hip_side *self, const bpmf_hip_side *other)
{
    const bpmf_hip_ctx *c = self->ctx;
    if (other->ctx != c || other->ncols != self->nrows) return fail(BPMF_HIP_EINVAL, std::string(who) + ": the two sides do not belong together");
    const int rc = require_single_gpu(who, c, self, other);
    if (rc) return rc;
    if (self->reduce_on || other->reduce_on) return fail(BPMF_HIP_EINVAL, std::string(who) + ": not together with the BPMF_REDUCE formulation");
    return 0;
}

// both sums of the side's log-likelihood: under its own table and under the proposal `cutp` (nlev - 1 cutpoints).  Enqueues and waits.
int loglik_pass(const char *who, bpmf_hip_side *self, bpmf_hip_side *other, const double *cutp, double *out)
{
    bpmf_hip_ctx *c = self->ctx;
    bpmf_ordinal *o = self->ordinal.get();
    std::vector<double> tab((size_t)o->nlev + 1);
    tab[0] = -kInf; tab[(size_t)o->nlev] = kInf;
    for (int i = 0; i + 1 < o->nlev; ++i) tab[(size_t)i + 1] = cutp[i];
    HIP_TRY(hipSetDevice(c->device));
    // (a blocking copy of at most 136 bytes: the pass that read the previous proposal was waited for below, and this call waits again)
    HIP_TRY(hipMemcpy(o->g_prop.get(), tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    // S0 holds the newest sampler of both sides and d_items is the copy it writes, as in bpmf_hip_train_sse
    bpmf_launch::OrdinalLoglikLaunch p{};
    p.m = side_csc(self); p.f = factor_pair(self, other); p.level = o->level.get();
    p.g0 = o->g.get(); p.g1 = o->g_prop.get(); p.nlev = o->nlev; p.partial = o->part.get();
    if (bpmf_launch::ordinal_loglik(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, std::string(who) + ": unsupported K " + std::to_string(c->K));
    ++o->loglik_launches;
    c->last_sampler_done = nullptr;                                   // (the newest thing on S0 is no longer a sampler)
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, std::string(who) + ": kernel launch failed");
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), who); if (rs_) return rs_; }
    HIP_TRY(hipMemcpy(out, o->part.get() + 2 * bpmf_launch::ordinal_blocks(self->nnz), 2 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

namespace bpmf_capi {

// The latent kernel of the half-iteration being enqueued, on the stream its sampler goes on, ahead of it: the place and the
// copies of probit_latent_enqueue (capi_probit.hip).  It reads the side's cutpoint table on the device, which only changes
// while nothing is in flight (bpmf_hip_ordinal_cut_step and bpmf_hip_side_ordinal_cut_set wait first).
int ordinal_latent_enqueue(bpmf_hip_side *self, const bpmf_hip_side *other, int iter, double alpha, hipStream_t st)
{
    bpmf_hip_ctx *c = self->ctx;
    if (alpha != 1.0) return fail(BPMF_HIP_EINVAL, "ordinal: an ordinal side is sampled with alpha = 1 (the latent scores have unit variance)");
    if (c->comm || sharded(self) || self->reduce_on || self->item_n >= 0 || self->d_prop)
        return fail(BPMF_HIP_EINVAL, "ordinal: needs the side whole on one GPU, without a communicator, BPMF_REDUCE or propagated priors");
    bpmf_launch::OrdinalLatentLaunch p{};
    const bpmf_ordinal *o = self->ordinal.get();
    p.m = side_csc(self); p.f = factor_pair(self, other); p.level = o->level.get();
    p.iter = (uint32_t)iter; p.tag = o->tag; p.g = o->g.get(); p.nlev = o->nlev; p.z = o->z.get(); p.fail = o->fail.dev();
    if (bpmf_launch::ordinal_latent(p, st)) return fail(BPMF_HIP_EINVAL, "ordinal: unsupported K " + std::to_string(c->K));
    return 0;
}

}  // namespace bpmf_capi

extern "C" int bpmf_hip_side_set_ordinal(bpmf_hip_side *s, const double *levels, int nlevels, const double *cutpoints, unsigned tag)
{
    if (!s || !levels) return fail(BPMF_HIP_EINVAL, "side_set_ordinal: NULL argument");
    bpmf_hip_ctx *c = s->ctx;
    if (nlevels < 2 || nlevels > 16) return fail(BPMF_HIP_EINVAL, "side_set_ordinal: " + std::to_string(nlevels) + " levels (2 .. 16 are supported)");
    for (int i = 0; i < nlevels; ++i) {
        if (!std::isfinite(levels[i])) return fail(BPMF_HIP_EINVAL, "side_set_ordinal: level " + std::to_string(i + 1) + " is not finite");
        if (i > 0 && !(levels[i] > levels[i - 1])) return fail(BPMF_HIP_EINVAL, "side_set_ordinal: the levels are not strictly increasing");
    }
    if (s->ordinal) return fail(BPMF_HIP_EINVAL, "side_set_ordinal: the side is an ordinal side already");
    int rc = refuse("side_set_ordinal", s, {Not::bias, Not::probit, Not::censored, Not::robust, Not::weights, Not::features, Not::prop_posterior, Not::chain});
    if (rc) return rc;
    if (s->mean_rating != 0.0) return fail(BPMF_HIP_EINVAL, "side_set_ordinal: the side must have been created with mean_rating = 0");
    if (tag == 0) return fail(BPMF_HIP_EINVAL, "side_set_ordinal: tag must be >= 1 (key word 0 belongs to the samplers' streams)");
    if (cutpoints) { const int rk = check_cutpoints("side_set_ordinal", cutpoints, nlevels); if (rk) return rk; }
    if ((rc = require_single_gpu("side_set_ordinal", c, s)) || (rc = refuse("side_set_ordinal", s, {Not::reduce}))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    // the level of every rating, on the host: the ratings come back from the device once
    std::vector<double> vals((size_t)s->nnz);
    if (s->nnz > 0) HIP_TRY(hipMemcpy(vals.data(), s->d_vals, (size_t)s->nnz * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<uint8_t> lev((size_t)s->nnz);
    std::vector<int64_t> count((size_t)nlevels, 0);
    for (int64_t p = 0; p < s->nnz; ++p) {
        const double *it = std::lower_bound(levels, levels + nlevels, vals[(size_t)p]);
        if (it == levels + nlevels || *it != vals[(size_t)p])
            return fail(BPMF_HIP_EINVAL, "side_set_ordinal: rating " + std::to_string((long long)p) + " (" + std::to_string(vals[(size_t)p]) + ") is not one of the levels");
        lev[(size_t)p] = (uint8_t)(it - levels);
        ++count[(size_t)(it - levels)];
    }
    // default cutpoints: Phi^-1 of the cumulative frequency of the levels <= c.  A level without a rating would repeat a cutpoint:
    // every level then counts half a rating more.
    std::vector<double> cut((size_t)nlevels - 1);
    if (cutpoints) {
        std::copy(cutpoints, cutpoints + nlevels - 1, cut.begin());
    } else {
        if (s->nnz == 0) return fail(BPMF_HIP_EINVAL, "side_set_ordinal: a side without ratings has no default cutpoints");
        const bool absent = *std::min_element(count.begin(), count.end()) == 0;
        const double add = absent ? 0.5 : 0.0, total = (double)s->nnz + add * nlevels;
        double cum = 0.0;
        for (int i = 0; i + 1 < nlevels; ++i) { cum += (double)count[(size_t)i] + add; cut[(size_t)i] = normal_quantile(cum / total); }
        if ((rc = check_cutpoints("side_set_ordinal (default cutpoints)", cut.data(), nlevels))) return rc;
    }
    auto o = std::make_unique<bpmf_ordinal>();
    o->nlev = nlevels; o->tag = (uint32_t)tag;
    o->levels.assign(levels, levels + nlevels);
    o->cut.assign((size_t)nlevels + 1, 0.0);
    const size_t nblk = (size_t)bpmf_launch::ordinal_blocks(s->nnz);
    if ((rc = o->z.alloc((size_t)s->nnz)) || (rc = o->level.upload(lev.data(), (size_t)s->nnz)) || (rc = ensure_colptr(s)) ||
        (rc = o->g.alloc((size_t)nlevels + 1)) || (rc = o->g_prop.alloc((size_t)nlevels + 1)) || (rc = o->part.alloc(2 * nblk + 2)) ||
        (rc = o->fail.alloc(1)) || (rc = o->z.zero_async(c->stream.get())))
        return rc;
    *o->fail.host() = ~0ull;
    s->ordinal = std::move(o);
    if ((rc = store_cutpoints(s, cut.data()))) { s->ordinal.reset(); return rc; }
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_ordinal_info(bpmf_hip_side *s, int *nlevels, double *levels, int64_t *loglik_launches)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_ordinal_info: NULL");
    if (!s->ordinal) return fail(BPMF_HIP_EINVAL, "side_ordinal_info: not an ordinal side (bpmf_hip_side_set_ordinal)");
    if (nlevels) *nlevels = s->ordinal->nlev;
    if (levels) std::copy(s->ordinal->levels.begin(), s->ordinal->levels.end(), levels);
    if (loglik_launches) *loglik_launches = s->ordinal->loglik_launches;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_ordinal_latent(bpmf_hip_side *s, double *z_host)
{
    if (!s || !z_host) return fail(BPMF_HIP_EINVAL, "side_ordinal_latent: NULL argument");
    if (!s->ordinal) return fail(BPMF_HIP_EINVAL, "side_ordinal_latent: not an ordinal side (bpmf_hip_side_set_ordinal)");
    return latent_read_back(__func__, s, s->ordinal->z.get(), z_host);
}

extern "C" int bpmf_hip_side_ordinal_cut_get(bpmf_hip_side *s, double *cutpoints)
{
    if (!s || !cutpoints) return fail(BPMF_HIP_EINVAL, "side_ordinal_cut_get: NULL argument");
    if (!s->ordinal) return fail(BPMF_HIP_EINVAL, "side_ordinal_cut_get: not an ordinal side (bpmf_hip_side_set_ordinal)");
    std::copy(s->ordinal->cut.begin() + 1, s->ordinal->cut.end() - 1, cutpoints);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_ordinal_cut_set(bpmf_hip_side *s, const double *cutpoints)
{
    if (!s || !cutpoints) return fail(BPMF_HIP_EINVAL, "side_ordinal_cut_set: NULL argument");
    if (!s->ordinal) return fail(BPMF_HIP_EINVAL, "side_ordinal_cut_set: not an ordinal side (bpmf_hip_side_set_ordinal)");
    { const int rk = check_cutpoints("side_ordinal_cut_set", cutpoints, s->ordinal->nlev); if (rk) return rk; }
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }     // (a latent kernel in flight reads the old table)
    return store_cutpoints(s, cutpoints);
}

extern "C" int bpmf_hip_ordinal_loglik(bpmf_hip_side *self, bpmf_hip_side *other, const double *cutpoints_prop, double *out)
{
    if (!self || !other || !cutpoints_prop || !out) return fail(BPMF_HIP_EINVAL, "ordinal_loglik: NULL argument");
    if (!self->ordinal) return fail(BPMF_HIP_EINVAL, "ordinal_loglik: not an ordinal side (bpmf_hip_side_set_ordinal)");
    int rc = check_pair("ordinal_loglik", self, other);
    if (rc) return rc;
    if ((rc = check_cutpoints("ordinal_loglik", cutpoints_prop, self->ordinal->nlev))) return rc;
    return loglik_pass("ordinal_loglik", self, other, cutpoints_prop, out);
}

// One Metropolis-Hastings step of all cutpoints given the factors (Cowles 1996), z integrated out.  The random numbers are the
// Philox4x32-10 blocks (counter = BPMF_ORDINAL_COUNTER(iter), c, 0, n; key = 42, 0):
//   proposal of cutpoint c = 1 .. C - 1, attempt n = 0 .. 63: u1 = 1 - canonical53(w3, w2), u2 = canonical53(w1, w0),
//       rho = sqrt(-2 ln u1), x1 = g_c + s rho cos(2 pi u2), x2 = g_c + s rho sin(2 pi u2); the first of x1, x2 inside
//       (g'_{c-1}, g_{c+1}) is g'_c, else the next attempt; after 64 attempts g'_c = g_c
//   accept: c = 0, n = 0: u = 1 - canonical53(w3, w2); accepted if ln u < l(g') - l(g) + the proposal correction
extern "C" int bpmf_hip_ordinal_cut_step(bpmf_hip_side *movies, bpmf_hip_side *users, int iter, double step, int *accepted)
{
    if (!movies || !users || !accepted) return fail(BPMF_HIP_EINVAL, "ordinal_cut_step: NULL argument");
    if (!movies->ordinal || !users->ordinal) return fail(BPMF_HIP_EINVAL, "ordinal_cut_step: both sides must be ordinal sides (bpmf_hip_side_set_ordinal)");
    bpmf_ordinal *om = movies->ordinal.get(), *ou = users->ordinal.get();
    if (om->nlev != ou->nlev || om->cut != ou->cut) return fail(BPMF_HIP_EINVAL, "ordinal_cut_step: the two sides do not hold the same cutpoints");
    if (!(step > 0.0) || !std::isfinite(step)) return fail(BPMF_HIP_EINVAL, "ordinal_cut_step: the step size must be positive and finite");
    if (iter < 0) return fail(BPMF_HIP_EINVAL, "ordinal_cut_step: iter < 0");
    int rc = check_pair("ordinal_cut_step", movies, users);
    if (rc) return rc;
    const int C = om->nlev;
    const uint32_t c0 = BPMF_ORDINAL_COUNTER(iter);
    const std::vector<double> &g = om->cut;                           // g[0] = -inf .. g[C] = +inf
    std::vector<double> gp((size_t)C + 1);
    gp[0] = -kInf; gp[(size_t)C] = kInf;
    for (int k = 1; k < C; ++k) {
        const double lo = gp[(size_t)k - 1], hi = g[(size_t)k + 1];
        double x = g[(size_t)k];
        for (int n = 0; n < 64; ++n) {
            const bpmf::Philox4 w = bpmf::philox4x32_10(c0, (uint32_t)k, 0u, (uint32_t)n, 42u, 0u);
            const double u1 = 1.0 - bpmf::canonical53(w.w[3], w.w[2]), u2 = bpmf::canonical53(w.w[1], w.w[0]);
            const double rho = std::sqrt(-2.0 * std::log(u1)), ang = 2.0 * 3.14159265358979323846 * u2;
            const double x1 = g[(size_t)k] + step * (rho * std::cos(ang)), x2 = g[(size_t)k] + step * (rho * std::sin(ang));
            if (x1 > lo && x1 < hi) { x = x1; break; }
            if (x2 > lo && x2 < hi) { x = x2; break; }
        }
        gp[(size_t)k] = x;
    }
    double ll[2];
    if ((rc = loglik_pass("ordinal_cut_step", movies, users, gp.data() + 1, ll))) return rc;
    double corr = 0.0;
    for (int k = 1; k < C; ++k)
        corr += logmass((gp[(size_t)k - 1] - g[(size_t)k]) / step, (g[(size_t)k + 1] - g[(size_t)k]) / step) -
                logmass((g[(size_t)k - 1] - gp[(size_t)k]) / step, (gp[(size_t)k + 1] - gp[(size_t)k]) / step);
    const bpmf::Philox4 w = bpmf::philox4x32_10(c0, 0u, 0u, 0u, 42u, 0u);
    const double u = 1.0 - bpmf::canonical53(w.w[3], w.w[2]);
    const double ratio = (ll[1] - ll[0]) + corr;
    *accepted = std::log(u) < ratio ? 1 : 0;                          // (a NaN ratio -- a proposal of no mass -- is a rejection)
    if (!*accepted) return BPMF_HIP_OK;
    // (loglik_pass has waited for S0: nothing in flight reads the tables)
    if ((rc = store_cutpoints(movies, gp.data() + 1)) || (rc = store_cutpoints(users, gp.data() + 1))) return rc;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_test_ordinal_add(bpmf_hip_test *t, bpmf_hip_side *self, bpmf_hip_side *other)
{
    if (!t || !self || !other) return fail(BPMF_HIP_EINVAL, "test_ordinal_add: NULL argument");
    bpmf_hip_ctx *c = self->ctx;
    if (t->side != self) return fail(BPMF_HIP_EINVAL, "test_ordinal_add: the test matrix belongs to another side");
    if (!self->ordinal) return fail(BPMF_HIP_EINVAL, "test_ordinal_add: not an ordinal side (bpmf_hip_side_set_ordinal)");
    { const int rc = check_pair("test_ordinal_add", self, other); if (rc) return rc; }
    const bpmf_ordinal *o = self->ordinal.get();
    HIP_TRY(hipSetDevice(c->device));
    if (!t->ord_sum) {
        int rc = t->ord_sum.alloc((size_t)t->nnz * (size_t)o->nlev);
        if (!rc) rc = t->ord_sum.zero_async(c->stream.get());
        if (rc) return rc;
        t->ord_nlev = o->nlev; t->ord_n = 0;
    }
    if (t->ord_nlev != o->nlev) return fail(BPMF_HIP_EINVAL, "test_ordinal_add: the number of levels changed");
    bpmf_launch::OrdinalProbLaunch p{};
    p.tcol = t->d_tcol.get(); p.trow = t->d_trow.get(); p.nnz = t->nnz; p.f = factor_pair(self, other);
    p.g = o->g.get(); p.nlev = o->nlev; p.sum = t->ord_sum.get();
    if (bpmf_launch::ordinal_prob(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, "test_ordinal_add: unsupported K " + std::to_string(c->K));
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "test_ordinal_add: kernel launch failed");
    c->last_sampler_done = nullptr;                                   // (the newest thing on S0 is no longer a sampler)
    ++t->ord_n;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_test_ordinal_get(bpmf_hip_test *t, double *prob_host, int *nlevels, int *nsamples)
{
    if (!t || !prob_host) return fail(BPMF_HIP_EINVAL, "test_ordinal_get: NULL argument");
    if (nsamples) *nsamples = t->ord_n;
    if (nlevels) *nlevels = t->ord_nlev;
    if (!t->ord_sum || t->ord_n == 0) return fail(BPMF_HIP_EINVAL, "test_ordinal_get: nothing added (bpmf_hip_test_ordinal_add)");
    bpmf_hip_ctx *c = t->side->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    const size_t n = (size_t)t->nnz, C = (size_t)t->ord_nlev;
    std::vector<double> sum(n * C);
    if (n > 0) HIP_TRY(hipMemcpy(sum.data(), t->ord_sum.get(), n * C * sizeof(double), hipMemcpyDeviceToHost));
    const double inv = (double)t->ord_n;
    for (size_t q = 0; q < n; ++q)
        for (size_t k = 0; k < C; ++k) prob_host[q * C + k] = sum[k * n + q] / inv;
    return BPMF_HIP_OK;
}
