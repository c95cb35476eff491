// capi_foldin.hip -- fold-in: rows that arrive after training with a few ratings and no features get their factors from the kept
// posterior samples (bpmf_hip_side_hyper_* / bpmf_hip_foldin*; kernel in kernels_foldin.h).  Given kept sample s
// of the other side and this side's (alpha_s, mu_s, Lambda_s), the factor of a new row has the conditional the column samplers draw
// from: one Gram, one factorisation and one draw per (row, sample), nothing else of the chain moves.  The draws go into a ring of
// the bpmf_ring layout and are predicted and ranked by the kernels that serve the in-matrix rows (w = NULL: the draw carries the
// row's own uncertainty; the observation noise 1 / alpha is NOT included).
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

namespace {

std::string mib(size_t bytes) { return std::to_string(bytes >> 20) + " MiB"; }

// what a side must be to keep a hyper ring and to be folded into
int foldin_refusals(const char *who, const bpmf_hip_side *side, const bpmf_hip_side *cand)
{
    const std::string w(who);
    const bpmf_hip_ctx *c = side->ctx;
    if (cand && cand->ctx != c) return fail(BPMF_HIP_EINVAL, w + ": the two sides belong to different contexts");
    int rc = require_single_gpu(who, c, side, cand);
    if (rc) return rc;
    if (side->reduce_on || (cand && cand->reduce_on)) return fail(BPMF_HIP_EINVAL, w + ": does not go together with the BPMF_REDUCE formulation (bpmf_hip_sys_set_reduce)");
    if (side->d_prop) return fail(BPMF_HIP_EINVAL, w + ": the side has propagated priors (bpmf_hip_side_set_prop_posterior): a new row has none");
    const auto either_is = [&](Likelihood k) { return likelihood(side) == k || (cand && likelihood(cand) == k); };
    if (either_is(Likelihood::probit))
        return fail(BPMF_HIP_EINVAL, w + ": a probit side cannot be folded into (labels would need a latent iteration of their own)");
    if (either_is(Likelihood::ordinal))
        return fail(BPMF_HIP_EINVAL, w + ": an ordinal side cannot be folded into (levels would need a latent iteration of their own)");
    if (side->link)
        return fail(BPMF_HIP_EINVAL, w + ": the side has features: the prior mean of a new row needs its features (bpmf_hip_side_newrows_set predicts such rows)");
    return 0;
}

int foldin_free_set(bpmf_hip_side *s)
{
    bpmf_foldin *f = s->foldin.get();
    if (!f || !f->ring) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    { const int rc = bounded_stream_sync(c, c->stream.get(), __func__); if (rc) return rc; }
    f->rowptr.reset(); f->colidx.reset(); f->ring.reset();
    f->n = 0; f->S = 0;
    if (f->hmax == 0) s->foldin.reset();
    return BPMF_HIP_OK;
}

// the folded-in rows of `side` against the sample ring of `cand`: the checks both consumers share
int foldin_pair(const char *who, bpmf_hip_side *side, bpmf_hip_side *cand)
{
    const std::string w(who);
    if (!side || !cand) return fail(BPMF_HIP_EINVAL, w + ": NULL side");
    if (side->ctx != cand->ctx) return fail(BPMF_HIP_EINVAL, w + ": the two sides belong to different contexts");
    bpmf_hip_ctx *c = side->ctx;
    int rc = require_single_gpu(who, c, side, cand);
    if (rc) return rc;
    if (!side->foldin || !side->foldin->ring) return fail(BPMF_HIP_EINVAL, w + ": the side has no folded-in rows (bpmf_hip_foldin)");
    if (cand->ncols != side->nrows) return fail(BPMF_HIP_EINVAL, w + ": the candidate side has the wrong number of columns");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(side)) || (rc = settle_async(cand))) return rc;
    if (!cand->ring) return fail(BPMF_HIP_EINVAL, w + ": no sample ring on the candidate side (bpmf_hip_side_samples_reserve)");
    { const int rb = refuse(w.c_str(), cand, {Not::bias}); if (rb) return rb; }      // (its ring has bias rows the folded-in rows have not)
    if (cand->ring->count != side->foldin->S)
        return fail(BPMF_HIP_EINVAL, w + ": the rows were folded in against " + std::to_string(side->foldin->S) + " samples, the candidate side holds " +
                    std::to_string(cand->ring->count));
    return 0;
}

}  // namespace

extern "C" int bpmf_hip_side_hyper_reserve(bpmf_hip_side *s, int max_samples)
{
    if (!s || max_samples < 0) return fail(BPMF_HIP_EINVAL, "side_hyper_reserve: bad argument");
    if (max_samples > 0 && s->implicit) return fail(BPMF_HIP_EINVAL, "side_hyper_reserve: not on an implicit side (fold-in under the implicit model would need G)");
    if (max_samples > 0) { const int rb = refuse("side_hyper_reserve", s, {Not::bias}); if (rb) return rb; }
    if (max_samples == 0) {
        if (s->foldin) {
            bpmf_foldin *f = s->foldin.get();
            f->hmax = f->hcount = 0;
            std::vector<double>().swap(f->alpha); std::vector<double>().swap(f->mu); std::vector<double>().swap(f->lam); std::vector<double>().swap(f->lmu);
            if (!f->ring) s->foldin.reset();
        }
        return BPMF_HIP_OK;
    }
    { const int rc = foldin_refusals("side_hyper_reserve", s, nullptr); if (rc) return rc; }
    const size_t kt = (size_t)s->ctx->Kt, n = (size_t)max_samples;
    if (!s->foldin) s->foldin = std::make_unique<bpmf_foldin>();
    bpmf_foldin *f = s->foldin.get();
    try {
        f->alpha.assign(n, 0.0); f->mu.assign(n * kt, 0.0); f->lam.assign(n * kt * kt, 0.0); f->lmu.assign(n * kt, 0.0);
    } catch (const std::bad_alloc &) {
        f->hmax = f->hcount = 0;
        return fail(BPMF_HIP_ENOMEM, "side_hyper_reserve: " + std::to_string(max_samples) + " samples of " + std::to_string(kt * kt + 2 * kt + 1) +
                    " doubles (" + mib(n * (kt * kt + 2 * kt + 1) * sizeof(double)) + ") do not fit in host memory");
    }
    f->hmax = max_samples; f->hcount = 0;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_hyper_add(bpmf_hip_side *s, double alpha, const double *mu, const double *LambdaF)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_hyper_add: NULL");
    bpmf_foldin *f = s->foldin.get();
    if (!f || f->hmax == 0) return fail(BPMF_HIP_EINVAL, "side_hyper_add: no hyper ring (bpmf_hip_side_hyper_reserve)");
    if (f->hcount >= f->hmax) return fail(BPMF_HIP_EINVAL, "side_hyper_add: the ring is full (" + std::to_string(f->hmax) + " samples)");
    if ((mu == nullptr) != (LambdaF == nullptr)) return fail(BPMF_HIP_EINVAL, "side_hyper_add: mu and LambdaF are given together or not at all");
    if (!(std::isfinite(alpha) && alpha >= 0.0)) return fail(BPMF_HIP_EINVAL, "side_hyper_add: alpha must be finite and >= 0");
    const size_t kt = (size_t)s->ctx->Kt;
    if (!mu) {                                                          // the hyper-parameters the side's newest half-iteration ran with
        HIP_TRY(hipSetDevice(s->ctx->device));
        { const int rc = settle_async(s); if (rc) return rc; }         // (waits for its collection, as bpmf_hip_sys_state)
        if (s->hp_mu.size() != kt || s->hp_LambdaF.size() != kt * kt || s->iter < 0)
            return fail(BPMF_HIP_EINVAL, "side_hyper_add: the side has no hyper-parameters yet (after a bpmf_hip_sys_sample)");
        mu = s->hp_mu.data(); LambdaF = s->hp_LambdaF.data();
    }
    for (size_t q = 0; q < kt; ++q)
        if (!std::isfinite(mu[q])) return fail(BPMF_HIP_EINVAL, "side_hyper_add: mu[" + std::to_string(q) + "] is not finite");
    for (size_t q = 0; q < kt * kt; ++q)
        if (!std::isfinite(LambdaF[q])) return fail(BPMF_HIP_EINVAL, "side_hyper_add: LambdaF[" + std::to_string(q) + "] is not finite");
    const size_t slot = (size_t)f->hcount;
    f->alpha[slot] = alpha;
    memcpy(&f->mu[slot * kt], mu, kt * sizeof(double));
    memcpy(&f->lam[slot * kt * kt], LambdaF, kt * kt * sizeof(double));
    for (size_t r = 0; r < kt; ++r) {                                   // Lambda mu, the prior's share of every right-hand side
        double acc = 0.0;
        for (size_t q = 0; q < kt; ++q) acc += LambdaF[r + q * kt] * mu[q];
        f->lmu[slot * kt + r] = acc;
    }
    ++f->hcount;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_hyper_count(const bpmf_hip_side *s) { return s && s->foldin ? s->foldin->hcount : 0; }

extern "C" int bpmf_hip_side_hyper_get(const bpmf_hip_side *s, double *alpha, double *mu, double *LambdaF)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_hyper_get: NULL");
    const bpmf_foldin *f = s->foldin.get();
    if (!f || f->hcount < 1) return fail(BPMF_HIP_EINVAL, "side_hyper_get: the side holds no hyper-parameters (bpmf_hip_side_hyper_add)");
    const size_t kt = (size_t)s->ctx->Kt, n = (size_t)f->hcount;
    if (alpha) memcpy(alpha, f->alpha.data(), n * sizeof(double));
    if (mu) memcpy(mu, f->mu.data(), n * kt * sizeof(double));
    if (LambdaF) memcpy(LambdaF, f->lam.data(), n * kt * kt * sizeof(double));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_foldin(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int64_t n_new, const int64_t *rowptr,
                               const int32_t *colidx, const double *vals, unsigned tag, int draw)
{
    if (!side) return fail(BPMF_HIP_EINVAL, "foldin: NULL side");
    if (n_new == 0) return foldin_free_set(side);
    if (!cand) return fail(BPMF_HIP_EINVAL, "foldin: NULL side");
    // everything that can be refused is refused on the host, before the device is touched
    { const int rc = foldin_refusals("foldin", side, cand); if (rc) return rc; }
    if (n_new < 1 || n_new > 0x7FFFFFFF) return fail(BPMF_HIP_EINVAL, "foldin: n_new must be >= 1 (0 frees the folded-in rows)");
    if (!rowptr) return fail(BPMF_HIP_EINVAL, "foldin: NULL rowptr");
    if (tag < 1) return fail(BPMF_HIP_EINVAL, "foldin: tag must be >= 1 (0 is the key of the samplers' streams)");
    if (!std::isfinite(mean_rating)) return fail(BPMF_HIP_EINVAL, "foldin: mean_rating is not finite");
    if (cand->ncols != side->nrows) return fail(BPMF_HIP_EINVAL, "foldin: the candidate side has the wrong number of columns");
    if (rowptr[0] != 0) return fail(BPMF_HIP_EINVAL, "foldin: rowptr[0] must be 0");
    for (int64_t i = 0; i < n_new; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(BPMF_HIP_EINVAL, "foldin: rowptr decreases at row " + std::to_string((long long)i));
    const int64_t nnz = rowptr[n_new];
    if (nnz > 0 && (!colidx || !vals)) return fail(BPMF_HIP_EINVAL, "foldin: NULL colidx / vals");
    for (int64_t i = 0; i < n_new; ++i)
        for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            const int64_t j = colidx[p];
            if (j < 0 || j >= cand->ncols)
                return fail(BPMF_HIP_EINVAL, "foldin: row " + std::to_string((long long)i) + " rates column " + std::to_string((long long)j) +
                            ", out of range (the candidate side has " + std::to_string((long long)cand->ncols) + " columns)");
            if (p > rowptr[i] && j <= colidx[p - 1])
                return fail(BPMF_HIP_EINVAL, "foldin: row " + std::to_string((long long)i) + (j == colidx[p - 1] ? " rates column " : " lists column ") +
                            std::to_string((long long)j) + (j == colidx[p - 1] ? " twice" : " out of order (the columns of a row must ascend)"));
            if (!std::isfinite(vals[p]))
                return fail(BPMF_HIP_EINVAL, "foldin: the rating of row " + std::to_string((long long)i) + ", column " + std::to_string((long long)j) + " is not finite");
        }
    bpmf_foldin *f = side->foldin.get();
    const int S = f ? f->hcount : 0;
    if (S < 1) return fail(BPMF_HIP_EINVAL, "foldin: the side holds no hyper-parameters (bpmf_hip_side_hyper_reserve, bpmf_hip_side_hyper_add)");
    if (!cand->ring) return fail(BPMF_HIP_EINVAL, "foldin: no sample ring on the candidate side (bpmf_hip_side_samples_reserve)");
    { const int rb = refuse("foldin", cand, {Not::bias}); if (rb) return rb; }      // (a folded-in row would need a bias of its own)
    if (cand->ring->count != S)
        return fail(BPMF_HIP_EINVAL, "foldin: the side holds the hyper-parameters of " + std::to_string(S) + " samples, the candidate side's ring " +
                    std::to_string(cand->ring->count) + ": they must be the same samples");
    if (n_new * (int64_t)S > 0x7FFFFFFF) return fail(BPMF_HIP_EINVAL, "foldin: n_new x samples exceeds 2^31 - 1: fold in fewer rows per call");

    bpmf_hip_ctx *c = side->ctx;
    const bpmf_ring *cr = cand->ring.get();
    const size_t kt = (size_t)c->Kt;
    const int kp = cr->kp;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = settle_async(side)) || (rc = settle_async(cand))) return rc;
    if (f->ring) {                                                      // an earlier set: nothing on the stream may still read it
        if ((rc = bounded_stream_sync(c, c->stream.get(), __func__))) return rc;
        f->rowptr.reset(); f->colidx.reset(); f->ring.reset(); f->n = 0; f->S = 0;
    }
    const size_t ring_words = (size_t)n_new * (size_t)S * (size_t)kp;
    DevBuf<int64_t> d_ptr; DevBuf<int32_t> d_idx; DevBuf<double> d_vals, d_ring, d_alpha, d_lam, d_lmu;
    if (d_ring.alloc(ring_words))
        return fail(BPMF_HIP_ENOMEM, "foldin: " + std::to_string(S) + " samples of " + std::to_string((long long)n_new) + " new rows x " + std::to_string(kp) +
                    " doubles (" + mib(ring_words * sizeof(double)) + ") do not fit in device memory");
    if (!f->fail && (rc = f->fail.alloc(1))) return rc;
    if ((rc = d_ptr.upload(rowptr, (size_t)n_new + 1)) || (rc = d_idx.upload(colidx, (size_t)nnz)) || (rc = d_vals.upload(vals, (size_t)nnz)) ||
        (rc = d_alpha.upload(f->alpha.data(), (size_t)S)) || (rc = d_lam.upload(f->lam.data(), (size_t)S * kt * kt)) ||
        (rc = d_lmu.upload(f->lmu.data(), (size_t)S * kt)))
        return rc;
    __atomic_store_n(f->fail.host(), ~0ull, __ATOMIC_RELEASE);
    bpmf_launch::FoldinLaunch p{};
    p.rowptr = d_ptr.get(); p.colidx = d_idx.get(); p.vals = d_vals.get(); p.n_new = n_new;
    p.cring = cr->samples.get(); p.cstride = ring_view(cr).stride;
    p.alpha = d_alpha.get(); p.lam = d_lam.get(); p.lmu = d_lmu.get(); p.S = S;
    p.K = c->K; p.kt = c->Kt; p.kp = kp; p.mean_rating = mean_rating; p.tag = tag; p.draw = draw ? 1 : 0;
    p.out = d_ring.get(); p.fail = f->fail.dev();
    if ((rc = f->timed.begin(c->stream.get()))) return rc;
    if (bpmf_launch::foldin(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, "foldin: unsupported shape");
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "foldin: kernel launch failed");
    if ((rc = f->timed.end(c->stream.get()))) return rc;
    c->last_sampler_done = nullptr;
    if ((rc = bounded_stream_sync(c, c->stream.get(), "foldin"))) return rc;
    f->timed.resolve();
    f->rowptr = std::move(d_ptr); f->colidx = std::move(d_idx); f->ring = std::move(d_ring);
    f->n = n_new; f->S = S; f->kp = kp;
    const unsigned long long bad = __atomic_load_n(f->fail.host(), __ATOMIC_ACQUIRE);
    if (bad != ~0ull)
        return fail(BPMF_HIP_ECHOL, "foldin: Cholesky failed for new row " + std::to_string(bad) + " (a pivot of Lambda* is not positive and finite; "
                    "its factors are stored as zeros)");
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_foldin_count(const bpmf_hip_side *s) { return s && s->foldin && s->foldin->ring ? (int)s->foldin->n : 0; }

extern "C" int bpmf_hip_foldin_samples(const bpmf_hip_side *s) { return s && s->foldin && s->foldin->ring ? s->foldin->S : 0; }

extern "C" int bpmf_hip_foldin_get(bpmf_hip_side *s, double *E_host)
{
    if (!s || !E_host) return fail(BPMF_HIP_EINVAL, "foldin_get: NULL argument");
    const bpmf_foldin *f = s->foldin.get();
    if (!f || !f->ring) return fail(BPMF_HIP_EINVAL, "foldin_get: the side has no folded-in rows (bpmf_hip_foldin)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = bounded_stream_sync(c, c->stream.get(), "foldin_get"); if (rc) return rc; }
    const size_t kt = (size_t)c->Kt, kp = (size_t)f->kp, rows = (size_t)f->n * (size_t)f->S;
    HIP_TRY(hipMemcpy2D(E_host, kt * sizeof(double), f->ring.get(), kp * sizeof(double), kt * sizeof(double), rows, hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_foldin_get_padded(bpmf_hip_side *s, double *E_host)
{
    if (!s || !E_host) return fail(BPMF_HIP_EINVAL, "foldin_get_padded: NULL argument");
    const bpmf_foldin *f = s->foldin.get();
    if (!f || !f->ring) return fail(BPMF_HIP_EINVAL, "foldin_get_padded: the side has no folded-in rows (bpmf_hip_foldin)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = bounded_stream_sync(c, c->stream.get(), "foldin_get_padded"); if (rc) return rc; }
    HIP_TRY(hipMemcpy(E_host, f->ring.get(), (size_t)f->n * (size_t)f->S * (size_t)f->kp * sizeof(double), hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_foldin_predict(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to, int64_t c_from,
                                       int64_t c_to, double *mean_out, double *std_out)
{
    { const int rc = foldin_pair("foldin_predict", side, cand); if (rc) return rc; }
    const bpmf_foldin *f = side->foldin.get();
    return predict_rings("foldin_predict", side->ctx, ring_pair(f, cand->ring.get()), f->n, cand->ncols, nullptr, mean_rating, q_from, q_to, c_from,
                         c_to, mean_out, std_out);
}

extern "C" int bpmf_hip_foldin_topn(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int n, int exclude_rated, int32_t *idx_out,
                                    double *mean_out, double *std_out)
{
    { const int rc = foldin_pair("foldin_topn", side, cand); if (rc) return rc; }
    { const int rc = refuse_topn_n("foldin_topn", n); if (rc) return rc; }
    if (!idx_out || !mean_out || !std_out) return fail(BPMF_HIP_EINVAL, "foldin_topn: NULL output");
    const bpmf_foldin *f = side->foldin.get();
    // the rows' own ratings are the exclusion lists: sorted columns of the candidate side per query, the format the ranking takes
    return topn_rings(side->ctx, ring_pair(f, cand->ring.get()), mean_rating, n, 0, f->n, cand->ncols, exclude_rated ? f->rowptr.get() : nullptr,
                      exclude_rated ? f->colidx.get() : nullptr, idx_out, mean_out, std_out);
}

extern "C" int bpmf_hip_foldin_last_ms(const bpmf_hip_side *s, float *ms)
{
    return last_ms("foldin_last_ms", s, s && s->foldin ? &s->foldin->timed : nullptr, ms, "no launch of the side has been timed (bpmf_hip_foldin)");
}

extern "C" int bpmf_hip_foldin_chunk(void) { return bpmf_launch::foldin_chunk(); }
