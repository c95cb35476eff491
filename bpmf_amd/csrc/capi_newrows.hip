// capi_newrows.hip -- dense blocks of posterior predictions from two sample rings (bpmf_hip_predict_block) and the prediction of
// rows unseen in training from their features (bpmf_hip_side_newrows_* / bpmf_hip_newrows_*; kernels in kernels_predblock.h;
// DESIGN.md section 17).  A side with features draws u ~ N(mu_s + beta_s^T f, Lambda_s^-1) in kept sample s, so a new entity with
// features f has the conditional mean e_s = mu_s + beta_s^T f: those are kept in a ring of their own, one slot per kept sample,
// and predicted against the other side's sample ring.  std holds the spread between the samples plus the spread of a cold row's
// factors around e_s, (1/S) sum_s v_s(c)^T Lambda_s^-1 v_s(c); the observation noise 1 / alpha is NOT included.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"
#include "link_sparse.h"

using namespace bpmf_capi;

namespace {

std::string mib(size_t words) { return std::to_string(words * sizeof(double) >> 20) + " MiB"; }

// what both kinds of features share: the refusals, then the ring and the work arrays (zeroed); *out is not attached to `s` yet
int newrows_attach(const char *who, bpmf_hip_side *s, int64_t n_new, int max_samples, bool sparse, std::unique_ptr<bpmf_newrows> *out)
{
    const std::string w(who);
    bpmf_hip_ctx *c = s->ctx;
    int rc = require_single_gpu(who, c, s);
    if (rc) return rc;
    if (!s->link) return fail(BPMF_HIP_EINVAL, w + ": the side has no features (bpmf_hip_side_set_features)");
    if (sparse != (s->link->sparse != nullptr))
        return fail(BPMF_HIP_EINVAL, w + ": the side's features are " + (s->link->sparse ? "sparse" : "dense") + ", the new rows' must be of the same kind");
    if (n_new < 1 || n_new > 0x7FFFFFFF) return fail(BPMF_HIP_EINVAL, w + ": n_new must be >= 1");
    if (max_samples < 1) return fail(BPMF_HIP_EINVAL, w + ": max_samples must be >= 1 (0 frees the new rows)");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    if (s->newrows) {
        if ((rc = bounded_stream_sync(c, c->stream.get(), __func__))) return rc;
        s->newrows.reset();
    }
    auto nr = std::make_unique<bpmf_newrows>();
    nr->n = n_new; nr->nw = s->nrows; nr->D = s->link->D; nr->max = max_samples; nr->kp = (c->Kt + 3) / 4 * 4;
    const size_t ring_words = (size_t)n_new * (size_t)max_samples * (size_t)nr->kp, y_words = (size_t)nr->nw * (size_t)nr->kp;
    if (nr->ring.alloc(ring_words) || nr->w.alloc((size_t)nr->nw) || nr->y.alloc(y_words) || nr->rinv.alloc((size_t)c->Kt * c->Kt) ||
        nr->mu.alloc((size_t)c->K))
        return fail(BPMF_HIP_ENOMEM, w + ": " + std::to_string(max_samples) + " samples of " + std::to_string((long long)n_new) + " new rows x " +
                    std::to_string(nr->kp) + " doubles (" + mib(ring_words) + ") and " + std::to_string((long long)nr->nw) + " x " +
                    std::to_string(nr->kp) + " doubles of work (" + mib(y_words) + ") do not fit in device memory");
    if ((rc = nr->ring.zero_async(c->stream.get())) || (rc = nr->w.zero_async(c->stream.get()))) return rc;
    if ((rc = nr->stage.alloc(2 * ((size_t)c->Kt * c->Kt + c->Kt)))) return rc;
    for (Event &e : nr->staged) { const int re = e.create(hipEventDisableTiming); if (re) return re; }
    *out = std::move(nr);
    return 0;
}

int newrows_free(bpmf_hip_side *s)
{
    bpmf_hip_ctx *c = s->ctx;
    if (!s->newrows) return BPMF_HIP_OK;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    { const int rc = bounded_stream_sync(c, c->stream.get(), __func__); if (rc) return rc; }
    s->newrows.reset();
    return BPMF_HIP_OK;
}

}  // namespace

namespace bpmf_capi {

// mean / std (nq x nc each) of queries [q_from, q_to) against candidates [c_from, c_to) of two rings of S samples; waits.
// device_out: mean_out / std_out are device memory of the context's device and written in place, else host arrays
int predict_rings(const char *who, bpmf_hip_ctx *c, const bpmf_launch::RingPair &r, int64_t nqcols, int64_t nccols, const double *w, double mean_rating,
                  int64_t q_from, int64_t q_to, int64_t c_from, int64_t c_to, double *mean_out, double *std_out, bool device_out)
{
    const std::string ws(who);
    { const int rc = refuse_range(who, "query", q_from, q_to, nqcols); if (rc) return rc; }
    { const int rc = refuse_range(who, "candidate", c_from, c_to, nccols); if (rc) return rc; }
    const int64_t nq = q_to - q_from, nc = c_to - c_from;
    if (nq == 0 || nc == 0) return BPMF_HIP_OK;
    if (!mean_out || !std_out) return fail(BPMF_HIP_EINVAL, ws + ": NULL output");
    const size_t cells = (size_t)nq * (size_t)nc;
    const bool in_place = device_out;
    if (in_place) {
        for (const void *p : {(const void *)mean_out, (const void *)std_out}) {
            hipPointerAttribute_t at;
            if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return fail(BPMF_HIP_EINVAL, ws + ": the outputs must be device memory"); }
            if (at.type != hipMemoryTypeDevice || at.device != c->device)
                return fail(BPMF_HIP_EINVAL, ws + ": the outputs must be device memory of the context's device");
        }
    }
    DevBuf<double> out;
    if (!in_place && out.alloc(2 * cells))
        return fail(BPMF_HIP_ENOMEM, ws + ": a block of " + std::to_string((long long)nq) + " x " + std::to_string((long long)nc) + " means and deviations (" +
                    mib(2 * cells) + ") does not fit in device memory: predict in smaller ranges");
    bpmf_launch::PredBlockLaunch p{};
    p.r = r; p.mean_rating = mean_rating;
    p.q_from = q_from; p.nq = nq; p.c_from = c_from; p.nc = nc; p.w = w;
    p.mean = in_place ? mean_out : out.get(); p.std = in_place ? std_out : out.get() + cells;
    if (bpmf_launch::predict_block(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, ws + ": unsupported shape of the block");
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, ws + ": kernel launch failed");
    { const int rc = bounded_stream_sync(c, c->stream.get(), who); if (rc) return rc; }
    return in_place ? BPMF_HIP_OK : copy_back(ws, {{mean_out, out.get(), cells}, {std_out, out.get() + cells, cells}});
}

}  // namespace bpmf_capi

namespace {

// the new rows of `side` against the sample ring of `cand`: the checks both consumers share
int newrows_pair(const char *who, bpmf_hip_side *side, bpmf_hip_side *cand)
{
    const std::string w(who);
    if (!side || !cand) return fail(BPMF_HIP_EINVAL, w + ": NULL side");
    if (side->ctx != cand->ctx) return fail(BPMF_HIP_EINVAL, w + ": the two sides belong to different contexts");
    bpmf_hip_ctx *c = side->ctx;
    int rc = require_single_gpu(who, c, side, cand);
    if (rc) return rc;
    if (!side->newrows) return fail(BPMF_HIP_EINVAL, w + ": the side has no new rows (bpmf_hip_side_newrows_set)");
    if (cand->ncols != side->nrows) return fail(BPMF_HIP_EINVAL, w + ": the candidate side has the wrong number of columns");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(side)) || (rc = settle_async(cand))) return rc;
    if (!cand->ring) return fail(BPMF_HIP_EINVAL, w + ": no sample ring on the candidate side (bpmf_hip_side_samples_reserve)");
    { const int rb = refuse(w.c_str(), cand, {Not::bias}); if (rb) return rb; }      // (its ring has bias rows the new rows have not)
    const int S = side->newrows->count;
    if (S < 1 || cand->ring->count != S)
        return fail(BPMF_HIP_EINVAL, w + ": the new rows and the candidate side must hold the same number (>= 1) of samples: " + std::to_string(S) +
                    " and " + std::to_string(cand->ring->count));
    return 0;
}

}  // namespace

extern "C" int bpmf_hip_side_newrows_set(bpmf_hip_side *s, int64_t n_new, const double *F_host, int max_samples)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_newrows_set: NULL");
    if (max_samples == 0) return newrows_free(s);
    if (!F_host) return fail(BPMF_HIP_EINVAL, "side_newrows_set: NULL argument");
    std::unique_ptr<bpmf_newrows> nr;
    if (s->link && !s->link->sparse && n_new >= 1) {
        const size_t nD = (size_t)n_new * (size_t)s->link->D;
        for (size_t q = 0; q < nD; ++q)
            if (!std::isfinite(F_host[q])) return fail(BPMF_HIP_EINVAL, "side_newrows_set: feature " + std::to_string(q) + " is not finite");
    }
    int rc = newrows_attach("side_newrows_set", s, n_new, max_samples, false, &nr);
    if (rc) return rc;
    const size_t nD = (size_t)n_new * (size_t)nr->D;
    if (nr->F.alloc(nD)) return fail(BPMF_HIP_ENOMEM, "side_newrows_set: " + std::to_string((long long)n_new) + " x " + std::to_string(nr->D) + " features (" + mib(nD) + ") do not fit in device memory");
    HIP_TRY(hipMemcpy(nr->F.get(), F_host, nD * sizeof(double), hipMemcpyHostToDevice));
    s->newrows = std::move(nr);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_newrows_set_sparse(bpmf_hip_side *s, int64_t n_new, const int64_t *rowptr, const int32_t *colidx, const double *vals,
                                                int max_samples)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_newrows_set_sparse: NULL");
    if (max_samples == 0) return newrows_free(s);
    if (!rowptr) return fail(BPMF_HIP_EINVAL, "side_newrows_set_sparse: NULL argument");
    int rc;
    if (s->link && s->link->sparse && n_new >= 1 && (rc = link_check_csr("side_newrows_set_sparse", n_new, s->link->D, rowptr, colidx, vals))) return rc;
    std::unique_ptr<bpmf_newrows> nr;
    if ((rc = newrows_attach("side_newrows_set_sparse", s, n_new, max_samples, true, &nr))) return rc;
    static const int32_t none = 0;
    nr->sp = std::make_unique<bpmf_launch::SpMat>();
    if ((rc = bpmf_launch::sp_upload(*nr->sp, n_new, rowptr, colidx ? colidx : &none, vals, s->ctx->Kt))) return rc;
    s->newrows = std::move(nr);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_newrows_count(const bpmf_hip_side *s) { return s && s->newrows ? s->newrows->count : 0; }

extern "C" int bpmf_hip_side_newrows_add(bpmf_hip_side *s, bpmf_hip_side *other)
{
    if (!s || !other) return fail(BPMF_HIP_EINVAL, "side_newrows_add: NULL argument");
    if (other->ctx != s->ctx) return fail(BPMF_HIP_EINVAL, "side_newrows_add: sides belong to different contexts");
    bpmf_hip_ctx *c = s->ctx;
    int rc = require_single_gpu("side_newrows_add", c, s, other);
    if (rc) return rc;
    bpmf_newrows *nr = s->newrows.get();
    if (!nr) return fail(BPMF_HIP_EINVAL, "side_newrows_add: the side has no new rows (bpmf_hip_side_newrows_set)");
    if (!s->link) return fail(BPMF_HIP_EINVAL, "side_newrows_add: the side has no features (bpmf_hip_side_set_features)");
    if (other->ncols != s->nrows) return fail(BPMF_HIP_EINVAL, "side_newrows_add: other side has the wrong number of columns");
    if (nr->count >= nr->max) return fail(BPMF_HIP_EINVAL, "side_newrows_add: the ring is full (" + std::to_string(nr->max) + " samples)");
    const int K = c->K, Kt = c->Kt, kp = nr->kp;
    if ((int)s->hp_mu.size() != Kt || (int)s->hp_LambdaU.size() != Kt * Kt)
        return fail(BPMF_HIP_EINVAL, "side_newrows_add: the side has no hyper-parameters yet (after a bpmf_hip_link_sample)");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s)) || (rc = settle_async(other))) return rc;
    hipStream_t st = c->stream.get();
    const bpmf_link *L = s->link.get();
    const int slot = nr->count;
    const int64_t stride = ring_view(nr).stride;
    // R^-1 (upper triangular, row-major) of Lambda = R^T R, R = LambdaU (upper, column-major): K^3 on the host, into one of two
    // pinned halves (R^-1 | mu) taken in turn; the event of a half says that the copies which read it two calls ago are done
    const std::vector<double> &LU = s->hp_LambdaU;
    const int half = slot & 1;
    if (slot >= 2) HIP_TRY(hipEventSynchronize(nr->staged[half].get()));
    double *Rinv = nr->stage.host() + (size_t)half * ((size_t)Kt * Kt + Kt), *mu = Rinv + (size_t)Kt * Kt;
    std::fill(Rinv, Rinv + (size_t)Kt * Kt, 0.0);
    for (int col = 0; col < Kt; ++col)
        for (int i = col; i >= 0; --i) {
            double v = i == col ? 1.0 : 0.0;
            for (int j = i + 1; j <= col; ++j) v -= LU[(size_t)j * Kt + i] * Rinv[(size_t)j * Kt + col];
            Rinv[(size_t)i * Kt + col] = v / LU[(size_t)i * Kt + i];
        }
    for (int q = 0; q < Kt * Kt; ++q)
        if (!std::isfinite(Rinv[q])) return fail(BPMF_HIP_ENUM, "side_newrows_add: Lambda of the side is singular");
    memcpy(mu, s->hp_mu.data(), sizeof(double) * Kt);
    HIP_TRY(hipMemcpyAsync(nr->mu.get(), mu, sizeof(double) * Kt, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(nr->rinv.get(), Rinv, sizeof(double) * Kt * Kt, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(nr->staged[half].get(), st));
    // E[:, slot, :] = F_new beta (pad rows zero) + 1 mu^T
    double *E = nr->ring.get() + (size_t)slot * kp;
    if (nr->sp) {
        if (bpmf_launch::sp_product(*nr->sp, L->beta.get(), K, Kt, kp, E, stride, 0.0, nullptr, 0, st))
            return fail(BPMF_HIP_EINVAL, "side_newrows_add: unsupported shape of the sparse product");
        HIP_TRY(hipGetLastError());
    } else if ((rc = link_nn_product(nr->F.get(), nr->D, L->beta.get(), K, nr->n, nr->D, Kt, E, stride, kp, st)))
        return rc;
    bpmf_launch::ring_add_mu(nr->ring.get(), stride, slot, kp, Kt, nr->n, nr->mu.get(), st);
    // w[c] += |R^-T v(c)|^2 on the other side's current factors: Y = V R^-1, then the squares of its rows in a fixed order
    if ((rc = link_nn_product(other->d_items, K, nr->rinv.get(), Kt, nr->nw, Kt, Kt, nr->y.get(), kp, kp, st))) return rc;
    bpmf_launch::rowsq_add(nr->y.get(), kp, Kt, nr->nw, nr->w.get(), st);
    HIP_TRY(hipGetLastError());
    c->last_sampler_done = nullptr;
    ++nr->count;
    return BPMF_HIP_OK;
}

// the S held samples of every new row as the ring stores them (n x S x kp, pad components included), in one copy; waits
static int newrows_ring_to_host(const char *who, bpmf_hip_side *s, std::vector<double> *out)
{
    const std::string w(who);
    if (!s) return fail(BPMF_HIP_EINVAL, w + ": NULL");
    const bpmf_newrows *nr = s->newrows.get();
    if (!nr) return fail(BPMF_HIP_EINVAL, w + ": the side has no new rows (bpmf_hip_side_newrows_set)");
    if (nr->count < 1) return fail(BPMF_HIP_EINVAL, w + ": nothing added (bpmf_hip_side_newrows_add)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), who); if (rs_) return rs_; }
    if (!out) return BPMF_HIP_OK;
    const size_t kp = (size_t)nr->kp, S = (size_t)nr->count;
    out->resize((size_t)nr->n * S * kp);
    HIP_TRY(hipMemcpy2D(out->data(), S * kp * sizeof(double), nr->ring.get(), (size_t)ring_view(nr).stride * sizeof(double), S * kp * sizeof(double),
                        (size_t)nr->n, hipMemcpyDeviceToHost));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_newrows_get(bpmf_hip_side *s, double *E_host, double *w_host)
{
    std::vector<double> ring;
    { const int rc = newrows_ring_to_host("side_newrows_get", s, E_host ? &ring : nullptr); if (rc) return rc; }
    const bpmf_newrows *nr = s->newrows.get();
    const size_t Kt = (size_t)s->ctx->Kt, kp = (size_t)nr->kp, rows = (size_t)nr->n * (size_t)nr->count;
    if (E_host)
        for (size_t r = 0; r < rows; ++r) memcpy(E_host + r * Kt, ring.data() + r * kp, Kt * sizeof(double));
    if (w_host && nr->nw > 0) {
        HIP_TRY(hipMemcpy(w_host, nr->w.get(), (size_t)nr->nw * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t q = 0; q < nr->nw; ++q) w_host[q] /= (double)nr->count;
    }
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_newrows_get_padded(bpmf_hip_side *s, double *E_host)
{
    if (!E_host) return fail(BPMF_HIP_EINVAL, "side_newrows_get_padded: NULL output");
    std::vector<double> ring;
    { const int rc = newrows_ring_to_host("side_newrows_get_padded", s, &ring); if (rc) return rc; }
    memcpy(E_host, ring.data(), ring.size() * sizeof(double));
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_newrows_predict(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to, int64_t c_from,
                                        int64_t c_to, double *mean_out, double *std_out)
{
    { const int rc = newrows_pair("newrows_predict", side, cand); if (rc) return rc; }
    const bpmf_newrows *nr = side->newrows.get();
    return predict_rings("newrows_predict", side->ctx, ring_pair(nr, cand->ring.get()), nr->n, cand->ncols, nr->w.get(), mean_rating, q_from, q_to, c_from, c_to, mean_out, std_out);
}

static int predict_block_of(const char *who, bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to, int64_t c_from,
                            int64_t c_to, double *mean_out, double *std_out, bool device_out)
{
    int rc;
    bpmf_launch::RingPair r;
    if ((rc = pair_check_sides(who, query, cand, true)) || (rc = pair_open_rings(who, query, cand, &r))) return rc;
    return predict_rings(who, query->ctx, r, query->ncols, cand->ncols, nullptr, mean_rating, q_from, q_to, c_from, c_to, mean_out, std_out, device_out);
}

extern "C" int bpmf_hip_predict_block(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to, int64_t c_from,
                                      int64_t c_to, double *mean_out, double *std_out)
{
    return predict_block_of("predict_block", query, cand, mean_rating, q_from, q_to, c_from, c_to, mean_out, std_out, false);
}

extern "C" int bpmf_hip_predict_block_device(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to,
                                             int64_t c_from, int64_t c_to, double *mean_dev, double *std_dev)
{
    return predict_block_of("predict_block_device", query, cand, mean_rating, q_from, q_to, c_from, c_to, mean_dev, std_dev, true);
}

extern "C" int bpmf_hip_newrows_topn(bpmf_hip_side *side, bpmf_hip_side *cand, double mean_rating, int n, int new_are_queries, int32_t *idx_out,
                                     double *mean_out, double *std_out)
{
    { const int rc = newrows_pair("newrows_topn", side, cand); if (rc) return rc; }
    { const int rc = refuse_topn_n("newrows_topn", n); if (rc) return rc; }
    if (!idx_out || !mean_out || !std_out) return fail(BPMF_HIP_EINVAL, "newrows_topn: NULL output");
    bpmf_hip_ctx *c = side->ctx;
    const bpmf_newrows *nr = side->newrows.get();
    const bpmf_ring *cr = cand->ring.get();
    const int S = nr->count;
    const int64_t nq = new_are_queries ? nr->n : cand->ncols, nc = new_are_queries ? cand->ncols : nr->n;
    if (nq == 0) return BPMF_HIP_OK;
    int rc = topn_rings(c, new_are_queries ? ring_pair(nr, cr) : ring_pair(cr, nr), mean_rating, n, 0, nq, nc, nullptr, nullptr, idx_out, mean_out, std_out);
    if (rc) return rc;
    // the total deviation: the spread between the samples (k_topn_std) and w / S of the pair's in-matrix column, joined on the host
    std::vector<double> w((size_t)std::max<int64_t>(nr->nw, 1));
    if (nr->nw > 0) HIP_TRY(hipMemcpy(w.data(), nr->w.get(), (size_t)nr->nw * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < nq; ++q)
        for (int r = 0; r < n; ++r) {
            const size_t at = (size_t)q * n + r;
            if (idx_out[at] < 0) continue;
            const double wc = w[(size_t)(new_are_queries ? idx_out[at] : q)] / (double)S;
            std_out[at] = std::sqrt(std_out[at] * std_out[at] + wc);
        }
    return BPMF_HIP_OK;
}
