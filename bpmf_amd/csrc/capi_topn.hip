// capi_topn.hip -- sample rings of the sides, the posterior top-N ranking (bpmf_hip_topn; kernels in kernels_topn.h) and the ranks of
// held-out candidates (bpmf_hip_rank_eval; kernels in kernels_rank.h)
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

static int ring_kp(const bpmf_hip_ctx *c) { return (c->Kt + 3) / 4 * 4; }

extern "C" int bpmf_hip_side_samples_reserve(bpmf_hip_side *s, int max_samples)
{
    if (!s || max_samples < 0) return fail(BPMF_HIP_EINVAL, "samples_reserve: bad argument");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    if (s->ring) {
        { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
        s->ring.reset();
    }
    if (max_samples == 0) return BPMF_HIP_OK;
    // a side with bias terms keeps two more rows per sample (capi_bias.hip); the ring kernels serve at most 128 rows
    if (s->bias && c->Kt > 126)
        return fail(BPMF_HIP_EINVAL, "samples_reserve: num_latent " + std::to_string(c->Kt) + " > 126 leaves no room for the two bias rows of a sample");
    auto ring = std::make_unique<bpmf_ring>();
    ring->max = max_samples; ring->kp = s->bias ? (c->Kt + 2 + 3) / 4 * 4 : ring_kp(c);
    const size_t words = (size_t)s->ncols * (size_t)max_samples * (size_t)ring->kp;
    if (ring->samples.alloc(words))
        return fail(BPMF_HIP_ENOMEM, "samples_reserve: " + std::to_string(max_samples) + " samples of " + std::to_string((long long)s->ncols) +
                    " columns x " + std::to_string(ring->kp) + " doubles (" + std::to_string(words * sizeof(double) >> 20) + " MiB) do not fit in device memory");
    { const int rc = ring->samples.zero_async(c->stream.get()); if (rc) return rc; }
    s->ring = std::move(ring);
    return BPMF_HIP_OK;
}

// the current factors into the next slot, ordered like bpmf_hip_side_aggr_add (behind the side's samplers, on its copy)
extern "C" int bpmf_hip_side_samples_add(bpmf_hip_side *s)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "samples_add: NULL");
    bpmf_ring *ring = s->ring.get();
    if (!ring) return fail(BPMF_HIP_EINVAL, "samples_add: no sample ring (bpmf_hip_side_samples_reserve)");
    if (ring->count >= ring->max) return fail(BPMF_HIP_EINVAL, "samples_add: the ring is full (" + std::to_string(ring->max) + " samples)");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    const int64_t stride = ring_view(ring).stride;
    bpmf_launch::samples_add(s->d_items, c->dtype == BPMF_HIP_F32, c->K, c->Kt, ring->kp, s->ncols, ring->samples.get(), stride, ring->count, c->stream.get());
    if (s->bias)                                                      // behind the factor rows: (b, 1) or (1, b), by the side's role
        bpmf_launch::samples_add_bias(s->bias->b.get(), s->ncols, s->bias->role, c->Kt, ring->samples.get(), stride, ring->kp, ring->count, c->stream.get());
    HIP_TRY(hipGetLastError());
    c->last_sampler_done = nullptr;
    ++ring->count;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_samples_count(const bpmf_hip_side *s) { return s && s->ring ? s->ring->count : 0; }

// the rated candidates of every column of the side, sorted, on the host: read back from the device ratings
static int sorted_rows(bpmf_hip_side *s, std::vector<int32_t> &rows)
{
    if (s->from != 0 || s->to != s->ncols)
        return fail(BPMF_HIP_EINVAL, "topn: exclude_rated needs a query side that holds all its columns (this rank has " +
                    std::to_string((long long)s->from) + " .. " + std::to_string((long long)s->to) + ")");
    bpmf_hip_ctx *c = s->ctx;
    { const int rs_ = bounded_stream_sync(c, c->stream.get(), __func__); if (rs_) return rs_; }
    const std::vector<int64_t> &cp = s->h_colptr;
    rows.assign((size_t)std::max<int64_t>(s->nnz, 1), 0);
    if (s->nnz > 0) HIP_TRY(hipMemcpy(rows.data(), s->d_rowidx, (size_t)s->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < s->ncols; ++q) std::sort(rows.begin() + cp[(size_t)q], rows.begin() + cp[(size_t)q + 1]);
    return 0;
}

// the exclusion lists of the side's ring, built on the first ranking that excludes the rated candidates.  host_rows: also wanted on the host
static int build_exclusion(bpmf_hip_side *s, std::vector<int32_t> *host_rows = nullptr)
{
    if (s->ring->ex_ptr) return host_rows ? sorted_rows(s, *host_rows) : 0;
    std::vector<int32_t> local;
    std::vector<int32_t> &rows = host_rows ? *host_rows : local;
    int rc = sorted_rows(s, rows);
    if (rc) return rc;
    const std::vector<int64_t> &cp = s->h_colptr;
    DevBuf<int64_t> ptr; DevBuf<int32_t> sorted;
    if ((rc = ptr.upload(cp.data(), cp.size())) || (rc = sorted.upload(rows.data(), rows.size()))) return rc;
    s->ring->ex_ptr = std::move(ptr); s->ring->ex_rows = std::move(sorted);
    return 0;
}

namespace bpmf_capi {

// candidates split over workgroups when the query blocks alone do not fill the device (a split is a multiple of 64 candidates)
void topn_splits(const bpmf_hip_ctx *c, int64_t nq, int64_t nc, int64_t *nsplit_out, int64_t *cspan_out)
{
    const int64_t nqb = (nq + 63) / 64;
    int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>((2 * (int64_t)c->num_cu + nqb - 1) / nqb, (nc + 255) / 256));
    const int64_t cspan = ((nc + nsplit - 1) / nsplit + 63) / 64 * 64;
    nsplit = (nc + cspan - 1) / cspan;
    *nsplit_out = nsplit; *cspan_out = cspan;
}

static int ring_pair_check(const std::string &who, const bpmf_hip_side *q, const bpmf_hip_side *c)
{
    if (q->ring->kp != c->ring->kp)
        return fail(BPMF_HIP_EINVAL, who + ": the two sample rings hold " + std::to_string(q->ring->kp) + " and " + std::to_string(c->ring->kp) +
                                     " rows per sample (bias terms on one side only?)");
    if ((bool)q->bias != (bool)c->bias) return fail(BPMF_HIP_EINVAL, who + ": both sides of a pair carry bias terms or neither does (bpmf_hip_side_set_bias)");
    if (q->bias && q->bias->role == c->bias->role)
        return fail(BPMF_HIP_EINVAL, who + ": the two sides have the same bias role " + std::to_string(q->bias->role) + " (bpmf_hip_side_set_bias: 0 and 1)");
    return 0;
}

int pair_check_sides(const std::string &who, const bpmf_hip_side *query, const bpmf_hip_side *cand, bool single_gpu)
{
    if (!query || !cand) return fail(BPMF_HIP_EINVAL, who + ": NULL side");
    if (query->ctx != cand->ctx) return fail(BPMF_HIP_EINVAL, who + ": the two sides belong to different contexts");
    return single_gpu ? require_single_gpu(who.c_str(), query->ctx, query, cand) : 0;
}

// with bias rows (capi_bias.hip) both sides carry them, in opposite roles -- else the product is not mean + b + c + u . v
int pair_open_rings(const std::string &who, bpmf_hip_side *query, bpmf_hip_side *cand, bpmf_launch::RingPair *out)
{
    HIP_TRY(hipSetDevice(query->ctx->device));
    { const int rc = settle_async(query); if (rc) return rc; }        // every half-iteration in flight on both sides (as bpmf_hip_sys_state)
    { const int rc = settle_async(cand); if (rc) return rc; }
    if (!query->ring || !cand->ring) return fail(BPMF_HIP_EINVAL, who + ": no sample ring on both sides (bpmf_hip_side_samples_reserve)");
    { const int rb = ring_pair_check(who, query, cand); if (rb) return rb; }
    *out = ring_pair(query->ring.get(), cand->ring.get());
    if (out->S < 1 || cand->ring->count != out->S)
        return fail(BPMF_HIP_EINVAL, who + ": both sides must hold the same number (>= 1) of samples: " + std::to_string(out->S) + " and " +
                    std::to_string(cand->ring->count));
    return 0;
}

int refuse_topn_n(const char *who, int n)
{
    if (n >= 1 && n <= bpmf_launch::topn_max_n()) return 0;
    return fail(BPMF_HIP_EINVAL, std::string(who) + ": n = " + std::to_string(n) + " (1 .. " + std::to_string(bpmf_launch::topn_max_n()) + ")");
}

int refuse_range(const char *who, const char *what, int64_t from, int64_t to, int64_t ncols)
{
    if (from >= 0 && to >= from && to <= ncols) return 0;
    return fail(BPMF_HIP_EINVAL, std::string(who) + ": " + what + " range out of bounds");
}

int copy_back(const std::string &who, std::initializer_list<CopyBack> list)
{
    for (const CopyBack &cb : list)
        if (cb.dst && cb.bytes && hipMemcpy(cb.dst, cb.src, cb.bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(BPMF_HIP_ENODEV, who + ": copying the results back failed");
    return 0;
}

int last_ms(const char *who, const bpmf_hip_side *s, const Timed *t, float *ms, const char *none_msg)
{
    if (!s || !ms) return fail(BPMF_HIP_EINVAL, std::string(who) + ": NULL argument");
    if (!t || t->ms < 0.f) return fail(BPMF_HIP_EINVAL, std::string(who) + ": " + none_msg);
    *ms = t->ms;
    return BPMF_HIP_OK;
}

int TopnLists::alloc(const char *who, int64_t nsplit_, int64_t nq, int n, bool scored_)
{
    pn = (size_t)nq * (size_t)n; nsplit = (size_t)nsplit_; scored = scored_;
    if (part.alloc((scored ? 3 : 1) * nsplit * pn) || pidx.alloc(nsplit * pn) || out.alloc((scored ? 3 : 2) * pn) || oidx.alloc(pn))
        return fail(BPMF_HIP_ENOMEM, std::string(who) + ": device allocation of the result lists failed");
    return 0;
}

int TopnLists::read_back(const char *who, int32_t *idx, double *score, double *mean, double *std) const
{
    return copy_back(who, {{score, out_score(), pn}, {mean, out_mean(), pn}, {std, out_std(), pn}, {idx, out_idx(), pn}});
}

int topn_rings(bpmf_hip_ctx *c, const bpmf_launch::RingPair &r, double mean_rating, int n, int64_t q_from, int64_t nq, int64_t nc,
               const int64_t *ex_ptr, const int32_t *ex_rows, int32_t *idx_out, double *mean_out, double *std_out)
{
    int64_t nsplit, cspan;
    topn_splits(c, nq, nc, &nsplit, &cspan);
    TopnLists l;
    { const int rc = l.alloc("topn", nsplit, nq, n, false); if (rc) return rc; }
    bpmf_launch::TopnLaunch p{};
    p.r = r; p.n = n; p.mean_rating = mean_rating;
    p.q_from = q_from; p.nq = nq; p.nc = nc; p.cspan = cspan; p.nsplit = (int)nsplit;
    p.ex_ptr = ex_ptr; p.ex_rows = ex_rows;
    p.part_mean = l.part_mean(); p.part_idx = l.part_idx();
    p.out_mean = l.out_mean(); p.out_std = l.out_std(); p.out_idx = l.out_idx();
    bpmf_launch::topn(p, c->stream.get());
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "topn: kernel launch failed");
    { const int rc = bounded_stream_sync(c, c->stream.get(), __func__); if (rc) return rc; }
    return l.read_back("topn", idx_out, nullptr, mean_out, std_out);
}

}  // namespace bpmf_capi

// what bpmf_hip_topn, bpmf_hip_topn_scored and bpmf_hip_rank_eval do between their own argument checks and their launches: the rings,
// then exclude_rated against the shapes of the sides (a shard is served: only exclude_rated is refused on one, by sorted_rows)
static int ranking_open(const char *who, bpmf_hip_side *query, bpmf_hip_side *cand, int exclude_rated, bpmf_launch::RingPair *r)
{
    { const int rc = pair_open_rings(who, query, cand, r); if (rc) return rc; }
    if (exclude_rated && query->nrows != cand->ncols)
        return fail(BPMF_HIP_EINVAL, std::string(who) + ": exclude_rated needs the query side's rows to be the candidate side's columns");
    return 0;
}

extern "C" int bpmf_hip_topn(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int n, int64_t q_from, int64_t q_to,
                             int exclude_rated, int32_t *idx_out, double *mean_out, double *std_out)
{
    int rc;
    if ((rc = pair_check_sides("topn", query, cand, false)) || (rc = refuse_topn_n("topn", n)) ||
        (rc = refuse_range("topn", "query", q_from, q_to, query->ncols)))
        return rc;
    const int64_t nq = q_to - q_from;
    if (nq > 0 && (!idx_out || !mean_out || !std_out)) return fail(BPMF_HIP_EINVAL, "topn: NULL output");
    bpmf_launch::RingPair r;
    if ((rc = ranking_open("topn", query, cand, exclude_rated, &r))) return rc;
    if (nq == 0) return BPMF_HIP_OK;
    if (exclude_rated && (rc = build_exclusion(query))) return rc;
    const bpmf_ring *qr = query->ring.get();
    return topn_rings(query->ctx, r, mean_rating, n, q_from, nq, cand->ncols, exclude_rated ? qr->ex_ptr.get() : nullptr,
                      exclude_rated ? qr->ex_rows.get() : nullptr, idx_out, mean_out, std_out);
}

extern "C" int bpmf_hip_topn_scored(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int n, int64_t q_from, int64_t q_to,
                                    int exclude_rated, int kind, double param, double sigma, int32_t *idx_out, double *score_out,
                                    double *mean_out, double *std_out)
{
    int rc;
    if ((rc = pair_check_sides("topn_scored", query, cand, false))) return rc;
    if (kind != BPMF_HIP_SCORE_UCB && kind != BPMF_HIP_SCORE_PROB && kind != BPMF_HIP_SCORE_EI)
        return fail(BPMF_HIP_EINVAL, "topn_scored: unknown score kind " + std::to_string(kind) + " (BPMF_HIP_SCORE_UCB, _PROB or _EI)");
    if (!std::isfinite(param))
        return fail(BPMF_HIP_EINVAL, std::string("topn_scored: ") + (kind == BPMF_HIP_SCORE_UCB ? "kappa" : "the threshold") + " is not finite");
    if (kind != BPMF_HIP_SCORE_UCB && !(std::isfinite(sigma) && sigma >= 0.0))
        return fail(BPMF_HIP_EINVAL, "topn_scored: sigma must be finite and >= 0");
    if ((rc = refuse_topn_n("topn_scored", n)) || (rc = refuse_range("topn_scored", "query", q_from, q_to, query->ncols))) return rc;
    const int64_t nq = q_to - q_from;
    if (nq > 0 && (!idx_out || !score_out || !mean_out || !std_out)) return fail(BPMF_HIP_EINVAL, "topn_scored: NULL output");
    bpmf_launch::TopnScoredLaunch p{};
    if ((rc = ranking_open("topn_scored", query, cand, exclude_rated, &p.r))) return rc;
    if (nq == 0) return BPMF_HIP_OK;
    if (exclude_rated && (rc = build_exclusion(query))) return rc;

    bpmf_hip_ctx *c = query->ctx;
    const bpmf_ring *qr = query->ring.get();
    const int64_t nc = cand->ncols;
    int64_t nsplit, cspan;
    topn_splits(c, nq, nc, &nsplit, &cspan);
    TopnLists l;
    if ((rc = l.alloc("topn_scored", nsplit, nq, n, true))) return rc;
    p.n = n; p.mean_rating = mean_rating;
    p.kind = kind; p.param = param; p.sigma = kind == BPMF_HIP_SCORE_UCB ? 0.0 : sigma;
    p.q_from = q_from; p.nq = nq; p.nc = nc; p.cspan = cspan; p.nsplit = (int)nsplit;
    p.ex_ptr = exclude_rated ? qr->ex_ptr.get() : nullptr; p.ex_rows = exclude_rated ? qr->ex_rows.get() : nullptr;
    p.part_score = l.part_score(); p.part_mean = l.part_mean(); p.part_std = l.part_std(); p.part_idx = l.part_idx();
    p.out_score = l.out_score(); p.out_mean = l.out_mean(); p.out_std = l.out_std(); p.out_idx = l.out_idx();
    const int lrc = bpmf_launch::topn_scored(p, c->stream.get());
    if (lrc == -2) return fail(BPMF_HIP_ENODEV, "topn_scored: the device refused the LDS of lists of " + std::to_string(n));
    if (lrc) return fail(BPMF_HIP_EINVAL, "topn_scored: unsupported shape");
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "topn_scored: kernel launch failed");
    if ((rc = bounded_stream_sync(c, c->stream.get(), __func__))) return rc;
    return l.read_back("topn_scored", idx_out, score_out, mean_out, std_out);
}

// rank of every held-out (query, candidate) among the candidates the query has not rated, by bpmf_hip_topn's score and order
// (kernels_rank.h)
extern "C" int bpmf_hip_rank_eval(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t q_from, int64_t q_to,
                                  int exclude_rated, const int64_t *tptr, const int32_t *tcand, int32_t *rank_out, int32_t *ncand_out)
{
    int rc;
    if ((rc = pair_check_sides("rank_eval", query, cand, false))) return rc;
    if (!std::isfinite(mean_rating)) return fail(BPMF_HIP_EINVAL, "rank_eval: mean_rating is not finite");
    if ((rc = refuse_range("rank_eval", "query", q_from, q_to, query->ncols))) return rc;
    const int64_t nq = q_to - q_from, nc = cand->ncols;
    if (!tptr) return fail(BPMF_HIP_EINVAL, "rank_eval: NULL held-out pointer array");
    if (tptr[0] != 0) return fail(BPMF_HIP_EINVAL, "rank_eval: tptr[0] must be 0");
    for (int64_t q = 0; q < nq; ++q)
        if (tptr[q + 1] < tptr[q]) return fail(BPMF_HIP_EINVAL, "rank_eval: tptr decreases at query " + std::to_string((long long)(q_from + q)));
    const int64_t nt = tptr[nq];
    if (nt > 0 && (!tcand || !rank_out)) return fail(BPMF_HIP_EINVAL, "rank_eval: NULL held-out array");
    if (nq > 0 && !ncand_out) return fail(BPMF_HIP_EINVAL, "rank_eval: NULL output");
    if (nc > std::numeric_limits<int32_t>::max()) return fail(BPMF_HIP_EINVAL, "rank_eval: too many candidates");
    for (int64_t q = 0; q < nq; ++q)
        for (int64_t p = tptr[q]; p < tptr[q + 1]; ++p) {
            if (tcand[p] < 0 || tcand[p] >= nc)
                return fail(BPMF_HIP_EINVAL, "rank_eval: held-out candidate " + std::to_string(tcand[p]) + " of query " +
                            std::to_string((long long)(q_from + q)) + " is out of range");
            if (p > tptr[q] && tcand[p] <= tcand[p - 1])
                return fail(BPMF_HIP_EINVAL, "rank_eval: the held-out candidates of query " + std::to_string((long long)(q_from + q)) +
                            " are not ascending and distinct (" + std::to_string(tcand[p - 1]) + ", " + std::to_string(tcand[p]) + ")");
        }
    bpmf_launch::RankLaunch p{};
    if ((rc = ranking_open("rank_eval", query, cand, exclude_rated, &p.r))) return rc;
    if (nq == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = query->ctx;
    const bpmf_ring *qr = query->ring.get();
    if (exclude_rated) {
        // a held-out entry that is a rated cell would be scored -inf: refused while the lists are on the host
        std::vector<int32_t> rows;
        if ((rc = build_exclusion(query, &rows))) return rc;
        const std::vector<int64_t> &cp = query->h_colptr;
        for (int64_t q = 0; q < nq; ++q) {
            const auto b = rows.begin() + cp[(size_t)(q_from + q)], e = rows.begin() + cp[(size_t)(q_from + q) + 1];
            for (int64_t p = tptr[q]; p < tptr[q + 1]; ++p)
                if (std::binary_search(b, e, tcand[p]))
                    return fail(BPMF_HIP_EINVAL, "rank_eval: the held-out cell (query " + std::to_string((long long)(q_from + q)) + ", candidate " +
                                std::to_string(tcand[p]) + ") is a rated cell of the query side");
        }
    }
    int64_t nsplit, cspan;
    topn_splits(c, nq, nc, &nsplit, &cspan);
    DevBuf<int64_t> d_tptr;
    DevBuf<int32_t> d_tcand, part_cnt, part_ncand, d_rank, d_ncand;
    DevBuf<double> tscore;
    const size_t ntz = (size_t)std::max<int64_t>(nt, 1);
    if ((rc = d_tptr.upload(tptr, (size_t)nq + 1)) || (rc = d_tcand.upload(nt > 0 ? tcand : nullptr, (size_t)nt)) || (rc = tscore.alloc(ntz)) ||
        (rc = part_cnt.alloc((size_t)nsplit * ntz)) || (rc = part_ncand.alloc((size_t)nsplit * (size_t)nq)) || (rc = d_rank.alloc(ntz)) ||
        (rc = d_ncand.alloc((size_t)nq)))
        return rc;
    p.mean_rating = mean_rating;
    p.q_from = q_from; p.nq = nq; p.nc = nc; p.cspan = cspan; p.nsplit = (int)nsplit;
    p.ex_ptr = exclude_rated ? qr->ex_ptr.get() : nullptr; p.ex_rows = exclude_rated ? qr->ex_rows.get() : nullptr;
    p.tptr = d_tptr.get(); p.tcand = d_tcand.get(); p.nt = nt; p.tscore = tscore.get();
    p.part_cnt = part_cnt.get(); p.part_ncand = part_ncand.get(); p.rank = d_rank.get(); p.ncand = d_ncand.get();
    bpmf_launch::rank_eval(p, c->stream.get());
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "rank_eval: kernel launch failed");
    if ((rc = bounded_stream_sync(c, c->stream.get(), __func__))) return rc;
    return copy_back("rank_eval", {{rank_out, d_rank.get(), (size_t)nt}, {ncand_out, d_ncand.get(), (size_t)nq}});
}
