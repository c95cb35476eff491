// capi_model.hip -- what a saved model needs of the sample rings: their read-back and load (bpmf_hip_side_samples_get / _set) and the
// prediction of a list of cells from them (bpmf_hip_predict_cells; kernels in kernels_predcells.h).  The hyper
// ring needs nothing new: bpmf_hip_side_hyper_get reads it, bpmf_hip_side_hyper_reserve + _add fill it.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

namespace {

// columns of a ring repacked per pass: the staging buffer stays at 64 MiB whatever the ring
int64_t pack_cols(int n, int kt) { return std::max<int64_t>(1, ((int64_t)1 << 23) / ((int64_t)n * kt)); }

}  // namespace

extern "C" int bpmf_hip_side_samples_get(bpmf_hip_side *s, int s_from, int s_to, double *host)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "samples_get: NULL");
    bpmf_ring *ring = s->ring.get();
    if (!ring) return fail(BPMF_HIP_EINVAL, "samples_get: no sample ring (bpmf_hip_side_samples_reserve)");
    { const int rb = refuse("samples_get", s, {Not::bias}); if (rb) return rb; }      // (the packed form has Kt rows per sample: no bias rows)
    if (s_from < 0 || s_to < s_from || s_to > ring->count)
        return fail(BPMF_HIP_EINVAL, "samples_get: samples " + std::to_string(s_from) + " .. " + std::to_string(s_to) + " are out of range (the ring holds " +
                    std::to_string(ring->count) + ")");
    const int n = s_to - s_from;
    if (n == 0 || s->ncols == 0) return BPMF_HIP_OK;
    if (!host) return fail(BPMF_HIP_EINVAL, "samples_get: NULL output");
    bpmf_hip_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    const int kt = c->Kt;
    const int64_t step = pack_cols(n, kt);
    DevBuf<double> packed;
    { const int rc = packed.alloc((size_t)std::min<int64_t>(step, s->ncols) * (size_t)n * (size_t)kt); if (rc) return rc; }
    for (int64_t c0 = 0; c0 < s->ncols; c0 += step) {
        const int64_t nc = std::min<int64_t>(step, s->ncols - c0);
        bpmf_launch::samples_pack(ring->samples.get(), ring_view(ring).stride, ring->kp, kt, c0, nc, s_from, n, packed.get(), c->stream.get());
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "samples_get: kernel launch failed");
        { const int rc = bounded_stream_sync(c, c->stream.get(), "samples_get"); if (rc) return rc; }
        HIP_TRY(hipMemcpy(host + (size_t)c0 * (size_t)n * (size_t)kt, packed.get(), (size_t)nc * (size_t)n * (size_t)kt * sizeof(double), hipMemcpyDeviceToHost));
    }
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_samples_set(bpmf_hip_side *s, int nsamples, const double *host)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "samples_set: NULL");
    bpmf_ring *ring = s->ring.get();
    if (!ring) return fail(BPMF_HIP_EINVAL, "samples_set: no sample ring (bpmf_hip_side_samples_reserve)");
    { const int rb = refuse("samples_set", s, {Not::bias}); if (rb) return rb; }
    if (nsamples < 0 || nsamples > ring->max)
        return fail(BPMF_HIP_EINVAL, "samples_set: " + std::to_string(nsamples) + " samples do not fit the ring (reserved for " + std::to_string(ring->max) + ")");
    if (nsamples > 0 && s->ncols > 0 && !host) return fail(BPMF_HIP_EINVAL, "samples_set: NULL input");
    bpmf_hip_ctx *c = s->ctx;
    const int kt = c->Kt, n = nsamples;
    for (int64_t col = 0; col < s->ncols; ++col)                              // refused on the host, before the device is touched
        for (int sm = 0; sm < n; ++sm) {
            const double *v = host + ((size_t)col * (size_t)n + (size_t)sm) * (size_t)kt;
            for (int k = 0; k < kt; ++k)
                if (!std::isfinite(v[k]))
                    return fail(BPMF_HIP_EINVAL, "samples_set: the value of column " + std::to_string((long long)col) + ", sample " + std::to_string(sm) +
                                ", row " + std::to_string(k) + " is not finite");
        }
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    { const int rc = bounded_stream_sync(c, c->stream.get(), "samples_set"); if (rc) return rc; }      // nothing on the stream may still read the ring
    if (n > 0 && s->ncols > 0) {
        const int64_t step = pack_cols(n, kt);
        DevBuf<double> packed;
        { const int rc = packed.alloc((size_t)std::min<int64_t>(step, s->ncols) * (size_t)n * (size_t)kt); if (rc) return rc; }
        for (int64_t c0 = 0; c0 < s->ncols; c0 += step) {
            const int64_t nc = std::min<int64_t>(step, s->ncols - c0);
            HIP_TRY(hipMemcpy(packed.get(), host + (size_t)c0 * (size_t)n * (size_t)kt, (size_t)nc * (size_t)n * (size_t)kt * sizeof(double), hipMemcpyHostToDevice));
            bpmf_launch::samples_unpack(packed.get(), ring_view(ring).stride, ring->kp, kt, c0, nc, n, ring->samples.get(), c->stream.get());
            if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "samples_set: kernel launch failed");
            { const int rc = bounded_stream_sync(c, c->stream.get(), "samples_set"); if (rc) return rc; }
        }
    }
    ring->count = n;
    return BPMF_HIP_OK;
}

// What the cell lists (here, capi_diag.hip, capi_score.hip) refuse alike, reported as `who`, on the host alone: the sides and the list
int bpmf_capi::cells_check_list(const std::string &who, bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q,
                                const int32_t *cc)
{
    { const int rc = pair_check_sides(who, query, cand, true); if (rc) return rc; }
    if (n < 0 || n > 0x7fffffff) return fail(BPMF_HIP_EINVAL, who + ": n must be 0 .. 2^31 - 1");
    if (!std::isfinite(mean_rating)) return fail(BPMF_HIP_EINVAL, who + ": mean_rating is not finite");
    if (n > 0 && (!q || !cc)) return fail(BPMF_HIP_EINVAL, who + ": NULL cell list");
    const int64_t nq = query->ncols, nc = cand->ncols;
    for (int64_t i = 0; i < n; ++i)                                             // before the device is used
        if (q[i] < 0 || q[i] >= nq || cc[i] < 0 || cc[i] >= nc)
            return fail(BPMF_HIP_EINVAL, who + ": cell " + std::to_string((long long)i) + " (" + std::to_string(q[i]) + ", " + std::to_string(cc[i]) +
                        ") is out of range (" + std::to_string((long long)nq) + " queries x " + std::to_string((long long)nc) + " candidates)");
    return BPMF_HIP_OK;
}

// the list grouped by query (stable counting sort)
CellsSorted bpmf_capi::cells_sort(int64_t nq, int64_t n, const int32_t *q, const int32_t *cc)
{
    std::vector<int64_t> at((size_t)nq + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++at[(size_t)q[i] + 1];
    for (int64_t j = 0; j < nq; ++j) at[(size_t)j + 1] += at[(size_t)j];
    CellsSorted s;
    s.query.resize((size_t)n); s.cand.resize((size_t)n); s.orig.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t p = at[(size_t)q[i]]++;
        s.query[(size_t)p] = q[i]; s.cand[(size_t)p] = cc[i]; s.orig[(size_t)p] = (int32_t)i;
    }
    return s;
}

// every query's run among the sorted cells of a batch cut into the segments a workgroup takes
bpmf_capi::CellsPlan::CellsPlan(const CellsSorted &s, int64_t n_, int64_t step_, int seg) : sorted(s), n(n_), step(step_)
{
    for (int64_t b0 = 0; b0 < n; b0 += step) {
        first.push_back(seg_q.size());
        const int64_t b1 = std::min<int64_t>(n, b0 + step);
        for (int64_t b = b0; b < b1;) {
            int64_t e = b + 1;
            while (e < b1 && e - b < seg && s.query[(size_t)e] == s.query[(size_t)b]) ++e;
            seg_q.push_back(s.query[(size_t)b]); seg_beg.push_back((int32_t)b); seg_cnt.push_back((int32_t)(e - b));
            b = e;
        }
    }
    first.push_back(seg_q.size());
}

int bpmf_capi::CellsPlan::upload()
{
    int rc;
    if ((rc = d_segq.upload(seg_q.data(), seg_q.size())) || (rc = d_segb.upload(seg_beg.data(), seg_beg.size())) ||
        (rc = d_segc.upload(seg_cnt.data(), seg_cnt.size())) || (rc = d_cand.upload(sorted.cand.data(), sorted.cand.size())) ||
        (rc = d_orig.upload(sorted.orig.data(), sorted.orig.size())))
        return rc;
    return 0;
}

void bpmf_capi::CellsPlan::bind(bpmf_launch::PredCellsLaunch &p, size_t b) const
{
    p.nseg = (int64_t)(first[b + 1] - first[b]);
    p.seg_q = d_segq.get() + first[b]; p.seg_beg = d_segb.get() + first[b]; p.seg_cnt = d_segc.get() + first[b];
    p.cand = d_cand.get(); p.orig = d_orig.get();
}

extern "C" int bpmf_hip_predict_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q, const int32_t *cc,
                                      int want_prob, double t, double sigma, double *mean_out, double *std_out, double *prob_out)
{
    { const int rc = cells_check_list("predict_cells", query, cand, mean_rating, n, q, cc); if (rc) return rc; }
    if (want_prob && !std::isfinite(t)) return fail(BPMF_HIP_EINVAL, "predict_cells: the threshold is not finite");
    if (want_prob && !(std::isfinite(sigma) && sigma >= 0.0)) return fail(BPMF_HIP_EINVAL, "predict_cells: sigma must be finite and >= 0");
    if (n > 0 && (!mean_out || !std_out || (want_prob && !prob_out))) return fail(BPMF_HIP_EINVAL, "predict_cells: NULL output");
    bpmf_launch::PredCellsLaunch p{};
    int rc;
    if ((rc = pair_open_rings("predict_cells", query, cand, &p.r))) return rc;
    if (n == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = query->ctx;
    Timed &timed = query->ring->cells;

    const CellsSorted sorted = cells_sort(query->ncols, n, q, cc);
    CellsPlan plan(sorted, n, n, bpmf_launch::predict_cells_segment(p.r.Kp));      // one batch
    DevBuf<double> out;
    if ((rc = plan.upload()) || (rc = out.alloc((size_t)(want_prob ? 3 : 2) * (size_t)n))) return rc;
    p.mean_rating = mean_rating;
    p.want_prob = want_prob ? 1 : 0; p.t = want_prob ? t : 0.0; p.sigma = want_prob ? sigma : 0.0;
    plan.bind(p, 0);
    p.mean = out.get(); p.std = out.get() + n; p.prob = want_prob ? out.get() + 2 * n : nullptr;
    if ((rc = timed.begin(c->stream.get()))) return rc;
    if (bpmf_launch::predict_cells(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, "predict_cells: unsupported shape");
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "predict_cells: kernel launch failed");
    if ((rc = timed.end(c->stream.get())) || (rc = bounded_stream_sync(c, c->stream.get(), "predict_cells"))) return rc;
    timed.resolve();
    return copy_back("predict_cells", {{mean_out, out.get(), (size_t)n}, {std_out, out.get() + n, (size_t)n},
                                       {want_prob ? prob_out : nullptr, out.get() + 2 * n, (size_t)n}});
}

extern "C" int bpmf_hip_predict_cells_last_ms(const bpmf_hip_side *query, float *ms)
{
    return last_ms("predict_cells_last_ms", query, query && query->ring ? &query->ring->cells : nullptr, ms,
                   "no launch with the side as the queries has been timed (bpmf_hip_predict_cells)");
}
