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
        bpmf_launch::samples_pack(ring->samples.get(), (int64_t)ring->max * ring->kp, ring->kp, kt, c0, nc, s_from, n, packed.get(), c->stream.get());
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
            bpmf_launch::samples_unpack(packed.get(), (int64_t)ring->max * ring->kp, ring->kp, kt, c0, nc, n, ring->samples.get(), c->stream.get());
            if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "samples_set: kernel launch failed");
            { const int rc = bounded_stream_sync(c, c->stream.get(), "samples_set"); if (rc) return rc; }
        }
    }
    ring->count = n;
    return BPMF_HIP_OK;
}

// What bpmf_hip_predict_cells and bpmf_hip_diag_cells (capi_diag.hip) refuse alike, reported as `who`.  cells_check_list: the sides and
// the list, on the host alone; cells_check_rings: waits for the sides' work in flight, then the rings; *S_out: the samples both hold
int bpmf_capi::cells_check_list(const std::string &who, bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q,
                                const int32_t *cc)
{
    if (!query || !cand) return fail(BPMF_HIP_EINVAL, who + ": NULL side");
    if (query->ctx != cand->ctx) return fail(BPMF_HIP_EINVAL, who + ": the two sides belong to different contexts");
    { const int rc = require_single_gpu(who.c_str(), query->ctx, query, cand); if (rc) return rc; }
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

int bpmf_capi::cells_check_rings(const std::string &who, bpmf_hip_side *query, bpmf_hip_side *cand, int *S_out)
{
    HIP_TRY(hipSetDevice(query->ctx->device));
    { const int rc = settle_async(query); if (rc) return rc; }
    { const int rc = settle_async(cand); if (rc) return rc; }
    if (!query->ring || !cand->ring) return fail(BPMF_HIP_EINVAL, who + ": no sample ring on both sides (bpmf_hip_side_samples_reserve)");
    { const int rb = ring_pair_check(who, query, cand); if (rb) return rb; }
    const int S = query->ring->count;
    if (S < 1 || cand->ring->count != S)
        return fail(BPMF_HIP_EINVAL, who + ": both sides must hold the same number (>= 1) of samples: " + std::to_string(S) + " and " +
                    std::to_string(cand->ring->count));
    *S_out = S;
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

// every query's run among the sorted cells [b0, b1) cut into the segments a workgroup takes, appended to the three lists
void bpmf_capi::cells_segments(const CellsSorted &s, int64_t b0, int64_t b1, int seg, std::vector<int32_t> *seg_q, std::vector<int32_t> *seg_beg,
                               std::vector<int32_t> *seg_cnt)
{
    for (int64_t b = b0; b < b1;) {
        int64_t e = b + 1;
        while (e < b1 && e - b < seg && s.query[(size_t)e] == s.query[(size_t)b]) ++e;
        seg_q->push_back(s.query[(size_t)b]); seg_beg->push_back((int32_t)b); seg_cnt->push_back((int32_t)(e - b));
        b = e;
    }
}

extern "C" int bpmf_hip_predict_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q, const int32_t *cc,
                                      int want_prob, double t, double sigma, double *mean_out, double *std_out, double *prob_out)
{
    { const int rc = cells_check_list("predict_cells", query, cand, mean_rating, n, q, cc); if (rc) return rc; }
    if (want_prob && !std::isfinite(t)) return fail(BPMF_HIP_EINVAL, "predict_cells: the threshold is not finite");
    if (want_prob && !(std::isfinite(sigma) && sigma >= 0.0)) return fail(BPMF_HIP_EINVAL, "predict_cells: sigma must be finite and >= 0");
    if (n > 0 && (!mean_out || !std_out || (want_prob && !prob_out))) return fail(BPMF_HIP_EINVAL, "predict_cells: NULL output");
    int S = 0;
    { const int rc = cells_check_rings("predict_cells", query, cand, &S); if (rc) return rc; }
    if (n == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = query->ctx;
    bpmf_ring *qr = query->ring.get();
    const bpmf_ring *cr = cand->ring.get();

    const CellsSorted sorted = cells_sort(query->ncols, n, q, cc);
    const std::vector<int32_t> &scand = sorted.cand, &orig = sorted.orig;
    std::vector<int32_t> seg_q, seg_beg, seg_cnt;
    cells_segments(sorted, 0, n, bpmf_launch::predict_cells_segment(qr->kp), &seg_q, &seg_beg, &seg_cnt);
    DevBuf<int32_t> d_segq, d_segb, d_segc, d_cand, d_orig;
    DevBuf<double> out;
    int rc;
    if ((rc = d_segq.upload(seg_q.data(), seg_q.size())) || (rc = d_segb.upload(seg_beg.data(), seg_beg.size())) ||
        (rc = d_segc.upload(seg_cnt.data(), seg_cnt.size())) || (rc = d_cand.upload(scand.data(), scand.size())) ||
        (rc = d_orig.upload(orig.data(), orig.size())) || (rc = out.alloc((size_t)(want_prob ? 3 : 2) * (size_t)n)))
        return rc;
    bpmf_launch::PredCellsLaunch p{};
    p.qring = qr->samples.get(); p.cring = cr->samples.get();
    p.qstride = (int64_t)qr->max * qr->kp; p.cstride = (int64_t)cr->max * cr->kp;
    p.Kp = qr->kp; p.S = S; p.mean_rating = mean_rating;
    p.want_prob = want_prob ? 1 : 0; p.t = want_prob ? t : 0.0; p.sigma = want_prob ? sigma : 0.0;
    p.nseg = (int64_t)seg_q.size();
    p.seg_q = d_segq.get(); p.seg_beg = d_segb.get(); p.seg_cnt = d_segc.get(); p.cand = d_cand.get(); p.orig = d_orig.get();
    p.mean = out.get(); p.std = out.get() + n; p.prob = want_prob ? out.get() + 2 * n : nullptr;
    for (Event &e : qr->timed) if (!e) { const int re = e.create(); if (re) return re; }
    qr->cells_ms = -1.f;
    HIP_TRY(hipEventRecord(qr->timed[0].get(), c->stream.get()));
    if (bpmf_launch::predict_cells(p, c->stream.get())) return fail(BPMF_HIP_EINVAL, "predict_cells: unsupported shape");
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "predict_cells: kernel launch failed");
    HIP_TRY(hipEventRecord(qr->timed[1].get(), c->stream.get()));
    if ((rc = bounded_stream_sync(c, c->stream.get(), "predict_cells"))) return rc;
    if (hipEventElapsedTime(&qr->cells_ms, qr->timed[0].get(), qr->timed[1].get()) != hipSuccess) { (void)hipGetLastError(); qr->cells_ms = -1.f; }
    if (hipMemcpy(mean_out, out.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(std_out, out.get() + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        (want_prob && hipMemcpy(prob_out, out.get() + 2 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
        return fail(BPMF_HIP_ENODEV, "predict_cells: copying the results back failed");
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_predict_cells_last_ms(const bpmf_hip_side *query, float *ms)
{
    if (!query || !ms) return fail(BPMF_HIP_EINVAL, "predict_cells_last_ms: NULL argument");
    if (!query->ring || query->ring->cells_ms < 0.f)
        return fail(BPMF_HIP_EINVAL, "predict_cells_last_ms: no launch with the side as the queries has been timed (bpmf_hip_predict_cells)");
    *ms = query->ring->cells_ms;
    return BPMF_HIP_OK;
}
