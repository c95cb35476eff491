// capi_similar.hip -- similar columns of one side by posterior cosine / distance over the side's sample ring (bpmf_hip_similar,
// bpmf_hip_similar_block; kernels in kernels_similar.h)
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

namespace {

// the checks both entry points share, then the norm table of the ring (rebuilt by every call: nothing cached, nothing to drop)
int similar_prepare(const char *who, bpmf_hip_side *s, int kind, DevBuf<double> &tab)
{
    const std::string w(who);
    if (!s) return fail(BPMF_HIP_EINVAL, w + ": NULL side");
    if (kind != BPMF_HIP_SIM_COSINE && kind != BPMF_HIP_SIM_EUCLID)
        return fail(BPMF_HIP_EINVAL, w + ": unknown kind " + std::to_string(kind) + " (BPMF_HIP_SIM_COSINE or _EUCLID)");
    bpmf_hip_ctx *c = s->ctx;
    int rc = require_single_gpu(who, c, s);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = settle_async(s))) return rc;
    const bpmf_ring *ring = s->ring.get();
    if (!ring) return fail(BPMF_HIP_EINVAL, w + ": no sample ring (bpmf_hip_side_samples_reserve)");
    { const int rb = refuse(w.c_str(), s, {Not::bias}); if (rb) return rb; }      // (the two bias rows of its ring would enter the cosine)
    if (ring->count < 1) return fail(BPMF_HIP_EINVAL, w + ": the sample ring is empty");
    if (s->ncols > std::numeric_limits<int32_t>::max()) return fail(BPMF_HIP_EINVAL, w + ": too many columns");
    if (s->ncols < 1) return BPMF_HIP_OK;
    if (tab.alloc(2 * (size_t)ring->count * (size_t)s->ncols))
        return fail(BPMF_HIP_ENOMEM, w + ": device allocation of the norm table failed");
    return BPMF_HIP_OK;
}

}  // namespace

extern "C" int bpmf_hip_similar(bpmf_hip_side *side, int kind, double kappa, int n, int64_t q_from, int64_t q_to, const uint8_t *cand_ok,
                                int32_t *idx_out, double *score_out, double *mean_out, double *std_out)
{
    if (!side) return fail(BPMF_HIP_EINVAL, "similar: NULL side");
    if (!(std::isfinite(kappa) && kappa >= 0.0)) return fail(BPMF_HIP_EINVAL, "similar: kappa must be finite and >= 0");
    if (n < 1 || n > bpmf_launch::topn_max_n())
        return fail(BPMF_HIP_EINVAL, "similar: n = " + std::to_string(n) + " (1 .. " + std::to_string(bpmf_launch::topn_max_n()) + ")");
    if (q_from < 0 || q_to < q_from || q_to > side->ncols) return fail(BPMF_HIP_EINVAL, "similar: query range out of bounds");
    const int64_t nq = q_to - q_from, nc = side->ncols;
    if (nq > 0 && (!idx_out || !score_out || !mean_out || !std_out)) return fail(BPMF_HIP_EINVAL, "similar: NULL output");
    DevBuf<double> tab;
    int rc = similar_prepare("similar", side, kind, tab);
    if (rc) return rc;
    if (nq == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = side->ctx;
    bpmf_ring *ring = side->ring.get();

    int64_t nsplit, cspan;
    topn_splits(c, nq, nc, &nsplit, &cspan);
    const size_t pn = (size_t)nq * (size_t)n;
    DevBuf<double> part, out;                                             // score | mean | std of the splits / of the result
    DevBuf<int32_t> part_idx, out_idx;
    DevBuf<uint8_t> d_ok;
    if (part.alloc(3 * (size_t)nsplit * pn) || part_idx.alloc((size_t)nsplit * pn) || out.alloc(3 * pn) || out_idx.alloc(pn))
        return fail(BPMF_HIP_ENOMEM, "similar: device allocation of the result lists failed");
    if (cand_ok && (rc = d_ok.upload(cand_ok, (size_t)nc))) return rc;
    bpmf_launch::SimilarLaunch p{};
    p.ring = ring->samples.get(); p.stride = (int64_t)ring->max * ring->kp; p.tab = tab.get();
    p.Kp = ring->kp; p.S = ring->count; p.n = n; p.kind = kind; p.kappa = kappa;
    p.q_from = q_from; p.nq = nq; p.nc = nc; p.cspan = cspan; p.nsplit = (int)nsplit;
    p.cand_ok = cand_ok ? d_ok.get() : nullptr;
    p.part_score = part.get(); p.part_mean = part.get() + (size_t)nsplit * pn; p.part_std = part.get() + 2 * (size_t)nsplit * pn;
    p.part_idx = part_idx.get();
    p.out_score = out.get(); p.out_mean = out.get() + pn; p.out_std = out.get() + 2 * pn; p.out_idx = out_idx.get();
    for (Event &e : ring->sim_timed) if (!e) { const int re = e.create(); if (re) return re; }
    ring->sim_ms = -1.f;
    HIP_TRY(hipEventRecord(ring->sim_timed[0].get(), c->stream.get()));
    if (bpmf_launch::ring_norms(p.ring, p.stride, p.Kp, p.S, nc, tab.get(), c->stream.get())) return fail(BPMF_HIP_EINVAL, "similar: unsupported shape of the ring");
    const int lrc = bpmf_launch::similar_topn(p, c->stream.get());
    if (lrc == -2) return fail(BPMF_HIP_ENODEV, "similar: the device refused the LDS of lists of " + std::to_string(n));
    if (lrc) return fail(BPMF_HIP_EINVAL, "similar: unsupported shape");
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "similar: kernel launch failed");
    HIP_TRY(hipEventRecord(ring->sim_timed[1].get(), c->stream.get()));
    if ((rc = bounded_stream_sync(c, c->stream.get(), "similar"))) return rc;
    if (hipEventElapsedTime(&ring->sim_ms, ring->sim_timed[0].get(), ring->sim_timed[1].get()) != hipSuccess) { (void)hipGetLastError(); ring->sim_ms = -1.f; }
    if (hipMemcpy(score_out, out.get(), pn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(mean_out, out.get() + pn, pn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(std_out, out.get() + 2 * pn, pn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(idx_out, out_idx.get(), pn * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(BPMF_HIP_ENODEV, "similar: copying the results back failed");
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_similar_block(bpmf_hip_side *side, int kind, int64_t q_from, int64_t q_to, int64_t c_from, int64_t c_to,
                                      double *mean_out, double *std_out)
{
    if (!side) return fail(BPMF_HIP_EINVAL, "similar_block: NULL side");
    if (q_from < 0 || q_to < q_from || q_to > side->ncols) return fail(BPMF_HIP_EINVAL, "similar_block: query range out of bounds");
    if (c_from < 0 || c_to < c_from || c_to > side->ncols) return fail(BPMF_HIP_EINVAL, "similar_block: candidate range out of bounds");
    const int64_t nq = q_to - q_from, nc = c_to - c_from;
    if (nq > 0 && nc > 0 && (!mean_out || !std_out)) return fail(BPMF_HIP_EINVAL, "similar_block: NULL output");
    DevBuf<double> tab;
    int rc = similar_prepare("similar_block", side, kind, tab);
    if (rc) return rc;
    if (nq == 0 || nc == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = side->ctx;
    const bpmf_ring *ring = side->ring.get();
    const size_t cells = (size_t)nq * (size_t)nc;
    DevBuf<double> out;
    if (out.alloc(2 * cells))
        return fail(BPMF_HIP_ENOMEM, "similar_block: a block of " + std::to_string((long long)nq) + " x " + std::to_string((long long)nc) +
                    " means and deviations does not fit in device memory: ask for smaller ranges");
    bpmf_launch::SimilarBlockLaunch p{};
    p.ring = ring->samples.get(); p.stride = (int64_t)ring->max * ring->kp; p.tab = tab.get();
    p.Kp = ring->kp; p.S = ring->count; p.kind = kind;
    p.ncols = side->ncols; p.q_from = q_from; p.nq = nq; p.c_from = c_from; p.nc = nc;
    p.mean = out.get(); p.std = out.get() + cells;
    if (bpmf_launch::ring_norms(p.ring, p.stride, p.Kp, p.S, side->ncols, tab.get(), c->stream.get()) || bpmf_launch::similar_block(p, c->stream.get()))
        return fail(BPMF_HIP_EINVAL, "similar_block: unsupported shape of the block");
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "similar_block: kernel launch failed");
    if ((rc = bounded_stream_sync(c, c->stream.get(), "similar_block"))) return rc;
    if (hipMemcpy(mean_out, out.get(), cells * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(std_out, out.get() + cells, cells * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(BPMF_HIP_ENODEV, "similar_block: copying the results back failed");
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_similar_last_ms(const bpmf_hip_side *side, float *ms)
{
    if (!side || !ms) return fail(BPMF_HIP_EINVAL, "similar_last_ms: NULL argument");
    if (!side->ring || side->ring->sim_ms < 0.f)
        return fail(BPMF_HIP_EINVAL, "similar_last_ms: no ranking of the side has been timed (bpmf_hip_similar)");
    *ms = side->ring->sim_ms;
    return BPMF_HIP_OK;
}
