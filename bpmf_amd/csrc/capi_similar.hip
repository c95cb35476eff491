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
    int rc;
    if ((rc = refuse_topn_n("similar", n)) || (rc = refuse_range("similar", "query", q_from, q_to, side->ncols))) return rc;
    const int64_t nq = q_to - q_from, nc = side->ncols;
    if (nq > 0 && (!idx_out || !score_out || !mean_out || !std_out)) return fail(BPMF_HIP_EINVAL, "similar: NULL output");
    DevBuf<double> tab;
    if ((rc = similar_prepare("similar", side, kind, tab))) return rc;
    if (nq == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = side->ctx;
    bpmf_ring *ring = side->ring.get();
    const RingView v = ring_view(ring);

    int64_t nsplit, cspan;
    topn_splits(c, nq, nc, &nsplit, &cspan);
    TopnLists l;
    DevBuf<uint8_t> d_ok;
    if ((rc = l.alloc("similar", nsplit, nq, n, true))) return rc;
    if (cand_ok && (rc = d_ok.upload(cand_ok, (size_t)nc))) return rc;
    bpmf_launch::SimilarLaunch p{};
    p.ring = v.ring; p.stride = v.stride; p.tab = tab.get();
    p.Kp = v.kp; p.S = v.count; p.n = n; p.kind = kind; p.kappa = kappa;
    p.q_from = q_from; p.nq = nq; p.nc = nc; p.cspan = cspan; p.nsplit = (int)nsplit;
    p.cand_ok = cand_ok ? d_ok.get() : nullptr;
    p.part_score = l.part_score(); p.part_mean = l.part_mean(); p.part_std = l.part_std(); p.part_idx = l.part_idx();
    p.out_score = l.out_score(); p.out_mean = l.out_mean(); p.out_std = l.out_std(); p.out_idx = l.out_idx();
    if ((rc = ring->sim.begin(c->stream.get()))) return rc;
    if (bpmf_launch::ring_norms(p.ring, p.stride, p.Kp, p.S, nc, tab.get(), c->stream.get())) return fail(BPMF_HIP_EINVAL, "similar: unsupported shape of the ring");
    const int lrc = bpmf_launch::similar_topn(p, c->stream.get());
    if (lrc == -2) return fail(BPMF_HIP_ENODEV, "similar: the device refused the LDS of lists of " + std::to_string(n));
    if (lrc) return fail(BPMF_HIP_EINVAL, "similar: unsupported shape");
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "similar: kernel launch failed");
    if ((rc = ring->sim.end(c->stream.get())) || (rc = bounded_stream_sync(c, c->stream.get(), "similar"))) return rc;
    ring->sim.resolve();
    return l.read_back("similar", idx_out, score_out, mean_out, std_out);
}

extern "C" int bpmf_hip_similar_block(bpmf_hip_side *side, int kind, int64_t q_from, int64_t q_to, int64_t c_from, int64_t c_to,
                                      double *mean_out, double *std_out)
{
    if (!side) return fail(BPMF_HIP_EINVAL, "similar_block: NULL side");
    int rc;
    if ((rc = refuse_range("similar_block", "query", q_from, q_to, side->ncols)) || (rc = refuse_range("similar_block", "candidate", c_from, c_to, side->ncols)))
        return rc;
    const int64_t nq = q_to - q_from, nc = c_to - c_from;
    if (nq > 0 && nc > 0 && (!mean_out || !std_out)) return fail(BPMF_HIP_EINVAL, "similar_block: NULL output");
    DevBuf<double> tab;
    if ((rc = similar_prepare("similar_block", side, kind, tab))) return rc;
    if (nq == 0 || nc == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = side->ctx;
    const RingView v = ring_view(side->ring.get());
    const size_t cells = (size_t)nq * (size_t)nc;
    DevBuf<double> out;
    if (out.alloc(2 * cells))
        return fail(BPMF_HIP_ENOMEM, "similar_block: a block of " + std::to_string((long long)nq) + " x " + std::to_string((long long)nc) +
                    " means and deviations does not fit in device memory: ask for smaller ranges");
    bpmf_launch::SimilarBlockLaunch p{};
    p.ring = v.ring; p.stride = v.stride; p.tab = tab.get();
    p.Kp = v.kp; p.S = v.count; p.kind = kind;
    p.ncols = side->ncols; p.q_from = q_from; p.nq = nq; p.c_from = c_from; p.nc = nc;
    p.mean = out.get(); p.std = out.get() + cells;
    if (bpmf_launch::ring_norms(p.ring, p.stride, p.Kp, p.S, side->ncols, tab.get(), c->stream.get()) || bpmf_launch::similar_block(p, c->stream.get()))
        return fail(BPMF_HIP_EINVAL, "similar_block: unsupported shape of the block");
    if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "similar_block: kernel launch failed");
    if ((rc = bounded_stream_sync(c, c->stream.get(), "similar_block"))) return rc;
    return copy_back("similar_block", {{mean_out, out.get(), cells}, {std_out, out.get() + cells, cells}});
}

extern "C" int bpmf_hip_similar_last_ms(const bpmf_hip_side *side, float *ms)
{
    return last_ms("similar_last_ms", side, side && side->ring ? &side->ring->sim : nullptr, ms, "no ranking of the side has been timed (bpmf_hip_similar)");
}
