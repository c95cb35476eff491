// kdiag.hip -- launchers of the convergence diagnostics (kernels_diag.h, see launch.h).
#include "launch.h"
#include "kernels_diag.h"

namespace bpmf_launch {

int diag_min_samples() { return bpmf::kDiagMinSamples; }
int diag_max_samples() { return bpmf::kDiagMaxSamples; }
int cell_traces_segment(int Kp) { return bpmf::ct_segment(Kp); }

int cell_traces(const PredCellsLaunch &p, double *trace, int64_t tbase, hipStream_t st)
{
    if (!ring_pair_ok(p.r) || p.nseg < 0 || p.nseg > 0x7fffffff || !trace) return -1;
    if (p.nseg == 0) return 0;
    bpmf::CellTracesArgs a;
    a.qring = p.r.qring; a.cring = p.r.cring; a.qstride = p.r.qstride; a.cstride = p.r.cstride; a.Kp = p.r.Kp; a.S = p.r.S;
    a.mean_rating = p.mean_rating;
    a.seg_q = p.seg_q; a.seg_beg = p.seg_beg; a.seg_cnt = p.seg_cnt; a.cand = p.cand; a.orig = p.orig;
    a.mean = p.mean; a.std = p.std;
    a.trace = trace; a.tbase = tbase;
    const dim3 grid((unsigned)p.nseg), block(256);
#define BPMF_CT_LAUNCH(G_) case G_: hipLaunchKernelGGL((bpmf::k_cell_traces<G_>), grid, block, 0, st, a); break;
    switch (bpmf::ct_group(p.r.Kp)) {
    BPMF_CT_LAUNCH(2) BPMF_CT_LAUNCH(4) BPMF_CT_LAUNCH(8) BPMF_CT_LAUNCH(16) BPMF_CT_LAUNCH(32) BPMF_CT_LAUNCH(64)
    default: return -1;
    }
#undef BPMF_CT_LAUNCH
    return 0;
}

int trace_diag(const double *traces, int64_t ntr, int S, const int32_t *orig, double *rhat, double *ess, hipStream_t st)
{
    if (S < bpmf::kDiagMinSamples || S > bpmf::kDiagMaxSamples || ntr < 0) return -1;
    if (ntr == 0) return 0;
    const int w = bpmf::diag_waves(S);
    const int64_t nblk = (ntr + w - 1) / w;
    if (nblk > 0x7fffffff) return -1;
    const size_t lds = (size_t)w * (size_t)bpmf::diag_lds_doubles(S) * sizeof(double);      // <= 64 KiB
    hipLaunchKernelGGL(bpmf::k_trace_diag, dim3((unsigned)nblk), dim3(64 * w), lds, st, traces, ntr, S, orig, rhat, ess);
    return 0;
}

}  // namespace bpmf_launch
