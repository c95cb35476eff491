// kscore.hip -- launcher of the model comparison kernel (kernels_score.h, see launch.h).
#include "launch.h"
#include "kernels_score.h"
#include "../../include/bpmf_hip.h"

namespace bpmf_launch {

int score_cells_segment(int Kp) { return bpmf::sc_segment(Kp); }

int score_cells(const ScoreCellsLaunch &s, hipStream_t st)
{
    const PredCellsLaunch &p = s.cells;
    if (!ring_pair_ok(p.r) || p.nseg < 0 || p.nseg > 0x7fffffff || !s.y || !s.c0 || !s.lpd || !s.pw) return -1;
    int kind;
    switch (s.kind) {
    case BPMF_HIP_LOGDENS_GAUSSIAN: kind = s.flag ? bpmf::kScoreGaussFlags : bpmf::kScoreGauss; if (!s.as || (s.flag && !s.sa)) return -1; break;
    case BPMF_HIP_LOGDENS_STUDENT: kind = bpmf::kScoreStudent; if (!s.as || s.flag || s.w) return -1; break;
    case BPMF_HIP_LOGDENS_PROBIT: kind = bpmf::kScoreProbit; if (!s.flag || s.w) return -1; break;
    default: return -1;
    }
    if (p.nseg == 0) return 0;
    bpmf::ScoreCellsArgs a;
    a.qring = p.r.qring; a.cring = p.r.cring; a.qstride = p.r.qstride; a.cstride = p.r.cstride; a.Kp = p.r.Kp; a.S = p.r.S;
    a.mean_rating = p.mean_rating;
    a.seg_q = p.seg_q; a.seg_beg = p.seg_beg; a.seg_cnt = p.seg_cnt; a.cand = p.cand; a.orig = p.orig;
    a.y = s.y; a.w = s.w; a.flag = s.flag; a.c0 = s.c0; a.as = s.as; a.sa = s.sa; a.hnu1 = 0.5 * (s.nu + 1.0);
    a.mean = p.mean; a.std = p.std; a.lpd = s.lpd; a.pw = s.pw;
    const dim3 grid((unsigned)p.nseg), block(256);
#define BPMF_SC_KIND(G_, K_) case K_: hipLaunchKernelGGL((bpmf::k_cells_logdens<G_, K_>), grid, block, 0, st, a); break;
#define BPMF_SC_LAUNCH(G_)                                                                                                          \
    case G_:                                                                                                                        \
        switch (kind) {                                                                                                             \
        BPMF_SC_KIND(G_, bpmf::kScoreGauss) BPMF_SC_KIND(G_, bpmf::kScoreGaussFlags) BPMF_SC_KIND(G_, bpmf::kScoreStudent)          \
        BPMF_SC_KIND(G_, bpmf::kScoreProbit)                                                                                        \
        }                                                                                                                           \
        break;
    switch (bpmf::sc_group(p.r.Kp)) {
    BPMF_SC_LAUNCH(2) BPMF_SC_LAUNCH(4) BPMF_SC_LAUNCH(8) BPMF_SC_LAUNCH(16) BPMF_SC_LAUNCH(32) BPMF_SC_LAUNCH(64)
    default: return -1;
    }
#undef BPMF_SC_LAUNCH
#undef BPMF_SC_KIND
    return 0;
}

}  // namespace bpmf_launch
