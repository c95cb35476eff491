// kloo.hip -- launcher of the PSIS-LOO kernel (kernels_loo.h, see launch.h).
#include "launch.h"
#include "kernels_loo.h"
#include "../../include/bpmf_hip.h"

namespace bpmf_launch {

int loo_max_samples() { return bpmf::kLooMaxSamples; }

int trace_psis(const TracePsisLaunch &p, hipStream_t st)
{
    if (p.S < 1 || p.S > bpmf::kLooMaxSamples || p.ntr < 0 || !p.traces || !p.elpd || !p.khat || !p.lpd) return -1;
    if (bpmf::loo_tail(p.S) > bpmf::kLooMaxTail) return -1;
    int kind;
    switch (p.kind) {
    case -1: kind = bpmf::kLooTraces; break;
    case BPMF_HIP_LOGDENS_GAUSSIAN: kind = p.flag ? bpmf::kScoreGaussFlags : bpmf::kScoreGauss; if (!p.as || (p.flag && !p.sa)) return -1; break;
    case BPMF_HIP_LOGDENS_STUDENT: kind = bpmf::kScoreStudent; if (!p.as || p.flag || p.w) return -1; break;
    case BPMF_HIP_LOGDENS_PROBIT: kind = bpmf::kScoreProbit; if (!p.flag || p.w) return -1; break;
    default: return -1;
    }
    if (kind != bpmf::kLooTraces && (!p.y || !p.c0)) return -1;
    if (p.ntr == 0) return 0;
    const int w = bpmf::loo_waves(p.S);
    const int64_t nblk = (p.ntr + w - 1) / w;
    if (nblk > 0x7fffffff) return -1;
    bpmf::TracePsisArgs a{};
    a.traces = p.traces; a.ntr = p.ntr; a.S = p.S; a.orig = p.orig;
    a.mean_rating = p.mean_rating; a.y = p.y; a.w = p.w; a.flag = p.flag; a.c0 = p.c0; a.as = p.as; a.sa = p.sa; a.hnu1 = 0.5 * (p.nu + 1.0);
    a.elpd = p.elpd; a.khat = p.khat; a.lpd = p.lpd;
    const size_t lds = (size_t)w * (size_t)bpmf::loo_lds_doubles(p.S) * sizeof(double);      // <= 64 KiB
    const dim3 grid((unsigned)nblk), block(64 * w);
    switch (kind) {
#define BPMF_LOO_KIND(K_) case K_: hipLaunchKernelGGL((bpmf::k_trace_psis<K_>), grid, block, lds, st, a); break;
    BPMF_LOO_KIND(bpmf::kScoreGauss) BPMF_LOO_KIND(bpmf::kScoreGaussFlags) BPMF_LOO_KIND(bpmf::kScoreStudent) BPMF_LOO_KIND(bpmf::kScoreProbit)
    BPMF_LOO_KIND(bpmf::kLooTraces)
#undef BPMF_LOO_KIND
    }
    return 0;
}

}  // namespace bpmf_launch
