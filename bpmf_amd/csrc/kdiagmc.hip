// kdiagmc.hip -- launcher of the multi-chain rank-normalised convergence diagnostics (kernels_diag_mc.h, see launch.h).
#include "launch.h"
#include "kernels_diag_mc.h"

namespace bpmf_launch {

int diag_mc_max_chains() { return bpmf::kDiagMcMaxChains; }
int diag_mc_min_samples() { return bpmf::kDiagMcMinSamples; }
int diag_mc_max_values() { return bpmf::kDiagMcMaxValues; }

int trace_diag_mc(const double *traces, int64_t ntr, int C, int S, const int32_t *orig, double *rhat, double *ess_bulk, double *ess_tail,
                  hipStream_t st)
{
    if (!bpmf::dmc_shape_ok(C, S) || ntr < 0) return -1;
    if (ntr == 0) return 0;
    const int w = bpmf::dmc_waves(C, S);
    const int64_t nblk = (ntr + w - 1) / w;
    if (nblk > 0x7fffffff) return -1;
    const size_t lds = (size_t)w * (size_t)bpmf::dmc_lds_bytes(C, S);                        // <= 64 KiB
    if (lds > 65536) return -1;
    bpmf::TraceDiagMcArgs a;
    a.traces = traces; a.ntr = ntr; a.C = C; a.S = S; a.orig = orig; a.rhat = rhat; a.ess_bulk = ess_bulk; a.ess_tail = ess_tail;
    hipLaunchKernelGGL(bpmf::k_trace_diag_mc, dim3((unsigned)nblk), dim3(64 * w), lds, st, a);
    return 0;
}

}  // namespace bpmf_launch
