// kinterval.hip -- launcher of the predictive intervals (kernels_interval.h, see launch.h).
#include "launch.h"
#include "kernels_interval.h"

namespace bpmf_launch {

int interval_max_samples() { return bpmf::kIntervalMaxSamples; }
int interval_max_quantiles() { return bpmf::kIntervalMaxQuantiles; }

int trace_quantiles(const TraceQuantLaunch &p, hipStream_t st)
{
    if (p.S < 1 || p.S > bpmf::kIntervalMaxSamples || p.ntr < 0 || p.nq < 0 || p.nq > bpmf::kIntervalMaxQuantiles || !p.traces) return -1;
    if ((p.y && !p.pit) || (p.nq > 0 && !p.quant) || (!p.y && p.nq == 0)) return -1;
    if (p.ntr == 0) return 0;
    const int w = bpmf::interval_waves(p.S);
    const int64_t nblk = (p.ntr + w - 1) / w;
    if (nblk > 0x7fffffff) return -1;
    bpmf::TraceQuantArgs a{};
    a.traces = p.traces; a.ntr = p.ntr; a.S = p.S; a.orig = p.orig;
    a.mean_rating = p.mean_rating; a.y = p.y; a.w = p.w; a.sa = p.sa; a.sa0 = p.sa0;
    a.nq = p.nq;
    for (int j = 0; j < p.nq; ++j) { a.tau[j] = p.tau[j]; a.z[j] = p.z[j]; }
    a.pit = p.pit; a.quant = p.quant;
    const size_t lds = (size_t)w * (size_t)bpmf::interval_lds_doubles(p.S) * sizeof(double);   // <= 64 KiB
    hipLaunchKernelGGL(bpmf::k_trace_quantiles, dim3((unsigned)nblk), dim3(64 * w), lds, st, a);
    return 0;
}

}  // namespace bpmf_launch
