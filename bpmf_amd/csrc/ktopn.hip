// ktopn.hip -- launchers of the posterior top-N kernels (kernels_topn.h, see launch.h).
#include "launch.h"
#include "kernels_topn.h"

namespace bpmf_launch {

void samples_add(const void *items, bool f32, int ld, int Kt, int Kp, int64_t ncols, double *ring, int64_t stride, int slot, hipStream_t st)
{
    const int64_t n = ncols * Kp;
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (f32) hipLaunchKernelGGL(bpmf::k_samples_add<float>, grid, dim3(256), 0, st, (const float *)items, ld, Kt, Kp, ncols, ring, stride, slot);
    else hipLaunchKernelGGL(bpmf::k_samples_add<double>, grid, dim3(256), 0, st, (const double *)items, ld, Kt, Kp, ncols, ring, stride, slot);
}

int topn_max_n() { return bpmf::kTopnMaxN; }

void topn(const TopnLaunch &p, hipStream_t st)
{
    bpmf::TopnArgs a;
    a.qring = p.r.qring; a.cring = p.r.cring; a.qstride = p.r.qstride; a.cstride = p.r.cstride;
    a.L = p.r.S * p.r.Kp; a.S = p.r.S; a.n = p.n; a.mean_rating = p.mean_rating;
    a.q_from = p.q_from; a.nq = p.nq; a.nc = p.nc; a.cspan = p.cspan;
    a.ex_ptr = p.ex_ptr; a.ex_rows = p.ex_rows; a.part_mean = p.part_mean; a.part_idx = p.part_idx;
    const size_t lds = sizeof(double) * ((size_t)bpmf::kTopnQ * bpmf::kTopnScLd + (size_t)bpmf::kTopnQ * p.n + bpmf::kTopnQ) +
                       sizeof(int) * (size_t)bpmf::kTopnQ * p.n;
    const unsigned nqb = (unsigned)((p.nq + bpmf::kTopnQ - 1) / bpmf::kTopnQ);
    hipLaunchKernelGGL(bpmf::k_topn_score, dim3(nqb, (unsigned)p.nsplit), dim3(256), lds, st, a);
    hipLaunchKernelGGL(bpmf::k_topn_merge, dim3((unsigned)((p.nq + 255) / 256)), dim3(256), 0, st,
                       p.part_mean, p.part_idx, p.nsplit, p.nq, p.n, p.out_mean, p.out_idx);
    const int64_t npairs = p.nq * p.n;
    hipLaunchKernelGGL(bpmf::k_topn_std, dim3((unsigned)((npairs + 3) / 4)), dim3(256), 0, st, p.r.qring, p.r.cring, p.r.qstride, p.r.cstride,
                       p.r.Kp, p.r.S, p.mean_rating, p.q_from, npairs, p.n, p.out_mean, p.out_idx, p.out_std);
}

}  // namespace bpmf_launch
