// krobust.hip -- launchers of the kernels of Student-t noise (kernels_robust.h, see launch.h).
#include "launch.h"
#include "kernels_robust.h"

namespace bpmf_launch {

int robust_weights(const RobustWeightsLaunch &p, hipStream_t st)
{
    if (p.m.nnz <= 0) return 0;
    const unsigned grid = (unsigned)((p.m.nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile);   // one tile of ratings per workgroup
    return dispatch_k(p.f.K, [&](auto k) {
        hipLaunchKernelGGL((bpmf::k_robust_weights<decltype(k)::value, double>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.m.colptr, p.m.ncols,
                           p.m.rowidx, p.vals, p.m.nnz, (const double *)p.f.items, (const double *)p.f.other, p.f.kt, p.iter, p.tag, p.mean,
                           p.sqrt_alpha, p.nu, p.dd, p.c, p.sw, p.zw, p.fail);
    });
}

void robust_accumulate(const double *sw, int64_t nnz, double *wsum, hipStream_t st)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(bpmf::k_robust_accumulate, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, sw, nnz, wsum);
}

}  // namespace bpmf_launch
