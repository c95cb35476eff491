// krobust.hip -- launchers of the kernels of Student-t noise (kernels_robust.h, see launch.h).
#include "launch.h"
#include "kernels_robust.h"

namespace bpmf_launch {

template <int K>
static void weights_launch(const RobustWeightsLaunch &p, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_robust_weights<K, double>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.colptr, p.ncols, p.rowidx, p.vals,
                       p.nnz, (const double *)p.items, (const double *)p.other, p.kt, p.iter, p.tag, p.mean, p.sqrt_alpha, p.nu, p.dd, p.c,
                       p.sw, p.zw, p.fail);
}

int robust_weights(const RobustWeightsLaunch &p, hipStream_t st)
{
    if (p.nnz <= 0) return 0;
    const unsigned grid = (unsigned)((p.nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile);     // one tile of ratings per workgroup
    switch (p.K) {
    case 8: weights_launch<8>(p, grid, st); break;
    case 16: weights_launch<16>(p, grid, st); break;
    case 32: weights_launch<32>(p, grid, st); break;
    case 64: weights_launch<64>(p, grid, st); break;
    case 128: weights_launch<128>(p, grid, st); break;
    default: return -1;
    }
    return 0;
}

void robust_accumulate(const double *sw, int64_t nnz, double *wsum, hipStream_t st)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(bpmf::k_robust_accumulate, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, sw, nnz, wsum);
}

}  // namespace bpmf_launch
