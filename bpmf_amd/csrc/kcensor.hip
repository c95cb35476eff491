// kcensor.hip -- launcher of the latent kernel of censored ratings (kernels_censor.h, see launch.h).
#include "launch.h"
#include "kernels_censor.h"

namespace bpmf_launch {

int censor_latent(const CensorLatentLaunch &p, hipStream_t st)
{
    if (p.n <= 0) return 0;                                           // a side without censored entries: no kernel
    const unsigned grid = (unsigned)((p.n + bpmf::kProbitTile - 1) / bpmf::kProbitTile);       // one tile of censored entries per workgroup
    return dispatch_kt(p.f.K, p.f.f32, [&](auto k, auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bpmf::k_censor_latent<decltype(k)::value, T>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.pos, p.col, p.row, p.sign,
                           p.n, p.vals, (const T *)p.f.items, (const T *)p.f.other, p.f.kt, p.iter, p.tag, p.mean, p.sqrt_alpha, p.inv_sqrt_alpha,
                           p.z, p.fail);
    });
}

}  // namespace bpmf_launch
