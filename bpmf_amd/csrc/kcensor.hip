// kcensor.hip -- launcher of the latent kernel of censored ratings (kernels_censor.h, see launch.h).
#include "launch.h"
#include "kernels_censor.h"

namespace bpmf_launch {

template <int K, typename T>
static void censor_launch(const CensorLatentLaunch &p, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_censor_latent<K, T>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.pos, p.col, p.row, p.sign, p.n, p.vals,
                       (const T *)p.items, (const T *)p.other, p.kt, p.iter, p.tag, p.mean, p.sqrt_alpha, p.inv_sqrt_alpha, p.z, p.fail);
}

// the instantiations of k_probit_latent (kprobit.hip)
int censor_latent(const CensorLatentLaunch &p, hipStream_t st)
{
    if (p.n <= 0) return 0;                                           // a side without censored entries: no kernel
    const unsigned grid = (unsigned)((p.n + bpmf::kProbitTile - 1) / bpmf::kProbitTile);       // one tile of censored entries per workgroup
    if (p.f32) {
        if (p.K != 128) return -1;
        censor_launch<128, float>(p, grid, st);
        return 0;
    }
    switch (p.K) {
    case 8: censor_launch<8, double>(p, grid, st); break;
    case 16: censor_launch<16, double>(p, grid, st); break;
    case 32: censor_launch<32, double>(p, grid, st); break;
    case 64: censor_launch<64, double>(p, grid, st); break;
    case 128: censor_launch<128, double>(p, grid, st); break;
    default: return -1;
    }
    return 0;
}

}  // namespace bpmf_launch
