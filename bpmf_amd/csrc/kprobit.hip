// kprobit.hip -- launchers of the probit kernels (kernels_probit.h, see launch.h).
#include "launch.h"
#include "kernels_probit.h"

namespace bpmf_launch {

void probit_sign(const double *vals, int64_t nnz, double threshold, int8_t *sign, hipStream_t st)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(bpmf::k_probit_sign, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, vals, nnz, threshold, sign);
}

template <int K, typename T>
static void latent_launch(const ProbitLatentLaunch &p, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_probit_latent<K, T>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.colptr, p.ncols, p.rowidx, p.sign,
                       p.nnz, (const T *)p.items, (const T *)p.other, p.kt, p.iter, p.tag, p.z, p.fail);
}

template <int K, typename T>
static void prob_launch(const ProbitProbLaunch &p, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_probit_prob<K, T>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.tcol, p.trow, p.nnz,
                       (const T *)p.items, (const T *)p.other, p.kt, p.sum);
}

#define BPMF_PROBIT_DISPATCH(fn)                                       \
    if (p.f32) {                                                       \
        if (p.K != 128) return -1;                                     \
        fn<128, float>(p, grid, st);                                   \
    } else {                                                           \
        switch (p.K) {                                                 \
        case 8: fn<8, double>(p, grid, st); break;                     \
        case 16: fn<16, double>(p, grid, st); break;                   \
        case 32: fn<32, double>(p, grid, st); break;                   \
        case 64: fn<64, double>(p, grid, st); break;                   \
        case 128: fn<128, double>(p, grid, st); break;                 \
        default: return -1;                                            \
        }                                                              \
    }

int probit_latent(const ProbitLatentLaunch &p, hipStream_t st)
{
    if (p.nnz <= 0) return 0;
    const unsigned grid = (unsigned)((p.nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile);     // one tile of ratings per workgroup
    BPMF_PROBIT_DISPATCH(latent_launch)
    return 0;
}

int probit_prob(const ProbitProbLaunch &p, hipStream_t st)
{
    if (p.nnz <= 0) return 0;
    const unsigned grid = (unsigned)((p.nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile);
    BPMF_PROBIT_DISPATCH(prob_launch)
    return 0;
}

}  // namespace bpmf_launch
