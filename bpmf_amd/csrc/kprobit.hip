// kprobit.hip -- launchers of the probit kernels (kernels_probit.h, see launch.h).
#include "launch.h"
#include "kernels_probit.h"

namespace bpmf_launch {

void probit_sign(const double *vals, int64_t nnz, double threshold, int8_t *sign, hipStream_t st)
{
    if (nnz <= 0) return;
    hipLaunchKernelGGL(bpmf::k_probit_sign, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, vals, nnz, threshold, sign);
}

int probit_latent(const ProbitLatentLaunch &p, hipStream_t st)
{
    if (p.m.nnz <= 0) return 0;
    const unsigned grid = (unsigned)((p.m.nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile);   // one tile of ratings per workgroup
    return dispatch_kt(p.f.K, p.f.f32, [&](auto k, auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bpmf::k_probit_latent<decltype(k)::value, T>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.m.colptr, p.m.ncols,
                           p.m.rowidx, p.sign, p.m.nnz, (const T *)p.f.items, (const T *)p.f.other, p.f.kt, p.iter, p.tag, p.z, p.fail);
    });
}

int probit_prob(const ProbitProbLaunch &p, hipStream_t st)
{
    if (p.nnz <= 0) return 0;
    const unsigned grid = (unsigned)((p.nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile);
    return dispatch_kt(p.f.K, p.f.f32, [&](auto k, auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bpmf::k_probit_prob<decltype(k)::value, T>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.tcol, p.trow, p.nnz,
                           (const T *)p.f.items, (const T *)p.f.other, p.f.kt, p.sum);
    });
}

}  // namespace bpmf_launch
