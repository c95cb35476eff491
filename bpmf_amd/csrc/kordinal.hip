// kordinal.hip -- launchers of the ordinal probit kernels (kernels_ordinal.h, see launch.h).
#include "launch.h"
#include "kernels_ordinal.h"

namespace bpmf_launch {

int64_t ordinal_blocks(int64_t nnz) { return (nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile; }

// All three refuse an unsupported K first; only then does "no ratings" mean that there is nothing to launch.
int ordinal_latent(const OrdinalLatentLaunch &p, hipStream_t st)
{
    return dispatch_kt(p.f.K, p.f.f32, [&](auto k, auto t) {
        using T = decltype(t);
        if (p.m.nnz <= 0) return;
        hipLaunchKernelGGL((bpmf::k_ordinal_latent<decltype(k)::value, T>), dim3((unsigned)ordinal_blocks(p.m.nnz)), dim3(bpmf::kProbitTile), 0, st,
                           p.m.colptr, p.m.ncols, p.m.rowidx, p.level, p.m.nnz, (const T *)p.f.items, (const T *)p.f.other, p.f.kt, p.iter, p.tag,
                           p.g, p.nlev, p.z, p.fail);
    });
}

int ordinal_loglik(const OrdinalLoglikLaunch &p, hipStream_t st)
{
    const int64_t nblk = ordinal_blocks(p.m.nnz);
    const int rc = dispatch_kt(p.f.K, p.f.f32, [&](auto k, auto t) {
        using T = decltype(t);
        if (p.m.nnz <= 0) return;
        hipLaunchKernelGGL((bpmf::k_ordinal_loglik<decltype(k)::value, T>), dim3((unsigned)nblk), dim3(bpmf::kProbitTile), 0, st, p.m.colptr,
                           p.m.ncols, p.m.rowidx, p.level, p.m.nnz, (const T *)p.f.items, (const T *)p.f.other, p.f.kt, p.g0, p.g1, p.nlev,
                           p.partial);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(bpmf::k_ordinal_loglik_final, dim3(1), dim3(bpmf::kProbitTile), 0, st, p.partial, nblk, p.partial + 2 * nblk);
    return 0;
}

int ordinal_prob(const OrdinalProbLaunch &p, hipStream_t st)
{
    return dispatch_kt(p.f.K, p.f.f32, [&](auto k, auto t) {
        using T = decltype(t);
        if (p.nnz <= 0) return;
        hipLaunchKernelGGL((bpmf::k_ordinal_prob<decltype(k)::value, T>), dim3((unsigned)ordinal_blocks(p.nnz)), dim3(bpmf::kProbitTile), 0, st,
                           p.tcol, p.trow, p.nnz, (const T *)p.f.items, (const T *)p.f.other, p.f.kt, p.g, p.nlev, p.sum);
    });
}

}  // namespace bpmf_launch
