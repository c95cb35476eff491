// knoise.hip -- launchers of the training-residual reduction (kernels_noise.h, see launch.h).
#include "launch.h"
#include "kernels_noise.h"

namespace bpmf_launch {

int train_sse_blocks(int64_t nnz, int num_cu)
{
    // ~256 ratings per workgroup, at most 16 workgroups per CU (the partials stay a few KB)
    return (int)std::max<int64_t>(1, std::min<int64_t>((nnz + 255) / 256, (int64_t)num_cu * 16));
}

int train_sse(const SseLaunch &p, hipStream_t st)
{
    if (p.m.nnz <= 0 || p.nblk < 1) return -1;
    const int64_t span = (p.m.nnz + p.nblk - 1) / p.nblk;
    const int rc = dispatch_kt(p.f.K, p.f.f32, [&](auto k, auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bpmf::k_train_sse<decltype(k)::value, T>), dim3((unsigned)p.nblk), dim3(bpmf::kSseThreads), 0, st, p.m.colptr, p.m.ncols,
                           p.m.rowidx, p.vals, p.m.nnz, span, (const T *)p.f.items, (const T *)p.f.other, p.f.kt, p.mean, p.partial);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(bpmf::k_train_sse_final, dim3(1), dim3(bpmf::kSseThreads), 0, st, p.partial, p.nblk, p.partial + p.nblk);
    return 0;
}

}  // namespace bpmf_launch
