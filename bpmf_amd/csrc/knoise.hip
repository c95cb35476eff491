// knoise.hip -- launchers of the training-residual reduction (kernels_noise.h, see launch.h).
#include "launch.h"
#include "kernels_noise.h"

namespace bpmf_launch {

int train_sse_blocks(int64_t nnz, int num_cu)
{
    // ~256 ratings per workgroup, at most 16 workgroups per CU (the partials stay a few KB)
    return (int)std::max<int64_t>(1, std::min<int64_t>((nnz + 255) / 256, (int64_t)num_cu * 16));
}

template <int K, typename T>
static void sse_launch(const SseLaunch &p, int64_t span, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_train_sse<K, T>), dim3((unsigned)p.nblk), dim3(bpmf::kSseThreads), 0, st, p.colptr, p.ncols, p.rowidx,
                       p.vals, p.nnz, span, (const T *)p.items, (const T *)p.other, p.kt, p.mean, p.partial);
}

int train_sse(const SseLaunch &p, hipStream_t st)
{
    if (p.nnz <= 0 || p.nblk < 1) return -1;
    const int64_t span = (p.nnz + p.nblk - 1) / p.nblk;
    if (p.f32) {
        if (p.K != 128) return -1;
        sse_launch<128, float>(p, span, st);
    } else {
        switch (p.K) {
        case 8: sse_launch<8, double>(p, span, st); break;
        case 16: sse_launch<16, double>(p, span, st); break;
        case 32: sse_launch<32, double>(p, span, st); break;
        case 64: sse_launch<64, double>(p, span, st); break;
        case 128: sse_launch<128, double>(p, span, st); break;
        default: return -1;
        }
    }
    hipLaunchKernelGGL(bpmf::k_train_sse_final, dim3(1), dim3(bpmf::kSseThreads), 0, st, p.partial, p.nblk, p.partial + p.nblk);
    return 0;
}

}  // namespace bpmf_launch
