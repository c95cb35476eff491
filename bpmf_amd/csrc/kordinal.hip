// kordinal.hip -- launchers of the ordinal probit kernels (kernels_ordinal.h, see launch.h).
#include "launch.h"
#include "kernels_ordinal.h"

namespace bpmf_launch {

int64_t ordinal_blocks(int64_t nnz) { return (nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile; }

template <int K, typename T>
static void latent_launch(const OrdinalLatentLaunch &p, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_ordinal_latent<K, T>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.colptr, p.ncols, p.rowidx, p.level,
                       p.nnz, (const T *)p.items, (const T *)p.other, p.kt, p.iter, p.tag, p.g, p.nlev, p.z, p.fail);
}

template <int K, typename T>
static void loglik_launch(const OrdinalLoglikLaunch &p, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_ordinal_loglik<K, T>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.colptr, p.ncols, p.rowidx, p.level,
                       p.nnz, (const T *)p.items, (const T *)p.other, p.kt, p.g0, p.g1, p.nlev, p.partial);
}

template <int K, typename T>
static void prob_launch(const OrdinalProbLaunch &p, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_ordinal_prob<K, T>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.tcol, p.trow, p.nnz,
                       (const T *)p.items, (const T *)p.other, p.kt, p.g, p.nlev, p.sum);
}

// (the K / type set of kprobit.hip)
#define BPMF_ORDINAL_DISPATCH(fn)                                      \
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

static bool ordinal_k_ok(bool f32, int K) { return f32 ? K == 128 : (K == 8 || K == 16 || K == 32 || K == 64 || K == 128); }

int ordinal_latent(const OrdinalLatentLaunch &p, hipStream_t st)
{
    if (!ordinal_k_ok(p.f32, p.K)) return -1;
    if (p.nnz <= 0) return 0;
    const unsigned grid = (unsigned)ordinal_blocks(p.nnz);
    BPMF_ORDINAL_DISPATCH(latent_launch)
    return 0;
}

int ordinal_loglik(const OrdinalLoglikLaunch &p, hipStream_t st)
{
    if (!ordinal_k_ok(p.f32, p.K)) return -1;
    const int64_t nblk = ordinal_blocks(p.nnz);
    if (p.nnz > 0) {
        const unsigned grid = (unsigned)nblk;
        BPMF_ORDINAL_DISPATCH(loglik_launch)
    }
    hipLaunchKernelGGL(bpmf::k_ordinal_loglik_final, dim3(1), dim3(bpmf::kProbitTile), 0, st, p.partial, nblk, p.partial + 2 * nblk);
    return 0;
}

int ordinal_prob(const OrdinalProbLaunch &p, hipStream_t st)
{
    if (!ordinal_k_ok(p.f32, p.K)) return -1;
    if (p.nnz <= 0) return 0;
    const unsigned grid = (unsigned)ordinal_blocks(p.nnz);
    BPMF_ORDINAL_DISPATCH(prob_launch)
    return 0;
}

}  // namespace bpmf_launch
