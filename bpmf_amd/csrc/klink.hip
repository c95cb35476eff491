// klink.hip -- launchers of the side-information kernels (kernels_link.h, see launch.h).
#include "launch.h"
#include "kernels_link.h"

namespace bpmf_launch {

int64_t link_chunks(int64_t N) { return (N + bpmf::kLinkChunk - 1) / bpmf::kLinkChunk; }
size_t link_tn_part_words(int64_t N, int D, int n) { return (size_t)std::max<int64_t>(link_chunks(N), 1) * (size_t)D * (size_t)n; }
int link_shift_blocks(int64_t total) { return (int)((total + bpmf::kLinkShiftBlock - 1) / bpmf::kLinkShiftBlock); }

// tiles of 16 columns a wave carries: the smallest instantiated count that covers n
static int tiles_for(int n) { return n <= 16 ? 1 : n <= 32 ? 2 : n <= 64 ? 4 : 8; }

template <int NT>
static void tn_launch(const LinkTnLaunch &p, dim3 grid, int wgc, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_link_gemm_tn<NT>), grid, dim3(256), 0, st, p.A, p.lda, p.B, p.ldb, p.bvec, p.N, p.D, p.n, wgc, p.part);
}

int link_gemm_tn(const LinkTnLaunch &p, hipStream_t st)
{
    if (p.N < 0 || p.D < 1 || p.n < 1 || p.n > 128 || !p.part) return -1;
    const int64_t nchunks = link_chunks(p.N);
    if (nchunks > 0) {
        // BPMF_LINK_WG_CHUNKS (read at every launch; the tests flip it): chunks one workgroup computes one after the other.  It
        // changes the grid, never the chunks or the order in which their partials are added.
        const int wgc = std::max(1, env_int("BPMF_LINK_WG_CHUNKS", 1));
        const dim3 grid((unsigned)((p.D + bpmf::kLinkRows - 1) / bpmf::kLinkRows), (unsigned)((nchunks + wgc - 1) / wgc));
        switch (tiles_for(p.n)) {
        case 1: tn_launch<1>(p, grid, wgc, st); break;
        case 2: tn_launch<2>(p, grid, wgc, st); break;
        case 4: tn_launch<4>(p, grid, wgc, st); break;
        default: tn_launch<8>(p, grid, wgc, st); break;
        }
    }
    const int64_t tot = (int64_t)p.D * p.n;
    hipLaunchKernelGGL(bpmf::k_link_sum_chunks, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, p.part, nchunks, p.D, p.n, p.C, p.ldc);
    return 0;
}

template <int NT>
static void nn_launch(const LinkNnLaunch &p, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_link_gemm_nn<NT>), dim3((unsigned)((p.N + bpmf::kLinkRows - 1) / bpmf::kLinkRows)), dim3(256), 0, st, p.A, p.lda,
                       p.B, p.ldb, p.N, p.Dr, p.n, p.C, p.ldc, p.ncw);
}

int link_gemm_nn(const LinkNnLaunch &p, hipStream_t st)
{
    if (p.N < 0 || p.Dr < 1 || p.n < 1 || p.ncw < p.n || p.ncw > 128 || p.ldc < p.ncw) return -1;
    if (p.N == 0) return 0;
    switch (tiles_for(p.ncw)) {
    case 1: nn_launch<1>(p, st); break;
    case 2: nn_launch<2>(p, st); break;
    case 4: nn_launch<4>(p, st); break;
    default: nn_launch<8>(p, st); break;
    }
    return 0;
}

int link_residual(const LinkResidualLaunch &p, hipStream_t st)
{
    if (p.m.nnz <= 0) return 0;
    const unsigned grid = (unsigned)((p.m.nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile);
    return dispatch_k(p.K, [&](auto k) {
        hipLaunchKernelGGL((bpmf::k_link_residual<decltype(k)::value>), dim3(grid), dim3(bpmf::kProbitTile), 0, st, p.m.colptr, p.m.ncols, p.m.rowidx,
                           p.vals, p.m.nnz, p.offs, p.other, p.kt, p.out);
    });
}

void link_shift(double *items, const double *offs, int64_t total, double *partial, hipStream_t st)
{
    if (total <= 0) return;
    hipLaunchKernelGGL(bpmf::k_link_shift, dim3((unsigned)link_shift_blocks(total)), dim3(256), 0, st, items, offs, total, partial);
}

}  // namespace bpmf_launch
