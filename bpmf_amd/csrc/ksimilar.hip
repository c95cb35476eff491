// ksimilar.hip -- launchers of the similar-columns kernels (kernels_similar.h, see launch.h).
#include "launch.h"
#include "kernels_similar.h"

namespace bpmf_launch {

namespace {

bool ring_shape_ok(int Kp, int S, int64_t stride, int64_t ncols)
{
    return Kp >= 4 && Kp <= 128 && Kp % 4 == 0 && S >= 1 && ncols >= 1 && stride >= (int64_t)S * Kp;
}

template <int KIND>
int launch_topn(const bpmf::SimilarArgs &a, dim3 grid, size_t lds, hipStream_t st)
{
    auto kern = bpmf::k_similar_topn<KIND>;
    // more than the default 64 KB of dynamic LDS (lists of n > 13): asked for explicitly
    if (lds > 65536 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return -2;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
    return 0;
}

}  // namespace

int ring_norms(const double *ring, int64_t stride, int Kp, int S, int64_t ncols, double *tab, hipStream_t st)
{
    if (!ring_shape_ok(Kp, S, stride, ncols)) return -1;
    const int64_t nb = (ncols * S + 255) / 256;
    if (nb > 0x7fffffff) return -1;
    hipLaunchKernelGGL(bpmf::k_ring_norms, dim3((unsigned)nb), dim3(256), 0, st, ring, stride, Kp, S, ncols, tab);
    return 0;
}

int similar_topn(const SimilarLaunch &p, hipStream_t st)
{
    if (!ring_shape_ok(p.Kp, p.S, p.stride, p.nc) || p.n < 1 || p.n > bpmf::kSimMaxN || p.nq < 1 || p.q_from < 0 || p.q_from + p.nq > p.nc ||
        p.nc > 0x7fffffff || p.cspan < 1 || p.cspan % bpmf::kSimC != 0 || p.nsplit < 1 || p.nsplit > 65535 ||
        (int64_t)p.nsplit * p.cspan < p.nc || (int64_t)(p.nsplit - 1) * p.cspan >= p.nc)
        return -1;
    bpmf::SimilarArgs a;
    a.ring = p.ring; a.stride = p.stride; a.tab = p.tab; a.Kp = p.Kp; a.S = p.S; a.n = p.n; a.kappa = p.kappa;
    a.q_from = p.q_from; a.nq = p.nq; a.nc = p.nc; a.cspan = p.cspan; a.cand_ok = p.cand_ok;
    a.part_score = p.part_score; a.part_mean = p.part_mean; a.part_std = p.part_std; a.part_idx = p.part_idx;
    const size_t lds = bpmf::similar_lds(p.n);
    const int64_t nqb = (p.nq + bpmf::kSimQ - 1) / bpmf::kSimQ;
    if (nqb > 0x7fffffff) return -1;
    const dim3 grid((unsigned)nqb, (unsigned)p.nsplit);
    int rc;
    switch (p.kind) {
    case bpmf::kSimCosine: rc = launch_topn<bpmf::kSimCosine>(a, grid, lds, st); break;
    case bpmf::kSimEuclid: rc = launch_topn<bpmf::kSimEuclid>(a, grid, lds, st); break;
    default: return -1;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(bpmf::k_similar_merge, dim3((unsigned)((p.nq + 255) / 256)), dim3(256), 0, st, p.part_score, p.part_mean, p.part_std,
                       p.part_idx, p.nsplit, p.nq, p.n, p.out_score, p.out_mean, p.out_std, p.out_idx);
    return 0;
}

int similar_block(const SimilarBlockLaunch &p, hipStream_t st)
{
    if (!ring_shape_ok(p.Kp, p.S, p.stride, p.ncols) || p.nq < 0 || p.nc < 0 || p.q_from < 0 || p.c_from < 0 || p.q_from + p.nq > p.ncols ||
        p.c_from + p.nc > p.ncols)
        return -1;
    if (p.nq == 0 || p.nc == 0) return 0;
    const int64_t gx = (p.nq + bpmf::kPredTile - 1) / bpmf::kPredTile, gy = (p.nc + bpmf::kPredTile - 1) / bpmf::kPredTile;
    if (gx > 0x7fffffff || gy > 65535) return -1;
    bpmf::SimilarBlockArgs a;
    a.ring = p.ring; a.stride = p.stride; a.tab = p.tab; a.Kp = p.Kp; a.S = p.S;
    a.q_from = p.q_from; a.nq = p.nq; a.c_from = p.c_from; a.nc = p.nc; a.mean = p.mean; a.std = p.std;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    switch (p.kind) {
    case bpmf::kSimCosine: hipLaunchKernelGGL(bpmf::k_similar_block<bpmf::kSimCosine>, grid, dim3(256), 0, st, a); break;
    case bpmf::kSimEuclid: hipLaunchKernelGGL(bpmf::k_similar_block<bpmf::kSimEuclid>, grid, dim3(256), 0, st, a); break;
    default: return -1;
    }
    return 0;
}

}  // namespace bpmf_launch
