// ktopnscore.hip -- launcher of the scored top-N kernels (kernels_topn_score.h, see launch.h).
#include <limits>

#include "launch.h"
#include "kernels_topn_score.h"

namespace bpmf_launch {

namespace {

template <int KIND, bool NOISY>
int launch_scored(const bpmf::TopnScoredArgs &a, dim3 grid, size_t lds, hipStream_t st)
{
    auto kern = bpmf::k_topn_scored<KIND, NOISY>;
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

int topn_scored(const TopnScoredLaunch &p, hipStream_t st)
{
    if (!ring_pair_ok(p.r) || p.n < 1 || p.n > bpmf::kTsMaxN || p.nq < 1 || p.nc < 1 || p.cspan < 1 || p.cspan % bpmf::kTsC != 0 || p.nsplit < 1 ||
        p.nsplit > 65535)
        return -1;
    bpmf::TopnScoredArgs a;
    a.qring = p.r.qring; a.cring = p.r.cring; a.qstride = p.r.qstride; a.cstride = p.r.cstride;
    a.Kp = p.r.Kp; a.S = p.r.S; a.n = p.n; a.mean_rating = p.mean_rating; a.param = p.param; a.sigma = p.sigma;
    a.q_from = p.q_from; a.nq = p.nq; a.nc = p.nc; a.cspan = p.cspan;
    a.ex_ptr = p.ex_ptr; a.ex_rows = p.ex_rows;
    a.part_score = p.part_score; a.part_mean = p.part_mean; a.part_std = p.part_std; a.part_idx = p.part_idx;
    const size_t lds = bpmf::topn_scored_lds(p.n);
    const int64_t nqb = (p.nq + bpmf::kTsQ - 1) / bpmf::kTsQ;
    if (nqb > 0x7fffffff) return -1;
    const dim3 grid((unsigned)nqb, (unsigned)p.nsplit);
    // a sigma below the smallest normal double is the sigma = 0 form: 1 / sigma would overflow and 0 * inf poison p_s == t
    const bool noisy = p.sigma >= std::numeric_limits<double>::min();
    int rc;
    switch (p.kind) {
    case bpmf::kScoreUcb: rc = launch_scored<bpmf::kScoreUcb, false>(a, grid, lds, st); break;
    case bpmf::kScoreProb:
        rc = noisy ? launch_scored<bpmf::kScoreProb, true>(a, grid, lds, st) : launch_scored<bpmf::kScoreProb, false>(a, grid, lds, st);
        break;
    case bpmf::kScoreEi:
        rc = noisy ? launch_scored<bpmf::kScoreEi, true>(a, grid, lds, st) : launch_scored<bpmf::kScoreEi, false>(a, grid, lds, st);
        break;
    default: return -1;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(bpmf::k_topn_scored_merge, dim3((unsigned)((p.nq + 255) / 256)), dim3(256), 0, st, p.part_score, p.part_mean, p.part_std,
                       p.part_idx, p.nsplit, p.nq, p.n, p.out_score, p.out_mean, p.out_std, p.out_idx);
    return 0;
}

}  // namespace bpmf_launch
