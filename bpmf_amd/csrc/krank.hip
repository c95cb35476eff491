// krank.hip -- launcher of the held-out rank kernels (kernels_rank.h, see launch.h).
#include "launch.h"
#include "kernels_rank.h"

namespace bpmf_launch {

void rank_eval(const RankLaunch &p, hipStream_t st)
{
    bpmf::RankArgs a;
    a.qring = p.r.qring; a.cring = p.r.cring; a.qstride = p.r.qstride; a.cstride = p.r.cstride;
    a.L = p.r.S * p.r.Kp; a.S = p.r.S; a.mean_rating = p.mean_rating;
    a.q_from = p.q_from; a.nq = p.nq; a.nc = p.nc; a.cspan = p.cspan;
    a.ex_ptr = p.ex_ptr; a.ex_rows = p.ex_rows; a.tptr = p.tptr; a.tcand = p.tcand; a.nt = p.nt;
    a.tscore = p.tscore; a.part_cnt = p.part_cnt; a.part_ncand = p.part_ncand;
    const size_t lds = sizeof(double) * ((size_t)bpmf::kRankQ * bpmf::kRankScLd + bpmf::kRankQ);
    const dim3 grid((unsigned)((p.nq + bpmf::kRankQ - 1) / bpmf::kRankQ), (unsigned)p.nsplit);
    if (p.nt > 0) {
        (void)hipMemsetAsync(p.part_cnt, 0, (size_t)p.nsplit * (size_t)p.nt * sizeof(int32_t), st);
        hipLaunchKernelGGL(bpmf::k_rank_eval<false>, grid, dim3(256), lds, st, a);
    }
    hipLaunchKernelGGL(bpmf::k_rank_eval<true>, grid, dim3(256), lds, st, a);
    const int64_t n = p.nt > p.nq ? p.nt : p.nq;
    hipLaunchKernelGGL(bpmf::k_rank_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p.part_cnt, p.part_ncand, p.nsplit, p.nt, p.nq,
                       p.rank, p.ncand);
}

}  // namespace bpmf_launch
