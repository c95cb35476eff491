// kpredcells.hip -- launchers of the cell-list prediction and of the ring repacking (kernels_predcells.h, see launch.h).
#include "launch.h"
#include "kernels_predcells.h"

namespace bpmf_launch {

int predict_cells_segment(int Kp) { return bpmf::pc_segment(Kp); }

int predict_cells(const PredCellsLaunch &p, hipStream_t st)
{
    if (!ring_pair_ok(p.r) || p.nseg < 0 || p.nseg > 0x7fffffff) return -1;
    if (p.nseg == 0) return 0;
    bpmf::PredCellsArgs a;
    a.qring = p.r.qring; a.cring = p.r.cring; a.qstride = p.r.qstride; a.cstride = p.r.cstride; a.Kp = p.r.Kp; a.S = p.r.S;
    a.mean_rating = p.mean_rating; a.t = p.t; a.sigma = p.sigma;
    a.seg_q = p.seg_q; a.seg_beg = p.seg_beg; a.seg_cnt = p.seg_cnt; a.cand = p.cand; a.orig = p.orig;
    a.mean = p.mean; a.std = p.std; a.prob = p.prob;
    const dim3 grid((unsigned)p.nseg), block(256);
#define BPMF_PC_LAUNCH(G_)                                                                                              \
    case G_:                                                                                                            \
        if (p.want_prob) hipLaunchKernelGGL((bpmf::k_predict_cells<G_, true>), grid, block, 0, st, a);                  \
        else hipLaunchKernelGGL((bpmf::k_predict_cells<G_, false>), grid, block, 0, st, a);                             \
        break;
    switch (bpmf::pc_group(p.r.Kp)) {
    BPMF_PC_LAUNCH(2) BPMF_PC_LAUNCH(4) BPMF_PC_LAUNCH(8) BPMF_PC_LAUNCH(16) BPMF_PC_LAUNCH(32) BPMF_PC_LAUNCH(64)
    default: return -1;
    }
#undef BPMF_PC_LAUNCH
    return 0;
}

void samples_pack(const double *ring, int64_t stride, int Kp, int Kt, int64_t c_from, int64_t nc, int s_from, int n, double *packed,
                  hipStream_t st)
{
    const int64_t e = nc * n * Kt;
    if (e <= 0) return;
    hipLaunchKernelGGL(bpmf::k_samples_pack, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, st, ring, stride, Kp, Kt, c_from, nc, s_from, n, packed);
}

void samples_unpack(const double *packed, int64_t stride, int Kp, int Kt, int64_t c_from, int64_t nc, int n, double *ring, hipStream_t st)
{
    const int64_t e = nc * n * Kp;
    if (e <= 0) return;
    hipLaunchKernelGGL(bpmf::k_samples_unpack, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, st, packed, stride, Kp, Kt, c_from, nc, n, ring);
}

}  // namespace bpmf_launch
