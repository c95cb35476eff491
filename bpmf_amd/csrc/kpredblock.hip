// kpredblock.hip -- launchers of the prediction-block kernels (kernels_predblock.h, see launch.h).
#include "launch.h"
#include "kernels_predblock.h"

namespace bpmf_launch {

int predict_block(const PredBlockLaunch &p, hipStream_t st)
{
    if (!ring_pair_ok(p.r) || p.nq < 0 || p.nc < 0) return -1;
    if (p.nq == 0 || p.nc == 0) return 0;
    const int64_t gx = (p.nq + bpmf::kPredTile - 1) / bpmf::kPredTile, gy = (p.nc + bpmf::kPredTile - 1) / bpmf::kPredTile;
    if (gx > 0x7fffffff || gy > 65535) return -1;
    bpmf::PredBlockArgs a;
    a.qring = p.r.qring; a.cring = p.r.cring; a.qstride = p.r.qstride; a.cstride = p.r.cstride; a.Kp = p.r.Kp; a.S = p.r.S;
    a.mean_rating = p.mean_rating; a.q_from = p.q_from; a.nq = p.nq; a.c_from = p.c_from; a.nc = p.nc; a.w = p.w;
    a.mean = p.mean; a.std = p.std;
    hipLaunchKernelGGL(bpmf::k_predict_block, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, a);
    return 0;
}

void rowsq_add(const double *Y, int64_t ldy, int n, int64_t ncols, double *w, hipStream_t st)
{
    if (ncols <= 0) return;
    hipLaunchKernelGGL(bpmf::k_rowsq_add, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, st, Y, ldy, n, ncols, w);
}

void ring_add_mu(double *ring, int64_t stride, int slot, int Kp, int Kt, int64_t nrows, const double *mu, hipStream_t st)
{
    const int64_t n = nrows * Kt;
    if (n <= 0) return;
    hipLaunchKernelGGL(bpmf::k_ring_add_mu, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ring, stride, slot, Kp, Kt, nrows, mu);
}

}  // namespace bpmf_launch
