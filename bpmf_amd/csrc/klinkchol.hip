// klinkchol.hip -- launchers of the device factorisation of G(lambda) and of the two blocked triangular solves
// (kernels_link_chol.h, see launch.h).
#include "launch.h"
#include "kernels_link_chol.h"

namespace bpmf_launch {

int link_chol_dp(int D) { return (D + bpmf::kCholBlock - 1) / bpmf::kCholBlock * bpmf::kCholBlock; }

int link_chol_factor(const LinkCholLaunch &p, hipStream_t st)
{
    if (p.D < 1 || p.D > 1024 || !p.FtF || !p.Lp || !p.Linv || !p.LinvT || !p.flag) return -1;
    const int dp = link_chol_dp(p.D), nb = dp / bpmf::kCholBlock;
    const int64_t tot = (int64_t)dp * dp;
    hipLaunchKernelGGL(bpmf::k_chol_form, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, p.FtF, p.D, p.lambda, p.Lp, dp);
    for (int j = 0; j < nb; ++j) {
        hipLaunchKernelGGL(bpmf::k_chol_diag, dim3(1), dim3(64), 0, st, p.Lp, dp, j, p.Linv, p.LinvT, p.flag);
        const unsigned m = (unsigned)(nb - 1 - j);
        if (m == 0) break;
        hipLaunchKernelGGL(bpmf::k_chol_panel, dim3(m), dim3(256), 0, st, p.Lp, dp, j, (const double *)p.LinvT);
        hipLaunchKernelGGL(bpmf::k_chol_trail, dim3(m, m), dim3(256), 0, st, p.Lp, dp, j);
    }
    return 0;
}

int link_chol_solve(const LinkCholSolveLaunch &p, hipStream_t st)
{
    if (p.D < 1 || p.D > 1024 || p.n < 1 || p.n > bpmf::kCholRhs || p.ncw < p.n || p.ncw > bpmf::kCholRhs || p.ldo < p.ncw || p.ldp < p.n ||
        (p.E && p.lde < p.n) || !p.P || !p.Xp || !p.Ep || !p.out)
        return -1;
    const int dp = link_chol_dp(p.D), nb = dp / bpmf::kCholBlock;
    const unsigned pg = (unsigned)(((int64_t)dp * bpmf::kCholRhs + 255) / 256);
    const unsigned cg = (unsigned)((p.n + bpmf::kCholSolveCols - 1) / bpmf::kCholSolveCols);
    hipLaunchKernelGGL(bpmf::k_chol_pack, dim3(pg), dim3(256), 0, st, p.P, p.ldp, p.D, p.n, p.Xp, dp);
    if (p.E) hipLaunchKernelGGL(bpmf::k_chol_pack, dim3(pg), dim3(256), 0, st, p.E, p.lde, p.D, p.n, p.Ep, dp);
    const double *E = p.E ? p.Ep : nullptr;
    for (int j = 0; j < nb; ++j)
        hipLaunchKernelGGL((bpmf::k_chol_solve<false>), dim3(cg), dim3(256), 0, st, p.Lp, dp, j, p.Linv, p.Xp, (const double *)nullptr);
    for (int j = nb - 1; j >= 0; --j)
        hipLaunchKernelGGL((bpmf::k_chol_solve<true>), dim3(cg), dim3(256), 0, st, p.Lp, dp, j, p.LinvT, p.Xp, E);
    const int64_t tot = (int64_t)p.D * p.ncw;
    hipLaunchKernelGGL(bpmf::k_chol_unpack, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const double *)p.Xp, p.D, p.n, p.out, p.ldo, p.ncw);
    return 0;
}

}  // namespace bpmf_launch
