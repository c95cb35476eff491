// ktensor.hip -- launcher of the Khatri-Rao kernel of the tensor factorisation (kernels_tensor.h, see launch.h).
#include "launch.h"
#include "kernels_tensor.h"

namespace bpmf_launch {

int khatri_rao(const KhatriRaoLaunch &p, hipStream_t st)
{
    if (p.n <= 0) return 0;
    return dispatch_k(p.ld, [&](auto ld) {
        // (events ride on the dispatch packet, as in BPMF_LAUNCH: no marker packet between this kernel and the sampler behind it)
        constexpr int LD = decltype(ld)::value, epb = bpmf::kKhatriRaoBlock / (LD / 2);            // entries per workgroup
        hipExtLaunchKernelGGL((bpmf::k_khatri_rao<LD>), dim3((unsigned)((p.n + epb - 1) / epb)), dim3(bpmf::kKhatriRaoBlock), 0, st, p.ev_start,
                              p.ev_stop, 0, p.A, p.B, p.ia, p.ib, p.n, p.kt, p.P);
    });
}

}  // namespace bpmf_launch
