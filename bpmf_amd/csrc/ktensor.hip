// ktensor.hip -- launcher of the Khatri-Rao kernel of the tensor factorisation (kernels_tensor.h, see launch.h).
#include "launch.h"
#include "kernels_tensor.h"

namespace bpmf_launch {

template <int LD>
static void khatri_rao_launch(const KhatriRaoLaunch &p, hipStream_t st)
{
    // (events ride on the dispatch packet, as in BPMF_LAUNCH: no marker packet between this kernel and the sampler behind it)
    constexpr int epb = bpmf::kKhatriRaoBlock / (LD / 2);             // entries per workgroup
    hipExtLaunchKernelGGL((bpmf::k_khatri_rao<LD>), dim3((unsigned)((p.n + epb - 1) / epb)), dim3(bpmf::kKhatriRaoBlock), 0, st, p.ev_start,
                          p.ev_stop, 0, p.A, p.B, p.ia, p.ib, p.n, p.kt, p.P);
}

int khatri_rao(const KhatriRaoLaunch &p, hipStream_t st)
{
    if (p.n <= 0) return 0;
    switch (p.ld) {
    case 8: khatri_rao_launch<8>(p, st); break;
    case 16: khatri_rao_launch<16>(p, st); break;
    case 32: khatri_rao_launch<32>(p, st); break;
    case 64: khatri_rao_launch<64>(p, st); break;
    case 128: khatri_rao_launch<128>(p, st); break;
    default: return -1;
    }
    return 0;
}

}  // namespace bpmf_launch
