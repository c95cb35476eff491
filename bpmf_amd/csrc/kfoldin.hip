// kfoldin.hip -- launcher of the fold-in kernel (kernels_foldin.h, see launch.h).
#include "launch.h"
#include "kernels_foldin.h"

namespace bpmf_launch {

int foldin_chunk() { return bpmf::kFoldinChunk; }

int foldin(const FoldinLaunch &p, hipStream_t st)
{
    if (p.kt < 1 || p.kt > p.K || p.kp != (p.kt + 3) / 4 * 4 || p.S < 1 || p.n_new < 1 || p.cstride < (int64_t)p.S * p.kp) return -1;
    const int64_t items = p.n_new * p.S;
    if (items > 0x7fffffff) return -1;
    bpmf::FoldinArgs a;
    a.rowptr = p.rowptr; a.colidx = p.colidx; a.vals = p.vals; a.cring = p.cring; a.cstride = p.cstride;
    a.alpha = p.alpha; a.lam = p.lam; a.lmu = p.lmu; a.mean_rating = p.mean_rating; a.S = p.S; a.kt = p.kt; a.kp = p.kp;
    a.tag = p.tag; a.draw = p.draw; a.out = p.out; a.fail = p.fail;
    return dispatch_k(p.K, [&](auto k) {
        constexpr int KP = decltype(k)::value;
        hipLaunchKernelGGL(bpmf::k_foldin<KP>, dim3((unsigned)items), dim3(KP <= 32 ? 64 : 256), 0, st, a);
    });
}

}  // namespace bpmf_launch
