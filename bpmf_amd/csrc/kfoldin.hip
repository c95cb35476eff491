// kfoldin.hip -- launcher of the fold-in kernel (kernels_foldin.h, see launch.h).
#include "launch.h"
#include "kernels_foldin.h"

namespace bpmf_launch {

int foldin_chunk() { return bpmf::kFoldinChunk; }

template <int KP>
static void foldin_launch(const bpmf::FoldinArgs &a, int64_t items, hipStream_t st)
{
    hipLaunchKernelGGL(bpmf::k_foldin<KP>, dim3((unsigned)items), dim3(KP <= 32 ? 64 : 256), 0, st, a);
}

int foldin(const FoldinLaunch &p, hipStream_t st)
{
    if (p.kt < 1 || p.kt > p.K || p.kp != (p.kt + 3) / 4 * 4 || p.S < 1 || p.n_new < 1 || p.cstride < (int64_t)p.S * p.kp) return -1;
    const int64_t items = p.n_new * p.S;
    if (items > 0x7fffffff) return -1;
    bpmf::FoldinArgs a;
    a.rowptr = p.rowptr; a.colidx = p.colidx; a.vals = p.vals; a.cring = p.cring; a.cstride = p.cstride;
    a.alpha = p.alpha; a.lam = p.lam; a.lmu = p.lmu; a.mean_rating = p.mean_rating; a.S = p.S; a.kt = p.kt; a.kp = p.kp;
    a.tag = p.tag; a.draw = p.draw; a.out = p.out; a.fail = p.fail;
    switch (p.K) {
    case 8: foldin_launch<8>(a, items, st); return 0;
    case 16: foldin_launch<16>(a, items, st); return 0;
    case 32: foldin_launch<32>(a, items, st); return 0;
    case 64: foldin_launch<64>(a, items, st); return 0;
    case 128: foldin_launch<128>(a, items, st); return 0;
    }
    return -1;
}

}  // namespace bpmf_launch
