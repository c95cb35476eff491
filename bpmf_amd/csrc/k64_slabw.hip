// k64_slabw.hip -- K = 64 fp64 with per-rating weights: k_sample_slabw<64, double> and its fused twin k_sample1sw<64>
// (kernels_slab.h).  A unit of its own, like every weighted form (see k128_f64w.hip).
#include "launch.h"
#include "kernels_slab.h"

namespace bpmf_launch {

void k64_slabw(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a)
{
    BPMF_LAUNCH((bpmf::k_sample_slabw<64, double>), dim3(grid), dim3(64), st, e0, e1, a);
}

void k64_1sw(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a, const bpmf::FusedArgs &f)
{
    BPMF_LAUNCH(bpmf::k_sample1sw<64>, dim3(grid), dim3(64), st, e0, e1, a, f);
}

}  // namespace bpmf_launch
