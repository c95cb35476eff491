// k128_f64w.hip -- num_latent = 128 in fp64 with per-rating weights: k_sample_wg2w<128, 4, double> (kernels_wg2.h).
// A unit of its own, like every weighted form: the units of the unweighted kernels compile exactly what they compiled before.
#include "launch.h"
#include "kernels_wg2.h"

namespace bpmf_launch {

void k128_wg2w_f64(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a, const bpmf::StatRiders &r)
{
    grid += r.nblocks;                                              // (riders: ahead of the items)
    BPMF_LAUNCH((bpmf::k_sample_wg2w<128, 4, double>), dim3(grid), dim3(256), st, e0, e1, a, r);
}

}  // namespace bpmf_launch
