// launch_w.h -- definitions of launch.h's sample1w / sample4w: the weighted forms of the K <= 32 samplers, instantiated one K
// per unit (kw8.hip, kw16.hip, kw32.hip).
#pragma once
#include "launch.h"
#include "kernels.h"
#include "kernels_q4.h"

namespace bpmf_launch {

template <int K>
void sample1w(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a, const bpmf::FusedArgs &f)
{
    BPMF_LAUNCH(bpmf::k_sample1w<K>, dim3(grid), dim3(64), st, e0, e1, a, f);
}

template <int K>
void sample4w(int grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const bpmf::SampleArgs &a)
{
    BPMF_LAUNCH(bpmf::k_sample4w<K>, dim3(grid), dim3(64), st, e0, e1, a);
}

}  // namespace bpmf_launch

#define BPMF_INSTANTIATE_KW(KK)                                                                                                             \
    template void bpmf_launch::sample1w<KK>(int, hipStream_t, hipEvent_t, hipEvent_t, const bpmf::SampleArgs &, const bpmf::FusedArgs &); \
    template void bpmf_launch::sample4w<KK>(int, hipStream_t, hipEvent_t, hipEvent_t, const bpmf::SampleArgs &);
