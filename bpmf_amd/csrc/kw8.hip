// kw8.hip -- num_latent = 8 with per-rating weights: k_sample1w<8> and k_sample4w<8> (kernels.h, kernels_q4.h).
// A unit of its own, like every weighted form (see k128_f64w.hip).
#include "launch_w.h"

BPMF_INSTANTIATE_KW(8)
