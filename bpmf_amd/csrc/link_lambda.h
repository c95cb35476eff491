// link_lambda.h -- the sampled link precision lambda_beta and the device-factor mode of a side with dense features
// (capi_link_lambda.hip, kernels_link_chol.h).
#pragma once
#include "launch.h"

namespace bpmf_capi {

// Puts a side with dense features into device-factor mode (no-op if it is there, or if the features are sparse): forms F^T F on
// the device by the column tiles of k_link_gemm_tn, allocates the work arrays of the factorisation, releases W.
int link_chol_enter(bpmf_hip_side *s);
// beta = L^-T (L^-1 P + E) with G(lambda) = L L^T, [P ; E] = the side's stacked right-hand side; factors G only when lambda has
// changed since the last factorisation.  Waits for the pivot flag: BPMF_HIP_ENUM if G is not positive definite.
int link_chol_draw(bpmf_hip_side *s);
// The draw of lambda_beta at the start of half-iteration `iter` from the side's beta^T beta (btb: Kt x Kt, on the host) and the
// Lambda = R^T R the side's beta was drawn under (R = LU, upper triangular, column-major).  No draw at the side's first half-iteration.
int link_lambda_draw(bpmf_hip_side *s, const double *btb, int iter);
// C = A^T (B - 1 bvec^T) through the column tiles of k_link_gemm_tn (capi_link.hip)
int link_tn_product(const double *A, int64_t lda, const double *B, int64_t ldb, const double *bvec, int64_t N, int D, int n, double *C,
                    int64_t ldc, double *part, hipStream_t st);

}  // namespace bpmf_capi
