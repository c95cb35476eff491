// link_sparse.h -- host side of the sparse side information (kernels_link_sparse.h, klinksp.hip, capi_link_sparse.hip; DESIGN.md
// section 14): the launchers on a compressed matrix (SpMat) and the work arrays of a conjugate-gradient solve (CgWork), both in
// ext_state.h.
#pragma once
#include "launch.h"

namespace bpmf_launch {

// uploads ptr / idx / vals (vals may be NULL) and the long-row lists; max_n: the widest dense operand the matrix will meet
int sp_upload(SpMat &m, int64_t nrows, const int64_t *ptr, const int32_t *idx, const double *vals, int max_n);
// C (nrows x ncw, leading dimension ldc) = m V (+ lambda P), V: ? x n (leading dimension ldv); columns n .. ncw - 1 zero.
// -1: shape not supported (nothing launched)
int sp_product(const SpMat &m, const double *V, int64_t ldv, int n, int ncw, double *C, int64_t ldc, double lambda, const double *P,
               int64_t ldp, hipStream_t st);

int cg_alloc(CgWork &w, int64_t N, int64_t D, int64_t ld, bool with_t);
int64_t cg_blocks(int64_t D);
struct CgResult { int iters[128]; int iters_max = 0; double relres_max = 0.0; int hit_max_iter = 0; };
// (F^T F + lambda I) x = r from x = 0; r holds the right-hand side on entry and the recursion residual on exit.  Blocks.
int cg_solve(const SpMat &F, const SpMat &Ft, double lambda, double *x, double *r, int64_t ld, int n, int64_t D, double tol, int max_iter,
             CgWork &w, hipStream_t st, CgResult *res);

int noise_rows(int64_t nrows, int kt, uint32_t it, uint32_t key1, const double *d_Rinv, const double *d_base, int64_t ldb, const double *d_bvec,
               double scale, double *d_out, int64_t ldo, hipStream_t st);

}  // namespace bpmf_launch

namespace bpmf_capi {
int link_sparse_draw(bpmf_hip_side *s, const double *mu, const double *LU, int iter);     // steps 2' and 3' of a half-iteration
int link_sparse_offsets(bpmf_hip_side *s);                                                  // M = F beta
}
