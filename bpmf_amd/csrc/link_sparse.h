// link_sparse.h -- host side of the sparse side information (kernels_link_sparse.h, klinksp.hip, capi_link_sparse.hip; DESIGN.md
// section 14): a compressed matrix on the device, the work arrays of a conjugate-gradient solve, the launchers.
#pragma once
#include "launch.h"

namespace bpmf { struct CgState; }

namespace bpmf_launch {

// A matrix compressed by rows on the device (F by rows, or F^T by rows = F by columns).  Rows of more than kSpChunk nonzeros are
// "long": cut into chunks whose partial sums are added in chunk order.
struct SpMat {
    int64_t nrows = 0, nnz = 0;
    int64_t *d_ptr = nullptr;
    int32_t *d_idx = nullptr;
    double *d_vals = nullptr;                               // NULL: every stored value is 1
    int nlong = 0; int64_t nchunks = 0;
    int32_t *d_lrow = nullptr; int64_t *d_lfirst = nullptr, *d_cbeg = nullptr, *d_cend = nullptr;
    double *d_part = nullptr; int part_n = 0;               // nchunks x part_n doubles
};
// uploads ptr / idx / vals (vals may be NULL) and the long-row lists; max_n: the widest dense operand the matrix will meet
int sp_upload(SpMat &m, int64_t nrows, const int64_t *ptr, const int32_t *idx, const double *vals, int max_n);
void sp_free(SpMat &m);
// C (nrows x ncw, leading dimension ldc) = m V (+ lambda P), V: ? x n (leading dimension ldv); columns n .. ncw - 1 zero.
// -1: shape not supported (nothing launched)
int sp_product(const SpMat &m, const double *V, int64_t ldv, int n, int ncw, double *C, int64_t ldc, double lambda, const double *P,
               int64_t ldp, hipStream_t st);

// the work arrays of K solves in lockstep on D x ld arrays
struct CgWork {
    double *d_p = nullptr, *d_q = nullptr, *d_t = nullptr;  // D x ld, D x ld, N x ld
    double *d_partial = nullptr;                            // cg_blocks(D) x 128
    bpmf::CgState *d_state = nullptr;
    int *h_word = nullptr;                                  // pinned: the number of active columns, written by the device
};
int cg_alloc(CgWork &w, int64_t N, int64_t D, int64_t ld, bool with_t);
void cg_free(CgWork &w);
int64_t cg_blocks(int64_t D);
struct CgResult { int iters[128]; int iters_max = 0; double relres_max = 0.0; int hit_max_iter = 0; };
// (F^T F + lambda I) x = r from x = 0; r holds the right-hand side on entry and the recursion residual on exit.  Blocks.
int cg_solve(const SpMat &F, const SpMat &Ft, double lambda, double *x, double *r, int64_t ld, int n, int64_t D, double tol, int max_iter,
             CgWork &w, hipStream_t st, CgResult *res);

int noise_rows(int64_t nrows, int kt, uint32_t it, uint32_t key1, const double *d_Rinv, const double *d_base, int64_t ldb, const double *d_bvec,
               double scale, double *d_out, int64_t ldo, hipStream_t st);

}  // namespace bpmf_launch

// what a side with sparse features owns (bpmf_hip_side::link_sp)
struct bpmf_link_sparse {
    bpmf_launch::SpMat F, Ft;
    bpmf_launch::CgWork cg;
    double *d_rhs = nullptr, *d_rinv = nullptr;             // D x K: right-hand side, then residual; Kt x Kt
    double tol = 1e-6; int max_iter = 1000;
    int iters_last = 0; int64_t iters_total = 0; double relres_max_last = 0.0; int hit_max_iter = 0;
};

namespace bpmf_capi {
int link_sparse_draw(bpmf_hip_side *s, const double *mu, const double *LU, int iter);     // steps 2' and 3' of a half-iteration
int link_sparse_offsets(bpmf_hip_side *s);                                                  // M = F beta
void link_sparse_free(bpmf_hip_side *s);
}
