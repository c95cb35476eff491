// capi_link_sparse.hip -- side information with a sparse feature matrix (kernels in kernels_link_sparse.h):
// F is kept compressed by rows and by columns, the link matrix is drawn by K conjugate-gradient solves in lockstep on a
// noise-injected right-hand side whose normals are generated on the device.  bpmf_hip_link_sample (capi_link.hip) dispatches here
// for steps 2' and 3'; everything else of the half-iteration is shared with the dense path.
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"
#include "link_sparse.h"

using namespace bpmf_capi;
using bpmf_launch::SpMat;

namespace {

constexpr unsigned kTagLimit = 0x10000u;                               // key words tag + 0x10000 (Z1) and tag + 0x20000 (Z2)

bool sharded(const bpmf_hip_side *s) { return s->from != 0 || s->to != s->ncols || !s->bounds.empty(); }

template <typename T>
void free_dev(T *&p) { if (p) (void)hipFree(p); p = nullptr; }

// canonical CSR: rowptr[0] = 0, non-decreasing; column indices inside [0, D), strictly increasing within a row; finite values
int check_csr(const char *who, int64_t N, int64_t D, const int64_t *rowptr, const int32_t *colidx, const double *vals)
{
    const std::string w(who);
    if (!rowptr) return fail(BPMF_HIP_EINVAL, w + ": NULL argument");
    if (N < 0 || N > 0x7FFFFFFF) return fail(BPMF_HIP_EINVAL, w + ": the number of rows must fit 31 bits");
    if (D < 1 || D > 0x7FFFFFFF) return fail(BPMF_HIP_EINVAL, w + ": D must be >= 1");
    if (rowptr[0] != 0) return fail(BPMF_HIP_EINVAL, w + ": rowptr[0] must be 0");
    for (int64_t i = 0; i < N; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(BPMF_HIP_EINVAL, w + ": rowptr decreases at row " + std::to_string(i));
    if (rowptr[N] > 0 && !colidx) return fail(BPMF_HIP_EINVAL, w + ": NULL argument");
    for (int64_t i = 0; i < N; ++i)
        for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            if (colidx[p] < 0 || colidx[p] >= D) return fail(BPMF_HIP_EINVAL, w + ": column index outside [0, D) in row " + std::to_string(i));
            if (p > rowptr[i] && colidx[p] <= colidx[p - 1])
                return fail(BPMF_HIP_EINVAL, w + ": column indices of row " + std::to_string(i) + " are not sorted or hold a duplicate");
            if (vals && !std::isfinite(vals[p])) return fail(BPMF_HIP_EINVAL, w + ": feature " + std::to_string(p) + " is not finite");
        }
    return 0;
}

// F by columns: (D + 1) pointers, row numbers ascending within a column, the values in that order
void transpose_csr(int64_t N, int64_t D, const int64_t *rowptr, const int32_t *colidx, const double *vals, std::vector<int64_t> &cptr,
                   std::vector<int32_t> &ridx, std::vector<double> &cvals)
{
    const int64_t nnz = rowptr[N];
    cptr.assign((size_t)D + 1, 0);
    for (int64_t p = 0; p < nnz; ++p) ++cptr[(size_t)colidx[p] + 1];
    for (int64_t d = 0; d < D; ++d) cptr[(size_t)d + 1] += cptr[(size_t)d];
    ridx.resize((size_t)std::max<int64_t>(nnz, 1));
    if (vals) cvals.resize((size_t)std::max<int64_t>(nnz, 1));
    std::vector<int64_t> at(cptr.begin(), cptr.end() - 1);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            const int64_t q = at[(size_t)colidx[p]]++;
            ridx[(size_t)q] = (int32_t)i;
            if (vals) cvals[(size_t)q] = vals[p];
        }
}

int upload_both(SpMat &F, SpMat &Ft, int64_t N, int64_t D, const int64_t *rowptr, const int32_t *colidx, const double *vals, int max_n)
{
    static const int32_t none = 0;
    int rc = bpmf_launch::sp_upload(F, N, rowptr, colidx ? colidx : &none, vals, max_n);
    if (rc) return rc;
    std::vector<int64_t> cptr; std::vector<int32_t> ridx; std::vector<double> cvals;
    transpose_csr(N, D, rowptr, colidx, vals, cptr, ridx, cvals);
    rc = bpmf_launch::sp_upload(Ft, D, cptr.data(), ridx.data(), vals ? cvals.data() : nullptr, max_n);
    if (rc) bpmf_launch::sp_free(F);
    return rc;
}

}  // namespace

namespace bpmf_capi {

void link_sparse_free(bpmf_hip_side *s)
{
    bpmf_link_sparse *sp = s->link_sp;
    if (!sp) return;
    bpmf_launch::sp_free(sp->F); bpmf_launch::sp_free(sp->Ft); bpmf_launch::cg_free(sp->cg);
    free_dev(sp->d_rhs); free_dev(sp->d_rinv);
    delete sp;
    s->link_sp = nullptr;
}

int link_sparse_offsets(bpmf_hip_side *s)
{
    const bpmf_hip_ctx *c = s->ctx;
    if (bpmf_launch::sp_product(s->link_sp->F, s->d_link_beta, c->K, c->Kt, c->K, s->d_link_m, c->K, 0.0, nullptr, 0, c->stream))
        return fail(BPMF_HIP_EINVAL, "link: unsupported shape of the sparse product");
    HIP_TRY(hipGetLastError());
    return 0;
}

int link_sparse_draw(bpmf_hip_side *s, const double *mu, const double *LU, int iter)
{
    bpmf_hip_ctx *c = s->ctx;
    bpmf_link_sparse *sp = s->link_sp;
    const int K = c->K, Kt = c->Kt, D = s->link_d;
    const int64_t N = s->ncols;
    hipStream_t st = c->stream;
    // R^-1 (upper triangular, row-major) of Lambda = R^T R, R = LambdaU (upper, column-major): K^3 on the host
    std::vector<double> Rinv((size_t)Kt * Kt, 0.0), pad((size_t)K, 0.0);
    for (int col = 0; col < Kt; ++col)
        for (int i = col; i >= 0; --i) {
            double v = i == col ? 1.0 : 0.0;
            for (int j = i + 1; j <= col; ++j) v -= LU[(size_t)j * Kt + i] * Rinv[(size_t)j * Kt + col];
            Rinv[(size_t)i * Kt + col] = v / LU[(size_t)i * Kt + i];
        }
    memcpy(pad.data(), mu, sizeof(double) * Kt);
    HIP_TRY(hipMemcpyAsync(s->d_link_mu, pad.data(), sizeof(double) * K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sp->d_rinv, Rinv.data(), Rinv.size() * sizeof(double), hipMemcpyHostToDevice, st));
    // X = U - 1 mu^T + Z1 R^-T (N x K, in the work array of F p), E = sqrt(lambda) Z2 R^-T, RHS = F^T X + E
    int rc = bpmf_launch::noise_rows(N, Kt, (uint32_t)iter, s->link_tag + 0x10000u, sp->d_rinv, s->d_items, K, s->d_link_mu, 1.0, sp->cg.d_t, K, st);
    if (!rc) rc = bpmf_launch::noise_rows(D, Kt, (uint32_t)iter, s->link_tag + 0x20000u, sp->d_rinv, nullptr, 0, nullptr, std::sqrt(s->link_lambda),
                                          sp->d_rhs, K, st);
    if (!rc) rc = bpmf_launch::sp_product(sp->Ft, sp->cg.d_t, K, Kt, Kt, sp->d_rhs, K, 1.0, sp->d_rhs, K, st);
    if (rc) return fail(BPMF_HIP_EINVAL, "link_sample: unsupported shape of the sparse right-hand side");
    HIP_TRY(hipGetLastError());
    bpmf_launch::CgResult res;
    rc = bpmf_launch::cg_solve(sp->F, sp->Ft, s->link_lambda, s->d_link_beta, sp->d_rhs, K, Kt, D, sp->tol, sp->max_iter, sp->cg, st, &res);
    if (rc) return rc;
    sp->iters_last = res.iters_max; sp->iters_total += res.iters_max; sp->relres_max_last = res.relres_max;
    sp->hit_max_iter = res.hit_max_iter;
    return link_sparse_offsets(s);
}

}  // namespace bpmf_capi

extern "C" int bpmf_hip_side_set_features_sparse(bpmf_hip_side *s, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals,
                                                 double lambda_beta, unsigned tag)
{
    if (!s || !rowptr) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: NULL argument");
    bpmf_hip_ctx *c = s->ctx;
    if (s->d_link_f) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: the side has features already");
    if (D < 1) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: D must be >= 1");
    if (!(lambda_beta > 0.0) || !std::isfinite(lambda_beta)) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: lambda_beta must be positive and finite");
    if (tag == 0) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: tag must be >= 1 (key word 0 belongs to the samplers' streams)");
    if (tag >= kTagLimit) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: tag must be < 0x10000 (the noise streams use tag + 0x10000 and tag + 0x20000)");
    if (c->dtype != BPMF_HIP_F64) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: not on an fp32 context");
    if (c->comm || sharded(s)) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: needs the side whole on one GPU, on a context without a communicator");
    if (s->reduce_on) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: not together with the BPMF_REDUCE formulation");
    if (s->d_probit_z) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: not on a probit side");
    if (s->d_prop) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: not together with propagated priors");
    const int64_t N = s->ncols;
    { const int rc = check_csr("side_set_features_sparse", N, D, rowptr, colidx, vals); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = settle_async(s); if (rc) return rc; }
    const int K = c->K, Kt = c->Kt;
    const size_t ld = (size_t)K;
    bpmf_link_sparse *sp = new bpmf_link_sparse();
    s->link_sp = sp;
    int rc = upload_both(sp->F, sp->Ft, N, D, rowptr, colidx, vals, Kt);
    if (!rc) rc = bpmf_launch::cg_alloc(sp->cg, N, D, (int64_t)ld, true);
    const size_t part_words = bpmf_launch::link_tn_part_words(D, Kt, Kt);
    const int nblk = std::max(bpmf_launch::link_shift_blocks((int64_t)N * K), bpmf_launch::link_shift_blocks((int64_t)D * K));
    if (!rc) rc = dev_upload<double>(&s->d_link_f, nullptr, 1);                                   // (the mark of a side with features)
    if (!rc) rc = dev_upload<double>(&sp->d_rhs, nullptr, (size_t)D * ld);
    if (!rc) rc = dev_upload<double>(&sp->d_rinv, nullptr, (size_t)Kt * Kt);
    if (!rc) rc = dev_upload<double>(&s->d_link_beta, nullptr, (size_t)D * ld);
    if (!rc) rc = dev_upload<double>(&s->d_link_beta_sum, nullptr, (size_t)D * ld);
    if (!rc) rc = dev_upload<double>(&s->d_link_m, nullptr, (size_t)N * ld);
    if (!rc) rc = dev_upload<double>(&s->d_link_r, nullptr, (size_t)s->nnz);
    if (!rc) rc = dev_upload<double>(&s->d_link_part, nullptr, part_words);
    if (!rc) rc = dev_upload<double>(&s->d_link_mu, nullptr, ld);
    if (!rc) rc = dev_upload<double>(&s->d_link_btb, nullptr, (size_t)Kt * Kt);
    if (!rc) rc = dev_upload<double>(&s->d_link_norm, nullptr, (size_t)nblk);
    if (!rc) rc = dev_upload(&s->d_link_colptr, s->h_colptr.data(), s->h_colptr.size());
    if (!rc) {
        hipError_t e = hipMemsetAsync(s->d_link_beta, 0, std::max<size_t>((size_t)D * ld, 1) * sizeof(double), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(s->d_link_beta_sum, 0, std::max<size_t>((size_t)D * ld, 1) * sizeof(double), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(s->d_link_m, 0, std::max<size_t>((size_t)N * ld, 1) * sizeof(double), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(sp->d_rhs, 0, std::max<size_t>((size_t)D * ld, 1) * sizeof(double), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(sp->cg.d_t, 0, std::max<size_t>((size_t)N * ld, 1) * sizeof(double), c->stream);
        if (e == hipSuccess && s->nnz > 0) e = hipMemcpyAsync(s->d_link_r, s->d_vals, (size_t)s->nnz * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) rc = fail(BPMF_HIP_ENODEV, std::string("side_set_features_sparse: ") + hipGetErrorString(e));
    }
    if (rc) { (void)hipGetLastError(); const std::string keep = g_err; link_free(s); g_err = keep; return rc; }
    s->link_d = D; s->link_lambda = lambda_beta; s->link_tag = (uint32_t)tag; s->link_nsum = 0;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_cg_set(bpmf_hip_side *s, double tol, int max_iter)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_link_cg_set: NULL");
    if (!s->link_sp) return fail(BPMF_HIP_EINVAL, "side_link_cg_set: the side has no sparse features (bpmf_hip_side_set_features_sparse)");
    if (!(tol > 0.0) || !(tol < 1.0)) return fail(BPMF_HIP_EINVAL, "side_link_cg_set: tol must lie in (0, 1)");
    if (max_iter < 1) return fail(BPMF_HIP_EINVAL, "side_link_cg_set: max_iter must be >= 1");
    s->link_sp->tol = tol; s->link_sp->max_iter = max_iter;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_cg_stats(bpmf_hip_side *s, int *iters_last, int64_t *iters_total, double *relres_max_last, int *hit_max_iter)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_link_cg_stats: NULL");
    if (!s->link_sp) return fail(BPMF_HIP_EINVAL, "side_link_cg_stats: the side has no sparse features (bpmf_hip_side_set_features_sparse)");
    if (iters_last) *iters_last = s->link_sp->iters_last;
    if (iters_total) *iters_total = s->link_sp->iters_total;
    if (relres_max_last) *relres_max_last = s->link_sp->relres_max_last;
    if (hit_max_iter) *hit_max_iter = s->link_sp->hit_max_iter;
    return BPMF_HIP_OK;
}

// ---- on host arrays (tests, tools) -----------------------------------------------------------------------------------------

extern "C" int bpmf_hip_link_spmm_nn(int device, int64_t N, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals, const double *V,
                                     int n, double *Y)
{
    if (!V || !Y || N < 1 || n < 1 || n > 128) return fail(BPMF_HIP_EINVAL, "link_spmm_nn: bad argument (N >= 1, 1 <= n <= 128)");
    { const int rc = check_csr("link_spmm_nn", N, D, rowptr, colidx, vals); if (rc) return rc; }
    HIP_TRY(hipSetDevice(device));
    static const int32_t none = 0;
    SpMat F;
    double *dV = nullptr, *dY = nullptr;
    int rc = bpmf_launch::sp_upload(F, N, rowptr, colidx ? colidx : &none, vals, n);
    if (!rc) rc = dev_upload(&dV, V, (size_t)D * n);
    if (!rc) rc = dev_upload<double>(&dY, nullptr, (size_t)N * n);
    if (!rc && bpmf_launch::sp_product(F, dV, n, n, n, dY, n, 0.0, nullptr, 0, nullptr)) rc = fail(BPMF_HIP_EINVAL, "link_spmm_nn: unsupported shape");
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(BPMF_HIP_ENODEV, "link_spmm_nn: kernel failed");
    if (!rc && hipMemcpy(Y, dY, (size_t)N * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(BPMF_HIP_ENODEV, "link_spmm_nn: copy failed");
    bpmf_launch::sp_free(F); free_dev(dV); free_dev(dY);
    return rc;
}

extern "C" int bpmf_hip_link_spmm_tn(int device, int64_t N, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals, const double *X,
                                     int n, double lambda, const double *P, double *C)
{
    if (!X || !C || N < 1 || n < 1 || n > 128) return fail(BPMF_HIP_EINVAL, "link_spmm_tn: bad argument (N >= 1, 1 <= n <= 128)");
    { const int rc = check_csr("link_spmm_tn", N, D, rowptr, colidx, vals); if (rc) return rc; }
    HIP_TRY(hipSetDevice(device));
    SpMat Ft;
    double *dX = nullptr, *dP = nullptr, *dC = nullptr;
    std::vector<int64_t> cptr; std::vector<int32_t> ridx; std::vector<double> cvals;
    transpose_csr(N, D, rowptr, colidx, vals, cptr, ridx, cvals);
    int rc = bpmf_launch::sp_upload(Ft, D, cptr.data(), ridx.data(), vals ? cvals.data() : nullptr, n);
    if (!rc) rc = dev_upload(&dX, X, (size_t)N * n);
    if (!rc && P) rc = dev_upload(&dP, P, (size_t)D * n);
    if (!rc) rc = dev_upload<double>(&dC, nullptr, (size_t)D * n);
    if (!rc && bpmf_launch::sp_product(Ft, dX, n, n, n, dC, n, lambda, dP, n, nullptr)) rc = fail(BPMF_HIP_EINVAL, "link_spmm_tn: unsupported shape");
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(BPMF_HIP_ENODEV, "link_spmm_tn: kernel failed");
    if (!rc && hipMemcpy(C, dC, (size_t)D * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(BPMF_HIP_ENODEV, "link_spmm_tn: copy failed");
    bpmf_launch::sp_free(Ft); free_dev(dX); free_dev(dP); free_dev(dC);
    return rc;
}

extern "C" int bpmf_hip_link_cg_solve(int device, int64_t N, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals, double lambda,
                                      const double *RHS, int n, double tol, int max_iter, double *X, int *iters, int *hit_max_iter)
{
    if (!RHS || !X || N < 1 || n < 1 || n > 128) return fail(BPMF_HIP_EINVAL, "link_cg_solve: bad argument (N >= 1, 1 <= n <= 128)");
    if (!(lambda > 0.0) || !std::isfinite(lambda)) return fail(BPMF_HIP_EINVAL, "link_cg_solve: lambda must be positive and finite");
    if (!(tol > 0.0) || !(tol < 1.0) || max_iter < 1) return fail(BPMF_HIP_EINVAL, "link_cg_solve: tol must lie in (0, 1), max_iter >= 1");
    { const int rc = check_csr("link_cg_solve", N, D, rowptr, colidx, vals); if (rc) return rc; }
    for (size_t q = 0; q < (size_t)D * n; ++q)
        if (!std::isfinite(RHS[q])) return fail(BPMF_HIP_EINVAL, "link_cg_solve: the right-hand side is not finite");
    HIP_TRY(hipSetDevice(device));
    SpMat F, Ft;
    bpmf_launch::CgWork w;
    bpmf_launch::CgResult res;
    double *dR = nullptr, *dX = nullptr;
    int rc = upload_both(F, Ft, N, D, rowptr, colidx, vals, n);
    if (!rc) rc = bpmf_launch::cg_alloc(w, N, D, n, true);
    if (!rc) rc = dev_upload(&dR, RHS, (size_t)D * n);
    if (!rc) rc = dev_upload<double>(&dX, nullptr, (size_t)D * n);
    if (!rc) rc = bpmf_launch::cg_solve(F, Ft, lambda, dX, dR, n, n, D, tol, max_iter, w, nullptr, &res);
    if (!rc && hipMemcpy(X, dX, (size_t)D * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(BPMF_HIP_ENODEV, "link_cg_solve: copy failed");
    if (!rc) {
        if (iters) memcpy(iters, res.iters, sizeof(int) * n);
        if (hit_max_iter) *hit_max_iter = res.hit_max_iter;
    }
    bpmf_launch::sp_free(F); bpmf_launch::sp_free(Ft); bpmf_launch::cg_free(w); free_dev(dR); free_dev(dX);
    return rc;
}

extern "C" int bpmf_hip_link_noise_rows(int device, int64_t nrows, int K, uint32_t it, uint32_t key_word, const double *Rinv, double *out)
{
    if (!out || nrows < 1 || K < 1 || K > 128) return fail(BPMF_HIP_EINVAL, "link_noise_rows: bad argument (nrows >= 1, 1 <= K <= 128)");
    if (Rinv)
        for (int q = 0; q < K * K; ++q)
            if (!std::isfinite(Rinv[q])) return fail(BPMF_HIP_EINVAL, "link_noise_rows: Rinv is not finite");
    HIP_TRY(hipSetDevice(device));
    double *dR = nullptr, *dO = nullptr;
    int rc = Rinv ? dev_upload(&dR, Rinv, (size_t)K * K) : 0;
    if (!rc) rc = dev_upload<double>(&dO, nullptr, (size_t)nrows * K);
    if (!rc && bpmf_launch::noise_rows(nrows, K, it, key_word, dR, nullptr, 0, nullptr, 1.0, dO, K, nullptr)) rc = fail(BPMF_HIP_EINVAL, "link_noise_rows: unsupported shape");
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(BPMF_HIP_ENODEV, "link_noise_rows: kernel failed");
    if (!rc && hipMemcpy(out, dO, (size_t)nrows * K * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(BPMF_HIP_ENODEV, "link_noise_rows: copy failed");
    free_dev(dR); free_dev(dO);
    return rc;
}
