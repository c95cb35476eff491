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
    return bpmf_launch::sp_upload(Ft, D, cptr.data(), ridx.data(), vals ? cvals.data() : nullptr, max_n);
}

}  // namespace

namespace bpmf_capi {

int link_check_csr(const char *who, int64_t N, int64_t D, const int64_t *rowptr, const int32_t *colidx, const double *vals)
{
    return check_csr(who, N, D, rowptr, colidx, vals);
}

int link_sparse_offsets(bpmf_hip_side *s)
{
    const bpmf_hip_ctx *c = s->ctx;
    const bpmf_link *L = s->link.get();
    if (bpmf_launch::sp_product(L->sparse->F, L->beta.get(), c->K, c->Kt, c->K, L->m.get(), c->K, 0.0, nullptr, 0, c->stream.get()))
        return fail(BPMF_HIP_EINVAL, "link: unsupported shape of the sparse product");
    HIP_TRY(hipGetLastError());
    return 0;
}

int link_sparse_draw(bpmf_hip_side *s, const double *mu, const double *LU, int iter)
{
    bpmf_hip_ctx *c = s->ctx;
    bpmf_link *L = s->link.get();
    bpmf_link_sparse *sp = L->sparse.get();
    const int K = c->K, Kt = c->Kt, D = L->D;
    const int64_t N = s->ncols;
    hipStream_t st = c->stream.get();
    // R^-1 (upper triangular, row-major) of Lambda = R^T R, R = LambdaU (upper, column-major): K^3 on the host
    std::vector<double> Rinv((size_t)Kt * Kt, 0.0), pad((size_t)K, 0.0);
    for (int col = 0; col < Kt; ++col)
        for (int i = col; i >= 0; --i) {
            double v = i == col ? 1.0 : 0.0;
            for (int j = i + 1; j <= col; ++j) v -= LU[(size_t)j * Kt + i] * Rinv[(size_t)j * Kt + col];
            Rinv[(size_t)i * Kt + col] = v / LU[(size_t)i * Kt + i];
        }
    memcpy(pad.data(), mu, sizeof(double) * Kt);
    HIP_TRY(hipMemcpyAsync(L->mu.get(), pad.data(), sizeof(double) * K, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sp->rinv.get(), Rinv.data(), Rinv.size() * sizeof(double), hipMemcpyHostToDevice, st));
    // X = U - 1 mu^T + Z1 R^-T (N x K, in the work array of F p), E = sqrt(lambda) Z2 R^-T, RHS = F^T X + E
    int rc = bpmf_launch::noise_rows(N, Kt, (uint32_t)iter, L->tag + 0x10000u, sp->rinv.get(), s->d_items, K, L->mu.get(), 1.0, sp->cg.t.get(), K, st);
    if (!rc) rc = bpmf_launch::noise_rows(D, Kt, (uint32_t)iter, L->tag + 0x20000u, sp->rinv.get(), nullptr, 0, nullptr, std::sqrt(L->lambda),
                                          sp->rhs.get(), K, st);
    if (!rc) rc = bpmf_launch::sp_product(sp->Ft, sp->cg.t.get(), K, Kt, Kt, sp->rhs.get(), K, 1.0, sp->rhs.get(), K, st);
    if (rc) return fail(BPMF_HIP_EINVAL, "link_sample: unsupported shape of the sparse right-hand side");
    HIP_TRY(hipGetLastError());
    bpmf_launch::CgResult res;
    rc = bpmf_launch::cg_solve(sp->F, sp->Ft, L->lambda, L->beta.get(), sp->rhs.get(), K, Kt, D, sp->tol, sp->max_iter, sp->cg, st, &res);
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
    if (tag >= kTagLimit) return fail(BPMF_HIP_EINVAL, "side_set_features_sparse: tag must be < 0x10000 (the noise streams use tag + 0x10000 and tag + 0x20000)");
    const int64_t N = s->ncols;
    int rc = check_csr("side_set_features_sparse", N, D, rowptr, colidx, vals);
    if (rc) return rc;
    const int K = c->K, Kt = c->Kt;
    std::unique_ptr<bpmf_link> L;
    if ((rc = link_attach_common("side_set_features_sparse", s, D, lambda_beta, tag, bpmf_launch::link_tn_part_words(D, Kt, Kt), &L))) return rc;
    auto sp = std::make_unique<bpmf_link_sparse>();
    if ((rc = upload_both(sp->F, sp->Ft, N, D, rowptr, colidx, vals, Kt)) || (rc = bpmf_launch::cg_alloc(sp->cg, N, D, K, true)) ||
        (rc = sp->rhs.alloc((size_t)D * K)) || (rc = sp->rinv.alloc((size_t)Kt * Kt)) || (rc = sp->rhs.zero_async(c->stream.get())) ||
        (rc = sp->cg.t.zero_async(c->stream.get())))
        return rc;
    L->sparse = std::move(sp);
    s->link = std::move(L);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_cg_set(bpmf_hip_side *s, double tol, int max_iter)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_link_cg_set: NULL");
    if (!(s->link && s->link->sparse)) return fail(BPMF_HIP_EINVAL, "side_link_cg_set: the side has no sparse features (bpmf_hip_side_set_features_sparse)");
    if (!(tol > 0.0) || !(tol < 1.0)) return fail(BPMF_HIP_EINVAL, "side_link_cg_set: tol must lie in (0, 1)");
    if (max_iter < 1) return fail(BPMF_HIP_EINVAL, "side_link_cg_set: max_iter must be >= 1");
    s->link->sparse->tol = tol; s->link->sparse->max_iter = max_iter;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_cg_stats(bpmf_hip_side *s, int *iters_last, int64_t *iters_total, double *relres_max_last, int *hit_max_iter)
{
    if (!s) return fail(BPMF_HIP_EINVAL, "side_link_cg_stats: NULL");
    if (!(s->link && s->link->sparse)) return fail(BPMF_HIP_EINVAL, "side_link_cg_stats: the side has no sparse features (bpmf_hip_side_set_features_sparse)");
    if (iters_last) *iters_last = s->link->sparse->iters_last;
    if (iters_total) *iters_total = s->link->sparse->iters_total;
    if (relres_max_last) *relres_max_last = s->link->sparse->relres_max_last;
    if (hit_max_iter) *hit_max_iter = s->link->sparse->hit_max_iter;
    return BPMF_HIP_OK;
}

// ---- on host arrays (tests, tools) -----------------------------------------------------------------------------------------

extern "C" int bpmf_hip_link_spmm_nn(int device, int64_t N, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals, const double *V,
                                     int n, double *Y)
{
    if (!V || !Y || N < 1 || n < 1 || n > 128) return fail(BPMF_HIP_EINVAL, "link_spmm_nn: bad argument (N >= 1, 1 <= n <= 128)");
    int rc = check_csr("link_spmm_nn", N, D, rowptr, colidx, vals);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    static const int32_t none = 0;
    SpMat F;
    DevBuf<double> dV, dY;
    if ((rc = bpmf_launch::sp_upload(F, N, rowptr, colidx ? colidx : &none, vals, n)) || (rc = dV.upload(V, (size_t)D * n)) || (rc = dY.alloc((size_t)N * n)))
        return rc;
    if (bpmf_launch::sp_product(F, dV.get(), n, n, n, dY.get(), n, 0.0, nullptr, 0, nullptr)) return fail(BPMF_HIP_EINVAL, "link_spmm_nn: unsupported shape");
    if (hipDeviceSynchronize() != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_spmm_nn: kernel failed");
    if (hipMemcpy(Y, dY.get(), (size_t)N * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_spmm_nn: copy failed");
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_link_spmm_tn(int device, int64_t N, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals, const double *X,
                                     int n, double lambda, const double *P, double *C)
{
    if (!X || !C || N < 1 || n < 1 || n > 128) return fail(BPMF_HIP_EINVAL, "link_spmm_tn: bad argument (N >= 1, 1 <= n <= 128)");
    int rc = check_csr("link_spmm_tn", N, D, rowptr, colidx, vals);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    SpMat Ft;
    DevBuf<double> dX, dP, dC;
    std::vector<int64_t> cptr; std::vector<int32_t> ridx; std::vector<double> cvals;
    transpose_csr(N, D, rowptr, colidx, vals, cptr, ridx, cvals);
    if ((rc = bpmf_launch::sp_upload(Ft, D, cptr.data(), ridx.data(), vals ? cvals.data() : nullptr, n)) || (rc = dX.upload(X, (size_t)N * n)) ||
        (P && (rc = dP.upload(P, (size_t)D * n))) || (rc = dC.alloc((size_t)D * n)))
        return rc;
    if (bpmf_launch::sp_product(Ft, dX.get(), n, n, n, dC.get(), n, lambda, dP.get(), n, nullptr)) return fail(BPMF_HIP_EINVAL, "link_spmm_tn: unsupported shape");
    if (hipDeviceSynchronize() != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_spmm_tn: kernel failed");
    if (hipMemcpy(C, dC.get(), (size_t)D * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_spmm_tn: copy failed");
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_link_cg_solve(int device, int64_t N, int D, const int64_t *rowptr, const int32_t *colidx, const double *vals, double lambda,
                                      const double *RHS, int n, double tol, int max_iter, double *X, int *iters, int *hit_max_iter)
{
    if (!RHS || !X || N < 1 || n < 1 || n > 128) return fail(BPMF_HIP_EINVAL, "link_cg_solve: bad argument (N >= 1, 1 <= n <= 128)");
    if (!(lambda > 0.0) || !std::isfinite(lambda)) return fail(BPMF_HIP_EINVAL, "link_cg_solve: lambda must be positive and finite");
    if (!(tol > 0.0) || !(tol < 1.0) || max_iter < 1) return fail(BPMF_HIP_EINVAL, "link_cg_solve: tol must lie in (0, 1), max_iter >= 1");
    int rc = check_csr("link_cg_solve", N, D, rowptr, colidx, vals);
    if (rc) return rc;
    for (size_t q = 0; q < (size_t)D * n; ++q)
        if (!std::isfinite(RHS[q])) return fail(BPMF_HIP_EINVAL, "link_cg_solve: the right-hand side is not finite");
    HIP_TRY(hipSetDevice(device));
    SpMat F, Ft;
    bpmf_launch::CgWork w;
    bpmf_launch::CgResult res;
    DevBuf<double> dR, dX;
    if ((rc = upload_both(F, Ft, N, D, rowptr, colidx, vals, n)) || (rc = bpmf_launch::cg_alloc(w, N, D, n, true)) ||
        (rc = dR.upload(RHS, (size_t)D * n)) || (rc = dX.alloc((size_t)D * n)))
        return rc;
    if ((rc = bpmf_launch::cg_solve(F, Ft, lambda, dX.get(), dR.get(), n, n, D, tol, max_iter, w, nullptr, &res))) return rc;
    if (hipMemcpy(X, dX.get(), (size_t)D * n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_cg_solve: copy failed");
    if (iters) memcpy(iters, res.iters, sizeof(int) * n);
    if (hit_max_iter) *hit_max_iter = res.hit_max_iter;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_link_noise_rows(int device, int64_t nrows, int K, uint32_t it, uint32_t key_word, const double *Rinv, double *out)
{
    if (!out || nrows < 1 || K < 1 || K > 128) return fail(BPMF_HIP_EINVAL, "link_noise_rows: bad argument (nrows >= 1, 1 <= K <= 128)");
    if (Rinv)
        for (int q = 0; q < K * K; ++q)
            if (!std::isfinite(Rinv[q])) return fail(BPMF_HIP_EINVAL, "link_noise_rows: Rinv is not finite");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> dR, dO;
    int rc;
    if ((Rinv && (rc = dR.upload(Rinv, (size_t)K * K))) || (rc = dO.alloc((size_t)nrows * K))) return rc;
    if (bpmf_launch::noise_rows(nrows, K, it, key_word, dR.get(), nullptr, 0, nullptr, 1.0, dO.get(), K, nullptr)) return fail(BPMF_HIP_EINVAL, "link_noise_rows: unsupported shape");
    if (hipDeviceSynchronize() != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_noise_rows: kernel failed");
    if (hipMemcpy(out, dO.get(), (size_t)nrows * K * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_noise_rows: copy failed");
    return BPMF_HIP_OK;
}
