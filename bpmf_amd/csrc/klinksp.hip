// klinksp.hip -- launchers of the sparse side-information kernels (kernels_link_sparse.h, see link_sparse.h).
#include "link_sparse.h"
#include "kernels_link_sparse.h"

namespace bpmf_launch {

namespace {

int lanes_for(int ncw) { return ncw <= 8 ? 8 : ncw <= 16 ? 16 : ncw <= 32 ? 32 : 64; }

// BPMF_LINK_WG_CHUNKS (read at every launch; the tests flip it): groups of rows / chunks one workgroup computes one after the
// other.  It changes the grid, never a sum.
int wg_groups() { return std::max(1, env_int("BPMF_LINK_WG_CHUNKS", 1)); }

template <int LPR>
void rows_launch(const SpMat &m, const double *V, int64_t ldv, int n, int ncw, double *C, int64_t ldc, double lambda, const double *P, int64_t ldp,
                 hipStream_t st)
{
    const int wgg = wg_groups();
    const int64_t per_wg = (int64_t)(256 / LPR) * wgg;
    hipLaunchKernelGGL((bpmf::k_sp_rows<LPR>), dim3((unsigned)((m.nrows + per_wg - 1) / per_wg)), dim3(256), 0, st, m.ptr.get(), m.idx.get(), m.vals.get(), m.nrows,
                       V, ldv, n, ncw, C, ldc, lambda, P, ldp, wgg);
    if (m.nlong > 0) {
        hipLaunchKernelGGL((bpmf::k_sp_chunks<LPR>), dim3((unsigned)((m.nchunks + per_wg - 1) / per_wg)), dim3(256), 0, st, m.cbeg.get(), m.cend.get(),
                           m.nchunks, m.idx.get(), m.vals.get(), V, ldv, n, m.part.get(), wgg);
        const int64_t tot = (int64_t)m.nlong * ncw;
        hipLaunchKernelGGL(bpmf::k_sp_sum_long, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, m.lrow.get(), m.lfirst.get(), m.nlong, m.part.get(), n, ncw,
                           C, ldc, lambda, P, ldp);
    }
}

template <int CW>
void dot_launch(const double *a, const double *b, int64_t ld, int64_t D, int n, double *partial, hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_cg_dot<CW>), dim3((unsigned)cg_blocks(D)), dim3(256), 0, st, a, b, ld, D, n, partial);
}

template <int CW>
void xr_launch(double *x, double *r, const double *p, const double *q, int64_t ld, int64_t D, int n, const bpmf::CgState *state, double *partial,
               hipStream_t st)
{
    hipLaunchKernelGGL((bpmf::k_cg_xr<CW>), dim3((unsigned)cg_blocks(D)), dim3(256), 0, st, x, r, p, q, ld, D, n, state, partial);
}

int width_for(int n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : n <= 64 ? 64 : 128; }

void cg_dot(const double *a, const double *b, int64_t ld, int64_t D, int n, double *partial, hipStream_t st)
{
    switch (width_for(n)) {
    case 8: dot_launch<8>(a, b, ld, D, n, partial, st); break;
    case 16: dot_launch<16>(a, b, ld, D, n, partial, st); break;
    case 32: dot_launch<32>(a, b, ld, D, n, partial, st); break;
    case 64: dot_launch<64>(a, b, ld, D, n, partial, st); break;
    default: dot_launch<128>(a, b, ld, D, n, partial, st); break;
    }
}

void cg_xr(double *x, double *r, const double *p, const double *q, int64_t ld, int64_t D, int n, const bpmf::CgState *state, double *partial,
           hipStream_t st)
{
    switch (width_for(n)) {
    case 8: xr_launch<8>(x, r, p, q, ld, D, n, state, partial, st); break;
    case 16: xr_launch<16>(x, r, p, q, ld, D, n, state, partial, st); break;
    case 32: xr_launch<32>(x, r, p, q, ld, D, n, state, partial, st); break;
    case 64: xr_launch<64>(x, r, p, q, ld, D, n, state, partial, st); break;
    default: xr_launch<128>(x, r, p, q, ld, D, n, state, partial, st); break;
    }
}

}  // namespace

int sp_upload(SpMat &m, int64_t nrows, const int64_t *ptr, const int32_t *idx, const double *vals, int max_n)
{
    m = SpMat{};
    m.nrows = nrows; m.nnz = ptr[nrows];
    std::vector<int32_t> lrow;
    std::vector<int64_t> lfirst, cbeg, cend;
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t beg = ptr[r], end = ptr[r + 1];
        if (end - beg <= bpmf::kSpChunk) continue;
        lrow.push_back((int32_t)r);
        lfirst.push_back((int64_t)cbeg.size());
        for (int64_t p = beg; p < end; p += bpmf::kSpChunk) { cbeg.push_back(p); cend.push_back(std::min<int64_t>(p + bpmf::kSpChunk, end)); }
    }
    lfirst.push_back((int64_t)cbeg.size());
    m.nlong = (int)lrow.size(); m.nchunks = (int64_t)cbeg.size(); m.part_n = max_n;
    int rc = m.ptr.upload(ptr, (size_t)nrows + 1);
    if (!rc) rc = m.idx.upload(idx, (size_t)m.nnz);
    if (!rc && vals) rc = m.vals.upload(vals, (size_t)m.nnz);
    if (!rc && m.nlong > 0) {
        rc = m.lrow.upload(lrow.data(), lrow.size());
        if (!rc) rc = m.lfirst.upload(lfirst.data(), lfirst.size());
        if (!rc) rc = m.cbeg.upload(cbeg.data(), cbeg.size());
        if (!rc) rc = m.cend.upload(cend.data(), cend.size());
        if (!rc) rc = m.part.alloc((size_t)m.nchunks * (size_t)max_n);
    }
    if (rc) m = SpMat{};
    return rc;
}

int sp_product(const SpMat &m, const double *V, int64_t ldv, int n, int ncw, double *C, int64_t ldc, double lambda, const double *P, int64_t ldp,
               hipStream_t st)
{
    if (m.nrows < 0 || n < 1 || ncw < n || ncw > 128 || ldc < ncw || ldv < n || (P && ldp < n) || (m.nlong > 0 && n > m.part_n)) return -1;
    if (m.nrows == 0) return 0;
    switch (lanes_for(ncw)) {
    case 8: rows_launch<8>(m, V, ldv, n, ncw, C, ldc, lambda, P, ldp, st); break;
    case 16: rows_launch<16>(m, V, ldv, n, ncw, C, ldc, lambda, P, ldp, st); break;
    case 32: rows_launch<32>(m, V, ldv, n, ncw, C, ldc, lambda, P, ldp, st); break;
    default: rows_launch<64>(m, V, ldv, n, ncw, C, ldc, lambda, P, ldp, st); break;
    }
    return 0;
}

int64_t cg_blocks(int64_t D) { return (D + bpmf::kCgBlock - 1) / bpmf::kCgBlock; }

int cg_alloc(CgWork &w, int64_t N, int64_t D, int64_t ld, bool with_t)
{
    w = CgWork{};
    int rc = w.p.alloc((size_t)D * (size_t)ld);
    if (!rc) rc = w.q.alloc((size_t)D * (size_t)ld);
    if (!rc && with_t) rc = w.t.alloc((size_t)N * (size_t)ld);
    if (!rc) rc = w.partial.alloc((size_t)cg_blocks(D) * bpmf::kCgMaxN);
    if (!rc) rc = w.state.alloc(1);
    if (!rc) rc = w.word.alloc(2);
    if (rc) w = CgWork{};
    return rc;
}

int cg_solve(const SpMat &F, const SpMat &Ft, double lambda, double *x, double *r, int64_t ld, int n, int64_t D, double tol, int max_iter, CgWork &w,
             hipStream_t st, CgResult *res)
{
    const auto bad = []() { return fail(BPMF_HIP_EINVAL, "link: unsupported shape of the CG solve"); };
    if (n < 1 || n > bpmf::kCgMaxN || D < 1 || ld < n || max_iter < 0 || !(tol >= 0.0)) return bad();
    const double tol2 = tol * tol;
    const int64_t nb = cg_blocks(D);
    const unsigned ge = (unsigned)((D * n + 255) / 256);
    // BPMF_LINK_CG_CHECK (read at every solve): iterations enqueued between two looks of the host at the convergence word.  A
    // column is frozen on the device the moment it converges, so the look-ahead iterations change nothing.
    const int check = std::max(1, env_int("BPMF_LINK_CG_CHECK", 4));
    double *const p = w.p.get(), *const q = w.q.get(), *const t = w.t.get(), *const partial = w.partial.get();
    bpmf::CgState *const state = w.state.get();
    w.word.host()[0] = -1;
    hipLaunchKernelGGL(bpmf::k_cg_start, dim3(ge), dim3(256), 0, st, x, p, r, ld, D, n);
    cg_dot(r, r, ld, D, n, partial, st);
    hipLaunchKernelGGL(bpmf::k_cg_init, dim3(1), dim3(bpmf::kCgMaxN), 0, st, partial, nb, n, tol2, state, w.word.dev());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    int done = 0;
    while (done < max_iter && __atomic_load_n(&w.word.host()[0], __ATOMIC_ACQUIRE) != 0) {
        const int batch = std::min(check, max_iter - done);
        for (int b = 0; b < batch; ++b) {
            if (sp_product(F, p, ld, n, n, t, ld, 0.0, nullptr, 0, st)) return bad();                        // t = F p
            if (sp_product(Ft, t, ld, n, n, q, ld, lambda, p, ld, st)) return bad();                   // q = F^T t + lambda p
            cg_dot(p, q, ld, D, n, partial, st);
            hipLaunchKernelGGL(bpmf::k_cg_alpha, dim3(1), dim3(bpmf::kCgMaxN), 0, st, partial, nb, n, state);
            cg_xr(x, r, p, q, ld, D, n, state, partial, st);
            hipLaunchKernelGGL(bpmf::k_cg_beta, dim3(1), dim3(bpmf::kCgMaxN), 0, st, partial, nb, n, tol2, state, w.word.dev());
            hipLaunchKernelGGL(bpmf::k_cg_p, dim3(ge), dim3(256), 0, st, p, r, ld, D, n, state);
        }
        done += batch;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (res) {
        bpmf::CgState hs;
        HIP_TRY(hipMemcpy(&hs, state, sizeof hs, hipMemcpyDeviceToHost));
        *res = CgResult{};
        for (int k = 0; k < n; ++k) {
            res->iters[k] = hs.iters[k];
            res->iters_max = std::max(res->iters_max, hs.iters[k]);
            if (hs.bb[k] > 0.0) res->relres_max = std::max(res->relres_max, std::sqrt(hs.rr[k] / hs.bb[k]));
        }
        res->hit_max_iter = hs.nactive > 0 ? 1 : 0;
    }
    return 0;
}

int noise_rows(int64_t nrows, int kt, uint32_t it, uint32_t key1, const double *d_Rinv, const double *d_base, int64_t ldb, const double *d_bvec,
               double scale, double *d_out, int64_t ldo, hipStream_t st)
{
    if (nrows < 0 || kt < 1 || kt > bpmf::kCgMaxN || ldo < kt || (d_base && (!d_bvec || ldb < kt))) return -1;
    if (nrows == 0) return 0;
    hipLaunchKernelGGL(bpmf::k_link_noise_rows, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, nrows, kt, it, key1, d_Rinv, d_base, ldb, d_bvec,
                       scale, d_out, ldo);
    return 0;
}

}  // namespace bpmf_launch
