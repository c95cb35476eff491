// capi_link_lambda.hip -- the sampled link precision lambda_beta of a side with features, and the device-factor mode it puts a
// dense side into: G(lambda_beta) = F^T F + lambda_beta I factored and solved against on the device every half-iteration
// (kernels in kernels_link_chol.h).
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"
#include "link_lambda.h"

using namespace bpmf_capi;

namespace {

constexpr int kMaxD = 1024, kMaxRhs = 128;

// the work arrays of a factorisation of a D x D matrix and of solves against it
struct CholWork { DevBuf<double> Lp, Linv, LinvT, Xp, Ep; DevBuf<int> flag; };

int chol_alloc(int D, DevBuf<double> &Lp, DevBuf<double> &Linv, DevBuf<double> &LinvT, DevBuf<double> &Xp, DevBuf<double> &Ep, DevBuf<int> &flag,
               hipStream_t st)
{
    const size_t dp = (size_t)bpmf_launch::link_chol_dp(D);
    int rc;
    if ((rc = Lp.alloc(dp * dp)) || (rc = Linv.alloc(dp * 64)) || (rc = LinvT.alloc(dp * 64)) || (rc = Xp.alloc(dp * kMaxRhs)) ||
        (rc = Ep.alloc(dp * kMaxRhs)) || (rc = flag.alloc(1)))
        return rc;
    return flag.zero_async(st);
}

// reads the pivot flag behind the work enqueued on st and lowers it again
int chol_collect(int *d_flag, hipStream_t st, const char *who)
{
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h) {
        HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), st));
        return fail(BPMF_HIP_ENUM, std::string(who) + ": the matrix is not positive definite (a pivot of the device factorisation was not positive and finite)");
    }
    return 0;
}

int need_link(const char *who, const bpmf_hip_side *s)
{
    if (!s) return fail(BPMF_HIP_EINVAL, std::string(who) + ": NULL");
    if (!s->link) return fail(BPMF_HIP_EINVAL, std::string(who) + ": the side has no features (bpmf_hip_side_set_features)");
    return 0;
}

}  // namespace

namespace bpmf_capi {

int link_chol_enter(bpmf_hip_side *s)
{
    bpmf_link *L = s->link.get();
    if (!L->dense || L->dense->devfac) return 0;
    bpmf_hip_ctx *c = s->ctx;
    bpmf_link_dense *dn = L->dense.get();
    const int D = L->D;
    const int64_t N = s->ncols;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = settle_async(s))) return rc;
    DevBuf<double> part0;
    if ((rc = dn->FtF.alloc((size_t)D * D)) || (rc = part0.alloc(bpmf_launch::link_tn_part_words(N, D, std::min(D, 128)))) ||
        (rc = chol_alloc(D, dn->Lp, dn->Linv, dn->LinvT, dn->Xp, dn->Ep, dn->flag, c->stream.get())))
        return rc;
    if ((rc = link_tn_product(dn->F.get(), D, dn->F.get(), D, nullptr, N, D, D, dn->FtF.get(), D, part0.get(), c->stream.get()))) return rc;
    if ((rc = bounded_stream_sync(c, c->stream.get(), __func__))) return rc;     // (part0 goes out of use here)
    dn->W.reset();
    dn->devfac = true;
    dn->fact_lambda = 0.0;                                                 // (no factor yet: lambda_beta > 0 always differs)
    return 0;
}

int link_chol_draw(bpmf_hip_side *s)
{
    bpmf_hip_ctx *c = s->ctx;
    bpmf_link *L = s->link.get();
    bpmf_link_dense *dn = L->dense.get();
    const int D = L->D, K = c->K, Kt = c->Kt;
    if (dn->fact_lambda != L->lambda) {
        bpmf_launch::LinkCholLaunch f{};
        f.FtF = dn->FtF.get(); f.D = D; f.lambda = L->lambda; f.Lp = dn->Lp.get(); f.Linv = dn->Linv.get(); f.LinvT = dn->LinvT.get();
        f.flag = dn->flag.get();
        if (bpmf_launch::link_chol_factor(f, c->stream.get())) return fail(BPMF_HIP_EINVAL, "link: unsupported shape of the device factorisation");
        dn->fact_lambda = 0.0;                                             // (valid only once the flag has been collected)
    }
    bpmf_launch::LinkCholSolveLaunch q{};
    q.Lp = dn->Lp.get(); q.Linv = dn->Linv.get(); q.LinvT = dn->LinvT.get(); q.D = D;
    q.P = dn->PE.get(); q.ldp = K; q.E = dn->PE.get() + (size_t)D * K; q.lde = K; q.n = Kt;
    q.Xp = dn->Xp.get(); q.Ep = dn->Ep.get(); q.out = L->beta.get(); q.ldo = K; q.ncw = K;
    if (bpmf_launch::link_chol_solve(q, c->stream.get())) return fail(BPMF_HIP_EINVAL, "link: unsupported shape of the device solves");
    HIP_TRY(hipGetLastError());
    const int rc = chol_collect(dn->flag.get(), c->stream.get(), "link_sample: F^T F + lambda_beta I");
    if (rc) return rc;
    dn->fact_lambda = L->lambda;
    return 0;
}

int link_lambda_draw(bpmf_hip_side *s, const double *btb, int iter)
{
    bpmf_link *L = s->link.get();
    if (s->iter < 0) return 0;                                             // the side's first half-iteration: no beta has been drawn
    const int Kt = s->ctx->Kt;
    const std::vector<double> &R = s->hp_LambdaU;                           // upper triangular, column-major: R_ia = R[a * Kt + i], i <= a
    if ((int)R.size() != Kt * Kt) return fail(BPMF_HIP_EINVAL, "link_sample: no Lambda of the previous half-iteration to draw lambda_beta from");
    double t = 0.0;                                                        // tr(R B R^T) = sum_i r_i^T B r_i, r_i = row i of R; fixed order
    for (int i = 0; i < Kt; ++i)
        for (int a = i; a < Kt; ++a) {
            double v = 0.0;
            for (int b = i; b < Kt; ++b) v += btb[(size_t)a * Kt + b] * R[(size_t)b * Kt + i];
            t += R[(size_t)a * Kt + i] * v;
        }
    if (!(t >= 0.0)) t = 0.0;                                              // (rounding of a trace that is zero)
    double lam = 0.0;
    const int rc = bpmf_hip_link_lambda_sample(L->a0, L->b0, t, (int64_t)L->D * Kt, iter, L->tag, &lam);
    if (rc) return rc;
    if (!(lam > 0.0) || !std::isfinite(lam)) return fail(BPMF_HIP_ENUM, "link_sample: the draw of lambda_beta is not positive and finite");
    L->lambda = lam;
    L->trace_last = t;
    return 0;
}

}  // namespace bpmf_capi

extern "C" int bpmf_hip_side_link_lambda_prior(bpmf_hip_side *s, double a0, double b0)
{
    { const int rc = need_link("side_link_lambda_prior", s); if (rc) return rc; }
    if (!(a0 > 0.0) || !(b0 >= 0.0) || !std::isfinite(a0) || !std::isfinite(b0))
        return fail(BPMF_HIP_EINVAL, "side_link_lambda_prior: needs a finite shape a0 > 0 and a finite rate b0 >= 0");
    bpmf_link *L = s->link.get();
    if (L->tag > 15) return fail(BPMF_HIP_EINVAL, "side_link_lambda_prior: the side's tag must be 1 .. 15 (it selects the lambda_beta stream)");
    if (s->iter >= 0) return fail(BPMF_HIP_EINVAL, "side_link_lambda_prior: only before the side's first half-iteration");
    const int rc = link_chol_enter(s);
    if (rc) return rc;
    L->a0 = a0; L->b0 = b0; L->sample_lambda = true;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_lambda_set(bpmf_hip_side *s, double lambda)
{
    { const int rc = need_link("side_link_lambda_set", s); if (rc) return rc; }
    if (!(lambda > 0.0) || !std::isfinite(lambda)) return fail(BPMF_HIP_EINVAL, "side_link_lambda_set: lambda_beta must be positive and finite");
    const int rc = link_chol_enter(s);
    if (rc) return rc;
    s->link->lambda = lambda;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_side_link_lambda_get(bpmf_hip_side *s, double *lambda, double *trace_last, int *sampled)
{
    { const int rc = need_link("side_link_lambda_get", s); if (rc) return rc; }
    if (lambda) *lambda = s->link->lambda;
    if (trace_last) *trace_last = s->link->trace_last;
    if (sampled) *sampled = s->link->sample_lambda ? 1 : 0;
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_link_chol_solve(int device, const double *A, int D, const double *P, const double *E, int n, double *X, double *L_out)
{
    if (!A || !P || !X || D < 1 || D > kMaxD || n < 1 || n > kMaxRhs)
        return fail(BPMF_HIP_EINVAL, "link_chol_solve: bad argument (1 <= D <= 1024, 1 <= n <= 128)");
    HIP_TRY(hipSetDevice(device));
    const size_t DD = (size_t)D * D, Dn = (size_t)D * n;
    DevBuf<double> dA, dP, dE, dX;
    CholWork w;
    int rc;
    if ((rc = dA.upload(A, DD)) || (rc = dP.upload(P, Dn)) || (E && (rc = dE.upload(E, Dn))) || (rc = dX.alloc(Dn)) ||
        (rc = chol_alloc(D, w.Lp, w.Linv, w.LinvT, w.Xp, w.Ep, w.flag, nullptr)))
        return rc;
    bpmf_launch::LinkCholLaunch f{};
    f.FtF = dA.get(); f.D = D; f.lambda = 0.0; f.Lp = w.Lp.get(); f.Linv = w.Linv.get(); f.LinvT = w.LinvT.get(); f.flag = w.flag.get();
    bpmf_launch::LinkCholSolveLaunch q{};
    q.Lp = w.Lp.get(); q.Linv = w.Linv.get(); q.LinvT = w.LinvT.get(); q.D = D; q.P = dP.get(); q.ldp = n; q.E = E ? dE.get() : nullptr; q.lde = n;
    q.n = n; q.Xp = w.Xp.get(); q.Ep = w.Ep.get(); q.out = dX.get(); q.ldo = n; q.ncw = n;
    if (bpmf_launch::link_chol_factor(f, nullptr) || bpmf_launch::link_chol_solve(q, nullptr)) return fail(BPMF_HIP_EINVAL, "link_chol_solve: unsupported shape");
    HIP_TRY(hipGetLastError());
    if (hipDeviceSynchronize() != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_chol_solve: kernel failed");
    if ((rc = chol_collect(w.flag.get(), nullptr, "link_chol_solve"))) return rc;
    if (hipMemcpy(X, dX.get(), Dn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(BPMF_HIP_ENODEV, "link_chol_solve: copy failed");
    if (L_out) {
        const size_t dp = (size_t)bpmf_launch::link_chol_dp(D);
        if (hipMemcpy2D(L_out, (size_t)D * sizeof(double), w.Lp.get(), dp * sizeof(double), (size_t)D * sizeof(double), (size_t)D, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(BPMF_HIP_ENODEV, "link_chol_solve: copy of the factor failed");
        for (int r = 0; r < D; ++r)
            for (int col = r + 1; col < D; ++col) L_out[(size_t)r * D + col] = 0.0;
    }
    return BPMF_HIP_OK;
}
