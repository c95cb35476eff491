// kbias.hip -- launchers of the bias kernels (kernels_bias.h, see launch.h).
#include "launch.h"
#include "kernels_bias.h"

namespace bpmf_launch {

int bias_piece() { return bpmf::kBiasPiece; }
int bias_light() { return bpmf::kBiasLight; }

int bias_step(const BiasStepLaunch &p, hipStream_t st)
{
    if (p.f.K != 8 && p.f.K != 16 && p.f.K != 32 && p.f.K != 64 && p.f.K != 128) return -1;
    const double *items = static_cast<const double *>(p.f.items), *other = static_cast<const double *>(p.f.other);
    if (p.m.nnz > 0) {
        const unsigned tiles = (unsigned)((p.m.nnz + bpmf::kProbitTile - 1) / bpmf::kProbitTile);
        dispatch_k(p.f.K, [&](auto k) {
            hipLaunchKernelGGL((bpmf::k_bias_resid<decltype(k)::value>), dim3(tiles), dim3(bpmf::kProbitTile), 0, st, p.m.colptr, p.m.ncols,
                               p.m.rowidx, p.vals, p.m.nnz, items, other, p.f.kt, p.mean, p.cbias, p.e, p.fail);
        });
        if (p.npieces > 0)
            hipLaunchKernelGGL(bpmf::k_bias_piece_sums, dim3((unsigned)((p.npieces + 3) / 4)), dim3(256), 0, st, p.m.colptr, p.pieceptr, p.m.ncols,
                               p.npieces, p.e, p.part);
    }
    if (p.m.ncols > 0)
        hipLaunchKernelGGL(bpmf::k_bias_draw, dim3((unsigned)((p.m.ncols + 255) / 256)), dim3(256), 0, st, p.m.colptr, p.pieceptr, p.m.ncols, p.e, p.part,
                           p.lambda, p.alpha, p.iter, p.tag, p.b);
    if (p.m.nnz > 0)
        hipLaunchKernelGGL(bpmf::k_bias_values, dim3((unsigned)((p.m.nnz + 255) / 256)), dim3(256), 0, st, p.m.colptr, p.m.ncols, p.m.rowidx, p.vals,
                           p.m.nnz, p.b, p.cbias, p.z);
    return 0;
}

void bias_lambda(const BiasLambdaLaunch &p, hipStream_t st)
{
    hipLaunchKernelGGL(bpmf::k_bias_lambda, dim3(1), dim3(256), 0, st, p.b, p.ncols, p.dd, p.c, p.b0, p.iter, p.tag, p.lambda, p.trace, p.cap, p.fail);
}

void samples_add_bias(const double *b, int64_t ncols, int role, int Kt, double *ring, int64_t stride, int Kp, int slot, hipStream_t st)
{
    if (ncols > 0) hipLaunchKernelGGL(bpmf::k_samples_add_bias, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, st, b, ncols, role, Kt, ring, stride, Kp, slot);
}

void bias_accumulate(const double *b, int64_t ncols, double *bsum, hipStream_t st)
{
    if (ncols > 0) hipLaunchKernelGGL(bpmf::k_bias_accumulate, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, st, b, ncols, bsum);
}

int bias_predict(bpmf_hip_test *t, const bpmf_hip_side *self, const bpmf_hip_side *other, const void *self_items, const void *other_items,
                 int n, hipStream_t ps)
{
    const int K = self->ctx->K;
    if (K != 8 && K != 16 && K != 32 && K != 64 && K != 128) return -1;
    t->pstream = ps;
    // users.predict(movies): one kernel for both copies when the entries match, else the twin's own launch ahead of this one
    const bool fused_twin = t->twin && t->d_twin_perm;
    if (t->twin && !fused_twin && t->twin->nnz > 0) {
        const int rc = bias_predict(t->twin, t->twin->side, self, other_items, self_items, n, ps);
        if (rc) return rc;
        t->twin->launched = true;
    }
    bpmf::TwinArgs tw{};
    if (fused_twin) {
        bpmf_hip_test *u = t->twin;
        tw.perm = t->d_twin_perm.get(); tw.pavg = u->d_pavg.get(); tw.pm2 = u->d_pm2.get(); tw.mean = u->side->mean_rating;
        tw.partial = u->d_partial.get(); tw.out = u->h_res.dev(); tw.flag = reinterpret_cast<unsigned *>(u->h_res.dev() + 2); tw.seq = ++u->seq;
        u->pstream = ps; u->launched = true;
    }
    unsigned *flag = reinterpret_cast<unsigned *>(t->h_res.dev() + 2);
    const unsigned pseq = ++t->seq;
    const double *bcol = self->bias->b.get(), *brow = other->bias->b.get();
    dispatch_k(K, [&](auto k) {
        constexpr int KK = decltype(k)::value;
        auto run = [&](auto kernel, unsigned wg) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)t->nblocks), dim3(wg), 0, ps, t->d_tcol.get(), t->d_trow.get(), t->d_tval.get(), t->nnz,
                               static_cast<const double *>(self_items), static_cast<const double *>(other_items), bcol, brow, self->mean_rating, n,
                               t->d_pavg.get(), t->d_pm2.get(), t->d_partial.get(), t->h_res.dev(), t->d_ticket.get(), flag, pseq, tw);
        };
        if (t->wg == 64) run(bpmf::k_predict_bias<KK, 64>, 64u);
        else run(bpmf::k_predict_bias<KK, 256>, 256u);
    });
    return 0;
}

}  // namespace bpmf_launch
