// capi_score.hip -- model comparison (kernel in kernels_score.h): the log pointwise predictive density of a list
// of observed cells over two sample rings and the per-cell variance of the log density that turns it into WAIC (bpmf_hip_score_cells).
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

namespace {

// Nothing is stored per sample, so a batch is bounded by the grid alone: 2^22 sorted cells are at least 2^22 / 512 workgroups
constexpr int64_t kBatchCells = (int64_t)1 << 22;
std::atomic<int> g_batch_cells{0};                                     // bpmf_hip_score_batch_cells (0: kBatchCells)

std::string cell_name(int64_t i, const int32_t *q, const int32_t *cc)
{
    return "cell " + std::to_string((long long)i) + " (" + std::to_string(q[i]) + ", " + std::to_string(cc[i]) + ")";
}

}  // namespace

int bpmf_capi::logdens_check_args(const std::string &who, int64_t n, const int32_t *q, const int32_t *cc, const double *y, const double *w, const int8_t *flag,
                                  int kind, double nu, int nalpha, const double *alpha, bool null_output)
{
    if (kind != BPMF_HIP_LOGDENS_GAUSSIAN && kind != BPMF_HIP_LOGDENS_STUDENT && kind != BPMF_HIP_LOGDENS_PROBIT)
        return fail(BPMF_HIP_EINVAL, who + ": unknown kind " + std::to_string(kind) + " (BPMF_HIP_LOGDENS_GAUSSIAN, _STUDENT, _PROBIT)");
    if (!alpha) return fail(BPMF_HIP_EINVAL, who + ": NULL alpha");
    if (n > 0 && (!y || null_output)) return fail(BPMF_HIP_EINVAL, who + ": NULL argument");
    if (kind != BPMF_HIP_LOGDENS_GAUSSIAN && flag) return fail(BPMF_HIP_EINVAL, who + ": censoring flags go with the gaussian kind alone");
    if (kind != BPMF_HIP_LOGDENS_GAUSSIAN && w) return fail(BPMF_HIP_EINVAL, who + ": weights go with the gaussian kind alone");
    if (kind == BPMF_HIP_LOGDENS_STUDENT && !(std::isfinite(nu) && nu >= 1.0))
        return fail(BPMF_HIP_EINVAL, who + ": the degrees of freedom nu must be finite and >= 1");
    if (nalpha < 1) return fail(BPMF_HIP_EINVAL, who + ": nalpha must be 1 or the number of samples");
    for (int s = 0; s < nalpha; ++s)
        if (!(std::isfinite(alpha[s]) && alpha[s] > 0.0))
            return fail(BPMF_HIP_EINVAL, who + ": alpha of sample " + std::to_string(s) + " is not finite and > 0");
    for (int64_t i = 0; i < n; ++i) {                                          // before the device is used
        if (!std::isfinite(y[i])) return fail(BPMF_HIP_EINVAL, who + ": the value of " + cell_name(i, q, cc) + " is not finite");
        if (w && !(std::isfinite(w[i]) && w[i] > 0.0)) return fail(BPMF_HIP_EINVAL, who + ": the weight of " + cell_name(i, q, cc) + " is not finite and > 0");
        if (flag && (flag[i] < -1 || flag[i] > 1))
            return fail(BPMF_HIP_EINVAL, who + ": the flag " + std::to_string((int)flag[i]) + " of " + cell_name(i, q, cc) + " is not -1, 0 or +1");
    }
    return 0;
}

std::vector<double> bpmf_capi::logdens_constants(int kind, double nu, int nalpha, const double *alpha, int S)
{
    std::vector<double> cst((size_t)3 * (size_t)S);
    const double kPi = 3.14159265358979323846;
    const double lg = kind == BPMF_HIP_LOGDENS_STUDENT ? std::lgamma(0.5 * (nu + 1.0)) - std::lgamma(0.5 * nu) : 0.0;
    for (int s = 0; s < S; ++s) {
        const double al = alpha[nalpha == 1 ? 0 : s];
        cst[(size_t)s] = kind == BPMF_HIP_LOGDENS_STUDENT ? lg + 0.5 * std::log(al / (nu * kPi)) : 0.5 * std::log(al / (2.0 * kPi));
        cst[(size_t)S + s] = kind == BPMF_HIP_LOGDENS_STUDENT ? al / nu : al;
        cst[(size_t)2 * S + s] = std::sqrt(al);
    }
    return cst;
}

extern "C" int bpmf_hip_score_batch_cells(int cells)
{
    if (cells < 0) return fail(BPMF_HIP_EINVAL, "score_batch_cells: the cells per batch must be >= 0 (0: automatic)");
    g_batch_cells.store(cells);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_score_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q, const int32_t *cc,
                                    const double *y, const double *w, const int8_t *flag, int kind, double nu, int nalpha, const double *alpha,
                                    double *lpd_out, double *pw_out, double *mean_out, double *std_out)
{
    { const int rc = cells_check_list("score_cells", query, cand, mean_rating, n, q, cc); if (rc) return rc; }
    { const int rc = logdens_check_args("score_cells", n, q, cc, y, w, flag, kind, nu, nalpha, alpha, !lpd_out || !pw_out || !mean_out || !std_out); if (rc) return rc; }
    bpmf_launch::ScoreCellsLaunch sl{};
    bpmf_launch::PredCellsLaunch &p = sl.cells;
    int rc;
    if ((rc = pair_open_rings("score_cells", query, cand, &p.r))) return rc;
    const int S = p.r.S;
    if (nalpha != 1 && nalpha != S)
        return fail(BPMF_HIP_EINVAL, "score_cells: " + std::to_string(nalpha) + " values of alpha for " + std::to_string(S) + " samples (1 or as many)");
    if (n == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = query->ctx;
    Timed &timed = query->ring->score;

    const std::vector<double> cst = logdens_constants(kind, nu, nalpha, alpha, S);     // c0 | as | sa
    std::vector<int8_t> sign;                                                  // probit: the label of a cell as the kernel's flag
    if (kind == BPMF_HIP_LOGDENS_PROBIT) {
        sign.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) sign[(size_t)i] = y[i] > 0.0 ? 1 : -1;
    }
    bool any_flag = false;
    if (flag) for (int64_t i = 0; i < n && !any_flag; ++i) any_flag = flag[i] != 0;

    // batches of sorted cells, one launch each, in stream order
    const CellsSorted sorted = cells_sort(query->ncols, n, q, cc);
    const int forced = g_batch_cells.load();
    CellsPlan plan(sorted, n, std::min<int64_t>(n, forced > 0 ? forced : kBatchCells), bpmf_launch::score_cells_segment(p.r.Kp));
    DevBuf<double> out, d_y, d_w, d_cst;
    DevBuf<int8_t> d_flag;
    if ((rc = plan.upload()) || (rc = out.alloc((size_t)4 * (size_t)n)) || (rc = d_y.upload(y, (size_t)n)) || (rc = d_cst.upload(cst.data(), cst.size())))
        return rc;
    if (w && (rc = d_w.upload(w, (size_t)n))) return rc;
    if (kind == BPMF_HIP_LOGDENS_PROBIT) { if ((rc = d_flag.upload(sign.data(), sign.size()))) return rc; }
    else if (any_flag && (rc = d_flag.upload(flag, (size_t)n))) return rc;
    p.mean_rating = mean_rating;
    p.mean = out.get() + 2 * n; p.std = out.get() + 3 * n;
    sl.kind = kind; sl.nu = nu;
    sl.y = d_y.get(); sl.w = w ? d_w.get() : nullptr;
    sl.flag = (kind == BPMF_HIP_LOGDENS_PROBIT || any_flag) ? d_flag.get() : nullptr;      // without a censored cell: the plain form
    sl.c0 = d_cst.get(); sl.as = d_cst.get() + S; sl.sa = d_cst.get() + 2 * (size_t)S;
    sl.lpd = out.get(); sl.pw = out.get() + n;
    if ((rc = timed.begin(c->stream.get()))) return rc;
    for (size_t b = 0; b < plan.nbatches(); ++b) {
        plan.bind(p, b);
        if (bpmf_launch::score_cells(sl, c->stream.get())) return fail(BPMF_HIP_EINVAL, "score_cells: unsupported shape");
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "score_cells: kernel launch failed");
    }
    if ((rc = timed.end(c->stream.get())) || (rc = bounded_stream_sync(c, c->stream.get(), "score_cells"))) return rc;
    timed.resolve();
    return copy_back("score_cells", {{lpd_out, out.get(), (size_t)n}, {pw_out, out.get() + n, (size_t)n}, {mean_out, out.get() + 2 * n, (size_t)n},
                                     {std_out, out.get() + 3 * n, (size_t)n}});
}

extern "C" int bpmf_hip_score_last_ms(const bpmf_hip_side *query, float *ms)
{
    return last_ms("score_last_ms", query, query && query->ring ? &query->ring->score : nullptr, ms,
                   "no scoring with the side as the queries has been timed (bpmf_hip_score_cells)");
}
