// capi_loo.hip -- PSIS-LOO cross-validation (kernel in kernels_loo.h): the Pareto-smoothed importance sampling
// estimate of the leave-one-out log predictive density, and its diagnostic khat, of a list of observed cells over two sample rings
// (bpmf_hip_loo_cells: k_cell_traces, then k_trace_psis on the traces it left) and of traces of log densities the host gives
// (bpmf_hip_loo_traces).
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

namespace {

std::atomic<int> g_batch_cells{0};                                     // bpmf_hip_loo_batch_cells (0: from the trace buffer's size)

int check_samples(const std::string &who, int S)
{
    if (S < 1 || S > bpmf_launch::loo_max_samples())
        return fail(BPMF_HIP_EINVAL, who + ": " + std::to_string(S) + " samples: the tail is sorted for 1 .. " + std::to_string(bpmf_launch::loo_max_samples()) +
                    " (BPMF_HIP_LOO_MAX_SAMPLES)");
    return 0;
}

}  // namespace

extern "C" int bpmf_hip_loo_batch_cells(int cells)
{
    if (cells < 0) return fail(BPMF_HIP_EINVAL, "loo_batch_cells: the cells per batch must be >= 0 (0: automatic)");
    g_batch_cells.store(cells);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_loo_traces(bpmf_hip_ctx *c, int64_t n, int S, const double *logdens, double *elpd_out, double *khat_out, double *lpd_out)
{
    const std::string who = "loo_traces";
    if (!c) return fail(BPMF_HIP_EINVAL, who + ": NULL context");
    if (n < 0 || n > 0x7fffffff) return fail(BPMF_HIP_EINVAL, who + ": n must be 0 .. 2^31 - 1");
    int rc;
    if ((rc = check_samples(who, S))) return rc;
    if (n == 0) return BPMF_HIP_OK;
    if (!logdens || !elpd_out || !khat_out) return fail(BPMF_HIP_EINVAL, who + ": NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t step = std::min<int64_t>(n, trace_batch_cells(S, g_batch_cells.load()));
    DevBuf<double> buf, out;
    if ((rc = out.alloc((size_t)3 * (size_t)n)) || (rc = buf.alloc((size_t)step * (size_t)S))) return rc;
    for (int64_t b0 = 0; b0 < n; b0 += step) {                             // batch b writes its outputs at b0 ..
        const int64_t nb = std::min<int64_t>(step, n - b0);
        HIP_TRY(hipMemcpyAsync(buf.get(), logdens + (size_t)b0 * (size_t)S, (size_t)nb * (size_t)S * sizeof(double), hipMemcpyHostToDevice, c->stream.get()));
        bpmf_launch::TracePsisLaunch t{};
        t.traces = buf.get(); t.ntr = nb; t.S = S; t.kind = -1;
        t.elpd = out.get() + b0; t.khat = out.get() + n + b0; t.lpd = out.get() + 2 * n + b0;
        if (bpmf_launch::trace_psis(t, c->stream.get())) return fail(BPMF_HIP_EINVAL, who + ": unsupported shape");
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, who + ": kernel launch failed");
        if ((rc = bounded_stream_sync(c, c->stream.get(), "loo_traces"))) return rc;          // the buffer is free for the next batch
    }
    return copy_back(who, {{elpd_out, out.get(), (size_t)n}, {khat_out, out.get() + n, (size_t)n}, {lpd_out, out.get() + 2 * n, (size_t)n}});
}

extern "C" int bpmf_hip_loo_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q, const int32_t *cc,
                                  const double *y, const double *w, const int8_t *flag, int kind, double nu, int nalpha, const double *alpha,
                                  double *elpd_out, double *khat_out, double *lpd_out, double *mean_out, double *std_out)
{
    const std::string who = "loo_cells";
    int rc;
    if ((rc = cells_check_list(who, query, cand, mean_rating, n, q, cc)) ||
        (rc = logdens_check_args(who, n, q, cc, y, w, flag, kind, nu, nalpha, alpha, !elpd_out || !khat_out)))
        return rc;
    bpmf_launch::PredCellsLaunch p{};
    if ((rc = pair_open_rings(who, query, cand, &p.r))) return rc;
    const int S = p.r.S;
    if (nalpha != 1 && nalpha != S)
        return fail(BPMF_HIP_EINVAL, who + ": " + std::to_string(nalpha) + " values of alpha for " + std::to_string(S) + " samples (1 or as many)");
    if ((rc = check_samples(who, S))) return rc;
    if (n == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = query->ctx;
    Timed &timed = query->ring->loo;

    const std::vector<double> cst = logdens_constants(kind, nu, nalpha, alpha, S);     // c0 | as | sa
    std::vector<int8_t> sign;                                                  // probit: the label of a cell as the kernel's flag
    if (kind == BPMF_HIP_LOGDENS_PROBIT) {
        sign.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) sign[(size_t)i] = y[i] > 0.0 ? 1 : -1;
    }
    bool any_flag = false;
    if (flag) for (int64_t i = 0; i < n && !any_flag; ++i) any_flag = flag[i] != 0;

    // batches of sorted cells: one trace buffer, filled by k_cell_traces and read by k_trace_psis of the batch, in stream order
    const CellsSorted sorted = cells_sort(query->ncols, n, q, cc);
    CellsPlan plan(sorted, n, std::min<int64_t>(n, trace_batch_cells(S, g_batch_cells.load())), bpmf_launch::cell_traces_segment(p.r.Kp));
    DevBuf<double> out, d_y, d_w, d_cst, trace;
    DevBuf<int8_t> d_flag;
    if ((rc = plan.upload()) || (rc = out.alloc((size_t)5 * (size_t)n)) || (rc = d_y.upload(y, (size_t)n)) || (rc = d_cst.upload(cst.data(), cst.size())) ||
        (rc = trace.alloc((size_t)plan.step * (size_t)S)))
        return rc;
    if (w && (rc = d_w.upload(w, (size_t)n))) return rc;
    if (kind == BPMF_HIP_LOGDENS_PROBIT) { if ((rc = d_flag.upload(sign.data(), sign.size()))) return rc; }
    else if (any_flag && (rc = d_flag.upload(flag, (size_t)n))) return rc;
    p.mean_rating = mean_rating;
    p.mean = out.get() + 3 * n; p.std = out.get() + 4 * n;
    bpmf_launch::TracePsisLaunch t{};
    t.traces = trace.get(); t.S = S; t.kind = kind; t.nu = nu; t.mean_rating = mean_rating;
    t.y = d_y.get(); t.w = w ? d_w.get() : nullptr;
    t.flag = (kind == BPMF_HIP_LOGDENS_PROBIT || any_flag) ? d_flag.get() : nullptr;       // without a censored cell: the plain form
    t.c0 = d_cst.get(); t.as = d_cst.get() + S; t.sa = d_cst.get() + 2 * (size_t)S;
    t.elpd = out.get(); t.khat = out.get() + n; t.lpd = out.get() + 2 * n;
    if ((rc = timed.begin(c->stream.get()))) return rc;
    for (size_t b = 0; b < plan.nbatches(); ++b) {
        plan.bind(p, b);
        t.ntr = plan.cells(b); t.orig = plan.orig() + plan.begin(b);
        if (bpmf_launch::cell_traces(p, trace.get(), plan.begin(b), c->stream.get()) || bpmf_launch::trace_psis(t, c->stream.get()))
            return fail(BPMF_HIP_EINVAL, who + ": unsupported shape");
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, who + ": kernel launch failed");
    }
    if ((rc = timed.end(c->stream.get())) || (rc = bounded_stream_sync(c, c->stream.get(), "loo_cells"))) return rc;
    timed.resolve();
    return copy_back(who, {{elpd_out, out.get(), (size_t)n}, {khat_out, out.get() + n, (size_t)n}, {lpd_out, out.get() + 2 * n, (size_t)n},
                           {mean_out, out.get() + 3 * n, (size_t)n}, {std_out, out.get() + 4 * n, (size_t)n}});
}

extern "C" int bpmf_hip_loo_last_ms(const bpmf_hip_side *query, float *ms)
{
    return last_ms("loo_last_ms", query, query && query->ring ? &query->ring->loo : nullptr, ms,
                   "no PSIS-LOO with the side as the queries has been timed (bpmf_hip_loo_cells)");
}
