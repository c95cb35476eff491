// capi_diag.hip -- convergence diagnostics (kernels in kernels_diag.h): split-Rhat and the effective sample size
// of traces the host gives (bpmf_hip_diag_traces) and of the predictions of a list of cells over two sample rings (bpmf_hip_diag_cells);
// and over several chains (kernels_diag_mc.h): the rank-normalised split-Rhat, bulk and tail ESS of chain-major
// traces (bpmf_hip_diag_traces_mc) and of a list of cells over two pooled rings (bpmf_hip_diag_cells_mc).
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

using namespace bpmf_capi;

// The trace buffer of a batch.  A batch must fill the device on its own (its two kernels run behind those of the batch before): at the
// ML-1M shape, 100 k cells, K = 32, S = 1000, batches of 8 388 cells (64 MiB) took 18.8 ms, of 32 768 cells 12.6 ms, one batch of all
// cells (800 MB) 10.2 ms, beside 9.6 ms of k_predict_cells
int64_t bpmf_capi::trace_batch_cells(int S, int forced)
{
    constexpr int64_t kTraceBytes = (int64_t)256 << 20;
    return forced > 0 ? forced : std::max<int64_t>(1, kTraceBytes / ((int64_t)S * (int64_t)sizeof(double)));
}

namespace {

std::atomic<int> g_batch_cells{0};                                     // bpmf_hip_diag_batch_cells (0: from the trace buffer's size)

int64_t batch_traces(int S) { return trace_batch_cells(S, g_batch_cells.load()); }

int refuse_samples(const std::string &who, int S)
{
    if (S < bpmf_launch::diag_min_samples() || S > bpmf_launch::diag_max_samples())
        return fail(BPMF_HIP_EINVAL, who + ": " + std::to_string(S) + " samples: the estimator takes " + std::to_string(bpmf_launch::diag_min_samples()) +
                    " .. " + std::to_string(bpmf_launch::diag_max_samples()) + " (BPMF_HIP_DIAG_MAX_SAMPLES)");
    return 0;
}

int refuse_chains(const std::string &who, int C, int S)
{
    const int cmax = bpmf_launch::diag_mc_max_chains(), smin = bpmf_launch::diag_mc_min_samples(), vmax = bpmf_launch::diag_mc_max_values();
    if (C < 1 || C > cmax)
        return fail(BPMF_HIP_EINVAL, who + ": " + std::to_string(C) + " chains: the estimator takes 1 .. " + std::to_string(cmax));
    if (S < smin || (int64_t)C * (int64_t)S > vmax)
        return fail(BPMF_HIP_EINVAL, who + ": " + std::to_string(S) + " samples per chain in " + std::to_string(C) + " chains: the estimator takes " +
                    std::to_string(smin) + " or more per chain and " + std::to_string(vmax) + " in all (BPMF_HIP_DIAG_MAX_SAMPLES)");
    return 0;
}

}  // namespace

extern "C" int bpmf_hip_diag_batch_cells(int cells)
{
    if (cells < 0) return fail(BPMF_HIP_EINVAL, "diag_batch_cells: the cells per batch must be >= 0 (0: automatic)");
    g_batch_cells.store(cells);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_diag_traces(bpmf_hip_ctx *c, int64_t n, int S, const double *traces, double *rhat, double *ess)
{
    if (!c) return fail(BPMF_HIP_EINVAL, "diag_traces: NULL context");
    if (n < 0 || n > 0x7fffffff) return fail(BPMF_HIP_EINVAL, "diag_traces: n must be 0 .. 2^31 - 1");
    { const int rb = refuse_samples("diag_traces", S); if (rb) return rb; }
    if (n == 0) return BPMF_HIP_OK;
    if (!traces || !rhat || !ess) return fail(BPMF_HIP_EINVAL, "diag_traces: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t step = std::min<int64_t>(n, batch_traces(S));
    DevBuf<double> buf, out;
    int rc;
    if ((rc = buf.alloc((size_t)step * (size_t)S)) || (rc = out.alloc((size_t)2 * (size_t)step))) return rc;
    for (int64_t b0 = 0; b0 < n; b0 += step) {
        const int64_t nb = std::min<int64_t>(step, n - b0);
        HIP_TRY(hipMemcpyAsync(buf.get(), traces + (size_t)b0 * (size_t)S, (size_t)nb * (size_t)S * sizeof(double), hipMemcpyHostToDevice, c->stream.get()));
        if (bpmf_launch::trace_diag(buf.get(), nb, S, nullptr, out.get(), out.get() + step, c->stream.get()))
            return fail(BPMF_HIP_EINVAL, "diag_traces: unsupported shape");
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "diag_traces: kernel launch failed");
        if ((rc = bounded_stream_sync(c, c->stream.get(), "diag_traces")) ||
            (rc = copy_back("diag_traces", {{rhat + b0, out.get(), (size_t)nb}, {ess + b0, out.get() + step, (size_t)nb}})))
            return rc;
    }
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_diag_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q, const int32_t *cc,
                                   double *mean_out, double *std_out, double *rhat_out, double *ess_out)
{
    { const int rc = cells_check_list("diag_cells", query, cand, mean_rating, n, q, cc); if (rc) return rc; }
    if (n > 0 && (!mean_out || !std_out || !rhat_out || !ess_out)) return fail(BPMF_HIP_EINVAL, "diag_cells: NULL output");
    bpmf_launch::PredCellsLaunch p{};
    int rc;
    if ((rc = pair_open_rings("diag_cells", query, cand, &p.r)) || (rc = refuse_samples("diag_cells", p.r.S))) return rc;
    if (n == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = query->ctx;
    Timed &timed = query->ring->diag;
    const int S = p.r.S;

    // batches of sorted cells: one trace buffer, filled by k_cell_traces and read by k_trace_diag of the batch, in stream order (no
    // wait in between)
    const CellsSorted sorted = cells_sort(query->ncols, n, q, cc);
    CellsPlan plan(sorted, n, std::min<int64_t>(n, batch_traces(S)), bpmf_launch::cell_traces_segment(p.r.Kp));
    DevBuf<double> out, trace;
    if ((rc = plan.upload()) || (rc = out.alloc((size_t)4 * (size_t)n)) || (rc = trace.alloc((size_t)plan.step * (size_t)S))) return rc;
    p.mean_rating = mean_rating;
    p.mean = out.get(); p.std = out.get() + n;
    if ((rc = timed.begin(c->stream.get()))) return rc;
    for (size_t b = 0; b < plan.nbatches(); ++b) {
        plan.bind(p, b);
        if (bpmf_launch::cell_traces(p, trace.get(), plan.begin(b), c->stream.get()) ||
            bpmf_launch::trace_diag(trace.get(), plan.cells(b), S, plan.orig() + plan.begin(b), out.get() + 2 * n, out.get() + 3 * n, c->stream.get()))
            return fail(BPMF_HIP_EINVAL, "diag_cells: unsupported shape");
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "diag_cells: kernel launch failed");
    }
    if ((rc = timed.end(c->stream.get())) || (rc = bounded_stream_sync(c, c->stream.get(), "diag_cells"))) return rc;
    timed.resolve();
    return copy_back("diag_cells", {{mean_out, out.get(), (size_t)n}, {std_out, out.get() + n, (size_t)n}, {rhat_out, out.get() + 2 * n, (size_t)n},
                                    {ess_out, out.get() + 3 * n, (size_t)n}});
}

extern "C" int bpmf_hip_diag_traces_mc(bpmf_hip_ctx *c, int64_t n, int C, int S, const double *traces, double *rhat, double *ess_bulk,
                                       double *ess_tail)
{
    if (!c) return fail(BPMF_HIP_EINVAL, "diag_traces_mc: NULL context");
    if (n < 0 || n > 0x7fffffff) return fail(BPMF_HIP_EINVAL, "diag_traces_mc: n must be 0 .. 2^31 - 1");
    { const int rb = refuse_chains("diag_traces_mc", C, S); if (rb) return rb; }
    if (n == 0) return BPMF_HIP_OK;
    if (!traces || !rhat || !ess_bulk || !ess_tail) return fail(BPMF_HIP_EINVAL, "diag_traces_mc: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const int L = C * S;
    const int64_t step = std::min<int64_t>(n, batch_traces(L));
    DevBuf<double> buf, out;
    int rc;
    if ((rc = buf.alloc((size_t)step * (size_t)L)) || (rc = out.alloc((size_t)3 * (size_t)step))) return rc;
    for (int64_t b0 = 0; b0 < n; b0 += step) {
        const int64_t nb = std::min<int64_t>(step, n - b0);
        HIP_TRY(hipMemcpyAsync(buf.get(), traces + (size_t)b0 * (size_t)L, (size_t)nb * (size_t)L * sizeof(double), hipMemcpyHostToDevice, c->stream.get()));
        if (bpmf_launch::trace_diag_mc(buf.get(), nb, C, S, nullptr, out.get(), out.get() + step, out.get() + 2 * step, c->stream.get()))
            return fail(BPMF_HIP_EINVAL, "diag_traces_mc: unsupported shape");
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "diag_traces_mc: kernel launch failed");
        if ((rc = bounded_stream_sync(c, c->stream.get(), "diag_traces_mc")) ||
            (rc = copy_back("diag_traces_mc", {{rhat + b0, out.get(), (size_t)nb}, {ess_bulk + b0, out.get() + step, (size_t)nb},
                                               {ess_tail + b0, out.get() + 2 * step, (size_t)nb}})))
            return rc;
    }
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_diag_cells_mc(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q, const int32_t *cc,
                                      int C, double *mean_out, double *std_out, double *rhat_out, double *ess_bulk_out, double *ess_tail_out)
{
    { const int rc = cells_check_list("diag_cells_mc", query, cand, mean_rating, n, q, cc); if (rc) return rc; }
    if (n > 0 && (!mean_out || !std_out || !rhat_out || !ess_bulk_out || !ess_tail_out)) return fail(BPMF_HIP_EINVAL, "diag_cells_mc: NULL output");
    bpmf_launch::PredCellsLaunch p{};
    int rc;
    if ((rc = pair_open_rings("diag_cells_mc", query, cand, &p.r))) return rc;
    if (C < 1 || C > bpmf_launch::diag_mc_max_chains()) return refuse_chains("diag_cells_mc", C, bpmf_launch::diag_mc_min_samples());
    if (p.r.S % C != 0)
        return fail(BPMF_HIP_EINVAL, "diag_cells_mc: the rings hold " + std::to_string(p.r.S) + " samples, which is not " + std::to_string(C) +
                    " chains of one length");
    const int S = p.r.S / C, L = p.r.S;
    if ((rc = refuse_chains("diag_cells_mc", C, S))) return rc;
    if (n == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = query->ctx;
    Timed &timed = query->ring->diag;

    // as bpmf_hip_diag_cells: batches of sorted cells, k_cell_traces writes the chain-major traces (the order of the pooled rings)
    const CellsSorted sorted = cells_sort(query->ncols, n, q, cc);
    CellsPlan plan(sorted, n, std::min<int64_t>(n, batch_traces(L)), bpmf_launch::cell_traces_segment(p.r.Kp));
    DevBuf<double> out, trace;
    if ((rc = plan.upload()) || (rc = out.alloc((size_t)5 * (size_t)n)) || (rc = trace.alloc((size_t)plan.step * (size_t)L))) return rc;
    p.mean_rating = mean_rating;
    p.mean = out.get(); p.std = out.get() + n;
    if ((rc = timed.begin(c->stream.get()))) return rc;
    for (size_t b = 0; b < plan.nbatches(); ++b) {
        plan.bind(p, b);
        if (bpmf_launch::cell_traces(p, trace.get(), plan.begin(b), c->stream.get()) ||
            bpmf_launch::trace_diag_mc(trace.get(), plan.cells(b), C, S, plan.orig() + plan.begin(b), out.get() + 2 * n, out.get() + 3 * n,
                                       out.get() + 4 * n, c->stream.get()))
            return fail(BPMF_HIP_EINVAL, "diag_cells_mc: unsupported shape");
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, "diag_cells_mc: kernel launch failed");
    }
    if ((rc = timed.end(c->stream.get())) || (rc = bounded_stream_sync(c, c->stream.get(), "diag_cells_mc"))) return rc;
    timed.resolve();
    return copy_back("diag_cells_mc", {{mean_out, out.get(), (size_t)n}, {std_out, out.get() + n, (size_t)n}, {rhat_out, out.get() + 2 * n, (size_t)n},
                                       {ess_bulk_out, out.get() + 3 * n, (size_t)n}, {ess_tail_out, out.get() + 4 * n, (size_t)n}});
}

extern "C" int bpmf_hip_diag_last_ms(const bpmf_hip_side *query, float *ms)
{
    return last_ms("diag_last_ms", query, query && query->ring ? &query->ring->diag : nullptr, ms,
                   "no diagnostics with the side as the queries have been timed (bpmf_hip_diag_cells)");
}
