// capi_interval.hip -- predictive intervals (kernel in kernels_interval.h): the probability integral transform of an
// observed value and quantiles of the posterior predictive mixture, of a list of cells over two sample rings (bpmf_hip_interval_cells:
// k_cell_traces, then k_trace_quantiles on the traces it left) and of traces the host gives (bpmf_hip_interval_traces).
// (one of the translation units of the C ABI of include/bpmf_hip.h: see capi_internal.h for the map)
#include "capi_internal.h"

#include <functional>

using namespace bpmf_capi;

namespace {

std::atomic<int> g_batch_cells{0};                                     // bpmf_hip_interval_batch_cells (0: from the trace buffer's size)

// What both entry points refuse of their own arguments, on the host; name(i): how item i is called in a refusal
int check_args(const std::string &who, int64_t n, const double *y, const double *w, int nalpha, const double *alpha, int nq, const double *tau,
               const double *pit_out, const double *quant_out, const std::function<std::string(int64_t)> &name)
{
    const int maxq = bpmf_launch::interval_max_quantiles();
    if (nq < 0 || nq > maxq) return fail(BPMF_HIP_EINVAL, who + ": nq = " + std::to_string(nq) + " quantiles (0 .. " + std::to_string(maxq) + ")");
    if (!y && nq == 0) return fail(BPMF_HIP_EINVAL, who + ": nothing to do (y is NULL and nq = 0)");
    if (nq > 0 && !tau) return fail(BPMF_HIP_EINVAL, who + ": NULL tau");
    for (int j = 0; j < nq; ++j) {
        if (!(tau[j] >= 0.001 && tau[j] <= 0.999)) return fail(BPMF_HIP_EINVAL, who + ": tau " + std::to_string(j) + " is outside [0.001, 0.999]");
        if (j > 0 && !(tau[j] > tau[j - 1])) return fail(BPMF_HIP_EINVAL, who + ": tau " + std::to_string(j) + " is not above tau " + std::to_string(j - 1) + " (strictly increasing)");
    }
    if (!alpha) return fail(BPMF_HIP_EINVAL, who + ": NULL alpha");
    if (nalpha < 1) return fail(BPMF_HIP_EINVAL, who + ": nalpha must be 1 or the number of samples");
    for (int s = 0; s < nalpha; ++s)
        if (!(std::isfinite(alpha[s]) && alpha[s] > 0.0))
            return fail(BPMF_HIP_EINVAL, who + ": alpha of sample " + std::to_string(s) + " is not finite and > 0");
    for (int64_t i = 0; i < n; ++i) {
        if (y && !std::isfinite(y[i])) return fail(BPMF_HIP_EINVAL, who + ": the value of " + name(i) + " is not finite");
        if (w && !(std::isfinite(w[i]) && w[i] > 0.0)) return fail(BPMF_HIP_EINVAL, who + ": the weight of " + name(i) + " is not finite and > 0");
    }
    if (n > 0 && y && !pit_out) return fail(BPMF_HIP_EINVAL, who + ": NULL pit output with y given");
    if (n > 0 && nq > 0 && !quant_out) return fail(BPMF_HIP_EINVAL, who + ": NULL quantile output with nq > 0");
    return 0;
}

int check_samples(const std::string &who, int S, int nalpha)
{
    if (S < 1 || S > bpmf_launch::interval_max_samples())
        return fail(BPMF_HIP_EINVAL, who + ": " + std::to_string(S) + " samples: the root finder takes 1 .. " + std::to_string(bpmf_launch::interval_max_samples()) +
                    " (BPMF_HIP_INTERVAL_MAX_SAMPLES)");
    if (nalpha != 1 && nalpha != S)
        return fail(BPMF_HIP_EINVAL, who + ": " + std::to_string(nalpha) + " values of alpha for " + std::to_string(S) + " samples (1 or as many)");
    return 0;
}

// What the launches of a call share: y, w and sqrt(alpha_s) on the device, tau and z, the outputs pit | quant (n, n x nq doubles)
struct Inputs {
    DevBuf<double> d_y, d_w, d_sa, out;
    int fill(bpmf_launch::TraceQuantLaunch &t, int64_t n, int S, double mean_rating, const double *y, const double *w, int nalpha, const double *alpha,
             int nq, const double *tau)
    {
        int rc;
        if ((rc = out.alloc((size_t)n * (size_t)(1 + nq)))) return rc;
        if (y && (rc = d_y.upload(y, (size_t)n))) return rc;
        if (w && (rc = d_w.upload(w, (size_t)n))) return rc;
        if (nalpha != 1) {
            std::vector<double> sa((size_t)S);
            for (int s = 0; s < S; ++s) sa[(size_t)s] = std::sqrt(alpha[s]);
            if ((rc = d_sa.upload(sa.data(), sa.size()))) return rc;
        }
        t.S = S; t.mean_rating = mean_rating;
        t.y = y ? d_y.get() : nullptr; t.w = w ? d_w.get() : nullptr;
        t.sa = nalpha != 1 ? d_sa.get() : nullptr; t.sa0 = std::sqrt(alpha[0]);
        t.nq = nq;
        for (int j = 0; j < nq; ++j) { t.tau[j] = tau[j]; t.z[j] = normal_quantile(tau[j]); }
        t.pit = out.get(); t.quant = out.get() + n;
        return 0;
    }
};

}  // namespace

extern "C" int bpmf_hip_interval_batch_cells(int cells)
{
    if (cells < 0) return fail(BPMF_HIP_EINVAL, "interval_batch_cells: the cells per batch must be >= 0 (0: automatic)");
    g_batch_cells.store(cells);
    return BPMF_HIP_OK;
}

extern "C" int bpmf_hip_interval_traces(bpmf_hip_ctx *c, int64_t n, int S, const double *traces, double mean_rating, const double *y, const double *w,
                                        int nalpha, const double *alpha, int nq, const double *tau, double *pit_out, double *quant_out)
{
    const std::string who = "interval_traces";
    if (!c) return fail(BPMF_HIP_EINVAL, who + ": NULL context");
    if (n < 0 || n > 0x7fffffff) return fail(BPMF_HIP_EINVAL, who + ": n must be 0 .. 2^31 - 1");
    if (!std::isfinite(mean_rating)) return fail(BPMF_HIP_EINVAL, who + ": mean_rating is not finite");
    int rc;
    if ((rc = check_args(who, n, y, w, nalpha, alpha, nq, tau, pit_out, quant_out, [](int64_t i) { return "trace " + std::to_string((long long)i); })) ||
        (rc = check_samples(who, S, nalpha)))
        return rc;
    if (n == 0) return BPMF_HIP_OK;
    if (!traces) return fail(BPMF_HIP_EINVAL, who + ": NULL traces");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t step = std::min<int64_t>(n, trace_batch_cells(S, g_batch_cells.load()));
    bpmf_launch::TraceQuantLaunch t{};
    Inputs in;
    DevBuf<double> buf;
    if ((rc = in.fill(t, n, S, mean_rating, y, w, nalpha, alpha, nq, tau)) || (rc = buf.alloc((size_t)step * (size_t)S))) return rc;
    for (int64_t b0 = 0; b0 < n; b0 += step) {                             // batch b reads y, w and writes its outputs at b0 ..
        const int64_t nb = std::min<int64_t>(step, n - b0);
        HIP_TRY(hipMemcpyAsync(buf.get(), traces + (size_t)b0 * (size_t)S, (size_t)nb * (size_t)S * sizeof(double), hipMemcpyHostToDevice, c->stream.get()));
        bpmf_launch::TraceQuantLaunch tb = t;
        tb.traces = buf.get(); tb.ntr = nb; tb.orig = nullptr;
        if (tb.y) tb.y += b0;
        if (tb.w) tb.w += b0;
        tb.pit += b0; tb.quant += b0 * nq;
        if (bpmf_launch::trace_quantiles(tb, c->stream.get())) return fail(BPMF_HIP_EINVAL, who + ": unsupported shape");
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, who + ": kernel launch failed");
        if ((rc = bounded_stream_sync(c, c->stream.get(), "interval_traces"))) return rc;     // the buffer is free for the next batch
    }
    return copy_back(who, {{y ? pit_out : nullptr, in.out.get(), (size_t)n}, {quant_out, in.out.get() + n, (size_t)n * (size_t)nq}});
}

extern "C" int bpmf_hip_interval_cells(bpmf_hip_side *query, bpmf_hip_side *cand, double mean_rating, int64_t n, const int32_t *q, const int32_t *cc,
                                       const double *y, const double *w, int nalpha, const double *alpha, int nq, const double *tau, double *pit_out,
                                       double *quant_out, double *mean_out, double *std_out)
{
    const std::string who = "interval_cells";
    int rc;
    if ((rc = cells_check_list(who, query, cand, mean_rating, n, q, cc)) ||
        (rc = check_args(who, n, y, w, nalpha, alpha, nq, tau, pit_out, quant_out, [&](int64_t i) {
             return "cell " + std::to_string((long long)i) + " (" + std::to_string(q[i]) + ", " + std::to_string(cc[i]) + ")";
         })))
        return rc;
    bpmf_launch::PredCellsLaunch p{};
    if ((rc = pair_open_rings(who, query, cand, &p.r)) || (rc = check_samples(who, p.r.S, nalpha))) return rc;
    if (n == 0) return BPMF_HIP_OK;
    bpmf_hip_ctx *c = query->ctx;
    Timed &timed = query->ring->interval;
    const int S = p.r.S;

    // batches of sorted cells: one trace buffer, filled by k_cell_traces and read by k_trace_quantiles of the batch, in stream order
    const CellsSorted sorted = cells_sort(query->ncols, n, q, cc);
    CellsPlan plan(sorted, n, std::min<int64_t>(n, trace_batch_cells(S, g_batch_cells.load())), bpmf_launch::cell_traces_segment(p.r.Kp));
    bpmf_launch::TraceQuantLaunch t{};
    Inputs in;
    DevBuf<double> ms, trace;
    if ((rc = plan.upload()) || (rc = in.fill(t, n, S, mean_rating, y, w, nalpha, alpha, nq, tau)) || (rc = ms.alloc((size_t)2 * (size_t)n)) ||
        (rc = trace.alloc((size_t)plan.step * (size_t)S)))
        return rc;
    p.mean_rating = mean_rating;
    p.mean = ms.get(); p.std = ms.get() + n;
    t.traces = trace.get();
    if ((rc = timed.begin(c->stream.get()))) return rc;
    for (size_t b = 0; b < plan.nbatches(); ++b) {
        plan.bind(p, b);
        t.ntr = plan.cells(b); t.orig = plan.orig() + plan.begin(b);
        if (bpmf_launch::cell_traces(p, trace.get(), plan.begin(b), c->stream.get()) || bpmf_launch::trace_quantiles(t, c->stream.get()))
            return fail(BPMF_HIP_EINVAL, who + ": unsupported shape");
        if (hipGetLastError() != hipSuccess) return fail(BPMF_HIP_ENODEV, who + ": kernel launch failed");
    }
    if ((rc = timed.end(c->stream.get())) || (rc = bounded_stream_sync(c, c->stream.get(), "interval_cells"))) return rc;
    timed.resolve();
    return copy_back(who, {{y ? pit_out : nullptr, in.out.get(), (size_t)n}, {quant_out, in.out.get() + n, (size_t)n * (size_t)nq},
                           {mean_out, ms.get(), (size_t)n}, {std_out, ms.get() + n, (size_t)n}});
}

extern "C" int bpmf_hip_interval_last_ms(const bpmf_hip_side *query, float *ms)
{
    return last_ms("interval_last_ms", query, query && query->ring ? &query->ring->interval : nullptr, ms,
                   "no intervals with the side as the queries have been timed (bpmf_hip_interval_cells)");
}
