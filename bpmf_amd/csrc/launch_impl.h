// launch_impl.h -- definitions of launch.h's templates: which kernel of kernels*.h runs for which
// form of a side, and with what arguments.  Included by the per-K units only.
#pragma once
#include "launch.h"
#include "kernels.h"
#include "kernels_f32.h"
#include "kernels_q4.h"
#include "kernels_slab.h"

namespace bpmf_launch {


// The device work of one half-iteration, in three pieces that the synchronous (stateless) and
// the asynchronous (stateful) paths put on their streams:
//   launch_sampler: the per-column update, reading the parameter blob `d_in`
//   launch_exchange: multi-GPU only, in-place broadcast of every rank's fresh column range
//   launch_stats: sum x / sum x x^T of this rank's columns (+ all-reduce), published to `out_host_dev`
// F32: the fp32 context (K = 128 only).  K = 128 with F32 = false is the reference's fp64 arithmetic at num_latent 65 .. 128.
template <int K, bool F32>
// ev_start / ev_stop (optional): recorded by the dispatch packet of the sampler itself
// (hipExtLaunchKernel) instead of by marker packets before and after it -- every marker is a few
// microseconds on the stream between two samplers.
int sampler_into(bpmf_hip_side *self, double *out_items, const bpmf_hip_side *other, int iter, double alpha, double *d_in, hipStream_t st,
                        hipEvent_t ev_start, hipEvent_t ev_stop)
{
    using namespace bpmf;
    bpmf_hip_ctx *c = self->ctx;
    SampleArgs a = blob_args(self, out_items, d_in, iter, alpha);
    // the ratings, or what stands in for them: latent scores / values, residuals (state.h)
    const double *vals = sampler_values(self);
    a.rowidx = self->d_rowidx; a.vals = vals;
    // side with per-rating weights (capi_weights.hip): the weighted form of the side's family reads
    // zw = sqrt(w) (r - mean) as its values with mean 0 and multiplies every gathered row by sw = sqrt(w)
    const bool wt = self->weights != nullptr;
    if (wt) {
        if constexpr (F32) return fail(BPMF_HIP_EINVAL, "per-rating weights: not on an fp32 context");
        if (!reads_own_ratings(self) || self->d_prop || self->reduce_on)        // (a robust side has weights and passes)
            return fail(BPMF_HIP_EINVAL, "per-rating weights: not together with probit, censored ratings, features, propagated priors or BPMF_REDUCE");
        a.vals = self->weights->zw.get(); a.sw = self->weights->sw.get(); a.mean_rating = 0.0;
    }
    // (item window: the whole list, or the items of one part of the columns -- bpmf_hip_side_set_overlap)
    const int w0 = self->item_n >= 0 ? self->item_off : 0, nwork = self->item_n >= 0 ? self->item_n : self->nwork;
    a.wi_col = self->d_wi_col.get() + w0; a.wi_p0 = self->d_wi_p0.get() + w0; a.wi_len = self->d_wi_len.get() + w0; a.wi_mc = self->d_wi_mc.get() + w0; a.wi_chunk = self->d_wi_chunk.get() + w0;
    a.mc_slot0 = self->d_mc_slot0.get(); a.mc_nchunks = self->d_mc_nch.get(); a.mc_count = self->d_mc_count.get();
    a.partials = self->d_partials.get(); a.nwork = nwork;
    a.other_items = other->d_items;
    a.ablate = c->ablate; a.stamps = c->d_stamps.get();
    a.gate_flag = self->cur_gate_flag; a.gate_want = self->cur_gate_want;
    a.tmo = self->cur_gate_flag ? blob::tmo_word(self->a_h_out.dev(), K) : nullptr; a.wait_ticks = wait_ticks();
    a.zero_row = c->d_zero.get();
    a.lf32 = (lf32_words(c) && !self->d_prop.get()) ? reinterpret_cast<const float *>(d_in + c->in_words) : nullptr;
    const bpmf::StatRiders &rr = self->cur_riders;                   // (K = 128 fp32 only)
    if constexpr (F32) {                                             // fp32 factors (items / other_items are float arrays): kernels_wg2.h, T = float
        if (nwork > 0) k128_wg2(nwork, st, ev_start, ev_stop, a, rr);
        return 0;
    } else if constexpr (K == 128) {                                 // fp64 factors, workgroup of four waves per item (kernels_wg2.h, T = double)
        if (nwork > 0 && wt) k128_wg2w_f64(nwork, st, ev_start, ev_stop, a, rr);
        else if (nwork > 0) k128_wg2_f64(nwork, st, ev_start, ev_stop, a, rr);
        return 0;
    } else {
    if constexpr (K <= 32) {
        if (nwork > 0 && self->mode == 3) {                          // four columns per wave (k_sample4)
            if (wt) sample4w<K>((nwork + 3) / 4, st, ev_start, ev_stop, a);
            else BPMF_LAUNCH(k_sample4<K>, dim3((nwork + 3) / 4), dim3(64), st, ev_start, ev_stop, a);
            return 0;
        }
    }
    if constexpr (K == 64) {
        // (a weighted side: every column in the slab form -- the product form has no weighted variant)
        if (self->lr_n > 0 && !self->d_prop && !c->diag_only && !(c->ablate & 3u) && !wt) {
            // light columns (<= 16 ratings): product form over the shared factor of LambdaF (k_sample_pf); the others in the slab form
            if (self->hv_nwork > 0) {
                a.wi_col = self->d_hv_col.get(); a.wi_p0 = self->d_hv_p0.get(); a.wi_len = self->d_hv_len.get(); a.wi_mc = self->d_hv_mc.get();
                a.wi_chunk = self->d_hv_chunk.get(); a.nwork = self->hv_nwork;
                k64_slab(self->hv_nwork, st, ev_start, nullptr, a);
            }
            LrArgs l;
            l.rowidx = self->d_rowidx; l.vals = vals; l.col = self->d_lr_col.get(); l.p0 = self->d_lr_p0.get(); l.len = self->d_lr_len.get();
            l.nitems = self->lr_n; l.other_items = other->d_items; l.items = out_items; l.col_from = self->from;
            l.R0 = d_in + blob::par_R0(K); l.S0t = d_in + blob::par_S0t(K); l.y0 = d_in + blob::par_y0(K);
            l.Lmu = a.Lmu; l.fail = a.fail;
            l.mean_rating = self->mean_rating; l.alpha = alpha; l.sqrt_alpha = std::sqrt(alpha); l.iter_plus_1 = (uint32_t)(iter + 1); l.ktrue = c->Kt;
            // three instantiations (<= 3, <= 6, <= 16 ratings), persistent workgroups of eight waves with R0^-1 in LDS
            // (the events ride on the first / last launch of the side)
            l.Q = self->d_pf_q.get();
            bool started = self->hv_nwork > 0;
            if (self->pf_class[3] > self->pf_class[0] && self->d_pf_q) {
                // Q = U_other R0^-1 once per half-iteration (k_pf_prepare), ahead of the product-form launches
                const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((self->nrows + 7) / 8, (int64_t)c->num_cu * 4));
                k64_pf_prepare(grid, st, started ? nullptr : ev_start, l.S0t, other->d_items, self->nrows, self->d_pf_q.get());
                started = true;
            }
            int last_pf = -1;
            for (int pc = 0; pc < 3; ++pc) if (self->pf_class[pc + 1] > self->pf_class[pc]) last_pf = pc;
            for (int pc = 0; pc < 3; ++pc) {
                const int n0 = self->pf_class[pc], n1 = self->pf_class[pc + 1];
                if (n1 <= n0) continue;
                LrArgs lc = l;
                lc.col = l.col + n0; lc.p0 = l.p0 + n0; lc.len = l.len + n0; lc.nitems = n1 - n0;
                hipEvent_t e0 = started ? nullptr : ev_start, e1 = pc == last_pf ? ev_stop : nullptr;
                started = true;
                const int grid = std::max(1, std::min((n1 - n0 + 31) / 32, c->num_cu * 4));     // eight waves x four columns per pass
                k64_pf(pc, grid, st, e0, e1, lc);
            }
            return 0;
        }
        if (nwork > 0) {
            const FusedArgs &f = self->cur_fused;                    // (all zero outside the fused stateful path)
            if (f.gate_host || f.nstat) {                            // gate workgroup + statistics riders + items in one launch
                const dim3 grid((unsigned)(nwork + (f.gate_host ? 1 : 0) + f.nstat));
                if (wt) k64_1sw((int)grid.x, st, ev_start, ev_stop, a, f);
                else BPMF_LAUNCH(k_sample1s<K>, grid, dim3(64), st, ev_start, ev_stop, a, f);
            } else if (wt) {
                k64_slabw(nwork, st, ev_start, ev_stop, a);
            } else {
                k64_slab(nwork, st, ev_start, ev_stop, a);
            }
        }
        return 0;
    } else {
    if (nwork > 0) {                                                 // K <= 32: one work item per single-wave workgroup (k_sample1)
        const FusedArgs &f = self->cur_fused;                        // (all zero outside the fused stateful path)
        const dim3 grid((unsigned)(nwork + (f.gate_host ? 1 : 0) + f.nstat));
        if (wt) {                                                    // weighted index blocks (never the gather stream)
            sample1w<K>((int)grid.x, st, ev_start, ev_stop, a, f);
        } else if (uses_gather_stream(self) && vals == self->d_vals) {      // the Gram reads the side's gather stream (build_schedule)
            a.gs_rec = self->d_gs_rec.get(); a.gs_g0 = self->d_gs_g0.get() + w0; a.gs_ng = self->d_gs_ng.get() + w0;
            BPMF_LAUNCH(k_sample1<K>, grid, dim3(64), st, ev_start, ev_stop, a, f);
        } else {                                                     // other values than the side's own ratings: index blocks
            BPMF_LAUNCH(k_sample1i<K>, grid, dim3(64), st, ev_start, ev_stop, a, f);
        }
    }
    return 0;
    }
    }
}

template <int K, bool F32>
int exchange(bpmf_hip_side *self, hipStream_t st, int sub)
{
    bpmf_hip_ctx *c = self->ctx;
    if (!(c->comm != nullptr && !self->bounds.empty())) return 0;
    COMM_ALIVE_OR_FAIL(c, "exchange");
    // factors are fp64 (8 K bytes per column) or, in the fp32 context, fp32
    const bool f32 = c->dtype == BPMF_HIP_F32;
    const ncclDataType_t ty = f32 ? ncclFloat : ncclDouble;
    const size_t esz = f32 ? sizeof(float) : sizeof(double);
    char *items = reinterpret_cast<char *>(self->d_items);
    Rccl *R = rccl();
    if (!self->conn_send_ptr.empty()) {
        if constexpr (F32) return fail(BPMF_HIP_EINVAL, "the connectivity-aware exchange is fp64 only");
        else {
        // connectivity-aware form (c++/assign.cpp:204-241 conn_map + send_item, c++/sample.cpp:370): a column
        // only travels to the ranks whose ratings / test entries reference it.  Pack the columns of
        // every peer's list into one buffer, one grouped send / receive per peer, scatter what arrived.
        // Not cut into parts: the lists name columns of the whole range, so everything travels behind the LAST part -- the
        // exchange stream has then waited for every part's sampler.  (Rounds 3-5 sent it with part 0, i.e. while the parts
        // 1 .. n - 1 were still being sampled: stale columns to the peers and, at one rank, the scatter racing the samplers.
        // The combination parts + lists had no test; tests/_rccl1_worker.py is it, round 6.)
        if (sub >= 0 && self->nsub > 1 && sub != self->nsub - 1) return 0;
        const int64_t ns = self->conn_send_ptr.back(), nr = self->conn_recv_ptr.back();
        constexpr int P = K / 2;                                   // 16-byte pieces per column
        if (ns > 0)
            hipLaunchKernelGGL(bpmf::k_pack_cols<K>, dim3((unsigned)((ns * P + 255) / 256)), dim3(256), 0, st,
                               (const double *)self->d_items, (const int32_t *)self->d_conn_send.get(), ns, self->d_conn_sbuf.get());
        NcclGroup group(R);
        NCCL_TRY(group.start());
        for (int r = 0; r < c->nranks; ++r) {
            const int64_t s0 = self->conn_send_ptr[(size_t)r], s1 = self->conn_send_ptr[(size_t)r + 1];
            const int64_t r0 = self->conn_recv_ptr[(size_t)r], r1 = self->conn_recv_ptr[(size_t)r + 1];
            if (s1 > s0) NCCL_TRY(R->Send(self->d_conn_sbuf.get() + (size_t)s0 * K, (size_t)(s1 - s0) * K, ncclDouble, r, c->comm, st));
            if (r1 > r0) NCCL_TRY(R->Recv(self->d_conn_rbuf.get() + (size_t)r0 * K, (size_t)(r1 - r0) * K, ncclDouble, r, c->comm, st));
        }
        NCCL_TRY(group.end());
        if (nr > 0)
            hipLaunchKernelGGL(bpmf::k_unpack_cols<K>, dim3((unsigned)((nr * P + 255) / 256)), dim3(256), 0, st,
                               (const double *)self->d_conn_rbuf.get(), (const int32_t *)self->d_conn_recv.get(), nr, self->d_items);
        HIP_TRY(hipGetLastError());
        return 0;
        }
    }
    // columns [lo, hi) rank r contributes to this call
    auto range = [&](int r, int64_t &lo, int64_t &hi) {
        if (sub < 0 || self->nsub <= 1) { lo = self->bounds[(size_t)r]; hi = self->bounds[(size_t)r + 1]; }
        else { lo = self->sub_bounds[(size_t)r * (self->nsub + 1) + sub]; hi = self->sub_bounds[(size_t)r * (self->nsub + 1) + sub + 1]; }
    };
    // All-gather-v of disjoint, uneven ranges.  Default: a MESH of point-to-point transfers -- one grouped
    // ncclSend / ncclRecv pair per peer, every pair on its own xGMI link (the links are point-to-point:
    // seven per GPU) -- instead of nranks broadcasts, each of which is a ring / tree collective over all ranks.
    // BPMF_HIP_EXCHANGE=bcast keeps the broadcasts (and is what an RCCL without ncclSend / ncclRecv gets).
    static const bool want_mesh = [] { const char *e = getenv("BPMF_HIP_EXCHANGE"); return !(e && std::string(e) == "bcast"); }();
    int64_t mlo, mhi;
    range(c->rank, mlo, mhi);
    NcclGroup group(R);
    NCCL_TRY(group.start());
    if (want_mesh && R->Send && R->Recv) {
        for (int r = 0; r < c->nranks; ++r) {
            if (r == c->rank) continue;
            int64_t lo, hi;
            range(r, lo, hi);
            if (mhi > mlo) NCCL_TRY(R->Send(items + (size_t)mlo * K * esz, (size_t)(mhi - mlo) * K, ty, r, c->comm, st));
            if (hi > lo) NCCL_TRY(R->Recv(items + (size_t)lo * K * esz, (size_t)(hi - lo) * K, ty, r, c->comm, st));
        }
    } else {
        for (int r = 0; r < c->nranks; ++r) {
            int64_t lo, hi;
            range(r, lo, hi);
            if (hi > lo) {
                char *p = items + (size_t)lo * K * esz;
                NCCL_TRY(R->Broadcast(p, p, (size_t)(hi - lo) * K, ty, r, c->comm, st));
            }
        }
    }
    NCCL_TRY(group.end());
    return 0;
}

// one kernel of the statistics pass or of an evaluation, with a completion event on its dispatch packet when one is given
// (not BPMF_LAUNCH: that macro consumes next_flags(), which belongs to the next SAMPLER launch, and records into the probe)
template <typename... P, typename... A>
inline void launch_ev(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st, hipEvent_t ev_done, A... args)
{
    if (ev_done) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, nullptr, ev_done, 0, static_cast<P>(args)...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, st, static_cast<P>(args)...);
}

template <int K, bool F32>
int stats(bpmf_hip_side *self, hipStream_t st, const StatPass &p, hipEvent_t ev_done)
{
    using namespace bpmf;
    bpmf_hip_ctx *c = self->ctx;
    // single GPU: the sums go straight to the pinned blob.  Sharded: local sums into a device blob, all-reduced (cov is then
    // formed once from the GLOBAL sums: SURVEY Q19) together with the failed-column word, then published to the host -- on
    // the side's own stream: its own reduction blob and the second communicator
    const bool dist = c->comm != nullptr && !self->bounds.empty();
    const bool own = st != c->stream.get() && c->comm2 && self->a_d_red;
    if (dist) COMM_ALIVE_OR_FAIL(c, "statistics all-reduce");
    double *red = own ? self->a_d_red.get() : c->d_red.get();
    double *out = dist ? red : p.out;
    unsigned *flag = dist ? p.ticket + 8 : p.flag;
    const unsigned seq = dist ? 0u : p.seq;
    if (dist) ev_done = nullptr;
    ++self->stat_alone_passes;
    if constexpr (K == 128) {                           // one wave per (slice of columns, 16 x 16 tile): fp32 or fp64 factors, fp64 sums
        typedef typename std::conditional<F32, float, double>::type T;
        hipLaunchKernelGGL((k_colstats_f32<K, T>), dim3(p.nwaves * (K / 16) * (K / 16 + 1) / 2), dim3(64), 0, st, reinterpret_cast<const T *>(p.items),
                           p.c0, p.c1, p.nwaves, p.partials);
        launch_ev(k_colstats_f32_final<K>, dim3((blob::res_sums(K) + 255) / 256), dim3(256), st, ev_done,
                  p.partials, p.nwaves, p.fail_in, out, p.ticket, flag, seq);
    } else if (self->nstat_wg > 0) {
        launch_ev(k_colstats_wg<K>, dim3(self->nstat_wg), dim3(256), st, ev_done, reinterpret_cast<const double *>(p.items), p.c0, p.c1,
                  self->nstat_wg, p.partials, p.fail_in, out, p.ticket, flag, seq, p.tmo, wait_ticks(), nullptr, 0, self->nstat_wg, 1);
    } else {
        launch_ev(k_colstats<K>, dim3(p.nwaves), dim3(64), st, ev_done, reinterpret_cast<const double *>(p.items), p.c0, p.c1,
                  p.nwaves, p.partials, p.fail_in, out, p.ticket, flag, seq, p.tmo, wait_ticks());
    }
    if (dist) {
        NCCL_TRY(rccl()->AllReduce(red, red, (size_t)blob::res_reduced_words(K), ncclDouble, ncclSum, own ? c->comm2 : c->comm, st));
        publish(red, p.out, blob::res_reduced_words(K), p.flag, p.seq, blob::res_failD(K), st);
    }
    return 0;
}

template <int K, bool F32>
void predict(bpmf_hip_test *t, const bpmf_hip_side *self, const void *self_items, const void *other_items, int n,
                    hipStream_t ps, bool beside)
{
    typedef typename std::conditional<F32, float, double>::type T;
    bpmf_hip_ctx *c = self->ctx;
    unsigned *flag = reinterpret_cast<unsigned *>(t->h_res.dev() + 2);
    const bool dist = c->comm && !self->bounds.empty();
    t->pstream = ps;
    if (beside) (void)hipStreamWaitEvent(ps, t->in_ev, 0);
    // users.predict(movies) (c++/bpmf.cpp:190): the twin's entries with the roles of the two factor matrices swapped, on
    // the same stream and AHEAD of this evaluation, so that the completion event below covers both
    const bool fused_twin = t->twin && t->d_twin_perm && !dist;
    if (t->twin && !fused_twin && (t->twin->nnz > 0 || dist)) {      // (sharded: its all-reduce is collective, entries or not)
        t->twin->in_ev = t->in_ev;
        predict<K, F32>(t->twin, t->twin->side, other_items, self_items, n, ps, false);
        t->twin->launched = true;
    }
    // se | se_avg of this rank's test ratings: straight to the host, or -> all-reduce -> host
    double *red = c->d_red.get() + (t->owner ? blob::red_twin(K) : blob::red_eval(K));
    // one kernel, both copies of the test entries.  fp32 too (round 4: k_predict<K, 256, float>) -- as two kernels the second
    // one started when the partner's sampler had filled the chip and ended with it (347 us for 20 us of work), and the
    // host loop, which collects both sums before it enqueues the next iteration, came 45 us late every iteration
    bpmf::TwinArgs tw{};
    if (fused_twin) {
        bpmf_hip_test *u = t->twin;
        tw.perm = t->d_twin_perm.get(); tw.pavg = u->d_pavg.get(); tw.pm2 = u->d_pm2.get(); tw.mean = u->side->mean_rating;
        tw.partial = u->d_partial.get(); tw.out = u->h_res.dev(); tw.flag = reinterpret_cast<unsigned *>(u->h_res.dev() + 2); tw.seq = ++u->seq;
        u->pstream = ps; u->launched = true;
    }
    const unsigned pseq = dist ? 0u : ++t->seq;
    auto run = [&](auto kernel, unsigned wg, auto... twin) {          // (k_predict takes the twin's arguments, k_predict_f32 has none)
        launch_ev(kernel, dim3((unsigned)t->nblocks), dim3(wg), ps, nullptr, t->d_tcol.get(), t->d_trow.get(), t->d_tval.get(), t->nnz,
                  reinterpret_cast<const T *>(self_items), reinterpret_cast<const T *>(other_items), self->from, self->mean_rating, n,
                  t->d_pavg.get(), t->d_pm2.get(), t->d_partial.get(), dist ? red : t->h_res.dev(), t->d_ticket.get(), dist ? t->d_ticket.get() + 8 : flag, pseq, twin...);
    };
    if constexpr (F32) {
        if (fused_twin) run(bpmf::k_predict<K, 256, float>, 256u, tw);
        else run(bpmf::k_predict_f32<K>, 256u);
    } else {
        if (t->wg == 64) run(bpmf::k_predict<K, 64>, 64u, tw);        // single-wave workgroups (small test sets: see k_predict)
        else run(bpmf::k_predict<K, 256>, 256u, tw);
    }
    if (dist) {
        if (rccl()->AllReduce(red, red, 2, ncclDouble, ncclSum, c->comm, c->stream.get()) != ncclSuccess) return;
        publish(red, t->h_res.dev(), 2, flag, ++t->seq, -1, c->stream.get());
    }
    if (beside) (void)hipEventRecord(t->ev_done[t->seq & 1u].get(), ps);
}

}  // namespace bpmf_launch

#define BPMF_INSTANTIATE_K(KK, FF)                                                                                               \
    template int bpmf_launch::sampler_into<KK, FF>(bpmf_hip_side *, double *, const bpmf_hip_side *, int, double, double *, hipStream_t, \
                                               hipEvent_t, hipEvent_t);                                                          \
    template int bpmf_launch::exchange<KK, FF>(bpmf_hip_side *, hipStream_t, int);                                                        \
    template int bpmf_launch::stats<KK, FF>(bpmf_hip_side *, hipStream_t, const bpmf_launch::StatPass &, hipEvent_t);                        \
    template void bpmf_launch::predict<KK, FF>(bpmf_hip_test *, const bpmf_hip_side *, const void *, const void *, int, hipStream_t, bool);
