"""Ordinal probit likelihood (gibbs(..., ordinal=True), kernels_ordinal.h): what it costs and what it does.

    python tools/ordinal_bench.py kernel [ml1m chembl] [--reps 20]
        alternating in one session, on random factors: one stateless half-iteration of an ordinal side (k_ordinal_latent + the
        sampler), of a probit side (k_probit_latent + the sampler), one engine.ordinal_loglik (k_ordinal_loglik + its final kernel,
        enqueue and wait) and one engine.train_sse (k_train_sse, the same gather, enqueue and wait) of the same ratings; medians and
        spreads of the host-side times.  Run it under `rocprofv3 --kernel-trace --stats -- python ...`: the statistics then hold the
        four kernels side by side.
    python tools/ordinal_bench.py iter [ml1m chembl] [--secs 2] [--rounds 3]
        per-iteration time of the pipelined loop (bench.py's): fixed alpha, probit, ordinal with sampled cutpoints (one drain per
        iteration) and ordinal with fixed cutpoints (no drain), interleaved windows of >= secs each
    python tools/ordinal_bench.py planted
        the planted model of tests/test_ordinal_host.py (PLANTED) on the device: log-probability, accuracy, ordinal RMSE, the
        acceptance rate of the cutpoint step and where its step size ended

The ML-1M shape has the levels 1 .. 5; the real-valued ChEMBL-shaped activities are cut into five classes at their quintiles.
One JSON line per measurement.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bpmf_amd                                            # noqa: E402
from bpmf_amd import synth                                 # noqa: E402


def classes(A, edges):
    return (A[0], A[1], 1.0 + np.searchsorted(edges, A[2]).astype(np.float64))


def shape(name):
    if name == "ml1m":
        M, Mt, T, Tt, nu, nm = synth.ml1m_shaped(seed=42)
        K = 32
    else:
        M, Mt, T, Tt, nu, nm = synth.ratings(483500, 5775, 1_023_952, seed=42, real_valued=True)
        K = 64
    levels = np.unique(M[2])
    if len(levels) > 16 or not np.all(np.isin(T[2], levels)):
        edges = np.quantile(M[2], [0.2, 0.4, 0.6, 0.8])
        M, Mt, T, Tt = (classes(A, edges) for A in (M, Mt, T, Tt))
        levels = np.arange(1.0, 6.0)
    return dict(K=K, M=M, Mt=Mt, T=T, Tt=Tt, nu=nu, nm=nm, levels=levels)


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def kernel(names, reps):
    for name in names:
        d = shape(name)
        K, nu, nm, levels = d["K"], d["nu"], d["nm"], d["levels"]
        thr = float(d["M"][2].mean())
        eng = bpmf_amd.HipEngine(K)
        try:
            rng = np.random.default_rng(1)
            sigma = (2.0 / K) ** 0.25
            V, U = sigma * rng.standard_normal((nm, K)), sigma * rng.standard_normal((nu, K))
            for A, At, ncols, nrows, X, Y, label in ((d["M"], d["Mt"], nm, nu, V, U, "movies"), (d["Mt"], d["M"], nu, nm, U, V, "users")):
                od = eng.side_create(ncols, nrows, *A, 0.0)
                pb = eng.side_create(ncols, nrows, *A, 0.0)
                pl = eng.side_create(ncols, nrows, *A, 0.0)
                other = eng.side_create(nrows, ncols, *At, 0.0)
                eng.set_ordinal(od, levels, None, 11)
                eng.set_probit(pb, thr, 1)
                cut = eng.ordinal_cut_get(od)
                prop = cut + 0.01
                mu, LU, LF = bpmf_amd.engine.hyper_sample(K, ncols, np.eye(K) * 0.2, 3)
                eng.set_items(other, Y)
                t = dict(ordinal_half=[], probit_half=[], loglik=[], sse=[])
                for _ in range(reps):
                    for key, side in (("ordinal_half", od), ("probit_half", pb)):
                        eng.set_items(side, X)
                        t0 = time.perf_counter()
                        eng.sample_side(side, other, 3, 1.0, mu, LF)
                        t[key].append((time.perf_counter() - t0) * 1e3)
                    eng.set_items(od, X); eng.set_items(pl, X)
                    t0 = time.perf_counter()
                    eng.ordinal_loglik(od, other, prop)
                    t["loglik"].append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    eng.train_sse(pl, other)
                    t["sse"].append((time.perf_counter() - t0) * 1e3)
                print(json.dumps(dict(mode="kernel", shape=name, K=K, side=label, ncols=ncols, nnz=len(A[2]), levels=len(levels), reps=reps,
                                      ordinal_half_iteration_ms=spread(t["ordinal_half"]), probit_half_iteration_ms=spread(t["probit_half"]),
                                      ordinal_loglik_call_ms=spread(t["loglik"]), train_sse_call_ms=spread(t["sse"]))), flush=True)
                for s in (od, pb, pl, other):
                    eng.side_destroy(s)
        finally:
            eng.close()


def iters(names, secs, rounds):
    for name in names:
        d = shape(name)
        K = d["K"]
        args = (d["M"], d["Mt"], d["T"], d["nu"], d["nm"])
        thr = float(d["M"][2].mean())
        fixed_cut = np.linspace(-1.0, 1.0, len(d["levels"]) - 1)
        kw = {"fixed": dict(), "probit": dict(probit=True, threshold=thr), "ordinal": dict(ordinal=d["levels"]),
              "ordinal_fixed_cutpoints": dict(ordinal=d["levels"], cutpoints=fixed_cut)}
        probe = {}
        for mode in kw:                                      # size the windows
            eng = bpmf_amd.HipEngine(K)
            try:
                res = bpmf_amd.gibbs(eng, *args, nsims=40, burnin=10, Tt=d["Tt"], pipelined=True, **kw[mode])
            finally:
                eng.close()
            probe[mode] = statistics.median(res["secs"][5:])
        nsims = max(50, int(secs / min(probe.values())))
        per = {m: [] for m in kw}
        rate = []
        order = list(kw)
        for r in range(rounds):
            for mode in (order if r % 2 == 0 else order[::-1]):
                eng = bpmf_amd.HipEngine(K)
                try:
                    t0 = time.perf_counter()
                    res = bpmf_amd.gibbs(eng, *args, nsims=nsims, burnin=10, Tt=d["Tt"], pipelined=True, **kw[mode])
                    wall = time.perf_counter() - t0
                finally:
                    eng.close()
                ms = 1e3 * sum(res["secs"][10:]) / (nsims - 10)
                per[mode].append(ms)
                rec = dict(mode="iter", shape=name, K=K, likelihood=mode, round=r, nsims=nsims, window_s=round(wall, 2), ms_per_iter=round(ms, 4))
                if mode == "ordinal":
                    rec["accepted"] = round(float(np.mean(res["ordinal"]["accepted"][1:])), 3)
                    rec["step_x_sqrt_nnz"] = round(res["ordinal"]["step"][-1] * math.sqrt(len(d["M"][2])), 3)
                    rate.append(rec["accepted"])
                print(json.dumps(rec), flush=True)
        med = {m: statistics.median(v) for m, v in per.items()}
        print(json.dumps(dict(mode="iter_summary", shape=name, K=K, ms_per_iter={m: spread(v) for m, v in per.items()},
                              ordinal_minus_fixed_ms=round(med["ordinal"] - med["fixed"], 4),
                              ordinal_minus_probit_ms=round(med["ordinal"] - med["probit"], 4),
                              drain_ms=round(med["ordinal"] - med["ordinal_fixed_cutpoints"], 4), accepted=rate)), flush=True)


def planted():
    from tests import ordinal_ref as ref
    from tests.test_ordinal_host import PLANTED as P
    M, Mt, T, Tt, nu, nm = ref.planted(**P)
    levels = np.arange(1.0, 6.0)
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=P["nsims"], burnin=P["burnin"], Tt=Tt, pipelined=True, ordinal=levels)
        fix = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=P["nsims"], burnin=P["burnin"], Tt=Tt, pipelined=True)
        pavg, _ = eng.test_get(fix["movies"].test)
    finally:
        eng.close()
    o = res["ordinal"]
    true = T[2]
    freq = np.bincount(np.searchsorted(levels, M[2]), minlength=5) / len(M[2])
    print(json.dumps(dict(mode="planted", nsims=P["nsims"], burnin=P["burnin"], logp=res["logp"],
                          logp_marginal=float(np.mean(np.log(freq[np.searchsorted(levels, true)]))),
                          accuracy=float(np.mean(levels[np.argmax(res["cat_prob"], axis=1)] == true)),
                          accuracy_gaussian_rounded=float(np.mean(np.clip(np.rint(pavg), 1, 5) == true)),
                          rmse_expected=float(np.sqrt(np.mean((res["expected"] - true) ** 2))), rmse_gaussian=fix["final_rmse_avg"],
                          accepted=float(np.mean(o["accepted"][1:])), step_x_sqrt_nnz=o["step"][-1] * math.sqrt(len(M[2])),
                          cutpoints_last=[round(float(g), 4) for g in o["cutpoints"][-1]])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "iter", "planted"))
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--secs", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.mode == "kernel":
        kernel(a.shapes or ["ml1m", "chembl"], a.reps)
    elif a.mode == "iter":
        iters(a.shapes or ["ml1m", "chembl"], a.secs, a.rounds)
    else:
        planted()


if __name__ == "__main__":
    main()
