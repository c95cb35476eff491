"""Probit likelihood (gibbs(..., probit=True), kernels_probit.h): what it costs and what it does.

    python tools/probit_bench.py kernel [ml1m chembl] [--reps 30]
        per repetition one stateless half-iteration of each probit side (k_probit_latent + the sampler) and one engine.train_sse
        of the same side (k_train_sse: the same gather), on random factors.  Run it under
        `rocprofv3 --kernel-trace --stats -- python ...`: the statistics then hold both kernels side by side.
    python tools/probit_bench.py iter [ml1m chembl k128] [--secs 2] [--rounds 3]
        per-iteration time of the pipelined loop (bench.py's), fixed against probit, interleaved windows of >= secs each;
        k128 = the ML-1M shape at K = 128 fp64.  Labels: a rating above the mean rating is a positive.
    python tools/probit_bench.py auc
        the planted model of tests/probit_ref.py (RECOVERY): AUC / Brier of the probit chain, and the AUC of the fixed-alpha chain
        (alpha 2, the 0 / 1 labels as ratings, ranking by its posterior-mean prediction) on the same data

One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bpmf_amd                                            # noqa: E402
from bpmf_amd import synth                                 # noqa: E402


def shape(name):
    if name in ("ml1m", "k128"):
        M, Mt, T, Tt, nu, nm = synth.ml1m_shaped(seed=42)
        return dict(K=128 if name == "k128" else 32, M=M, Mt=Mt, T=T, Tt=Tt, nu=nu, nm=nm)
    M, Mt, T, Tt, nu, nm = synth.ratings(483500, 5775, 1_023_952, seed=42, real_valued=True)
    return dict(K=64, M=M, Mt=Mt, T=T, Tt=Tt, nu=nu, nm=nm)


def kernel(names, reps):
    for name in names:
        d = shape(name)
        K, nu, nm = d["K"], d["nu"], d["nm"]
        thr = float(d["M"][2].mean())
        eng = bpmf_amd.HipEngine(K)
        try:
            movies = eng.side_create(nm, nu, *d["M"], 0.0)
            users = eng.side_create(nu, nm, *d["Mt"], 0.0)
            eng.set_probit(movies, thr, 1)
            eng.set_probit(users, thr, 2)
            rng = np.random.default_rng(1)
            sigma = (2.0 / K) ** 0.25
            V, U = sigma * rng.standard_normal((nm, K)), sigma * rng.standard_normal((nu, K))
            for side, other, A, X, Y, label in ((movies, users, d["M"], V, U, "movies"), (users, movies, d["Mt"], U, V, "users")):
                ncols = len(A[0]) - 1
                mu, LU, LF = bpmf_amd.engine.hyper_sample(K, ncols, np.eye(K) * 0.2, 3)
                ms = []
                for _ in range(reps):
                    eng.set_items(side, X); eng.set_items(other, Y)
                    t0 = time.perf_counter()
                    eng.sample_side(side, other, 3, 1.0, mu, LF)
                    ms.append((time.perf_counter() - t0) * 1e3)
                    eng.train_sse(side, other)
                z = eng.probit_latent(side, len(A[2]))
                print(json.dumps(dict(mode="kernel", shape=name, K=K, side=label, ncols=ncols, nnz=len(A[2]),
                                      half_iteration_ms_median=round(statistics.median(ms), 4), mean_abs_z=round(float(np.abs(z).mean()), 4),
                                      gathered_MB=round((len(A[2]) * (4 + 1 + 8 + 8 * K) + ncols * (8 + 8 * K)) / 1e6, 1))), flush=True)
        finally:
            eng.close()


def iters(names, secs, rounds):
    for name in names:
        d = shape(name)
        K = d["K"]
        args = (d["M"], d["Mt"], d["T"], d["nu"], d["nm"])
        thr = float(d["M"][2].mean())
        kw = {"fixed": dict(), "probit": dict(probit=True, threshold=thr)}
        probe = {}
        for mode in kw:                                      # size the windows
            eng = bpmf_amd.HipEngine(K)
            try:
                res = bpmf_amd.gibbs(eng, *args, nsims=40, burnin=10, Tt=d["Tt"], pipelined=True, **kw[mode])
            finally:
                eng.close()
            probe[mode] = statistics.median(res["secs"][5:])
        nsims = max(50, int(secs / min(probe.values())))
        per = {"fixed": [], "probit": []}
        for r in range(rounds):
            for mode in (("fixed", "probit") if r % 2 == 0 else ("probit", "fixed")):
                eng = bpmf_amd.HipEngine(K)
                try:
                    t0 = time.perf_counter()
                    res = bpmf_amd.gibbs(eng, *args, nsims=nsims, burnin=10, Tt=d["Tt"], pipelined=True, **kw[mode])
                    wall = time.perf_counter() - t0
                finally:
                    eng.close()
                ms = 1e3 * sum(res["secs"][10:]) / (nsims - 10)
                per[mode].append(ms)
                print(json.dumps(dict(mode="iter", shape=name, K=K, likelihood=mode, round=r, nsims=nsims, window_s=round(wall, 2),
                                      ms_per_iter=round(ms, 4))), flush=True)
        f, p = statistics.median(per["fixed"]), statistics.median(per["probit"])
        print(json.dumps(dict(mode="iter_summary", shape=name, K=K, fixed_ms=round(f, 4), probit_ms=round(p, 4),
                              fixed_spread_ms=round(max(per["fixed"]) - min(per["fixed"]), 4), added_ms=round(p - f, 4),
                              probit_over_fixed=round(p / f, 3))), flush=True)


def auc():
    from tests import probit_ref as ref
    P = ref.RECOVERY
    M, Mt, T, Tt, nu, nm, ceiling = ref.recovery_data(**P)
    out = dict(mode="auc", ceiling=ceiling, nsims=P["nsims"], burnin=P["burnin"])
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=P["nsims"], burnin=P["burnin"], Tt=Tt, pipelined=True, probit=True)
        out["probit_auc"], out["probit_brier"] = res["auc"], res["brier"]
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=P["nsims"], burnin=P["burnin"], Tt=Tt, pipelined=True)
        pavg, _ = eng.test_get(res["movies"].test)
        out["fixed_auc"] = bpmf_amd.auc(pavg, T[2], 0.5)
        out["fixed_brier_clipped"] = float(np.mean((np.clip(pavg, 0.0, 1.0) - T[2]) ** 2))
    finally:
        eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "iter", "auc"))
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--secs", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.mode == "kernel":
        kernel(a.shapes or ["ml1m", "chembl"], a.reps)
    elif a.mode == "iter":
        iters(a.shapes or ["ml1m", "chembl", "k128"], a.secs, a.rounds)
    else:
        auc()


if __name__ == "__main__":
    main()
