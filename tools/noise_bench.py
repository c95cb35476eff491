"""Adaptive noise precision (gibbs(..., noise="adaptive"), kernels_noise.h): what it costs and what it does.

    python tools/noise_bench.py kernel [ml1m chembl] [--reps 50]
        engine.train_sse on random factors: median ms per call (host wall clock: launch + the two kernels + the wait), the
        bytes the reduction gathers and their share of 5.5 TB/s (whole random rows gathered chip-wide on an MI355X).  Run it under
        `rocprofv3 --kernel-trace --stats -- python ...` for the kernel times alone.
    python tools/noise_bench.py iter [ml1m chembl k128] [--secs 2] [--rounds 3]
        per-iteration time of the pipelined loop (bench.py's), fixed against adaptive, interleaved windows of >= secs each;
        k128 = the ML-1M shape at K = 128 fp64
    python tools/noise_bench.py trace [--nsims 30] [--cap F]
        the alpha trace on the ChEMBL shape (K = 64), without and with a cap (default: half the uncapped post-burn-in median)

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

GATHER_TBS = 5.5


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
        eng = bpmf_amd.HipEngine(K)
        try:
            mr = float(d["M"][2].mean())
            movies = eng.side_create(nm, nu, *d["M"], mr)
            users = eng.side_create(nu, nm, *d["Mt"], mr)
            rng = np.random.default_rng(1)
            eng.set_items(movies, 0.3 * rng.standard_normal((nm, K)))
            eng.set_items(users, 0.3 * rng.standard_normal((nu, K)))
            for side, other, A, label in ((movies, users, d["M"], "movies"), (users, movies, d["Mt"], "users")):
                first = eng.train_sse(side, other)
                ms = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    sse, n = eng.train_sse(side, other)
                    ms.append((time.perf_counter() - t0) * 1e3)
                    assert sse == first[0]
                ncols = len(A[0]) - 1
                nbytes = n * (4 + 8 + 8 * K) + ncols * (8 + 8 * K)     # rowidx + value + the other row per rating; colptr + own row per column
                med = statistics.median(ms)
                print(json.dumps(dict(mode="kernel", shape=name, K=K, side=label, ncols=ncols, nnz=n, ms_median=round(med, 4),
                                      ms_min=round(min(ms), 4), gathered_MB=round(nbytes / 1e6, 1),
                                      share_of_gather_rate=round(nbytes / (med * 1e-3) / (GATHER_TBS * 1e12), 3),
                                      train_rmse=math.sqrt(sse / n))), flush=True)
        finally:
            eng.close()


def iters(names, secs, rounds):
    for name in names:
        d = shape(name)
        K = d["K"]
        args = (d["M"], d["Mt"], d["T"], d["nu"], d["nm"])
        probe = {}
        for noise in ("fixed", "adaptive"):                 # size the windows
            eng = bpmf_amd.HipEngine(K)
            try:
                res = bpmf_amd.gibbs(eng, *args, nsims=40, burnin=10, Tt=d["Tt"], pipelined=True, noise=noise)
            finally:
                eng.close()
            probe[noise] = statistics.median(res["secs"][5:])
        nsims = max(50, int(secs / min(probe.values())))
        per = {"fixed": [], "adaptive": []}
        for r in range(rounds):
            for noise in (("fixed", "adaptive") if r % 2 == 0 else ("adaptive", "fixed")):
                eng = bpmf_amd.HipEngine(K)
                try:
                    t0 = time.perf_counter()
                    res = bpmf_amd.gibbs(eng, *args, nsims=nsims, burnin=10, Tt=d["Tt"], pipelined=True, noise=noise)
                    wall = time.perf_counter() - t0
                finally:
                    eng.close()
                ms = 1e3 * sum(res["secs"][10:]) / (nsims - 10)
                per[noise].append(ms)
                print(json.dumps(dict(mode="iter", shape=name, K=K, noise=noise, round=r, nsims=nsims, window_s=round(wall, 2),
                                      ms_per_iter=round(ms, 4))), flush=True)
        f, a = statistics.median(per["fixed"]), statistics.median(per["adaptive"])
        print(json.dumps(dict(mode="iter_summary", shape=name, K=K, fixed_ms=round(f, 4), adaptive_ms=round(a, 4),
                              adaptive_over_fixed=round(a / f, 3))), flush=True)


def trace(nsims, cap):
    d = shape("chembl")
    for alpha_max in (None, cap):
        if alpha_max == 0:                                  # (default: half the uncapped chain's post-burn-in median)
            alpha_max = 0.5 * statistics.median(res["alpha"][nsims // 3:])
        eng = bpmf_amd.HipEngine(d["K"])
        try:
            res = bpmf_amd.gibbs(eng, d["M"], d["Mt"], d["T"], d["nu"], d["nm"], nsims=nsims, burnin=nsims // 3, Tt=d["Tt"],
                                 pipelined=True, noise="adaptive", alpha_max=alpha_max)
        finally:
            eng.close()
        print(json.dumps(dict(mode="trace", shape="chembl", K=d["K"], alpha_max=alpha_max, alpha=[round(a, 4) for a in res["alpha"]],
                              train_rmse=[round(x, 4) for x in res["train_rmse"]], test_rmse=[round(x, 4) for x in res["rmse"]],
                              final_rmse_avg=round(res["final_rmse_avg"], 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "iter", "trace"))
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--secs", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nsims", type=int, default=30)
    ap.add_argument("--cap", type=float, default=0.0)
    a = ap.parse_args()
    if a.mode == "kernel":
        kernel(a.shapes or ["ml1m", "chembl"], a.reps)
    elif a.mode == "iter":
        iters(a.shapes or ["ml1m", "chembl", "k128"], a.secs, a.rounds)
    else:
        trace(a.nsims, a.cap)


if __name__ == "__main__":
    main()
