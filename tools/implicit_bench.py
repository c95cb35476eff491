"""Implicit feedback and the ranked evaluation (gibbs(..., implicit=W0, rank_eval=N)): what the held-out ranks
and the blocking implicit half-iteration cost.

    python tools/implicit_bench.py rank [--secs 2] [--rounds 3] [--held 10] [--samples 15]
        ms per call at the ML-1M shape (6 040 users x 3 706 movies, K = 32, 15 kept samples, ten held-out movies per user), in
        interleaved windows of >= secs each after a warm-up call, of
          topn       engine.topn(users, movies, n = 10): one sweep over the products, the top-N merge, the std of the picks
          rank_eval  engine.rank_eval(users, movies, ...): two sweeps over the same products and the counts
        Both calls include their allocations, the launch, the host wait and the copies of the results.
    python tools/implicit_bench.py iter [k32 k64 k128] [--secs 2] [--rounds 3]
        ms per Gibbs iteration of the BLOCKING loop (pipelined=False) at the ML-1M shape, in interleaved windows of >= secs each, of
          weighted   gibbs(weights=W): bpmf_hip_sys_sample of the weighted sides, drained once per iteration by the evaluation
          implicit   gibbs(implicit=0.3, weights=W): bpmf_hip_implicit_sample -- the same weighted launch behind the Gram product of the
                     other side, one K x K copy to the host and the host wait for it, twice per iteration
        implicit - weighted is what G costs.  W: a seeded confidence 0.35 + Gamma(2, 0.5) per training rating.

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


def rank(secs, rounds, held, samples):
    M, Mt, T, Tt, nu, nm = synth.ml1m_shaped(seed=42)
    K = 32
    rng = np.random.default_rng(11)
    tptr, tcand = [0], []
    for u in range(nu):                                      # `held` movies the user has not rated
        rated = set(Mt[1][Mt[0][u]:Mt[0][u + 1]].tolist())
        pick = set()
        while len(pick) < min(held, nm - len(rated)):
            c = int(rng.integers(0, nm))
            if c not in rated:
                pick.add(c)
        tcand += sorted(pick)
        tptr.append(len(tcand))
    tptr, tcand = np.array(tptr, np.int64), np.array(tcand, np.int32)
    eng = bpmf_amd.HipEngine(K)
    try:
        users = eng.side_create(nu, nm, *Mt, 0.0)
        movies = eng.side_create(nm, nu, *M, 0.0)
        eng.samples_reserve(users, samples); eng.samples_reserve(movies, samples)
        for _ in range(samples):
            eng.set_items(users, 0.5 * rng.standard_normal((nu, K))); eng.set_items(movies, 0.5 * rng.standard_normal((nm, K)))
            eng.samples_add(users); eng.samples_add(movies)
        calls = dict(topn=lambda: eng.topn(users, movies, 3.5, 10), rank_eval=lambda: eng.rank_eval(users, movies, tptr, tcand, 3.5))
        for f in calls.values():                             # warm-up (the exclusion lists are built here)
            f(); f()
        per = {name: [] for name in calls}
        for r in range(rounds):
            for name in (list(calls) if r % 2 == 0 else list(calls)[::-1]):
                reps, t0 = 0, time.perf_counter()
                while reps < 3 or time.perf_counter() - t0 < secs:   # a window of at least `secs`
                    calls[name]()
                    reps += 1
                wall = time.perf_counter() - t0
                per[name].append(1e3 * wall / reps)
                print(json.dumps(dict(mode="rank", call=name, round=r, reps=reps, window_s=round(wall, 2), ms_per_call=round(per[name][-1], 4))), flush=True)
        med = {k: statistics.median(v) for k, v in per.items()}
        print(json.dumps(dict(mode="rank_summary", users=nu, movies=nm, K=K, samples=samples, held_out=int(len(tcand)),
                              topn_ms=round(med["topn"], 4), rank_eval_ms=round(med["rank_eval"], 4),
                              rank_eval_over_topn=round(med["rank_eval"] / med["topn"], 3),
                              **{k + "_spread_ms": round(max(v) - min(v), 4) for k, v in per.items()})), flush=True)
    finally:
        eng.close()


def run(d, K, mode, W, nsims):
    extra = dict(weights=W) if mode == "weighted" else dict(implicit=0.3, weights=W)
    eng = bpmf_amd.HipEngine(K)
    try:
        t0 = time.perf_counter()
        res = bpmf_amd.gibbs(eng, d[0], d[1], d[2], d[4], d[5], nsims=nsims, burnin=nsims, Tt=d[3], pipelined=False, **extra)
        wall = time.perf_counter() - t0
        names = (eng.kernel_name(res["movies"].side), eng.kernel_name(res["users"].side))
    finally:
        eng.close()
    return res, wall, names


def iters(names, secs, rounds):
    d = synth.ml1m_shaped(seed=42)
    W = (d[0][0], d[0][1], 0.35 + np.random.default_rng(7).gamma(2.0, 0.5, len(d[0][2])))
    modes = ("weighted", "implicit")
    for name in names:
        K = int(name[1:])
        probe, kernels = {}, {}
        for mode in modes:                                   # warm-up, and size the windows
            res, _, kernels[mode] = run(d, K, mode, W, 12)
            probe[mode] = statistics.median(res["secs"][4:])
        nsims = max(20, int(secs / min(probe.values())))
        per = {m: [] for m in modes}
        for r in range(rounds):
            for mode in (modes if r % 2 == 0 else modes[::-1]):
                res, wall, _ = run(d, K, mode, W, nsims)
                ms = 1e3 * sum(res["secs"][5:]) / (nsims - 5)
                per[mode].append(ms)
                print(json.dumps(dict(mode="iter", shape=name, K=K, form=mode, round=r, nsims=nsims, window_s=round(wall, 2), ms_per_iter=round(ms, 4))),
                      flush=True)
        med = {m: statistics.median(per[m]) for m in modes}
        print(json.dumps(dict(mode="iter_summary", shape=name, K=K, kernels=kernels, **{m + "_ms": round(med[m], 4) for m in modes},
                              **{m + "_spread_ms": round(max(per[m]) - min(per[m]), 4) for m in modes},
                              gram_ms=round(med["implicit"] - med["weighted"], 4), implicit_over_weighted=round(med["implicit"] / med["weighted"], 3))),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rank", "iter"))
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--secs", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--held", type=int, default=10)
    ap.add_argument("--samples", type=int, default=15)
    a = ap.parse_args()
    if a.mode == "rank":
        rank(a.secs, a.rounds, a.held, a.samples)
    else:
        if any(s not in ("k32", "k64", "k128") for s in a.shapes):
            ap.error("shapes: k32, k64 or k128")
        iters(a.shapes or ["k32", "k64", "k128"], a.secs, a.rounds)


if __name__ == "__main__":
    main()
