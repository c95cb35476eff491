"""Row and column bias terms (gibbs(..., bias=LAMBDA)): what the bias step costs.

    python tools/bias_bench.py iter [ml1m chembl] [--secs 2] [--rounds 3]
        ms per Gibbs iteration of the blocking loop (pipelined=False: the loop a run with biases takes), in interleaved windows of
        >= secs each, of
          plain      the sides without biases in their default forms (K <= 32: the gather stream; K = 64: product form + slab)
          plain_idx  the same with BPMF_HIP_GATHER_STREAM=0: the index-block form a side with biases runs at K <= 32
          bias       both sides with biases, lambda = 1, no kept iteration (burnin = nsims): bias - plain_idx is two bias steps (four
                     launches each) and the two extra loads of k_predict_bias
    python tools/bias_bench.py step [ml1m chembl] [--reps 200]
        ms of one bias step of the movies' side alone (k_bias_resid, k_bias_piece_sums, k_bias_draw, k_bias_values back to back), timed
        with the host clock around `reps` half-iterations minus the same of a side without biases in the index-block form

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

MODES = ("plain", "plain_idx", "bias")
IDX_ENV = {"BPMF_HIP_GATHER_STREAM": "0"}


def shape(name):
    if name == "ml1m":
        M, Mt, T, Tt, nu, nm = synth.ml1m_shaped(seed=42)
        return dict(K=32, M=M, Mt=Mt, T=T, Tt=Tt, nu=nu, nm=nm)
    M, Mt, T, Tt, nu, nm = synth.ratings(483500, 5775, 1_023_952, seed=42, real_valued=True)
    return dict(K=64, M=M, Mt=Mt, T=T, Tt=Tt, nu=nu, nm=nm)


class _env:
    def __init__(self, kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(d, mode, nsims):
    with _env(IDX_ENV if mode == "plain_idx" else {}):
        eng = bpmf_amd.HipEngine(d["K"])
        try:
            res = bpmf_amd.gibbs(eng, d["M"], d["Mt"], d["T"], d["nu"], d["nm"], nsims=nsims, burnin=nsims, Tt=d["Tt"], pipelined=False,
                                 **(dict(bias=1.0) if mode == "bias" else {}))
        finally:
            eng.close()
    return res


def iters(names, secs, rounds):
    for name in names:
        d = shape(name)
        probe = {m: statistics.median(run(d, m, 30)["secs"][5:]) for m in MODES}
        nsims = max(40, int(secs / min(probe.values())))
        per = {m: [] for m in MODES}
        for r in range(rounds):
            for mode in (MODES if r % 2 == 0 else MODES[::-1]):
                res = run(d, mode, nsims)
                ms = 1e3 * sum(res["secs"][10:]) / (nsims - 10)
                per[mode].append(ms)
                print(json.dumps(dict(mode="iter", shape=name, K=d["K"], form=mode, round=r, nsims=nsims, ms_per_iter=round(ms, 4))), flush=True)
        med = {m: statistics.median(per[m]) for m in MODES}
        print(json.dumps(dict(mode="iter_summary", shape=name, K=d["K"], **{m + "_ms": round(med[m], 4) for m in MODES},
                              **{m + "_spread_ms": round(max(per[m]) - min(per[m]), 4) for m in MODES},
                              bias_steps_ms=round(med["bias"] - med["plain_idx"], 4), bias_over_plain=round(med["bias"] / med["plain"], 3))), flush=True)


def step(names, reps):
    for name in names:
        d = shape(name)
        K, M, nu, nm = d["K"], d["M"], d["nu"], d["nm"]
        rng = np.random.default_rng(5)
        sigma = (1.0 / K) ** 0.25
        V, U = sigma * rng.standard_normal((nm, K)), sigma * rng.standard_normal((nu, K))
        A = rng.standard_normal((K, 3 * K))
        mu, LU, LF = bpmf_amd.engine.hyper_sample(K, nm, A @ A.T / (3 * K), 0)
        mean = float(np.sum(M[2])) / len(M[2])
        ms = {}
        with _env(IDX_ENV):
            for mode in ("plain_idx", "bias", "plain_idx", "bias"):
                eng = bpmf_amd.HipEngine(K)
                try:
                    me = eng.side_create(nm, nu, *M, mean)
                    ot = eng.side_create(nu, nm, np.zeros(nu + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
                    if mode == "bias":
                        eng.set_bias(me, 1.0, 13, 0); eng.set_bias(ot, 1.0, 14, 1)
                    eng.set_items(me, V); eng.set_items(ot, U)
                    for it in range(5):
                        eng.sample_side(me, ot, it, 2.0, mu, LF)
                    t0 = time.perf_counter()
                    for it in range(reps):
                        eng.sample_side(me, ot, it, 2.0, mu, LF)
                    ms.setdefault(mode, []).append(1e3 * (time.perf_counter() - t0) / reps)
                finally:
                    eng.close()
        print(json.dumps(dict(mode="step", shape=name, K=K, ratings=len(M[2]), columns=nm, half_iteration_ms={m: [round(x, 4) for x in v] for m, v in ms.items()},
                              bias_step_ms=round(min(ms["bias"]) - min(ms["plain_idx"]), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("iter", "step"))
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--secs", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if a.mode == "iter":
        iters(a.shapes or ["ml1m", "chembl"], a.secs, a.rounds)
    else:
        step(a.shapes or ["ml1m", "chembl"], a.reps)


if __name__ == "__main__":
    main()
