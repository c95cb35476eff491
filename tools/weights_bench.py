"""Per-rating precision weights (gibbs(..., weights=W)) and Student-t noise (gibbs(..., robust=NU), section
21): what the weighted forms of the samplers and the redraw of the weights cost.

    python tools/weights_bench.py iter [ml1m chembl k128] [--secs 2] [--rounds 3] [--arms plain,plain_idx,weighted]
        ms per Gibbs iteration of the pipelined loop (bench.py's), in interleaved windows of >= secs each, of
          plain      the unweighted sides in their default forms (K <= 32: the gather stream; K = 64: product form + slab)
          plain_idx  the unweighted sides with BPMF_HIP_GATHER_STREAM=0 and BPMF_HIP_PF=0: the index-block form / every column in the
                     slab form -- the forms a weighted side runs, without the weights
          weighted   every training rating with a seeded weight Gamma(2, 0.5)
          robust         Student-t noise with nu = 4: the weighted forms behind two k_robust_weights launches per iteration, and one
                         k_robust_accumulate per kept iteration (what gibbs(robust=4) costs)
          robust_redraw  the same without a kept iteration (burnin = nsims): robust_redraw - weighted is the two k_robust_weights launches
          probit_idx     probit sides (labels: rating > median) with the environment of plain_idx and without a kept iteration:
                         probit_idx - plain_idx is two k_probit_latent launches, the yardstick of section 12 for the redraw
        plain_idx - plain is what losing the stream / the product form costs, weighted - plain_idx what the sqrt(w) loads and the
        multiplies cost.  --arms picks the forms (default: the first three; the summary's differences need their operands).  k128 = the ML-1M shape at K = 128 fp64 (neither a stream nor a product form: plain_idx = plain).
    python tools/weights_bench.py resources
        registers, LDS and resident workgroups of every weighted form beside its unweighted form (bpmf_hip_side_kernel_resources)

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

MODES = ("plain", "plain_idx", "weighted")
ALL_MODES = MODES + ("robust", "robust_redraw", "probit_idx")
IDX_ENV = {"BPMF_HIP_GATHER_STREAM": "0", "BPMF_HIP_PF": "0"}


def shape(name):
    if name in ("ml1m", "k128"):
        M, Mt, T, Tt, nu, nm = synth.ml1m_shaped(seed=42)
        return dict(K=128 if name == "k128" else 32, M=M, Mt=Mt, T=T, Tt=Tt, nu=nu, nm=nm)
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


def run(d, mode, W, nsims):
    """-> (gibbs result, wall seconds, the kernels of the two sides)"""
    extra = {}
    if mode == "weighted":
        extra = dict(weights=W)
    elif mode in ("robust", "robust_redraw"):
        extra = dict(robust=4.0)
    elif mode == "probit_idx":
        extra = dict(probit=True, threshold=float(np.median(d["M"][2])))
    burnin = nsims if mode in ("robust_redraw", "probit_idx") else 10
    with _env(IDX_ENV if mode in ("plain_idx", "probit_idx") else {}):
        eng = bpmf_amd.HipEngine(d["K"])
        try:
            t0 = time.perf_counter()
            res = bpmf_amd.gibbs(eng, d["M"], d["Mt"], d["T"], d["nu"], d["nm"], nsims=nsims, burnin=burnin, Tt=d["Tt"], pipelined=True,
                                 **extra)
            wall = time.perf_counter() - t0
            names = (eng.kernel_name(res["movies"].side), eng.kernel_name(res["users"].side))
        finally:
            eng.close()
    return res, wall, names


def iters(names, secs, rounds, MODES=MODES):
    for name in names:
        d = shape(name)
        K = d["K"]
        M = d["M"]
        W = (M[0], M[1], np.random.default_rng(7).gamma(2.0, 0.5, len(M[2])))
        probe, kernels = {}, {}
        for mode in MODES:                                   # size the windows
            res, _, kernels[mode] = run(d, mode, W, 40)
            probe[mode] = statistics.median(res["secs"][5:])
        nsims = max(50, int(secs / min(probe.values())))
        per = {m: [] for m in MODES}
        for r in range(rounds):
            for mode in (MODES if r % 2 == 0 else MODES[::-1]):
                res, wall, _ = run(d, mode, W, nsims)
                ms = 1e3 * sum(res["secs"][10:]) / (nsims - 10)
                per[mode].append(ms)
                print(json.dumps(dict(mode="iter", shape=name, K=K, form=mode, round=r, nsims=nsims, window_s=round(wall, 2),
                                      ms_per_iter=round(ms, 4))), flush=True)
        med = {m: statistics.median(per[m]) for m in MODES}
        derived = {}
        for key, a, b in (("lost_forms_ms", "plain_idx", "plain"), ("multiply_ms", "weighted", "plain_idx"),
                          ("redraw_ms", "robust_redraw", "weighted"), ("accumulate_ms", "robust", "robust_redraw"),
                          ("probit_latent_ms", "probit_idx", "plain_idx")):
            if a in med and b in med:
                derived[key] = round(med[a] - med[b], 4)
        for key, a, b in (("weighted_over_plain", "weighted", "plain"), ("robust_over_weighted", "robust", "weighted")):
            if a in med and b in med:
                derived[key] = round(med[a] / med[b], 3)
        print(json.dumps(dict(mode="iter_summary", shape=name, K=K, kernels={m: kernels[m] for m in MODES},
                              **{m + "_ms": round(med[m], 4) for m in MODES},
                              **{m + "_spread_ms": round(max(per[m]) - min(per[m]), 4) for m in MODES}, **derived)), flush=True)


def resources():
    """one small side per family: the forms do not depend on the data"""
    rng = np.random.default_rng(3)
    counts = np.concatenate([np.full(40, 20), np.full(8, 300)])
    colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    nrows = 400
    rowidx = np.concatenate([np.sort(rng.choice(nrows, size=c, replace=False)) for c in counts]).astype(np.int32)
    vals = rng.integers(1, 6, len(rowidx)).astype(np.float64)
    for K, env in ((8, {}), (8, {"BPMF_HIP_MODE": "3"}), (16, {}), (16, {"BPMF_HIP_MODE": "3"}), (32, {}), (32, {"BPMF_HIP_MODE": "3"}),
                   (64, {}), (128, {})):
        with _env(dict(env, **IDX_ENV)):
            eng = bpmf_amd.HipEngine(K)
            try:
                side = eng.side_create(len(counts), nrows, colptr, rowidx, vals, 3.0)
                plain = eng.kernel_resources(side)
                eng.set_weights(side, np.ones(len(vals)))
                weighted = eng.kernel_resources(side)
                print(json.dumps(dict(mode="resources", K=K, env=env, plain_name=eng.kernel_name(side).replace("w<", "<"),
                                      weighted_name=eng.kernel_name(side), plain=plain, weighted=weighted)), flush=True)
            finally:
                eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("iter", "resources"))
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--secs", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--arms", default=",".join(MODES), help="comma-separated forms of: " + ", ".join(ALL_MODES))
    a = ap.parse_args()
    arms = tuple(a.arms.split(","))
    if not arms or any(m not in ALL_MODES for m in arms):
        ap.error("--arms: unknown form (one of " + ", ".join(ALL_MODES) + ")")
    if a.mode == "iter":
        iters(a.shapes or ["ml1m", "chembl", "k128"], a.secs, a.rounds, arms)
    else:
        resources()


if __name__ == "__main__":
    main()
