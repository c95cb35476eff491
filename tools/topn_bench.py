"""Times engine.topn (posterior top-N on the device, kernels_topn.h) on the ML-1M shape (K = 32, S = 15, N = 10, every user)
and on the ChEMBL shape (K = 64, S = 15, N = 10, compounds per target), against the ceiling of the f64 16x16x4 MFMA
(48.4 TF, profiles/r05_mfma_shapes_probe.txt) and against a torch composition of the same ranking (matmul of the stacked
fp64 samples, masked_fill of the rated pairs, topk).  Prints one JSON line per shape.

    python tools/topn_bench.py [ml1m|chembl ...] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bpmf_amd                                            # noqa: E402
from bpmf_amd import synth                                 # noqa: E402

CEIL_TF = 48.4


def shape(name):
    if name == "ml1m":
        M, Mt, T, Tt, nu, nm = synth.ml1m_shaped()
        return dict(K=32, M=M, Mt=Mt, nu=nu, nm=nm, by_cols=False)
    M, Mt, T, Tt, nu, nm = synth.ratings(483500, 5775, 1000000, seed=3, real_valued=True)
    return dict(K=64, M=M, Mt=Mt, nu=nu, nm=nm, by_cols=True)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); out = fn(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return out, ms[len(ms) // 2], ms[0]


def run(name, S, n, reps, warmup):
    d = shape(name)
    K, nu, nm = d["K"], d["nu"], d["nm"]
    eng = bpmf_amd.HipEngine(K)
    mr = float(d["M"][2].mean())
    movies = eng.side_create(nm, nu, *d["M"], mr)
    users = eng.side_create(nu, nm, *d["Mt"], mr)
    rng = np.random.default_rng(1)
    eng.samples_reserve(users, S); eng.samples_reserve(movies, S)
    Us, Vs = [], []
    for _ in range(S):
        U = 0.3 * rng.standard_normal((nu, K)); V = 0.3 * rng.standard_normal((nm, K))
        eng.set_items(users, U); eng.set_items(movies, V)
        eng.samples_add(users); eng.samples_add(movies)
        Us.append(U); Vs.append(V)
    if d["by_cols"]:                                       # compounds (rows) per target (column)
        q, c, Q, C, rated = movies, users, Vs, Us, d["M"]
    else:                                                  # items (columns) per user (row)
        q, c, Q, C, rated = users, movies, Us, Vs, d["Mt"]
    nq, nc = q.ncols, c.ncols
    (idx, mean, std), ms, ms_min = timed(lambda: eng.topn(q, c, mr, n), reps, warmup)
    flop = 2.0 * nq * nc * S * K
    # torch composition on the same samples
    dev = torch.device("cuda")
    Qs = torch.from_numpy(np.concatenate(Q, axis=1)).to(dev)
    Cs = torch.from_numpy(np.concatenate(C, axis=1)).to(dev)
    colptr, rowidx = rated[0], rated[1]
    qcol = np.repeat(np.arange(nq), np.diff(colptr))
    mask = torch.zeros((nq, nc), dtype=torch.bool, device=dev)
    mask[torch.from_numpy(qcol).to(dev), torch.from_numpy(rowidx.astype(np.int64)).to(dev)] = True
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()

    def comp():
        s = torch.matmul(Qs, Cs.T).div_(S).add_(mr).masked_fill_(mask, float("-inf"))
        return torch.topk(s, n, dim=1)
    (tv, ti), tms, tms_min = timed(comp, reps, warmup)
    peak = torch.cuda.max_memory_allocated() - base
    ti = ti.cpu().numpy(); tv = tv.cpu().numpy()
    same_sets = float(np.mean([set(a.tolist()) == set(b.tolist()) for a, b in zip(idx, ti)]))
    rec = dict(shape=name, K=K, S=S, N=n, queries=nq, candidates=nc, gflop=flop / 1e9,
               topn_ms=ms, topn_ms_min=ms_min, topn_gflops=flop / ms / 1e6, frac_of_48_4_tf=flop / ms / 1e9 / CEIL_TF,
               topn_floor_ms=flop / CEIL_TF / 1e9,
               torch_ms=tms, torch_ms_min=tms_min, torch_peak_mib=peak / 2 ** 20,
               topn_result_mib=3 * idx.size * 8 / 2 ** 20,
               agree_sets=same_sets, max_mean_diff=float(np.abs(np.sort(mean, 1) - np.sort(tv, 1)).max()))
    print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["ml1m", "chembl"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("-n", type=int, default=10)
    a = ap.parse_args()
    for s in a.shapes:
        run(s, a.samples, a.n, a.reps, a.warmup)
