"""Times engine.topn_scored (top-N by an acquisition score, kernels_topn_score.h) for every kind on the two
shapes of tools/topn_bench.py -- ML-1M (K = 32, S = 15, N = 10, every user) and ChEMBL (K = 64, S = 15, N = 10, compounds per
target) -- and beside it
  (a) engine.topn, the mean ranking, on the same rings: the only fair yardstick in the tree,
  (b) the composition the feature replaces: predict_block_device into two device tensors, mean + kappa std, masked_fill of the
      rated pairs and torch.topk, in query ranges of --range queries so that the two blocks fit, with its peak memory,
  (c) the share of the ceiling of the f64 16x16x4 MFMA (48.4 TF, profiles/r05_mfma_shapes_probe.txt).
Every time is that of a blocking call on a host clock (launch, wait and the copy of the lists included); the median of --reps
calls.  Prints one JSON line per shape.

    python tools/topn_score_bench.py [ml1m|chembl ...] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

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
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return out, ms[len(ms) // 2], ms[0]


def run(name, S, n, reps, warmup, qrange):
    d = shape(name)
    K, nu, nm = d["K"], d["nu"], d["nm"]
    eng = bpmf_amd.HipEngine(K)
    mr = float(d["M"][2].mean())
    movies = eng.side_create(nm, nu, *d["M"], mr)
    users = eng.side_create(nu, nm, *d["Mt"], mr)
    rng = np.random.default_rng(1)
    eng.samples_reserve(users, S); eng.samples_reserve(movies, S)
    for _ in range(S):
        eng.set_items(users, 0.3 * rng.standard_normal((nu, K))); eng.set_items(movies, 0.3 * rng.standard_normal((nm, K)))
        eng.samples_add(users); eng.samples_add(movies)
    q, c, rated = (movies, users, d["M"]) if d["by_cols"] else (users, movies, d["Mt"])
    nq, nc = q.ncols, c.ncols
    flop = 2.0 * nq * nc * S * K
    rec = dict(shape=name, K=K, S=S, N=n, queries=nq, candidates=nc, gflop=flop / 1e9, floor_ms=flop / CEIL_TF / 1e9)
    (bi, bmean, bstd), ms, ms_min = timed(lambda: eng.topn(q, c, mr, n), reps, warmup)
    rec.update(mean_ms=ms, mean_ms_min=ms_min, mean_frac_of_48_4_tf=flop / ms / 1e9 / CEIL_TF)
    sigma, t, kappa = 1.0 / np.sqrt(2.0), mr + 0.5, 1.0
    outs = {}
    for kind, param in (("ucb", kappa), ("prob", t), ("ei", t)):
        outs[kind], ms, ms_min = timed(lambda: eng.topn_scored(q, c, mr, n, kind, param, sigma), reps, warmup)
        rec["%s_ms" % kind] = ms; rec["%s_ms_min" % kind] = ms_min
        rec["%s_frac_of_48_4_tf" % kind] = flop / ms / 1e9 / CEIL_TF
    rec["erfc_g_evals"] = nq * nc * S / 1e9

    # (b) predict_block_device + torch: ucb only (prob / ei are not functions of mean and std)
    dev = torch.device("cuda")
    colptr, rowidx = rated[0], rated[1]
    rows_dev = torch.from_numpy(rowidx.astype(np.int64)).to(dev)
    qcol_dev = torch.from_numpy(np.repeat(np.arange(nq), np.diff(colptr))).to(dev)
    qr = min(qrange, nq)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    mean = torch.empty((qr, nc), dtype=torch.float64, device=dev); std = torch.empty_like(mean)

    def comp():
        vals, ids = [], []
        for q0 in range(0, nq, qr):
            q1 = min(nq, q0 + qr)
            m, s = mean[:q1 - q0], std[:q1 - q0]
            eng.predict_block_device(q, c, mr, m.data_ptr(), s.data_ptr(), q0, q1)
            sc = s.mul_(kappa).add_(m)
            lo, hi = int(colptr[q0]), int(colptr[q1])
            sc[qcol_dev[lo:hi] - q0, rows_dev[lo:hi]] = float("-inf")
            v, i = torch.topk(sc, n, dim=1)
            vals.append(v); ids.append(i)
            # the two blocks are reused by the next range, which the engine writes on ITS stream: torch must be done reading them
            # first (a top-k over values that change under it selects more than n elements and writes past its output)
            torch.cuda.synchronize()
        return torch.cat(vals), torch.cat(ids)
    (tv, ti), tms, tms_min = timed(comp, reps, warmup)
    peak = torch.cuda.max_memory_allocated() - base
    ti = ti.cpu().numpy(); tv = tv.cpu().numpy()
    idx, score = outs["ucb"][0], outs["ucb"][1]
    rec.update(block_topk_ms=tms, block_topk_ms_min=tms_min, block_topk_peak_mib=peak / 2 ** 20, block_topk_query_range=qr,
               scored_result_mib=(3 * 8 + 4) * idx.size / 2 ** 20,
               agree_sets=float(np.mean([set(a.tolist()) == set(b.tolist()) for a, b in zip(idx, ti)])),
               max_score_diff=float(np.abs(np.sort(score, 1) - np.sort(tv, 1)).max()))
    print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["ml1m", "chembl"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("-n", type=int, default=10)
    ap.add_argument("--range", type=int, default=512, help="queries per block of the predict_block composition")
    a = ap.parse_args()
    for s in a.shapes:
        run(s, a.samples, a.n, a.reps, a.warmup, a.range)
