"""Times engine.predict_block (a dense block of posterior means and deviations from two sample rings, kernels_predblock.h) on
the ML-1M shape (all users x all movies, K = 32, S = 15) and on the ChEMBL shape (4 096 rows x 5 775 columns, K = 64, S = 15),
against the ceiling of the f64 16x16x4 MFMA (48.4 TF, profiles/r05_mfma_shapes_probe.txt) and against a torch composition on
the same rings: torch.bmm over the samples, then mean and var over them -- which materialises the S blocks.  The outputs of
predict_block_device are device tensors (written in place), so neither side pays for a copy to the host.  Every time is that of a
blocking call on a host clock, so the TF/s and the share of the ceiling are those of the call, launch and wait included.  Prints
one JSON line per shape.

    python tools/predblock_bench.py [ml1m|chembl ...] [--reps 20] [--warmup 3]
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

CEIL_TF = 48.4
SHAPES = dict(ml1m=dict(K=32, nq=6040, nc=3706), chembl=dict(K=64, nq=4096, nc=5775))


def one_rating(ncols, nrows):
    colptr = np.zeros(ncols + 1, np.int64); colptr[1:] = 1
    return colptr, np.zeros(1, np.int32), np.full(1, 3.0)


def timed(fn, reps, warmup):
    """median, minimum and maximum of `reps` blocking calls, ms: call times on a host clock (launch and wait included), not kernel times"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def run(name, S, reps, warmup):
    K, nq, nc = SHAPES[name]["K"], SHAPES[name]["nq"], SHAPES[name]["nc"]
    eng = bpmf_amd.HipEngine(K)
    q = eng.side_create(nq, nc, *one_rating(nq, nc), 0.0)
    c = eng.side_create(nc, nq, *one_rating(nc, nq), 0.0)
    rng = np.random.default_rng(1)
    eng.samples_reserve(q, S); eng.samples_reserve(c, S)
    Us, Vs = [], []
    for _ in range(S):
        U = 0.3 * rng.standard_normal((nq, K)); V = 0.3 * rng.standard_normal((nc, K))
        eng.set_items(q, U); eng.set_items(c, V)
        eng.samples_add(q); eng.samples_add(c)
        Us.append(U); Vs.append(V)
    dev = torch.device("cuda")
    mean = torch.empty((nq, nc), dtype=torch.float64, device=dev); std = torch.empty_like(mean)
    mr = 3.5
    ms, ms_min, ms_max = timed(lambda: eng.predict_block_device(q, c, mr, mean.data_ptr(), std.data_ptr()), reps, warmup)
    flop = 2.0 * nq * nc * S * K
    Ut = torch.from_numpy(np.stack(Us)).to(dev); Vt = torch.from_numpy(np.stack(Vs)).to(dev)      # [S, n, K]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()

    def comp():
        P = torch.bmm(Ut, Vt.transpose(1, 2))
        return P.mean(0).add_(mr), (P.var(0, unbiased=True).sqrt_() if S > 1 else torch.zeros_like(P[0]))
    tms, tms_min, tms_max = timed(comp, reps, warmup)
    peak = torch.cuda.max_memory_allocated() - base
    tmean, tstd = comp()
    rec = dict(shape=name, K=K, S=S, queries=nq, candidates=nc, gflop=flop / 1e9,
               predblock_ms=ms, predblock_ms_min=ms_min, predblock_ms_max=ms_max, call_tflops=flop / ms / 1e9, call_frac_of_48_4_tf=flop / ms / 1e9 / CEIL_TF,
               floor_ms=flop / CEIL_TF / 1e9, output_mib=2 * nq * nc * 8 / 2 ** 20,
               torch_ms=tms, torch_ms_min=tms_min, torch_ms_max=tms_max, torch_peak_mib=peak / 2 ** 20,
               max_mean_diff=float((mean - tmean).abs().max()), max_std_diff=float((std - tstd).abs().max()))
    print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["ml1m", "chembl"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=15)
    a = ap.parse_args()
    for s in a.shapes:
        run(s, a.samples, a.reps, a.warmup)
