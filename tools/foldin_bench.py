"""Times the fold-in (kernels_foldin.h): k_foldin by the two device events around its launch
(engine.foldin_last_ms), the median of --reps launches after --warmup, and engine.foldin_topn as a blocking call on a host clock.

Shape: --rows new rows x --ratings ratings each x --samples kept samples against a candidate side of --candidates columns, at every
--K.  Beside each time the (row, sample) rate -- one work item does the arithmetic of one column sample of a sampler launch at
that K and that many ratings (a K x K Gram over the ratings, a factorisation, two solves) -- to be read against the column
samples/s of `bench.py --gpus 1 --K <K>`.  Prints one JSON line per K.

    python tools/foldin_bench.py [--K 32 128] [--rows 10000] [--ratings 20] [--samples 100] [--candidates 300000] [-n 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bpmf_amd                                            # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def run(K, rows, ratings, S, nc, n, reps, warmup, distinct):
    eng = bpmf_amd.HipEngine(K)
    rng = np.random.default_rng(K)
    one = sp.coo_matrix((np.array([3.0]), (np.array([0]), np.array([0]))), shape=(nc, 2)).tocsc()
    csc = lambda A: (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64))
    side = eng.side_create(2, nc, *csc(one), 0.0)
    cand = eng.side_create(nc, 2, *csc(one.T.tocsc()), 0.0)
    eng.samples_reserve(cand, S); eng.hyper_reserve(side, S)
    Vs = [0.3 * rng.standard_normal((nc, K)) for _ in range(distinct)]       # a few distinct samples, taken in turn: the ring is S deep all the same
    for s in range(S):
        eng.set_items(cand, Vs[s % distinct]); eng.samples_add(cand)
        A = rng.standard_normal((K, K))
        eng.hyper_add(side, 2.0 + 0.01 * s, 0.1 * rng.standard_normal(K), A.T @ A / K + np.eye(K))
    # `ratings` distinct columns per row: a random start and a random stride below nc / ratings, ascending
    start = rng.integers(0, nc, rows)[:, None]; step = rng.integers(1, max(2, nc // ratings), rows)[:, None]
    cols = np.sort((start + step * np.arange(ratings)[None, :]) % nc, axis=1)
    assert (np.diff(cols, axis=1) > 0).all()
    R = (np.arange(rows + 1, dtype=np.int64) * ratings, cols.ravel().astype(np.int32), rng.integers(1, 6, rows * ratings).astype(np.float64))
    ms, wall = [], []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        eng.foldin(side, cand, 3.0, R, 7)
        if it >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3); ms.append(eng.foldin_last_ms(side))
    k_ms = median(ms)
    rec = dict(K=K, rows=rows, ratings=ratings, samples=S, candidates=nc, items=rows * S, k_foldin_ms=k_ms, k_foldin_ms_min=min(ms),
               k_foldin_ms_max=max(ms), row_samples_per_s=rows * S / k_ms * 1e3, foldin_call_ms=median(wall))
    tms = []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        idx, tm, ts = eng.foldin_topn(side, cand, 3.0, n)
        if it >= warmup:
            tms.append((time.perf_counter() - t0) * 1e3)
    rec.update(topn_n=n, foldin_topn_ms=median(tms), foldin_topn_ms_min=min(tms), topn_gflop=2.0 * rows * nc * S * K / 1e9)
    assert (idx >= 0).all() and np.isfinite(tm).all()
    print(json.dumps(rec), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="*", default=[32, 128])
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--ratings", type=int, default=20)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--candidates", type=int, default=300000)
    ap.add_argument("-n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--distinct", type=int, default=4, help="distinct random factor matrices the ring is filled from, in turn")
    a = ap.parse_args()
    for K in a.K:
        run(K, a.rows, a.ratings, a.samples, a.candidates, a.n, a.reps, a.warmup, a.distinct)
