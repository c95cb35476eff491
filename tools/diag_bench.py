"""Convergence diagnostics: what split-Rhat and ESS of a list of cells cost beside the prediction of the same cells.

    python tools/diag_bench.py cells [--cells 100000] [--reps 5] [--K 32] [--S 15,200,1000] [--batch-cells N]
        The ML-1M shape (6 040 users x 3 706 movies) with K = 32.  Per number of samples S, two pairs of rings: `iid` -- every factor
        an independent normal per sample, where the loop over the lag pairs stops after a pair or two -- and `halves_disagree` -- the
        users' factors keep one level over the first half of the samples and another over the second, so that every autocorrelation
        estimate stays positive and the loop runs to the lag limit (the worst case: (n / 2) n multiply-adds per half).  n random
        cells.  Reported per arm: the device time of k_predict_cells (predict_cells_last_ms) and of the kernels of diag_cells
        (diag_last_ms: k_cell_traces and k_trace_diag of every batch, between two events), medians over --reps calls after a warm-up,
        their ratio, the batches the list took, the bytes of the trace round trip (n S doubles written once and read once), and the
        wall time of the whole diag_cells call.  --batch-cells N: N cells per batch in place of what fits the 256 MiB trace buffer.
    python tools/diag_bench.py traces [--traces 100000] [--S 15,200,1000]
        diag_traces of random traces given by the host: wall time, which the upload dominates.
    python tools/diag_bench.py mc [--cells 100000] [--reps 5] [--K 32] [--CS 1x200,4x50,4x250,8x512]
        The multi-chain rank-normalised estimator on the same shape and the same two kinds of rings, which then
        hold C chains of S samples one after the other (`halves_disagree`: the level changes in the middle of every chain).  Per
        (C, S): the device time of diag_cells_mc (k_cell_traces and k_trace_diag_mc of every batch) beside diag_cells at the same
        C S samples and beside k_predict_cells, medians over --reps calls after a warm-up.
    python tools/diag_bench.py geometry
        per S: waves per workgroup and the LDS a workgroup of k_trace_diag takes, and the workgroups that fit the 160 KiB of a CU
        (no GPU needed; registers are the compiler's: -Rpass-analysis=kernel-resource-usage).

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

NU, NM = 6040, 3706                                        # the ML-1M shape
TRACE_BYTES = 256 << 20                                    # kTraceBytes of capi_diag.hip


def trace_geometry(S):
    """(waves per workgroup, LDS bytes per workgroup, workgroups per CU by LDS): diag_waves / diag_lds_doubles of kernels_diag.h"""
    two_n = S & ~1
    waves = 4 if two_n <= 2048 else 2
    lds = waves * two_n * 8
    return waves, lds, min(160 * 1024 // lds, 32 // waves)


def rings(eng, K, S, kind, seed=1, chains=1):
    """both sides over an empty matrix with chains * S samples in their rings"""
    empty_m = (np.zeros(NM + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    empty_u = (np.zeros(NU + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    movies = eng.side_create(NM, NU, *empty_m, 0.0)
    users = eng.side_create(NU, NM, *empty_u, 0.0)
    rng = np.random.default_rng(seed)
    for side, n in ((users, NU), (movies, NM)):
        eng.samples_reserve(side, chains * S)
        if kind == "iid":
            X = rng.standard_normal((n, S, K))
        else:                                              # a level per entity and half (the users') or per entity (the movies'), small noise
            X = 0.1 * rng.standard_normal((n, S, K))
            X += rng.standard_normal((n, 1, K))
            if side is users:
                X[:, S - S // 2:] += rng.standard_normal((n, 1, K))
        if chains > 1:                                     # the same construction per chain, chain-major
            X = np.concatenate([X] + [X + 0.05 * rng.standard_normal((n, 1, K)) for _ in range(chains - 1)], axis=1)
        eng.samples_set(side, X)
        del X
    return users, movies


def cells(args):
    K = args.K
    for S in args.S:
        for kind in ("iid", "halves_disagree"):
            eng = bpmf_amd.HipEngine(K)
            users, movies = rings(eng, K, S, kind)
            rng = np.random.default_rng(7)
            n = args.cells
            q = rng.integers(0, NU, n).astype(np.int32); c = rng.integers(0, NM, n).astype(np.int32)
            eng.diag_batch_cells(args.batch_cells)
            base = eng.diag_cells(users, movies, 3.5, q, c)                                   # warm-up; and the result the repeats must give
            eng.predict_cells(users, movies, 3.5, q, c)
            pms, dms, wall = [], [], []
            for _ in range(args.reps):
                eng.predict_cells(users, movies, 3.5, q, c)
                pms.append(eng.predict_cells_last_ms(users))
                t0 = time.perf_counter()
                got = eng.diag_cells(users, movies, 3.5, q, c)
                wall.append((time.perf_counter() - t0) * 1e3)
                dms.append(eng.diag_last_ms(users))
                assert all(base[k].tobytes() == got[k].tobytes() for k in base)
            p, d = statistics.median(pms), statistics.median(dms)
            ok = ~np.isnan(base["ess"])
            per_batch = args.batch_cells or max(1, TRACE_BYTES // (S * 8))
            print(json.dumps(dict(what="diag_cells", ring=kind, cells=n, K=K, S=S, predict_cells_ms=round(p, 4), diag_cells_ms=round(d, 4),
                                  diag_ms_min=round(min(dms), 4), diag_ms_max=round(max(dms), 4), ratio=round(d / p, 2),
                                  batches=-(-n // per_batch), trace_round_trip_MB=round(2 * n * S * 8 / 1e6, 1),
                                  ns_per_cell=round(d * 1e6 / n, 2), wall_ms_median=round(statistics.median(wall), 3),
                                  ess_median=round(float(np.median(base["ess"][ok])), 2), rhat_median=round(float(np.median(base["rhat"][ok])), 4),
                                  reps=args.reps)), flush=True)
            eng.close()


def mc(args):
    K = args.K
    for C, S in args.CS:
        for kind in ("iid", "halves_disagree"):
            eng = bpmf_amd.HipEngine(K)
            users, movies = rings(eng, K, S, kind, chains=C)
            rng = np.random.default_rng(7)
            n = args.cells
            q = rng.integers(0, NU, n).astype(np.int32); c = rng.integers(0, NM, n).astype(np.int32)
            base = eng.diag_cells_mc(users, movies, 3.5, q, c, C)                             # warm-up; and the result the repeats must give
            eng.diag_cells(users, movies, 3.5, q, c); eng.predict_cells(users, movies, 3.5, q, c)
            pms, dms, mms = [], [], []
            for _ in range(args.reps):
                eng.predict_cells(users, movies, 3.5, q, c)
                pms.append(eng.predict_cells_last_ms(users))
                eng.diag_cells(users, movies, 3.5, q, c)
                dms.append(eng.diag_last_ms(users))
                got = eng.diag_cells_mc(users, movies, 3.5, q, c, C)
                mms.append(eng.diag_last_ms(users))
                assert all(base[k].tobytes() == got[k].tobytes() for k in base)
            p, d, m = statistics.median(pms), statistics.median(dms), statistics.median(mms)
            ok = ~np.isnan(base["ess_bulk"])
            print(json.dumps(dict(what="diag_cells_mc", ring=kind, cells=n, K=K, C=C, S=S, predict_cells_ms=round(p, 4), diag_cells_ms=round(d, 4),
                                  diag_cells_mc_ms=round(m, 4), mc_ms_min=round(min(mms), 4), mc_ms_max=round(max(mms), 4),
                                  mc_over_diag=round(m / d, 2), mc_over_predict=round(m / p, 2), ns_per_cell=round(m * 1e6 / n, 2),
                                  ess_bulk_median=round(float(np.median(base["ess_bulk"][ok])), 2),
                                  rhat_median=round(float(np.median(base["rhat"][ok])), 4), reps=args.reps)), flush=True)
            eng.close()


def traces(args):
    eng = bpmf_amd.HipEngine(8)
    rng = np.random.default_rng(3)
    for S in args.S:
        X = rng.standard_normal((args.traces, S))
        eng.diag_traces(X)
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            eng.diag_traces(X)
            wall.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(what="diag_traces", traces=args.traces, S=S, wall_ms_median=round(statistics.median(wall), 3),
                              uploaded_MB=round(X.nbytes / 1e6, 1), reps=args.reps)), flush=True)
    eng.close()


def geometry(args):
    for S in (8, 15, 200, 1000, 2049, 2050, 4096):
        w, lds, per_cu = trace_geometry(S)
        print(json.dumps(dict(what="geometry", S=S, waves_per_workgroup=w, lds_bytes_per_workgroup=lds, workgroups_per_cu=per_cu,
                              waves_per_cu=per_cu * w)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("cells", "mc", "traces", "geometry"))
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--traces", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-cells", type=int, default=0)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--S", type=lambda s: [int(x) for x in s.split(",")], default=[15, 200, 1000])
    ap.add_argument("--CS", type=lambda s: [tuple(int(v) for v in x.split("x")) for x in s.split(",")], default=[(1, 200), (4, 50), (4, 250), (8, 512)])
    a = ap.parse_args()
    dict(cells=cells, mc=mc, traces=traces, geometry=geometry)[a.what](a)
