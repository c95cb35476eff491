"""Predictive intervals: what the probability integral transform and the quantiles of a list of cells cost beside the
prediction and the convergence diagnostics of the same cells, and how the mixture's intervals compare with the Gaussian shortcut.

    python tools/interval_bench.py cells [--cells 100000] [--reps 5] [--K 32] [--S 200,1000] [--nq 2,8]
        The ML-1M shape (6 040 users x 3 706 movies) with K = 32.  Per number of samples S one pair of rings (a level per entity and
        factor entry, a small move per sample, as a mixed chain leaves them) and one list of random cells with observed values.  Per
        number of quantiles, interleaved: the device time of k_predict_cells (predict_cells_last_ms), of k_cell_traces + k_trace_diag
        (diag_last_ms) and of k_cell_traces + k_trace_quantiles (interval_last_ms: the pit and nq quantiles), medians over --reps calls
        after a warm-up with the smallest and the largest, and the two ratios.  The repeats must give equal bytes.
    python tools/interval_bench.py planted [--nusers 600] [--nmovies 400] [--K 8] [--rank 4] [--density 0.15] [--nsims 120] [--burnin 20]
        A planted low-rank matrix with unit-variance noise of precision alpha = 2, a tenth of the cells held out.  The chain runs with
        intervals at 50 / 80 / 90 / 95 %; reported per level: the coverage of the held-out values with its binomial standard error,
        the mean width of the mixture's interval, and coverage and width of the shortcut mean +- z sqrt(std^2 + 1 / alpha).
    python tools/interval_bench.py geometry
        per S: waves per workgroup and dynamic LDS of k_trace_quantiles (no GPU needed).

One JSON line per measurement.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bpmf_amd                                            # noqa: E402

NU, NM = 6040, 3706                                        # the ML-1M shape


def rings(eng, K, S, seed=1):
    """both sides over an empty matrix with S samples in their rings; u . v has standard deviation about 1"""
    empty_m = (np.zeros(NM + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    empty_u = (np.zeros(NU + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    movies = eng.side_create(NM, NU, *empty_m, 0.0)
    users = eng.side_create(NU, NM, *empty_u, 0.0)
    rng = np.random.default_rng(seed)
    sigma = (1.0 / K) ** 0.25
    for side, n in ((users, NU), (movies, NM)):
        eng.samples_reserve(side, S)
        X = 0.3 * rng.standard_normal((n, S, K))
        X += rng.standard_normal((n, 1, K))
        X *= sigma
        eng.samples_set(side, X)
        del X
    return users, movies


def cells(args):
    K, n = args.K, args.cells
    for S in args.S:
        eng = bpmf_amd.HipEngine(K)
        users, movies = rings(eng, K, S)
        rng = np.random.default_rng(7)
        alpha = 1.5 + rng.random(S)
        q = rng.integers(0, NU, n).astype(np.int32); c = rng.integers(0, NM, n).astype(np.int32)
        mean, _ = eng.predict_cells(users, movies, 3.5, q, c)
        y = mean + rng.standard_normal(n) / np.sqrt(2.0)
        for nq in args.nq:
            tau = np.linspace(0.025, 0.975, nq)
            base = eng.interval_cells(users, movies, 3.5, q, c, alpha, tau, y=y)      # warm-up; and the result the repeats must give
            eng.predict_cells(users, movies, 3.5, q, c); eng.diag_cells(users, movies, 3.5, q, c)
            pms, dms, ims = [], [], []
            for _ in range(args.reps):
                eng.predict_cells(users, movies, 3.5, q, c)
                pms.append(eng.predict_cells_last_ms(users))
                eng.diag_cells(users, movies, 3.5, q, c)
                dms.append(eng.diag_last_ms(users))
                got = eng.interval_cells(users, movies, 3.5, q, c, alpha, tau, y=y)
                ims.append(eng.interval_last_ms(users))
                assert all(base[k].tobytes() == got[k].tobytes() for k in base)
            p, d, i = statistics.median(pms), statistics.median(dms), statistics.median(ims)
            print(json.dumps(dict(what="interval_cells", cells=n, K=K, S=S, nq=nq, predict_cells_ms=round(p, 4), diag_cells_ms=round(d, 4),
                                  interval_cells_ms=round(i, 4), interval_ms_min=round(min(ims), 4), interval_ms_max=round(max(ims), 4),
                                  ratio_to_predict=round(i / p, 3), ratio_to_diag=round(i / d, 3), ns_per_cell_sample=round(i * 1e6 / n / S, 4),
                                  ks=round(bpmf_amd.calibration_summary(base["pit"], ())["ks"], 4), reps=args.reps)), flush=True)
        eng.close()


def planted(args):
    import scipy.sparse as sp
    from scipy.special import ndtri
    rng = np.random.default_rng(3)
    nu, nm, alpha = args.nusers, args.nmovies, 2.0
    A, B = rng.standard_normal((nu, args.rank)), rng.standard_normal((nm, args.rank))
    mask = rng.random((nu, nm)) < args.density
    r, c = np.nonzero(mask)
    v = 3.0 + (A[r] * B[c]).sum(axis=1) / math.sqrt(args.rank) + rng.standard_normal(len(r)) / math.sqrt(alpha)
    test = rng.random(len(r)) < 0.1

    def csc(sel, shape, rows, cols):
        X = sp.coo_matrix((v[sel], (rows[sel], cols[sel])), shape=shape).tocsc(); X.sort_indices()
        return X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data.astype(np.float64)
    M, Mt = csc(~test, (nu, nm), r, c), csc(~test, (nm, nu), c, r)
    T, Tt = csc(test, (nu, nm), r, c), csc(test, (nm, nu), c, r)
    levels = (0.5, 0.8, 0.9, 0.95)
    eng = bpmf_amd.HipEngine(args.K)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=args.nsims, burnin=args.burnin, alpha=alpha, Tt=Tt, intervals=levels)
    d = res["intervals"]["test"]
    s = d["summary"]
    y = np.asarray(T[2])
    for k, l in enumerate(levels):
        half = ndtri((1.0 + l) / 2.0) * np.sqrt(d["std"] ** 2 + 1.0 / alpha)
        print(json.dumps(dict(what="planted", level=l, cells=s["n"], samples=d["samples"], coverage=round(s["coverage"][k], 4), se=round(s["se"][k], 4),
                              width=round(s["width"][k], 4), shortcut_coverage=round(float(np.mean(np.abs(y - d["mean"]) <= half)), 4),
                              shortcut_width=round(float(2.0 * half.mean()), 4), ks=round(s["ks"], 4), rmse=round(float(res["final_rmse_avg"]), 4))), flush=True)
    eng.close()


def geometry(args):
    for S in (1, 64, 200, 1000, 2048, 2049, 4096):
        per_wave = (S + 1) // 2 * 2
        w = 4 if 4 * per_wave * 8 <= 65536 else 2
        print(json.dumps(dict(what="geometry", S=S, waves_per_workgroup=w, lds_bytes_per_workgroup=w * per_wave * 8, terms_per_lane=-(-S // 64))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("cells", "planted", "geometry"))
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, default=None)
    ap.add_argument("--S", type=lambda s: [int(x) for x in s.split(",")], default=[200, 1000])
    ap.add_argument("--nq", type=lambda s: [int(x) for x in s.split(",")], default=[2, 8])
    ap.add_argument("--nusers", type=int, default=600)
    ap.add_argument("--nmovies", type=int, default=400)
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--nsims", type=int, default=120)
    ap.add_argument("--burnin", type=int, default=20)
    a = ap.parse_args()
    if a.K is None:
        a.K = 8 if a.what == "planted" else 32
    dict(cells=cells, planted=planted, geometry=geometry)[a.what](a)
