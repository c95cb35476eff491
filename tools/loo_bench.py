"""PSIS-LOO: what the cross-validation of a list of cells costs beside their scores and their intervals, and how its
estimate compares with WAIC and with a held-out set on planted data.

    python tools/loo_bench.py cells [--cells 100000] [--reps 5] [--K 32] [--S 200,1000]
        The ML-1M shape (6 040 users x 3 706 movies) with K = 32.  Per number of samples S one pair of rings (a level per entity and
        factor entry, a small move per sample, as a mixed chain leaves them) and one list of random cells with observed values.
        Interleaved: the device time of k_cells_logdens (score_last_ms), of k_cell_traces + k_trace_quantiles with the pit and two
        quantiles (interval_last_ms) and of k_cell_traces + k_trace_psis (loo_last_ms), medians over --reps calls after a warm-up, and the
        two ratios.  The repeats must give equal bytes.
    python tools/loo_bench.py planted [--nusers 600] [--nmovies 400] [--K 8] [--rank 4] [--density 0.15] [--nsims 120] [--burnin 20]
        A planted rank-4 matrix with noise of precision alpha = 2, a tenth of the cells held out.  The chain runs with score and loo;
        reported: elpd_loo / N and (lpd - p_waic) / N of the training cells beside the mean log density of the held-out cells (what
        both estimate), with their standard errors, p_loo beside p_waic, and the khat histogram.

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
        tau = np.array([0.05, 0.95])
        base = eng.loo_cells(users, movies, 3.5, q, c, y, alpha)                       # warm-up; and the result the repeats must give
        eng.score_cells(users, movies, 3.5, q, c, y, alpha); eng.interval_cells(users, movies, 3.5, q, c, alpha, tau, y=y)
        sms, ims, lms = [], [], []
        for _ in range(args.reps):
            eng.score_cells(users, movies, 3.5, q, c, y, alpha)
            sms.append(eng.score_last_ms(users))
            eng.interval_cells(users, movies, 3.5, q, c, alpha, tau, y=y)
            ims.append(eng.interval_last_ms(users))
            got = eng.loo_cells(users, movies, 3.5, q, c, y, alpha)
            lms.append(eng.loo_last_ms(users))
            assert all(base[k].tobytes() == got[k].tobytes() for k in base)
        s, i, l = statistics.median(sms), statistics.median(ims), statistics.median(lms)
        k = base["khat"]
        print(json.dumps(dict(what="loo_cells", cells=n, K=K, S=S, score_cells_ms=round(s, 4), interval_cells_ms=round(i, 4), loo_cells_ms=round(l, 4),
                              loo_ms_min=round(min(lms), 4), loo_ms_max=round(max(lms), 4), ratio_to_score=round(l / s, 3),
                              ratio_to_interval=round(l / i, 3), ns_per_cell_sample=round(l * 1e6 / n / S, 4),
                              khat_median=round(float(np.median(k)), 4), khat_above_07=round(float(np.mean(k > 0.7)), 4), reps=args.reps)), flush=True)
        eng.close()


def planted(args):
    import scipy.sparse as sp
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
    eng = bpmf_amd.HipEngine(args.K)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=args.nsims, burnin=args.burnin, alpha=alpha, Tt=Tt, score=True, loo=True)
    loo, waic, held = res["loo"]["summary"], res["score"]["train"]["summary"], res["score"]["test"]["summary"]
    n = loo["n"]
    print(json.dumps(dict(what="planted", train_cells=n, test_cells=held["n"], samples=loo["samples"], elpd_loo_per_cell=round(loo["elpd_loo"] / n, 5),
                          elpd_loo_se=round(loo["se"] / n, 5), elpd_waic_per_cell=round(waic["elpd"] / n, 5), elpd_waic_se=round(waic["se"] / n, 5),
                          held_out_lpd_per_cell=round(held["lpd_mean"], 5), held_out_se=round(held["se_lpd"] / held["n"], 5),
                          train_lpd_per_cell=round(waic["lpd_sum"] / n, 5), p_loo=round(loo["p_loo"], 2), p_waic=round(waic["p_waic"], 2),
                          pwaic_above_04=round(waic["pwaic_above"], 4), khat_counts=loo["khat_counts"], khat_threshold=round(loo["khat_threshold"], 4),
                          khat_above=round(loo["khat_above"], 4), rmse=round(float(res["final_rmse_avg"]), 4))), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("cells", "planted"))
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, default=None)
    ap.add_argument("--S", type=lambda s: [int(x) for x in s.split(",")], default=[200, 1000])
    ap.add_argument("--nusers", type=int, default=600)
    ap.add_argument("--nmovies", type=int, default=400)
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--density", type=float, default=0.15)
    ap.add_argument("--nsims", type=int, default=120)
    ap.add_argument("--burnin", type=int, default=20)
    a = ap.parse_args()
    if a.K is None:
        a.K = 8 if a.what == "planted" else 32
    dict(cells=cells, planted=planted)[a.what](a)
