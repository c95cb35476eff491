"""Model comparison: what the log predictive density and the WAIC correction of a list of cells cost beside the
prediction of the same cells.

    python tools/score_bench.py cells [--train 1000000] [--test 100000] [--reps 5] [--K 32] [--S 200,1000] [--kinds gaussian,student,probit]
        The ML-1M shape (6 040 users x 3 706 movies) with K = 32.  Per number of samples S one pair of rings (a level per entity and
        factor entry, a small move per sample, as a mixed chain leaves them), and two lists of random cells: `train` (the 10^6 cells
        WAIC runs over) and `test` (the 10^5 held-out cells).  Per list and kind, interleaved: the device time of k_predict_cells
        (predict_cells_last_ms) and of k_cells_logdens (score_last_ms, between two events around the launches), medians over --reps
        calls after a warm-up with the smallest and the largest, their ratio, and the wall time of the whole score_cells call (which
        the grouping of the list on the host and the copies dominate).  The repeats must give equal bytes.
    python tools/score_bench.py geometry
        per K: lanes per cell, cells per workgroup, samples per staged chunk (no GPU needed; registers are the compiler's:
        -Rpass-analysis=kernel-resource-usage).

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
    K = args.K
    for S in args.S:
        eng = bpmf_amd.HipEngine(K)
        users, movies = rings(eng, K, S)
        rng = np.random.default_rng(7)
        alpha = 1.5 + rng.random(S)
        for name, n in (("train", args.train), ("test", args.test)):
            q = rng.integers(0, NU, n).astype(np.int32); c = rng.integers(0, NM, n).astype(np.int32)
            mean, _ = eng.predict_cells(users, movies, 3.5, q, c)
            y = mean + rng.standard_normal(n) / np.sqrt(2.0)
            for kind in args.kinds:
                kw = dict(gaussian=dict(y=y, alpha=alpha), student=dict(y=y, alpha=alpha, nu=4.0),
                          probit=dict(y=np.where(y > mean, 1.0, -1.0), alpha=1.0))[kind]
                m0 = 0.0 if kind == "probit" else 3.5
                base = eng.score_cells(users, movies, m0, q, c, kind=kind, **kw)           # warm-up; and the result the repeats must give
                eng.predict_cells(users, movies, m0, q, c)
                pms, sms, wall = [], [], []
                for _ in range(args.reps):
                    eng.predict_cells(users, movies, m0, q, c)
                    pms.append(eng.predict_cells_last_ms(users))
                    t0 = time.perf_counter()
                    got = eng.score_cells(users, movies, m0, q, c, kind=kind, **kw)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    sms.append(eng.score_last_ms(users))
                    assert all(base[k].tobytes() == got[k].tobytes() for k in base)
                p, d = statistics.median(pms), statistics.median(sms)
                print(json.dumps(dict(what="score_cells", list=name, kind=kind, cells=n, K=K, S=S, predict_cells_ms=round(p, 4),
                                      predict_ms_min=round(min(pms), 4), predict_ms_max=round(max(pms), 4), score_cells_ms=round(d, 4),
                                      score_ms_min=round(min(sms), 4), score_ms_max=round(max(sms), 4), ratio=round(d / p, 3),
                                      ns_per_cell_sample=round(d * 1e6 / n / S, 4), wall_ms_median=round(statistics.median(wall), 3),
                                      lpd_mean=round(float(base["lpd"].mean()), 4), p_waic_mean=round(float(base["pwaic"].mean()), 4),
                                      reps=args.reps)), flush=True)
        eng.close()


def geometry(args):
    for K in (4, 8, 16, 32, 36, 64, 128):
        Kp = (K + 3) // 4 * 4
        g = 2
        while 2 * g <= Kp // 2 and g < 64:
            g *= 2
        print(json.dumps(dict(what="geometry", K=K, Kp=Kp, lanes_per_cell=g, cells_per_workgroup=4 * 256 // g, samples_per_chunk=2048 // Kp,
                              density_lanes_per_group=min(g, 4), lds_bytes_per_workgroup=16384)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("cells", "geometry"))
    ap.add_argument("--train", type=int, default=1000000)
    ap.add_argument("--test", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--S", type=lambda s: [int(x) for x in s.split(",")], default=[200, 1000])
    ap.add_argument("--kinds", type=lambda s: s.split(","), default=["gaussian", "student", "probit"])
    a = ap.parse_args()
    dict(cells=cells, geometry=geometry)[a.what](a)
