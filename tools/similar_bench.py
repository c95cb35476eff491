"""Similar columns: what ranking the neighbours of every column of a side costs, beside the two routes through
the existing scored top-N.

    python tools/similar_bench.py [--shapes 3706:32,3706:128,100000:32] [--S 15] [--n 10] [--reps 7]

Per shape (columns : num_latent) a side over an empty matrix with S random samples in its ring -- 3 706 columns is the ML-1M item
side -- and three arms, each the n best neighbours of EVERY column:
    similar           engine.similar(side, n, "cosine"): the norm table, k_similar_topn, the merge
    normalised_copy   engine.topn_scored("ucb", kappa = 0) over a normalised copy of the ring in a scratch pair of sides whose exclusion
                      list is the query's own column: what Python can assemble without the kernel; copy_MiB is the device memory of the
                      two scratch rings it needs beside the side's own
    topn_scored_self  engine.topn_scored("ucb", kappa = 0) of the side against itself, nothing excluded: the plain cost of the tile
                      product with moments and selection
Every arm is timed between two events recorded on the context's stream around the call (which allocates its result lists, launches,
waits and copies the lists back): median of --reps calls after a warm-up, with min and max.  For `similar` the line also carries the
library's own figure (similar_last_ms: events around the launches alone).  One JSON line per measurement.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bpmf_amd                                            # noqa: E402


def kp_of(K):
    return (K + 3) // 4 * 4


def csc_arrays(m):
    m = m.tocsc()
    return np.ascontiguousarray(m.indptr, np.int64), np.ascontiguousarray(m.indices, np.int32), np.ascontiguousarray(m.data, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3706:32,3706:128,100000:32")
    ap.add_argument("--S", type=int, default=15)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")

    def hip_ok(rc):
        if rc != 0:
            raise RuntimeError("HIP runtime error %d" % rc)

    for shape in args.shapes.split(","):
        nc, K = (int(v) for v in shape.split(":"))
        S, n, Kp = args.S, args.n, kp_of(K)
        eng = bpmf_amd.HipEngine(K)
        try:
            stream = C.c_void_p(eng.lib.bpmf_hip_ctx_stream(eng.ctx))
            e0, e1 = C.c_void_p(), C.c_void_p()
            hip_ok(hip.hipEventCreate(C.byref(e0))); hip_ok(hip.hipEventCreate(C.byref(e1)))
            rng = np.random.default_rng(nc + K)
            V = rng.standard_normal((nc, S, K))
            side = eng.side_create(nc, 1, np.zeros(nc + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
            eng.samples_reserve(side, S); eng.samples_set(side, V)
            eye = csc_arrays(sp.identity(nc, format="csc"))
            sq, sc = eng.side_create(nc, nc, *eye, 0.0), eng.side_create(nc, nc, *eye, 0.0)
            N = V / np.sqrt((V * V).sum(2, keepdims=True))
            for s in (sq, sc):
                eng.samples_reserve(s, S); eng.samples_set(s, N)
            arms = (("similar", lambda: eng.similar(side, n, "cosine", 0.0)),
                    ("normalised_copy", lambda: eng.topn_scored(sq, sc, 0.0, n, "ucb", 0.0)),
                    ("topn_scored_self", lambda: eng.topn_scored(side, side, 0.0, n, "ucb", 0.0, exclude_rated=False)))
            lists = {}
            for name, call in arms:
                lists[name] = call()                                           # warm-up
                ms, own = [], []
                for _ in range(args.reps):
                    hip_ok(hip.hipEventRecord(e0, stream))
                    call()
                    hip_ok(hip.hipEventRecord(e1, stream)); hip_ok(hip.hipEventSynchronize(e1))
                    t = C.c_float()
                    hip_ok(hip.hipEventElapsedTime(C.byref(t), e0, e1))
                    ms.append(t.value)
                    if name == "similar":
                        own.append(eng.similar_last_ms(side))
                med = statistics.median(ms)
                line = dict(what="similar_bench", arm=name, columns=nc, K=K, Kp=Kp, S=S, n=n, ms_median=round(med, 3), ms_min=round(min(ms), 3),
                            ms_max=round(max(ms), 3), ns_per_pair_sample=round(med * 1e6 / (float(nc) * nc * S), 5), reps=args.reps)
                if own:
                    line.update(launches_ms_median=round(statistics.median(own), 3), launches_ms_min=round(min(own), 3), launches_ms_max=round(max(own), 3))
                if name == "normalised_copy":
                    line.update(copy_MiB=round(2 * nc * S * Kp * 8 / 2.0 ** 20, 1), ring_MiB=round(nc * S * Kp * 8 / 2.0 ** 20, 1))
                print(json.dumps(line), flush=True)
            same = float((lists["similar"][0] == lists["normalised_copy"][0]).mean())
            print(json.dumps(dict(what="similar_bench", arm="agreement", columns=nc, K=K, same_neighbour_share=round(same, 6))), flush=True)
            hip_ok(hip.hipEventDestroy(e0)); hip_ok(hip.hipEventDestroy(e1))
        finally:
            eng.close()


if __name__ == "__main__":
    main()
