"""Saved models: what scoring a list of cells from the sample rings costs, beside the dense block, and what
saving and loading a model costs.

    python tools/model_bench.py cells [--cells 100000,1000000] [--reps 5] [--K 32] [--S 15]
        The ML-1M shape (6 040 users x 3 706 movies) with K = 32 and S = 15 random samples in both rings.  Per list length n: n random
        cells as drawn, and the same cells sorted by query.  Reported per arm: the device time of k_predict_cells between two events
        (predict_cells_last_ms: median and spread over --reps calls after a warm-up), the gathered bytes per second -- a cell reads
        2 S Kp doubles, the bytes the definition needs, whatever the caches keep -- ns per cell, and the wall time of the whole call
        (sort, uploads, launch, copy back).  Then bpmf_hip_predict_block_device over the whole 6 040 x 3 706 block (device events of
        the caller around the call): its ns per cell is what a cell costs when every cell is wanted.
    python tools/model_bench.py io [--K 32] [--S 15]
        save_model / load_model of the same rings: seconds and bytes on disk.
    python tools/model_bench.py geometry
        the launch geometry of k_predict_cells per num_latent: lanes per cell, cells per wave-wide load, cells per workgroup, samples
        per staged chunk (no GPU needed; registers and occupancy are the compiler's: -Rpass-analysis=kernel-resource-usage).

One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bpmf_amd                                            # noqa: E402

NU, NM = 6040, 3706                                        # the ML-1M shape


def kp_of(K):
    return (K + 3) // 4 * 4


def geometry(Kp):
    """(lanes per cell, cells per workgroup, samples per staged chunk): pc_group / pc_segment / pc_chunk of kernels_predcells.h"""
    g = 2
    while 2 * g <= Kp // 2 and g < 64:
        g *= 2
    return g, 4 * 256 // g, 2048 // Kp


def sides(eng, K, S, seed=1):
    """both sides over an empty matrix with S random samples in their rings"""
    empty_m = (np.zeros(NM + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    empty_u = (np.zeros(NU + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    movies = eng.side_create(NM, NU, *empty_m, 0.0)
    users = eng.side_create(NU, NM, *empty_u, 0.0)
    rng = np.random.default_rng(seed)
    for side, n in ((users, NU), (movies, NM)):
        eng.samples_reserve(side, S)
        eng.samples_set(side, rng.standard_normal((n, S, K)))
    return users, movies


def cells(args):
    K, S = args.K, args.S
    Kp = kp_of(K)
    eng = bpmf_amd.HipEngine(K)
    users, movies = sides(eng, K, S)
    rng = np.random.default_rng(7)
    g, seg, chunk = geometry(Kp)
    for n in args.cells:
        q = rng.integers(0, NU, n).astype(np.int32); c = rng.integers(0, NM, n).astype(np.int32)
        order = np.lexsort((c, q))
        for arm, (qq, cc) in (("random", (q, c)), ("sorted_by_query", (q[order], c[order]))):
            base = eng.predict_cells(users, movies, 3.5, qq, cc, 3.0, 0.7)             # warm-up; and the result the repeats must give
            ms, wall = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                got = eng.predict_cells(users, movies, 3.5, qq, cc, 3.0, 0.7)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(eng.predict_cells_last_ms(users))
                assert all(a.tobytes() == b.tobytes() for a, b in zip(base, got))
            med = statistics.median(ms)
            print(json.dumps(dict(what="predict_cells", arm=arm, cells=n, K=K, Kp=Kp, S=S, lanes_per_cell=g, cells_per_workgroup=seg,
                                  samples_per_chunk=chunk, device_ms_median=round(med, 4), device_ms_min=round(min(ms), 4),
                                  device_ms_max=round(max(ms), 4), gathered_GB_per_s=round(n * 2 * S * Kp * 8 / (med * 1e-3) / 1e9, 1),
                                  ns_per_cell=round(med * 1e6 / n, 3), wall_ms_median=round(statistics.median(wall), 3), reps=args.reps)), flush=True)
    # the dense block: every cell of the matrix, written on the device (memory and events of the HIP runtime the library runs on)
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")

    def hip_ok(rc):
        if rc != 0:
            raise RuntimeError("HIP runtime error %d" % rc)
    out = C.c_void_p()
    hip_ok(hip.hipMalloc(C.byref(out), C.c_size_t(2 * NU * NM * 8)))
    mean_ptr, std_ptr = out.value, out.value + NU * NM * 8
    stream = C.c_void_p(eng.lib.bpmf_hip_ctx_stream(eng.ctx))
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(e0))); hip_ok(hip.hipEventCreate(C.byref(e1)))
    eng.predict_block_device(users, movies, 3.5, mean_ptr, std_ptr)                             # warm-up (the call waits)
    ms = []
    for _ in range(args.reps):
        hip_ok(hip.hipEventRecord(e0, stream))
        eng.predict_block_device(users, movies, 3.5, mean_ptr, std_ptr)
        hip_ok(hip.hipEventRecord(e1, stream)); hip_ok(hip.hipEventSynchronize(e1))
        t = C.c_float()
        hip_ok(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        ms.append(t.value)
    hip_ok(hip.hipEventDestroy(e0)); hip_ok(hip.hipEventDestroy(e1)); hip_ok(hip.hipFree(out))
    med = statistics.median(ms)
    print(json.dumps(dict(what="predict_block_device", cells=NU * NM, K=K, S=S, ms_median=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                          ns_per_cell=round(med * 1e6 / (NU * NM), 4), note="events on the context's stream around the call",
                          reps=args.reps)), flush=True)
    eng.close()


def io(args):
    K, S = args.K, args.S
    eng = bpmf_amd.HipEngine(K)
    users, movies = sides(eng, K, S)
    rng = np.random.default_rng(3)
    for side in (users, movies):
        eng.hyper_reserve(side, S)
        for s in range(S):
            A = rng.standard_normal((K, K))
            eng.hyper_add(side, 2.0, rng.standard_normal(K), A @ A.T + K * np.eye(K))
    U = types_sys(eng, users, NU); V = types_sys(eng, movies, NM)
    res = dict(users=U, movies=V, foldin=True, model_info=dict(alpha=2.0, probit=False, probit_threshold=0.0, plain=True))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model")
        t0 = time.perf_counter(); bpmf_amd.save_model(res, path); t_save = time.perf_counter() - t0
        size = sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))
        other = bpmf_amd.HipEngine(K)
        t0 = time.perf_counter(); loaded = bpmf_amd.load_model(other, path); other.sync(); t_load = time.perf_counter() - t0
        assert other.samples_get(loaded["users"].side).tobytes() == eng.samples_get(users).tobytes()
        other.close()
    print(json.dumps(dict(what="save_load", K=K, S=S, rows=NU, cols=NM, bytes=size, save_s=round(t_save, 3), load_s=round(t_load, 3),
                          note="wall time, files on the local disk of the box; load includes creating both sides")), flush=True)
    eng.close()


def types_sys(eng, side, n):
    """what save_model reads of a Sys"""
    import types
    return types.SimpleNamespace(engine=eng, side=side, num=lambda: n, mean_rating=3.5)


def resources(args):
    for K in (1, 8, 20, 32, 64, 128):
        g, seg, chunk = geometry(kp_of(K))
        print(json.dumps(dict(what="geometry", K=K, Kp=kp_of(K), lanes_per_cell=g, cells_per_wave_load=64 // g, cells_per_workgroup=seg,
                              samples_per_chunk=chunk, lds_bytes=2048 * 8)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("cells", "io", "geometry"))
    ap.add_argument("--cells", type=lambda s: [int(x) for x in s.split(",")], default=[100000, 1000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--S", type=int, default=15)
    a = ap.parse_args()
    dict(cells=cells, io=io, geometry=resources)[a.what](a)
