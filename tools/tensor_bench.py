"""Measures the tensor factorisation (kernels_tensor.h, capi_tensor.hip) on a synthetic --dims tensor with --nnz
entries at every --K.  Prints one JSON line per K:

  khatri_rao   per mode the device time of one k_khatri_rao launch (events on its dispatch packet, engine.tensor_last_ms), the median
               of --reps launches after --warmup, with min / max; bytes = 8 ld nnz written + 8 nnz of indices read (the operand rows
               mostly come from the caches), and bytes / s
  sampler      per mode the device time of the sampler launch behind it (engine.last_kernel_ms of the mode's side), against the same
               columns as a MATRIX side: same column pointers, values and K, rows = the entries' index in the first other mode, the
               other side holding that mode's factors -- through the same blocking stateless call, the two alternating
  iteration    host clock around the three blocking half-iterations of one tensor iteration (hyper-parameter draws included)
  device_bytes what the device holds more than before the tensor was created (hipMemGetInfo)

    python tools/tensor_bench.py [--K 32 64 128] [--dims 6040 3706 36] [--nnz 1000000] [--reps 10] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bpmf_amd                                            # noqa: E402
from bpmf_amd import engine as E                           # noqa: E402


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def device_free():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return free.value


def synthetic(dims, nnz, seed):
    rng = np.random.default_rng(seed)
    ncell = dims[0] * dims[1] * dims[2]
    cells = np.unique(rng.integers(0, ncell, int(nnz * 1.02)))
    while len(cells) < nnz:
        cells = np.unique(np.concatenate([cells, rng.integers(0, ncell, nnz)]))
    cells = rng.permutation(cells)[:nnz]
    idx = np.stack(np.unravel_index(cells, dims), axis=1).astype(np.int32)
    return idx, rng.integers(1, 6, nnz).astype(np.float64)


def run(K, dims, nnz, reps, warmup):
    idx, vals = synthetic(dims, nnz, 11)
    mean = float(vals.mean())
    eng = bpmf_amd.HipEngine(K)
    ld = eng.ld()
    rng = np.random.default_rng(K)
    F = [(2.0 / K) ** 0.25 * rng.standard_normal((d, K)) for d in dims]
    free0 = device_free()
    T = eng.tensor_create(idx, vals, dims, mean)
    free1 = device_free()
    for m in range(3):
        eng.set_items(T.sides[m], F[m])
    rec = dict(K=K, ld=ld, dims=list(dims), nnz=nnz, reps=reps, device_bytes=free0 - free1, p_bytes=8 * ld * nnz)
    # -- the Khatri-Rao kernel ----------------------------------------------------------------------------------------------------------
    kr = [[] for _ in range(3)]
    for it in range(warmup + reps):
        for m in range(3):
            eng.tensor_product_run(T, m)
            if it >= warmup:
                kr[m].append(eng.tensor_last_ms(T))
    nbytes = 8 * ld * nnz + 8 * nnz
    rec["khatri_rao"] = [dict(stats(kr[m]), TBps=nbytes / (stats(kr[m])["median"] * 1e-3) / 1e12) for m in range(3)]
    # -- the samplers behind it, against the same columns as a matrix side ------------------------------------------------------------
    order = [np.argsort(idx[:, m], kind="stable") for m in range(3)]
    colptr = [np.concatenate([[0], np.cumsum(np.bincount(idx[:, m], minlength=dims[m]))]).astype(np.int64) for m in range(3)]
    pairs = []
    for m in range(3):
        a = 1 if m == 0 else 0
        me = eng.side_create(dims[m], dims[a], colptr[m], idx[order[m], a], vals[order[m]], mean)
        ot = eng.side_create(dims[a], dims[m], np.zeros(dims[a] + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
        eng.set_items(ot, F[a])
        pairs.append((me, ot))
    hyp = [E.hyper_sample(K, dims[m], np.eye(K) * 0.2, 4) for m in range(3)]
    ts = [[] for _ in range(3)]; ms_ = [[] for _ in range(3)]
    for it in range(warmup + reps):
        for m in range(3):
            mu, _, LF = hyp[m]
            for f in range(3):
                if f != m:
                    eng.set_items(T.sides[f], F[f])
            eng.tensor_sample(T, m, 4, 2.0, mu, LF)
            t_ms = eng.last_kernel_ms(T.sides[m])[0]
            eng.sample_side(pairs[m][0], pairs[m][1], 4, 2.0, mu, LF)
            m_ms = eng.last_kernel_ms(pairs[m][0])[0]
            if it >= warmup:
                ts[m].append(t_ms); ms_[m].append(m_ms)
    rec["sampler"] = [dict(mode=m, kernel=eng.kernel_name(T.sides[m]), matrix_kernel=eng.kernel_name(pairs[m][0]), tensor_ms=stats(ts[m]),
                           matrix_ms=stats(ms_[m])) for m in range(3)]
    for me, ot in pairs:
        eng.side_destroy(me); eng.side_destroy(ot)
    # -- a whole iteration ------------------------------------------------------------------------------------------------------------
    cov = [np.eye(K) * 0.2 for _ in range(3)]
    wall = []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        for m in (2, 1, 0):
            mu, _, LF = E.hyper_sample(K, dims[m], cov[m], it)
            s, prod, _ = eng.tensor_sample(T, m, it, 2.0, mu, LF)
            cov[m] = E.cov_from_sums(K, dims[m], s, prod)
        if it >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    rec["iteration_ms"] = stats(wall)
    eng.tensor_destroy(T)
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--dims", type=int, nargs=3, default=[6040, 3706, 36])
    ap.add_argument("--nnz", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for K in a.K:
        print(json.dumps(run(K, tuple(a.dims), a.nnz, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
