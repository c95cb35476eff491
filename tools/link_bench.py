"""Side information (gibbs(..., row_features=), kernels_link.h): what its kernels and its loop cost.

    python tools/link_bench.py kernels [ml1m chembl] [--reps 5]
        starts `rocprofv3 --kernel-trace --stats -- python tools/link_bench.py work SHAPE` as a child process of its own per shape and
        reads the kernel trace it leaves: per kernel and grid (the small products of the loop share the kernels of the tall ones) the
        median time, registers, LDS and scratch; for the two tall products (F^T (U - 1 mu^T): k_link_gemm_tn, M = F beta:
        k_link_gemm_nn) TF/s and bytes/s, and the same for the kernels torch.matmul launches for them in fp64 (the yardstick).
    python tools/link_bench.py work SHAPE [--reps 5]
        the work itself: user features on the shape (ml1m: N = 6 040, D = 64, K = 32; chembl: N = 483 500, D = 1024, K = 64),
        `reps` iterations of the features loop, `reps` torch.matmul of each product.
    python tools/link_bench.py iter [ml1m chembl] [--secs 2] [--rounds 3]
        per-iteration time of the features loop against the plain un-pipelined gibbs on the same matrix, interleaved windows.

One JSON line per measurement.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bpmf_amd                                            # noqa: E402
from bpmf_amd import synth                                 # noqa: E402

PEAK_TFLOPS, PEAK_TBS = 48.4, 8.0                          # the 16x16x4 f64 MFMA shape as measured; HBM


def shape(name):
    if name == "ml1m":
        M, Mt, T, Tt, nu, nm = synth.ml1m_shaped(seed=42)
        return dict(K=32, D=64, M=M, Mt=Mt, T=T, Tt=Tt, nu=nu, nm=nm)
    M, Mt, T, Tt, nu, nm = synth.ratings(483500, 5775, 1_023_952, seed=42, real_valued=True)
    return dict(K=64, D=1024, M=M, Mt=Mt, T=T, Tt=Tt, nu=nu, nm=nm)


def features(n, D):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    return torch.randn((n, D), dtype=torch.float64, device="cuda", generator=g)


def work(name, reps):
    import torch
    d = shape(name)
    K, D, nu, nm = d["K"], d["D"], d["nu"], d["nm"]
    Ft = features(nu, D)
    F = Ft.cpu().numpy()
    eng = bpmf_amd.HipEngine(K)
    try:
        movies = eng.side_create(nm, nu, *d["M"], float(d["M"][2].mean()))
        users = eng.side_create(nu, nm, *d["Mt"], float(d["Mt"][2].mean()))
        t0 = time.perf_counter()
        eng.set_features(users, F, 5.0, 4)
        t_set = time.perf_counter() - t0
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.link_sample(movies, users, 2.0)
            eng.link_sample(users, movies, 2.0)
            ms.append((time.perf_counter() - t0) * 1e3)
    finally:
        eng.close()
    U = torch.randn((nu, K), dtype=torch.float64, device="cuda")
    B = torch.randn((D, K), dtype=torch.float64, device="cuda")
    for _ in range(reps):
        P = Ft.T @ U
        Mo = Ft @ B
    torch.cuda.synchronize()
    print(json.dumps(dict(mode="work", shape=name, N=nu, D=D, K=K, set_features_s=round(t_set, 3), iteration_ms_median=round(statistics.median(ms), 3),
                          check=float(P[0, 0] + Mo[0, 0]))), flush=True)


def kernels(names, reps):
    for name in names:
        d = dict(ml1m=dict(N=6040, D=64, K=32), chembl=dict(N=483500, D=1024, K=64))[name]
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "link", "--", sys.executable, os.path.abspath(__file__), "work", name,
                   "--reps", str(reps)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    print(line, flush=True)
            if r.returncode != 0:
                print(json.dumps(dict(mode="kernels", shape=name, error=r.stderr[-600:])), flush=True)
                continue
            rows = []
            for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
                with open(path) as f:
                    rows += list(csv.DictReader(f))
        # per (kernel, grid): the loop's small products (beta^T beta, the beta update) share the kernels of the tall ones
        groups = {}
        for row in rows:
            nm_ = row.get("Kernel_Name", "")
            ours = "k_link_" in nm_
            blas = any(t in nm_ for t in ("Cijk", "gemm", "Gemm")) and not ours
            if not (ours or blas):
                continue
            key = (nm_, int(row.get("Grid_Size_X", 0) or 0), int(row.get("Grid_Size_Y", 0) or 0))
            groups.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), row.get("VGPR_Count"), row.get("Accum_VGPR_Count"),
                                               row.get("LDS_Block_Size"), row.get("Scratch_Size")))
        N, D, K = d["N"], d["D"], d["K"]
        nt = 1 if K <= 16 else 2 if K <= 32 else 4 if K <= 64 else 8
        flops, byts = 2.0 * N * D * K, 8.0 * N * (D + K)
        for (nm_, gx, gy), v in sorted(groups.items()):
            ns = statistics.median(x[0] for x in v)
            rec = dict(mode="kernels", shape=name, kernel=nm_[:90], grid=[gx, gy], calls=len(v), median_us=round(ns / 1e3, 2), vgpr=v[0][1], agpr=v[0][2],
                       lds=v[0][3], scratch=v[0][4])
            tall = (("k_link_gemm_tn<%d>" % nt) in nm_ and gx == 256 * ((D + 63) // 64) and gy == (N + 2047) // 2048) or \
                   (("k_link_gemm_nn<%d>" % nt) in nm_ and gx == 256 * ((N + 63) // 64)) or \
                   ("k_link_" not in nm_ and len(v) >= reps)
            if tall and ns > 0:
                rec["product"] = "N x D x K = %d x %d x %d" % (N, D, K)
                rec["tflops"] = round(flops / ns / 1e3, 3)
                rec["of_mfma_rate"] = round(flops / ns / 1e3 / PEAK_TFLOPS, 4)
                rec["tbytes_s"] = round(byts / ns / 1e3, 3)
                rec["of_hbm"] = round(byts / ns / 1e3 / PEAK_TBS, 4)
            print(json.dumps(rec), flush=True)


def iters(names, secs, rounds):
    for name in names:
        d = shape(name)
        K, D = d["K"], d["D"]
        F = features(d["nu"], D).cpu().numpy()
        args = (d["M"], d["Mt"], d["T"], d["nu"], d["nm"])
        kw = {"plain": dict(), "features": dict(row_features=F, lambda_beta=5.0)}
        per = {"plain": [], "features": []}
        nsims = {}
        for mode in kw:                                      # size the windows
            eng = bpmf_amd.HipEngine(K)
            try:
                res = bpmf_amd.gibbs(eng, *args, nsims=8, burnin=2, Tt=d["Tt"], **kw[mode])
            finally:
                eng.close()
            nsims[mode] = max(10, int(secs / statistics.median(res["secs"][2:])))
        for r in range(rounds):
            for mode in (("plain", "features") if r % 2 == 0 else ("features", "plain")):
                eng = bpmf_amd.HipEngine(K)
                try:
                    res = bpmf_amd.gibbs(eng, *args, nsims=nsims[mode], burnin=2, Tt=d["Tt"], **kw[mode])
                finally:
                    eng.close()
                per[mode].append(1e3 * statistics.median(res["secs"][2:]))
        p, f = statistics.median(per["plain"]), statistics.median(per["features"])
        print(json.dumps(dict(mode="iter", shape=name, K=K, D=D, plain_unpipelined_ms=round(p, 4), features_ms=round(f, 4), added_ms=round(f - p, 4),
                              plain_spread_ms=round(max(per["plain"]) - min(per["plain"]), 4),
                              features_spread_ms=round(max(per["features"]) - min(per["features"]), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "work", "iter"))
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--secs", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.mode == "kernels":
        kernels(a.shapes or ["ml1m", "chembl"], a.reps)
    elif a.mode == "work":
        work(a.shapes[0], a.reps)
    else:
        iters(a.shapes or ["ml1m", "chembl"], a.secs, a.rounds)


if __name__ == "__main__":
    main()
