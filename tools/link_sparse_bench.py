"""Sparse side information (gibbs(..., row_features=<scipy.sparse>), kernels_link_sparse.h): what its kernels and its loop cost.

    python tools/link_sparse_bench.py kernels [ml1m chembl] [--reps 3]
        starts `rocprofv3 --kernel-trace --stats -- python tools/link_sparse_bench.py work SHAPE` as a child process of its own per
        shape and reads the kernel trace it leaves: per kernel and grid the median time, registers, LDS and scratch; for the two
        sparse products at n = K the gathered bytes per second, and the same for the kernels torch.sparse.mm launches for them in
        fp64 on the same CSR operands (the yardstick).
    python tools/link_sparse_bench.py work SHAPE [--reps 3]
        the work itself: binary user features with the skewed column distribution (ml1m: N = 6 040, D = 4 096, 32 per row, K = 32;
        chembl: N = 483 500, D = 131 072, 64 per row, K = 64), `reps` of each product alone, two iterations of the features loop,
        `reps` torch.sparse.mm of each product.
    python tools/link_sparse_bench.py iter [ml1m chembl] [--secs 2] [--rounds 3]
        per-iteration time of the features loop against the plain un-pipelined gibbs on the same matrix, interleaved windows; CG
        iterations per draw.

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
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bpmf_amd                                            # noqa: E402
from bpmf_amd import engine, synth                         # noqa: E402

SHAPES = dict(ml1m=dict(N=6040, D=4096, per_row=32, K=32), chembl=dict(N=483500, D=131072, per_row=64, K=64))


def skewed_bits(n, D, per_row, seed):
    """[n, D] binary CSR: column d is on with probability ~ 1 / (d + 1), scaled to per_row bits per row on average and capped at 1.
    Column counts are binomial; the rows of a column are drawn with replacement and duplicates dropped (a deficit of count^2 / 2n)."""
    rng = np.random.default_rng(seed)
    w = 1.0 / (np.arange(D) + 1.0)
    scale = per_row / w.sum()
    for _ in range(200):
        prob = np.minimum(1.0, scale * w)
        scale *= per_row / prob.sum()
    prob = np.minimum(1.0, scale * w)
    full = prob >= 1.0
    counts = np.where(full, n, rng.binomial(n, np.where(full, 0.0, prob)))
    cols = np.repeat(np.arange(D, dtype=np.int64), counts)
    rows = rng.integers(0, n, len(cols))
    start = np.concatenate([[0], np.cumsum(counts)])
    for d in np.nonzero(full)[0]:
        rows[start[d]:start[d + 1]] = np.arange(n)
    F = sp.coo_matrix((np.ones(len(cols)), (rows, cols)), shape=(n, D)).tocsr()
    F.sum_duplicates()
    F.data[:] = 1.0
    F.sort_indices()
    return F


def ratings(name):
    if name == "ml1m":
        M, Mt, T, Tt, nu, nm = synth.ml1m_shaped(seed=42)
    else:
        M, Mt, T, Tt, nu, nm = synth.ratings(483500, 5775, 1_023_952, seed=42, real_valued=True)
    return dict(M=M, Mt=Mt, T=T, Tt=Tt, nu=nu, nm=nm)


def work(name, reps):
    import torch
    s = SHAPES[name]
    d = ratings(name)
    K, D, nu, nm = s["K"], s["D"], d["nu"], d["nm"]
    F = skewed_bits(nu, D, s["per_row"], 7)
    rng = np.random.default_rng(1)
    V, X = rng.standard_normal((D, K)), rng.standard_normal((nu, K))
    for _ in range(reps):                                    # the products alone (the trace has their kernels at these grids)
        Y = engine.link_spmm_nn(F, V)
        Cc = engine.link_spmm_tn(F, X)
    eng = bpmf_amd.HipEngine(K)
    try:
        movies = eng.side_create(nm, nu, *d["M"], float(d["M"][2].mean()))
        users = eng.side_create(nu, nm, *d["Mt"], float(d["Mt"][2].mean()))
        t0 = time.perf_counter()
        eng.set_features(users, F, 5.0, 4)
        t_set = time.perf_counter() - t0
        ms, its = [], []
        for _ in range(2):
            t0 = time.perf_counter()
            eng.link_sample(movies, users, 2.0)
            eng.link_sample(users, movies, 2.0)
            ms.append((time.perf_counter() - t0) * 1e3)
            its.append(eng.link_cg_stats(users)["iters_last"])
    finally:
        eng.close()
    Fc = torch.sparse_csr_tensor(torch.from_numpy(F.indptr.astype(np.int64)), torch.from_numpy(F.indices.astype(np.int64)),
                                 torch.from_numpy(F.data), size=F.shape, dtype=torch.float64, device="cuda")
    Ft = F.T.tocsr()
    Ftc = torch.sparse_csr_tensor(torch.from_numpy(Ft.indptr.astype(np.int64)), torch.from_numpy(Ft.indices.astype(np.int64)),
                                  torch.from_numpy(Ft.data), size=Ft.shape, dtype=torch.float64, device="cuda")
    Vt, Xt = torch.from_numpy(V).cuda(), torch.from_numpy(X).cuda()
    for _ in range(reps):
        Yt = torch.sparse.mm(Fc, Vt)
        Ct = torch.sparse.mm(Ftc, Xt)
    torch.cuda.synchronize()
    err = max(float(np.abs(Yt.cpu().numpy() - Y).max()), float(np.abs(Ct.cpu().numpy() - Cc).max()))
    print(json.dumps(dict(mode="work", shape=name, N=nu, D=D, K=K, nnz=int(F.nnz), longest_column=int(np.diff(Ft.indptr).max()),
                          set_features_s=round(t_set, 3), iteration_ms=[round(x, 3) for x in ms], cg_iters=its,
                          max_abs_diff_to_torch=err)), flush=True)


def kernels(names, reps):
    for name in names:
        s = SHAPES[name]
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "link", "--", sys.executable,
                   os.path.abspath(__file__), "work", name, "--reps", str(reps)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            nnz = None
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    print(line, flush=True)
                    nnz = json.loads(line).get("nnz", nnz)
            if r.returncode != 0:
                print(json.dumps(dict(mode="kernels", shape=name, error=r.stderr[-600:])), flush=True)
                continue
            rows = []
            for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
                with open(path) as f:
                    rows += list(csv.DictReader(f))
        groups = {}
        for row in rows:
            nm_ = row.get("Kernel_Name", "")
            ours = any(t in nm_ for t in ("k_sp_", "k_cg_", "k_link_"))
            theirs = any(t in nm_.lower() for t in ("csrmm", "spmm", "sparse", "csr"))
            if not (ours or theirs):
                continue
            key = (nm_, int(row.get("Grid_Size_X", 0) or 0))
            groups.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), row.get("VGPR_Count"), row.get("Accum_VGPR_Count"),
                                               row.get("LDS_Block_Size"), row.get("Scratch_Size")))
        for (nm_, gx), v in sorted(groups.items()):
            ns = statistics.median(x[0] for x in v)
            rec = dict(mode="kernels", shape=name, kernel=nm_[:100], grid=gx, calls=len(v), median_us=round(ns / 1e3, 2), total_ms=round(sum(x[0] for x in v) / 1e6, 3),
                       vgpr=v[0][1], agpr=v[0][2], lds=v[0][3], scratch=v[0][4])
            if nnz and ("k_sp_rows" in nm_ or "k_sp_chunks" in nm_ or not any(t in nm_ for t in ("k_sp_", "k_cg_", "k_link_"))):
                rec["gathered_tbytes_s_if_whole_product"] = round(nnz * 8.0 * s["K"] / ns / 1e3, 3)     # nnz rows of K doubles
            print(json.dumps(rec), flush=True)


def iters(names, secs, rounds):
    for name in names:
        s = SHAPES[name]
        d = ratings(name)
        K = s["K"]
        F = skewed_bits(d["nu"], s["D"], s["per_row"], 7)
        args = (d["M"], d["Mt"], d["T"], d["nu"], d["nm"])
        kw = {"plain": dict(), "features": dict(row_features=F, lambda_beta=5.0)}
        per = {"plain": [], "features": []}
        nsims, cg = {}, []
        for mode in kw:                                      # size the windows
            eng = bpmf_amd.HipEngine(K)
            try:
                res = bpmf_amd.gibbs(eng, *args, nsims=6, burnin=2, Tt=d["Tt"], **kw[mode])
            finally:
                eng.close()
            nsims[mode] = max(6, int(secs / statistics.median(res["secs"][2:])))
        for r in range(rounds):
            for mode in (("plain", "features") if r % 2 == 0 else ("features", "plain")):
                eng = bpmf_amd.HipEngine(K)
                try:
                    res = bpmf_amd.gibbs(eng, *args, nsims=nsims[mode], burnin=2, Tt=d["Tt"], **kw[mode])
                finally:
                    eng.close()
                per[mode].append(1e3 * statistics.median(res["secs"][2:]))
                if mode == "features":
                    cg += [iu for _, iu in res["link_cg_iters"][2:]]
        p, f = statistics.median(per["plain"]), statistics.median(per["features"])
        print(json.dumps(dict(mode="iter", shape=name, K=K, D=s["D"], nnz=int(F.nnz), plain_unpipelined_ms=round(p, 4), features_ms=round(f, 4),
                              added_ms=round(f - p, 4), plain_spread_ms=round(max(per["plain"]) - min(per["plain"]), 4),
                              features_spread_ms=round(max(per["features"]) - min(per["features"]), 4),
                              cg_iters_per_draw=[min(cg), statistics.median(cg), max(cg)],
                              added_ms_per_cg_iteration=round((f - p) / statistics.median(cg), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "work", "iter"))
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=3)
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
