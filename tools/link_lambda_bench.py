"""A sampled lambda_beta (gibbs(..., lambda_beta_prior=), kernels_link_chol.h): what the device factorisation and its loop cost.

    python tools/link_lambda_bench.py kernels [ml1m chembl] [--reps 5]
        starts `rocprofv3 --kernel-trace --stats -- python tools/link_lambda_bench.py work SHAPE` as a child process of its own per
        shape and reads the kernel trace it leaves: per k_chol_* kernel the launches per draw, the median and the summed time per
        draw, registers and LDS; the factorisation (form + diag + panel + trail) and the two solves (pack + solve + unpack) as
        sums per draw; and the kernels torch.linalg.cholesky + torch.cholesky_solve launch in fp64 for the same G and the same
        number of right-hand sides (the yardstick).
    python tools/link_lambda_bench.py work SHAPE [--reps 5]
        the work itself: user features on the shape (ml1m: N = 6 040, D = 64, K = 32; chembl: N = 483 500, D = 1024, K = 64), `reps`
        iterations of the features loop with the default prior, `reps` factorisations and solves in torch.
    python tools/link_lambda_bench.py iter [ml1m chembl] [--secs 2] [--rounds 3]
        per-iteration time of the features loop with a fixed lambda_beta (the parent commit's loop) against the loop with the prior,
        interleaved windows.

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpmf_amd                                            # noqa: E402
from link_bench import shape, features                     # noqa: E402

PRIOR = (5e-4, 5e-4)
FACTOR = ("k_chol_form", "k_chol_diag", "k_chol_panel", "k_chol_trail")
SOLVE = ("k_chol_pack", "k_chol_solve", "k_chol_unpack")


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
        eng.set_features(users, F, 5.0, 4)
        t0 = time.perf_counter()
        eng.link_lambda_prior(users, *PRIOR)
        t_enter = time.perf_counter() - t0
        ms, lam = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.link_sample(movies, users, 2.0)
            eng.link_sample(users, movies, 2.0)
            ms.append((time.perf_counter() - t0) * 1e3)
            lam.append(eng.link_lambda_get(users)[0])
    finally:
        eng.close()
    G = Ft.T @ Ft + 5.0 * torch.eye(D, dtype=torch.float64, device="cuda")
    P = torch.randn((D, K), dtype=torch.float64, device="cuda")
    for _ in range(reps):
        L = torch.linalg.cholesky(G)
        X = torch.cholesky_solve(P, L)
    torch.cuda.synchronize()
    print(json.dumps(dict(mode="work", shape=name, N=nu, D=D, K=K, reps=reps, enter_device_factor_mode_s=round(t_enter, 3),
                          iteration_ms_median=round(statistics.median(ms), 3), lambda_beta=lam, check=float(X[0, 0]))), flush=True)


def kernels(names, reps):
    for name in names:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "lambda", "--", sys.executable,
                   os.path.abspath(__file__), "work", name, "--reps", str(reps)]
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
        ours, other = {}, {}
        for row in rows:
            nm_ = row.get("Kernel_Name", "")
            ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            base = next((k for k in FACTOR + SOLVE if k in nm_), None)
            if base:
                ours.setdefault(base, []).append((ns, row.get("VGPR_Count"), row.get("Accum_VGPR_Count"), row.get("LDS_Block_Size"), row.get("Scratch_Size")))
            elif any(t in nm_ for t in ("potrf", "trsm", "Cijk", "gemm", "Gemm", "syrk", "herk", "potf2", "trtri")):
                other.setdefault(nm_[:90], []).append(ns)
        for k, v in ours.items():
            print(json.dumps(dict(mode="kernels", shape=name, kernel=k, launches_per_draw=round(len(v) / reps, 2), median_us=round(statistics.median(x[0] for x in v) / 1e3, 2),
                                  sum_per_draw_us=round(sum(x[0] for x in v) / reps / 1e3, 1), vgpr=v[0][1], agpr=v[0][2], lds=v[0][3], scratch=v[0][4])), flush=True)
        for label, group in (("factor", FACTOR), ("solves", SOLVE)):
            tot = sum(x[0] for k in group for x in ours.get(k, []))
            print(json.dumps(dict(mode="kernels", shape=name, part=label, launches_per_draw=round(sum(len(ours.get(k, [])) for k in group) / reps, 2),
                                  sum_per_draw_us=round(tot / reps / 1e3, 1))), flush=True)
        # the yardstick: every BLAS / solver kernel of the trace (the loop itself launches none); the products of work()'s F^T F are in it once
        for k, v in sorted(other.items()):
            print(json.dumps(dict(mode="kernels", shape=name, yardstick_kernel=k, calls=len(v), median_us=round(statistics.median(v) / 1e3, 2),
                                  sum_per_rep_us=round(sum(v) / reps / 1e3, 1))), flush=True)


def iters(names, secs, rounds):
    for name in names:
        d = shape(name)
        K, D = d["K"], d["D"]
        F = features(d["nu"], D).cpu().numpy()
        args = (d["M"], d["Mt"], d["T"], d["nu"], d["nm"])
        kw = {"fixed": dict(row_features=F, lambda_beta=5.0), "sampled": dict(row_features=F, lambda_beta=5.0, lambda_beta_prior=PRIOR)}
        per = {m: [] for m in kw}
        nsims = {}
        for mode in kw:                                      # size the windows
            eng = bpmf_amd.HipEngine(K)
            try:
                res = bpmf_amd.gibbs(eng, *args, nsims=8, burnin=2, Tt=d["Tt"], **kw[mode])
            finally:
                eng.close()
            nsims[mode] = max(10, int(secs / statistics.median(res["secs"][2:])))
        for r in range(rounds):
            for mode in (("fixed", "sampled") if r % 2 == 0 else ("sampled", "fixed")):
                eng = bpmf_amd.HipEngine(K)
                try:
                    res = bpmf_amd.gibbs(eng, *args, nsims=nsims[mode], burnin=2, Tt=d["Tt"], **kw[mode])
                finally:
                    eng.close()
                per[mode].append(1e3 * statistics.median(res["secs"][2:]))
        p, f = statistics.median(per["fixed"]), statistics.median(per["sampled"])
        print(json.dumps(dict(mode="iter", shape=name, K=K, D=D, fixed_lambda_ms=round(p, 4), sampled_lambda_ms=round(f, 4), added_ms=round(f - p, 4),
                              fixed_spread_ms=round(max(per["fixed"]) - min(per["fixed"]), 4),
                              sampled_spread_ms=round(max(per["sampled"]) - min(per["sampled"]), 4))), flush=True)


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
