#!/usr/bin/env python
"""bench.py -- user+item column samples/sec per Gibbs iteration on MI355X.

One "step" = one full Gibbs iteration of the reference's main loop
(c++/bpmf.cpp:182-195): movies.sample(users); users.sample(movies);
movies.predict(users) -- both host hyper-parameter draws, the device->host
reductions and the RMSE evaluation are inside the timed region, exactly what the
reference's `items/sec` covers.  value = (N_users + N_movies) * steps / seconds.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload ml1m|ml1m_k64|chembl|ml1m_k128|ml1m_k128_f64|ml1m_k100]

Workloads (BASELINE.json configs; synthetic stand-ins, the reference ships only ML-100K):
  ml1m        configs[1]  6040 x 3706, 1 000 209 ratings (90/10 split), K = 32 fp64   <- the headline / default
  ml1m_k64                the same matrix, K = 64 fp64
  chembl      configs[2]  483 500 x 5 775, 1 023 952 real-valued activities, K = 64 fp64
  ml1m_k128   configs[4]  the ML-1M shape, K = 128, fp32 factors (mixed-precision path; an explicit opt-in everywhere)
  ml1m_k128_f64           the ML-1M shape, K = 128 in the reference's fp64 (what `bpmf -d 128` / bpmf-128 of ci/multilatent.sh:5 runs)
  ml1m_k100               the ML-1M shape, K = 100 fp64 (BASELINE.md's "industrial" num_latent) on the K = 128 kernels, 28 padded dimensions
N > 1: one rank per GPU, RCCL inside the library.  Under a launcher (WORLD_SIZE / RANK / LOCAL_RANK set, e.g.
`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`) this process is one of the N ranks; without one,
`bench.py --gpus N` starts the N ranks itself (the job of `mpirun -np N` for the reference, c++/mpi_common.h:11-50) and
fails if fewer than N devices are visible -- it never reports a 1-rank run as N GPUs.  The line carries `rccl_nranks`,
the rank count the communication library reports (ncclCommCount).  Weak scaling of the
selected workload (N times the users and ratings) AND, next to it, the north star's strong-scaling
experiment as the sub-record `strong_10Mx1M` (configs[3]: the SAME device-generated 10M x 1M x 200
matrix at every N, N = 1 included; --no-strong skips it).

Timing: W warm-up steps and P = 256 more untimed steps (`--prewarm-steps`: a fresh chain needs ~250 steps
to reach its steady rate), then ONE block of exactly K timed steps bracketed by barrier + synchronize
(`ms_per_step` = block / K).  Same arguments, same inputs and the same W + P + K steps on the timed chain,
so what it leaves behind is the same from run to run.  `--prewarm-ms T` adds untimed steps until T ms have
gone by (speed-dependent), `--repeats R` times R blocks of K steps (0: as many as fill `--window-s`) and
reports the MEDIAN block (min / max beside it).

A plain run prints ONE JSON line (rank 0): the headline, `roofline` (the dominant kernel = the
per-column sampler, timed with HIP events on its own stream inside the library during the timed steps)
and `handover`.  `--dump-outputs DIR` writes what the timed path computed in its last step as
DIR/<name>.npy (float64).  `--full` adds what takes runs of its own: `parity` (a chain through the same
pipeline against the oracle's), `strong_10Mx1M`, `bpmf_exe`, `configs` (the other single-GPU
configurations, one child run each) and `cpu_baseline` (oracle/cpu_baseline.py: the oracle's OpenMP
build on the host cores, in a process of its own).
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# peaks (/opt/skills/guides/MI355X_MICROARCH.md; fp64 from the MI355X data sheet: vector = matrix = 78.6 TF)
HBM_PEAK_GBS = 8000.0
FP64_PEAK_TFLOPS = 78.6
FP32_PEAK_TFLOPS = 157.3
LDS_PER_CU = 160 * 1024

WORKLOADS = {
    #            K    dtype  (two unused fields: the LDS figures come from the library, bpmf_hip_side_kernel_resources)
    # (the kernel names of the roofline object come from the library: bpmf_hip_side_kernel_name)
    "ml1m":      (32, "f64", None, None),
    "ml1m_k64":  (64, "f64", None, None),
    "chembl":    (64, "f64", None, None),
    "ml1m_k128": (128, "f32", None, None),
    "ml1m_k128_f64": (128, "f64", None, None),
    "ml1m_k100": (100, "f64", None, None),
}


def algorithmic_bytes(nnz, ncols, K, s=8):
    """SURVEY 8(d), one half-iteration (= one launch of the sampler): per rating a row index,
    a value and one K-vector; per column the K-vector written back + its column pointer."""
    return nnz * (4 + s + K * s) + ncols * (K * s + 8)


def algorithmic_flops(nnz, ncols, K):
    return nnz * (K * (K + 1) + 2 * K) + ncols * (K ** 3 / 3.0 + 4 * K * K + 3 * K)


def executed_flops(info, nnz, ncols, K):
    """Flops one sampler launch of a side EXECUTES, given its schedule (bpmf_hip_side_schedule_info).  Columns in the
    regular forms: the algorithmic count.  Columns in the product form (k_sample_pf, K = 64, <= 16 ratings) are never
    factorised -- that is the point of the form -- so they are charged what the kernel does per column with n ratings:
    one dense K x K matrix-vector product on the MFMA (2 K^2), n(n-1)/2 + 2n solves with a rank-one factor (~11 K flops
    each: one product, a 6-step wave scan, the combine), n rank-one factors (~30 K: scan, two rsqrt + Newton, ratios),
    3 K per rating for the right-hand side, ~30 K for the normal draw; plus k_pf_prepare: 2 K^2 per ROW of the side."""
    npf = info["pf_le3"] + info["pf_4to6"] + info["pf_7to16"]
    if npf == 0:
        return algorithmic_flops(nnz, ncols, K)
    n1, n2 = info["pf_ratings"], info["pf_ratings_sq"]
    pf = npf * (2.0 * K * K + 30.0 * K) + K * (11.0 * ((n2 - n1) / 2.0 + 2.0 * n1) + 33.0 * n1)
    return pf + algorithmic_flops(nnz - n1, ncols - npf, K)


def kernel_source_sha():
    """sha256 (16 hex digits) over the sources the device code is built from: a PMC profile names the sha it was taken
    with, and figures of a profile of OTHER code are reported as stale, not as this run's."""
    import hashlib
    h = hashlib.sha256()
    # (everything device code is compiled from or launched with: the kernel headers, the per-K translation units --
    # launch bounds and template instantiations live there -- and launch_impl.h, which holds the grids and launch shapes;
    # capi_*.hip / hyper.cpp / io.cpp are host-only and do not change what a counter sees)
    for f in sorted(glob.glob(os.path.join(ROOT, "bpmf_amd", "csrc", "kernels*.h")) +
                    glob.glob(os.path.join(ROOT, "bpmf_amd", "csrc", "k*.hip")) +
                    [os.path.join(ROOT, "bpmf_amd", "csrc", n) for n in ("philox.h", "args.h", "launch_impl.h", "launch.h")]):
        h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def profiled(workload):
    """Per-launch PMC figures of the sampler from the committed rocprofv3 passes of this same command
    (profiles/r*_pmc_<workload>.txt, newest round; separate --pmc passes): HBM-side bytes and the LDS
    bank-conflict rate.  Not a live measurement: counters need rocprofv3.  HBM correction as
    MI355X_MICROARCH.md prescribes, calibrated on this kernel's own access pattern
    (tools/probes/fetch_calib.hip: 1 GiB read once with the sampler's 16-byte gathers reports
    0.50 GiB, 1 GiB written reports 1.00 GiB): traffic = 2 * FETCH_SIZE(KB) + WRITE_SIZE(KB)."""
    names = {"ml1m": "sampler"}
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_%s.txt" % workload)) +
                   glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_%s.txt" % names.get(workload, "-"))))
    if not files:
        return None, None, None, None
    vals = {}
    sha = None
    for line in open(files[-1]):
        if line.startswith("# kernel-source-sha:"):
            sha = line.split(":", 1)[1].strip()
        f = line.replace("avg=", "avg= ").split()
        if len(f) >= 4 and f[2] == "avg=" and "[" not in f[0]:         # (lines `pmc[grid=N] ...` are per launch shape: profiled_by_grid)
            try:
                vals[f[1]] = float(f[3])
            except ValueError:
                pass
    traffic = (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0 if "FETCH_SIZE" in vals and "WRITE_SIZE" in vals else None
    conflict = None
    if vals.get("SQ_LDS_IDX_ACTIVE") or vals.get("SQ_ACTIVE_INST_LDS"):
        conflict = vals.get("SQ_LDS_BANK_CONFLICT", 0.0) / (vals.get("SQ_LDS_IDX_ACTIVE") or vals.get("SQ_ACTIVE_INST_LDS"))
    return traffic, conflict, os.path.basename(files[-1]), sha


# cycles one SIMD is busy per MFMA of the shape that dominates a workload's sampler (tools/probes/mfma_probe.hip, mfma44_probe.hip,
# profiles/r05_mfma_shapes_probe.txt): v_mfma_f64_4x4x4_4b 18, v_mfma_f64_16x16x4 104, v_mfma_f32_16x16x4 38
MFMA_CYCLES = {"ml1m": 18.0, "ml1m_k64": 18.0, "chembl": 18.0, "ml1m_k128": 38.0, "ml1m_k128_f64": 104.0, "ml1m_k100": 104.0}
VALU_CYCLES = 4.2          # measured issue cost of a wave64 VALU instruction with >= 2 waves per SIMD (profiles/r04_valu_rate_probe.txt: 4.2 - 5)
CLOCK_GHZ = 2.4            # MI355X_MICROARCH.md: max engine clock (the sustained clock under load is lower: the bound is a floor)


def issue_bound_by_kernel(workload, num_cu=256):
    """The ChEMBL shape runs six sampler kernels per iteration: the same issue-time estimate per KERNEL, from the committed per-kernel
    counters (profiles/r*_pmc_by_kernel_<workload>.txt, tools/pmc_by_kernel.py) and the committed kernel trace's average durations
    (profiles/r*_kernel_trace_summary_<workload>.txt).  Both files are the builder's (rocprofv3 on the GPU box); `current` says
    whether they were taken with this build's kernel sources."""
    import re
    pm = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_by_kernel_%s.txt" % workload)))
    tr = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_kernel_trace_summary_%s.txt" % workload)))
    if not pm or not tr:
        return None
    sha, cur, counters = None, None, {}
    for line in open(pm[-1]):
        if line.startswith("# kernel-source-sha:"):
            sha = line.split(":", 1)[1].strip()
        elif line.startswith("    "):
            f = line.replace("avg=", "avg= ").split()
            if cur and len(f) >= 3 and f[1] == "avg=":
                counters.setdefault(cur, {})[f[0]] = float(f[2])
        elif not line.startswith("#"):
            m = re.search(r"(k_\w+<[^>]*>|k_\w+)", line)
            cur = m.group(1).replace(" ", "") if m else None
    dur = {}
    for line in open(tr[-1]):
        m = re.search(r"(k_\w+<[^>]*>|k_\w+)", line)
        f = line.split()
        if m and len(f) >= 5:
            try:
                dur[m.group(1).replace(" ", "")] = float(f[-4]) * 1e-6          # avg_us column
            except ValueError:
                pass
    out = {}
    for k, v in counters.items():
        if not k.startswith("k_sample") and not k.startswith("k_pf_prepare"):
            continue
        if "SQ_INSTS_VALU" not in v or "SQ_INSTS_MFMA" not in v or k not in dur:
            continue
        mfma = v["SQ_INSTS_MFMA"]; valu = max(0.0, v["SQ_INSTS_VALU"] - mfma)
        issue_s = (valu * VALU_CYCLES + mfma * 18.0) / (num_cu * 4) / (CLOCK_GHZ * 1e9)
        out[k] = {"valu_insts_per_launch": valu, "mfma_insts_per_launch": mfma, "issue_us": issue_s * 1e6, "launch_us": dur[k] * 1e6,
                  "frac_of_launch": issue_s / dur[k]}
    if not out:
        return None
    return {"per_kernel": out, "cycles_per_valu": VALU_CYCLES, "cycles_per_mfma": 18.0, "clock_ghz": CLOCK_GHZ, "simds": num_cu * 4,
            "source": [os.path.basename(pm[-1]), os.path.basename(tr[-1])], "current": bool(sha == kernel_source_sha()),
            "note": "per kernel: instruction-issue time of its own stream at the max clock / its average duration in the committed trace (the "
                    "targets-side launch shares the chip with the compounds side's statistics pass and the evaluation: its duration is not its own)"}


def issue_bound(workload, launch_s, num_cu=256):
    """Why the sampler is where it is against the flop peak, carried with the number: the time its instruction
    stream needs to ISSUE -- (VALU instructions x measured cycles + MFMA instructions x the shape's cycles) / SIMDs / clock --
    from the per-launch counters of the committed PMC pass, over the measured launch time.  SQ_INSTS_VALU counts the MFMAs too
    (checked against the static ISA of the Gram loop: 86 VALU + 144 MFMA per 64 ratings), so they are taken out of it; f64
    MFMA and VALU issue add on a SIMD.  Counters of a profile of OTHER kernel sources are history: null."""
    if workload == "chembl":
        return issue_bound_by_kernel(workload, num_cu)                # (six sampler kernels per iteration: one record per kernel)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_%s.txt" % workload)))
    if not files:
        return None
    vals, sha = {}, None
    for line in open(files[-1]):
        if line.startswith("# kernel-source-sha:"):
            sha = line.split(":", 1)[1].strip()
        f = line.replace("avg=", "avg= ").split()
        if len(f) >= 4 and f[2] == "avg=" and "[" not in f[0]:
            try:
                vals[f[1]] = float(f[3])
            except ValueError:
                pass
    if "SQ_INSTS_VALU" not in vals or "SQ_INSTS_MFMA" not in vals or launch_s <= 0:
        return None
    mfma = vals["SQ_INSTS_MFMA"]; valu = max(0.0, vals["SQ_INSTS_VALU"] - mfma)
    cyc = valu * VALU_CYCLES + mfma * MFMA_CYCLES.get(workload, 18.0)
    issue_s = cyc / (num_cu * 4) / (CLOCK_GHZ * 1e9)
    return {"valu_insts_per_launch": valu, "mfma_insts_per_launch": mfma, "cycles_per_valu": VALU_CYCLES,
            "cycles_per_mfma": MFMA_CYCLES.get(workload, 18.0), "simds": num_cu * 4, "clock_ghz": CLOCK_GHZ,
            "issue_us": issue_s * 1e6, "launch_us": launch_s * 1e6, "frac_of_launch": issue_s / launch_s,
            "source": os.path.basename(files[-1]), "current": bool(sha == kernel_source_sha()),
            "note": "instruction-issue time of the sampler's own stream at the max clock / measured launch time: the part of the launch that is "
                    "not waiting; the rest is latency, tails and the clock below 2.4 GHz.  What lifts roofline.frac is fewer instructions per column"}


def profiled_by_grid(workload):
    """TCC_HIT / TCC_MISS / FETCH / WRITE per launch SHAPE from the committed PMC file (lines `pmc[grid=N] COUNTER avg=..`, written by
    tools/pmc_dump.py ... bygrid): the smaller grid of the 10M x 1M record is the items side (1M columns), the larger the users side."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_%s.txt" % workload)))
    if not files:
        return None
    by = {}
    for line in open(files[-1]):
        f = line.replace("avg=", "avg= ").split()
        if len(f) >= 4 and f[0].startswith("pmc[grid=") and f[2] == "avg=":
            try:
                by.setdefault(int(f[0][9:-1]), {})[f[1]] = float(f[3])
            except ValueError:
                pass
    if len(by) != 2:
        return None
    out = {}
    for name, g in zip(("items_side", "users_side"), sorted(by)):
        v = by[g]
        hit, miss = v.get("TCC_HIT_sum"), v.get("TCC_MISS_sum")
        out[name] = {"grid": g, "TCC_HIT_sum": hit, "TCC_MISS_sum": miss, "l2_hit_rate": (hit / (hit + miss)) if hit is not None and miss else None,
                     "l2_memory_side_bytes": ((2.0 * v["FETCH_SIZE"] + v["WRITE_SIZE"]) * 1024.0) if "FETCH_SIZE" in v and "WRITE_SIZE" in v else None}
    return out


PARITY_TOL = {"f64": {"rmse": 1e-6, "items_rel": 1e-6, "norm_rel": 1e-7}, "f32": {"rmse": 1e-3, "items_rel": 2e-3, "norm_rel": 1e-3}}


def parity_record(gpu, ref, dtype, nsims, burnin, chain_info):
    """bench.py's `parity` object: the chain the timed pipeline produced against the oracle's chain on the same matrix
    and seeds ("test RMSE vs reference", the metric's second half; north star: RMSE within 1e-3).  gpu / ref: dicts with
    rmse, rmse_avg, norm_u, norm_m (per iteration), final_rmse_avg, num_predict, U, V."""
    tol = PARITY_TOL[dtype]
    g = {k: np.asarray(gpu[k], np.float64) for k in ("rmse", "rmse_avg", "norm_u", "norm_m")}
    r = {k: np.asarray(ref[k], np.float64) for k in ("rmse", "rmse_avg", "norm_u", "norm_m")}
    d_rmse = float(np.abs(g["rmse"] - r["rmse"]).max())
    d_avg = float(np.abs(g["rmse_avg"] - r["rmse_avg"]).max())
    d_final = abs(float(gpu["final_rmse_avg"]) - float(ref["final_rmse_avg"]))
    d_norm = float(max(np.abs(g["norm_u"] / r["norm_u"] - 1).max(), np.abs(g["norm_m"] / r["norm_m"] - 1).max()))
    d_u = float(np.abs(gpu["U"] - ref["U"]).max() / np.abs(ref["U"]).max())
    d_v = float(np.abs(gpu["V"] - ref["V"]).max() / np.abs(ref["V"]).max())
    ok = (d_rmse < tol["rmse"] and d_avg < tol["rmse"] and d_final < tol["rmse"] and d_norm < tol["norm_rel"]
          and d_u < tol["items_rel"] and d_v < tol["items_rel"] and int(gpu["num_predict"]) == int(ref["num_predict"]))
    out = {"iterations": nsims, "burnin": burnin,
           "path": "bpmf_amd.gibbs(pipelined=True) on the bench's own engine: the software-pipelined stateful loop the timed region runs "
                   "(default schedule, fused launches, riders, twin evaluation), from the reference's start (zero factors, iter = -1)",
           "against": "oracle/bpmf_oracle.c chain (CPU restatement of c++/bpmf.cpp:180-253 + c++/sample.cpp), same matrix, identical seeds",
           "rmse_gpu": float(g["rmse"][-1]), "rmse_cpu": float(r["rmse"][-1]),
           "final_avg_rmse_gpu": float(gpu["final_rmse_avg"]), "final_avg_rmse_cpu": float(ref["final_rmse_avg"]),
           "d_rmse_max": d_rmse, "d_rmse_avg_max": d_avg, "d_final_avg_rmse": d_final, "d_norm_rel": d_norm,
           "d_items_rel": {"U": d_u, "V": d_v}, "tolerance": dict(tol, north_star_rmse=1e-3), "ok": bool(ok),
           "oracle_pinned": os.path.exists(os.path.join(ROOT, "oracle", "_ref", "PINNED"))}
    out.update(chain_info or {})
    return out


def cpu_baseline(M, Mt, T, Tt, K, nusers, nmovies, budget_s=12.0, parity=None, parity_only=False):
    """oracle/cpu_baseline.py in a process of its own (placement: one thread per physical core, spread).
    parity = (nsims, burnin): the child also runs the oracle's chain of that length and this function returns its
    traces + factors under the key "parity_ref" (popped by the caller)."""
    fd, path = tempfile.mkstemp(suffix=".npz", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.close(fd)
    ppath = path[:-4] + "_parity.npz"
    try:
        arrs = {}
        for name, m in (("M", M), ("Mt", Mt), ("T", T), ("Tt", Tt)):
            for i in range(3):
                arrs["%s%d" % (name, i)] = m[i]
        np.savez(path, shape=np.array([nusers, nmovies]), **arrs)
        env = dict(os.environ)
        env.update({"OMP_PLACES": "cores", "OMP_PROC_BIND": "spread", "OMP_WAIT_POLICY": "active"})
        env.pop("OMP_NUM_THREADS", None)
        try:
            usable = len(os.sched_getaffinity(0))
        except AttributeError:
            usable = os.cpu_count() or 1
        cmd = [sys.executable, os.path.join(ROOT, "oracle", "cpu_baseline.py"), "--matrix", path, "--K", str(K),
               "--budget", str(budget_s), "--usable", str(usable)]
        if parity:
            cmd += ["--parity-nsims", str(parity[0]), "--parity-burnin", str(parity[1]), "--parity-out", ppath]
        if parity_only:
            cmd += ["--parity-only"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not line:
            raise RuntimeError("cpu_baseline.py rc=%d: %s" % (r.returncode, (r.stderr or r.stdout)[-400:]))
        rec = json.loads(line[-1])
        if parity and os.path.exists(ppath):
            z = np.load(ppath)
            rec["parity_ref"] = {"rmse": z["rmse"], "rmse_avg": z["rmse_avg"], "norm_u": z["norm_u"], "norm_m": z["norm_m"],
                                 "final_rmse_avg": float(z["final"][0]), "num_predict": int(z["final"][1]), "U": z["U"], "V": z["V"]}
        return rec
    finally:
        for f in (path, ppath):
            try:
                os.unlink(f)
            except OSError:
                pass


def timed_blocks(step_block, fence, steps, dist_max, min_blocks=5, max_blocks=4000, budget_s=20.0, window_s=2.5):
    """R blocks of exactly `steps` steps; returns the block times (max over ranks each).  Blocks are repeated until the
    TIMED time (the sum of the blocks, fences excluded) reaches `window_s`: at 0.1 ms per step a handful of 20-step blocks is
    50 ms of GPU work in a 20 s command, which an outside observer sampling the device's busy counter cannot see (VERDICT
    r5 "weak" 7); 2.5 s of back-to-back iterations can be seen.  Bounded by `max_blocks` and by `budget_s` of wall time."""
    times = []
    t_all = time.perf_counter()
    while True:
        fence()
        t0 = time.perf_counter()
        step_block(steps)
        fence()
        times.append(dist_max(time.perf_counter() - t0))
        done = (len(times) >= max_blocks or
                (len(times) >= min_blocks and (sum(times) >= window_s or time.perf_counter() - t_all > budget_s)))
        if dist_max(1.0 if done else 0.0) > 0.5:          # (every rank takes the same decision)
            return times


DUMP_BUDGET_BYTES = 60 * 2 ** 20


def dump_outputs(d, arrays, seed=0):
    """--dump-outputs DIR: every array as DIR/<name>.npy in float64, DUMP_BUDGET_BYTES in all.  An array above its equal share of
    the budget is stored as a fixed, seeded sample of its rows (ascending; the same rows for the same shape), so that two builds
    run with the same arguments can be compared output for output.  Returns {name: [shape written, rows sampled or None]}."""
    os.makedirs(d, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(1, len(arrays))
    out = {}
    for name, a in arrays.items():
        a = np.asarray(a, np.float64)
        sampled = None
        if a.nbytes > share and a.shape[0] > 0:
            n = max(1, share // (a.nbytes // a.shape[0]))
            rows = np.sort(np.random.default_rng(seed).choice(a.shape[0], size=n, replace=False))
            a, sampled = a[rows], int(n)
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a))
        out[name] = [list(a.shape), sampled]
    return out


METRIC = "user+item column samples/sec per Gibbs iter; test RMSE vs reference"


def error_line(msg, **extra):
    """The line of a run that could not be measured: same keys, value null, the reason under "error" (never silence)."""
    out = {"metric": METRIC, "value": None, "unit": "samples/s", "n_gpus": int(os.environ.get("WORLD_SIZE", "1")), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "data": "synthetic", "error": str(msg)[:1500]}
    out.update(extra)
    return json.dumps(out)


class Watchdog:
    """Wall-clock bound on every stage of the run (first contact with N real GPUs must not be able to hang): a daemon
    thread; when the stage in progress outlives its limit, rank 0 prints an error line and EVERY rank ends at once
    (os._exit: a rank stuck inside a collective cannot be unwound) -- the launcher then reaps the others.  The reference
    ends a job whose collective fails (c++/mpi_common.h:16 MPI_ERRORS_ARE_FATAL, c++/bpmf_gaspi.h:26-64 SUCCESS_OR_DIE);
    this is the same for a collective that never returns.  BPMF_BENCH_WATCHDOG_S: default limit per stage (120 s)."""

    def __init__(self, rank, extra=None):
        import threading
        self.rank, self.extra = rank, (extra if extra is not None else {})
        self.default = float(os.environ.get("BPMF_BENCH_WATCHDOG_S", "120"))
        # (start-up: the first `import torch` on a fresh box pages the image in -- minutes, not a hang)
        self.name, self.deadline, self.t0 = "start-up", time.time() + max(self.default, 900.0), time.time()
        self.lock = threading.Lock()
        self.done = False
        threading.Thread(target=self._run, daemon=True).start()

    def stage(self, name, limit=None):
        with self.lock:
            self.name, self.t0 = name, time.time()
            self.deadline = self.t0 + (limit if limit is not None else self.default)

    def stop(self):
        self.done = True

    def _run(self):
        while not self.done:
            time.sleep(0.25)
            with self.lock:
                late, name, dt = time.time() > self.deadline, self.name, time.time() - self.t0
            if late and not self.done:
                msg = "watchdog: stage '%s' did not finish within %.0f s on rank %d (a rank stalled or died, or a collective never returned)" % (name, dt, self.rank)
                sys.stderr.write("bench.py: " + msg + "\n"); sys.stderr.flush()
                if self.rank == 0:
                    sys.stdout.write(error_line(msg, stage=name, **self.extra) + "\n"); sys.stdout.flush()
                os._exit(3)


# The exchange configurations a sharded run may use, most aggressive first.  `env`: what the run itself is
# given; `preflight`: what the 4-iteration trial adds so that its small matrix takes the same code path (parts are automatic
# only above 64 MB of fresh columns per half-iteration).
LADDER = [
    {"name": "mesh+parts+2comms", "env": {}, "preflight": {"BPMF_HIP_OVERLAP": "4"}},
    {"name": "mesh+1comm", "env": {"BPMF_HIP_COMM_STREAMS": "1", "BPMF_HIP_OVERLAP": "1"}, "preflight": {}},
    {"name": "bcast+1comm", "env": {"BPMF_HIP_EXCHANGE": "bcast", "BPMF_HIP_COMM_STREAMS": "1", "BPMF_HIP_OVERLAP": "1"}, "preflight": {}},
]
LADDER_VARS = ("BPMF_HIP_EXCHANGE", "BPMF_HIP_COMM_STREAMS", "BPMF_HIP_OVERLAP")


def preflight_child():
    """One rank of a 4-iteration trial of ONE exchange configuration (the environment says which): a small sharded K = 32
    problem through the library's own RCCL path; every replica must hold the same bits afterwards.  Prints PREFLIGHT-OK."""
    import torch
    import torch.distributed as dist
    import bpmf_amd
    from bpmf_amd import synth
    from bpmf_amd.dist import NativeComm, build_sharded
    from bpmf_amd.sys import Sys
    R = Ranks()
    hang = os.environ.get("BPMF_BENCH_TEST_HANG_RUNG", "")           # test hook "rung-name:rank": that rank's trial of that rung never ends
    if hang and hang.split(":")[0] == os.environ.get("BPMF_BENCH_PREFLIGHT_RUNG") and int(hang.split(":")[1]) == R.rank:
        time.sleep(3600)
    torch.cuda.set_device(R.local_rank)
    dist.init_process_group("gloo")
    eng = bpmf_amd.HipEngine(32, device=R.local_rank)
    comm = NativeComm(eng)
    M, Mt, T, Tt, nu, nm = synth.ratings(4000 * R.world, 2000, 160000 * R.world, seed=7)
    Sys.nsims, Sys.burnin, Sys.alpha = 4, 1, 2.0
    movies, users = build_sharded(eng, comm, M, Mt, T, nu, nm, Tt=None, conn=False)
    for _ in range(4):
        movies.sample(users); users.sample(movies); movies.predict(users, True)
    eng.sync()
    U, V = users.items(), movies.items()
    if not (np.isfinite(movies.rmse) and np.isfinite(U).all() and np.isfinite(V).all()):
        raise SystemExit("preflight: non-finite results")
    sums = [None] * R.world
    dist.all_gather_object(sums, (float(U.sum()), float(np.abs(V).sum()), float(movies.rmse)))
    if any(x != sums[0] for x in sums):
        raise SystemExit("preflight: the ranks' replicas differ: %r" % (sums,))
    eng.close()
    dist.barrier()
    dist.destroy_process_group()
    print("PREFLIGHT-OK rank %d rmse %.6f" % (R.rank, movies.rmse), flush=True)


def preflight_ladder(R, wd):
    """Every rank starts a child that is ITS rank of a trial job (own rendez-vous port, own communicators), waits for it with
    a wall-clock limit (kill + reap), and the ranks agree on the outcome; the first configuration that every rank completed is
    the one the run uses.  Returns (record for the JSON line, None) or (record, error message)."""
    import torch.distributed as dist
    user_set = {k: os.environ[k] for k in LADDER_VARS if k in os.environ}
    if os.environ.get("BPMF_BENCH_PREFLIGHT", "1") == "0":
        return {"chosen": "environment" if user_set else LADDER[0]["name"], "env": user_set, "ladder": [], "preflight": "skipped (BPMF_BENCH_PREFLIGHT=0)"}, None
    rungs = [{"name": "environment", "env": {}, "preflight": {}}] if user_set else LADDER
    limit = float(os.environ.get("BPMF_BENCH_PREFLIGHT_TIMEOUT_S", "75"))
    record = []
    for idx, rung in enumerate(rungs):
        wd.stage("preflight of exchange configuration '%s'" % rung["name"], limit + 45)
        box = [None]
        if R.rank == 0:
            import socket
            s = socket.socket(); s.bind(("127.0.0.1", 0)); box[0] = s.getsockname()[1]; s.close()
        dist.broadcast_object_list(box, src=0)
        env = dict(os.environ, MASTER_PORT=str(box[0]), BPMF_BENCH_PREFLIGHT_CHILD="1", BPMF_BENCH_PREFLIGHT_RUNG=rung["name"])
        for k in [k for k in env if k.startswith("TORCHELASTIC_")]:       # (under torchrun: the trial's rank 0 hosts its own store, the agent's
            env.pop(k)                                                    #  store lives on the launcher's port -- every rank would wait as a client)
        env.setdefault("BPMF_HIP_COMM_TIMEOUT_MS", str(int(limit * 1000 * 0.4)))      # the library gives up (with a message) before the child is killed
        env.update(rung["env"]); env.update(rung["preflight"])
        t0 = time.time()
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--preflight-child"], env=env, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True)
        try:
            so, se = child.communicate(timeout=limit)
            ok, why = (child.returncode == 0 and "PREFLIGHT-OK" in so), ""
            if not ok:
                tail = [l for l in (se or so).strip().splitlines() if l.strip()][-3:]
                why = "rank %d: exit code %s: %s" % (R.rank, child.returncode, " | ".join(tail)[-400:])
        except subprocess.TimeoutExpired:
            child.kill()
            try:
                so, se = child.communicate(timeout=10)
            except subprocess.TimeoutExpired:
                so, se = "", ""
            ok, why = False, "rank %d: no result within %.0f s (killed)" % (R.rank, limit)
        res = R.gather({"ok": ok, "why": why})
        all_ok = all(r["ok"] for r in res)
        record.append({"config": rung["name"], "ok": all_ok, "seconds": round(time.time() - t0, 2),
                       "why": "; ".join(r["why"] for r in res if r["why"])[:800] or None})
        if all_ok:
            os.environ.update(rung["env"])
            return {"chosen": rung["name"], "env": dict(rung["env"], **user_set), "ladder": record}, None
    return {"chosen": None, "env": user_set, "ladder": record}, "no exchange configuration completed its 4-iteration preflight on every rank"


class Ranks:
    """The launcher side of a run: who am I, how do the ranks talk (torch.distributed is only the launcher and the
    clock here: barriers, the max of the block times, gathering the per-rank records; the data path is RCCL inside the
    library).  BPMF_BENCH_SHARED_GPU=1 (test set-up: every rank on device 0, the tests' RCCL double as
    BPMF_HIP_RCCL_LIBRARY) uses gloo for that, since the real RCCL -- torch's included -- refuses two ranks per device."""

    def __init__(self):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.shared_gpu = os.environ.get("BPMF_BENCH_SHARED_GPU") == "1"
        self.local_rank = 0 if self.shared_gpu else int(os.environ.get("LOCAL_RANK", "0"))
        self.force_dist = os.environ.get("BPMF_BENCH_FORCE_DIST") == "1"        # test hook: the sharded path with 1 rank
        self.dist = self.world > 1 or self.force_dist

    def init(self):
        import torch
        if not self.shared_gpu:                         # (shared GPU: gloo needs no device; run() opens it after the preflight)
            torch.cuda.set_device(self.local_rank)
        if self.dist:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29531")
            os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
            if self.shared_gpu:
                dist.init_process_group("gloo")
            else:
                dist.init_process_group("nccl", device_id=torch.device("cuda", self.local_rank))

    def barrier(self):
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()

    def max(self, x):
        if self.world == 1:
            return x
        import torch
        import torch.distributed as dist
        t = torch.tensor([x], dtype=torch.float64, device="cpu" if self.shared_gpu else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def gather(self, obj):
        """[obj of rank 0, obj of rank 1, ...] on every rank"""
        if self.world == 1:
            return [obj]
        import torch.distributed as dist
        out = [None] * self.world
        dist.all_gather_object(out, obj)
        return out

    def finish(self):
        if self.dist:
            import torch.distributed as dist
            dist.destroy_process_group()


def spot_check(sd, other, csc, cols, iter_, alpha):
    """Recomputes columns `cols` (global ids) of side `sd` on the host from nothing but the library's host-side normal
    stream (bpmf_randn_stream: rng_set_pos + randn of c++/mvnormal.cpp:34-43) and a dense solve -- Lambda* = LambdaF +
    alpha sum u u^T, b = LambdaF mu + alpha sum (r - mean) u, x = L^-T (L^-1 b + z), c++/sample.cpp:285-323 -- from the
    other side's CURRENT factors and the hyper-parameters the side was last sampled with, and returns
    max |x_host - x_device| / max |x|.  Valid straight after sd.sample(other).  No oracle involved."""
    import scipy.linalg
    from bpmf_amd import engine as _engine
    K = sd.K
    colptr, rowidx, vals = csc
    sd.refresh()
    mu, LF = np.asarray(sd.hp.mu), np.asarray(sd.hp.LambdaF)
    X = sd.engine.get_items(sd.side)
    O = other.engine.get_items(other.side)
    worst, scale = 0.0, 0.0
    for c in cols:
        l = c - sd.dom[0]
        p0, p1 = int(colptr[l]), int(colptr[l + 1])
        rows = rowidx[p0:p1]; v = vals[p0:p1]
        if hasattr(rows, "cpu"):
            rows = rows.cpu().numpy(); v = v.cpu().numpy()
        Uo = O[np.asarray(rows, np.int64)]
        Lam = LF + alpha * (Uo.T @ Uo)
        b = LF @ mu + alpha * (Uo.T @ (np.asarray(v, np.float64) - sd.mean_rating))
        L = np.linalg.cholesky(Lam)
        y = scipy.linalg.solve_triangular(L, b, lower=True)
        z = _engine.randn_host(((c + 1) * K * (iter_ + 1)) & 0xFFFFFFFF, K)
        x = scipy.linalg.solve_triangular(L.T, y + z, lower=False)
        worst = max(worst, float(np.abs(x - X[c]).max())); scale = max(scale, float(np.abs(x).max()))
    return worst / max(scale, 1e-300)


def pick_columns(colptr, c0, n=16, seed=1):
    """heaviest, lightest and random local columns (global ids)"""
    deg = np.diff(np.asarray(colptr))
    order = np.argsort(deg, kind="stable")
    rng = np.random.default_rng(seed)
    pick = list(order[-4:]) + list(order[:4]) + list(rng.choice(len(deg), size=min(n - 8, len(deg)), replace=False))
    return [int(c0 + c) for c in dict.fromkeys(pick)]


def strong_10Mx1M(R, steps, scale=1.0, check=True):
    """The north star's strong-scaling experiment (configs[3]): 10M x 1M x 200 per user, K = 32, the same
    matrix whatever N; rank r of N holds user chunks / item ranges [8r/N, 8(r+1)/N)."""
    import torch
    import bpmf_amd
    from bpmf_amd.synth_dev import BigMatrix
    from bpmf_amd.sys import Sys
    world, rank, local_rank = R.world, R.rank, R.local_rank
    K, G = 32, 8
    if G % world:
        return {"skipped": "needs a rank count that divides %d" % G}
    t_gen = time.perf_counter()
    dev = torch.device("cuda", local_rank)
    big = BigMatrix(dev, nusers=int(10_000_000 * scale), nitems=int(1_000_000 * scale), groups=G)
    parts = list(range(rank * G // world, (rank + 1) * G // world))
    bnd = big.item_bounds()
    bm = [bnd[r * G // world] for r in range(world)] + [big.NI]
    bu = [big.chunk_range(r * G // world)[0] for r in range(world)] + [big.NU]
    ucp, uri, uva, u0, u1 = big.users_csc(parts)
    mcp, mri, mva, i0, i1 = big.items_csc(parts)
    tcsc = big.test_csc(i0, i1)
    torch.cuda.synchronize()
    gen_s = time.perf_counter() - t_gen
    eng = bpmf_amd.HipEngine(K, device=local_rank)
    comm = None
    if world > 1:
        from bpmf_amd.dist import NativeComm
        comm = NativeComm(eng)
    Sys.nsims, Sys.burnin, Sys.alpha = 10 ** 6, 5, 2.0
    movies = Sys("movs", eng, (mcp, mri, mva), big.NI, big.NU, T=tcsc, dom=(i0, i1), mean_rating=big.mean_rating, comm=comm)
    users = Sys("users", eng, (ucp, uri, uva), big.NU, big.NI, dom=(u0, u1), mean_rating=big.mean_rating, comm=comm)
    if comm is not None:
        comm.register(movies, bm); comm.register(users, bu)

    def fence():
        eng.sync(); torch.cuda.synchronize()
        R.barrier(); torch.cuda.synchronize()

    def block(n):
        for i in range(n):
            movies.sample(users); users.sample(movies)
            if i > 0:
                movies.predict_finish()
            movies.predict_launch(users)
        movies.predict_finish()

    block(2)
    fence()
    base = {sd.name: eng.kernel_ms_sum(sd.side) for sd in (movies, users)}
    t0 = time.perf_counter()
    block(steps)
    fence()
    dt = R.max(time.perf_counter() - t0)
    out = {"workload": "device-generated %d users x %d items, %d ratings per user, K=32 fp64 (BASELINE configs[3]); the same matrix at every N"
                       % (big.NU, big.NI, big.PER),
           "n_gpus": world, "rccl_nranks": eng.comm_nranks(), "steps": steps, "ms_per_step": dt / steps * 1e3,
           "value": (big.NU + big.NI) * steps / dt, "unit": "samples/s",
           "scaling": "strong", "rmse": movies.rmse, "generate_s": gen_s,
           "kernel": {"items_side": eng.kernel_name(movies.side), "users_side": eng.kernel_name(users.side)}}
    kern = {}
    for sd in (movies, users):
        a1 = eng.kernel_ms_sum(sd.side); a0 = base[sd.name]
        nl = a1[2] - a0[2]
        kern[sd.name] = (a1[0] - a0[0]) / nl if nl > 0 else None
    mine = {"rank": rank, "items_side_columns": i1 - i0, "users_side_columns": u1 - u0}
    if kern["movs"] and kern["users"]:
        byt = algorithmic_bytes(movies.local_nnz, i1 - i0, K) + algorithmic_bytes(users.local_nnz, u1 - u0, K)
        ks = (kern["movs"] + kern["users"]) * 1e-3
        mine.update({"sampler_ms": {"items_side": kern["movs"], "users_side": kern["users"]},
                     "hbm_achieved_gbs": byt / ks / 1e9, "hbm_frac": byt / ks / 1e9 / HBM_PEAK_GBS,
                     "algorithmic_bytes_per_iteration_this_rank": byt,
                     # what one Gibbs iteration spends outside this rank's two sampler launches: exchange
                     # (all-gather of the fresh ranges + all-reduce of the sums), statistics, host draws
                     "exchange_and_rest_ms": dt / steps * 1e3 - (kern["movs"] + kern["users"])})
    if check:
        # parity probe of the very chain that was timed: >= 16 columns per side of this rank against a host solve.
        # users(i) were drawn from movies(i); one more movies.sample(users) gives movies(i+1) drawn from users(i).
        t_chk = time.perf_counter()
        errs, problems = {}, []
        for name, sd, other, csc, c0 in (("users_side", users, movies, (ucp, uri, uva), u0), ("items_side", movies, users, (mcp, mri, mva), i0)):
            if name == "items_side":
                movies.sample(users)                                   # (collective: every rank, whatever its own check did)
            try:
                errs[name] = spot_check(sd, other, csc, pick_columns(csc[0], c0), sd.iter, Sys.alpha)
            except Exception as e:
                problems.append("%s: %r" % (name, e))
        if problems:
            mine["spot_check"] = {"error": "; ".join(problems)[:400]}
        else:
            worst = max(errs.values())
            mine["spot_check"] = {"columns_per_side": 16, "max_err_users_side": errs["users_side"], "max_err_items_side": errs["items_side"],
                                  "max_err": worst, "tolerance": 1e-9, "ok": bool(worst < 1e-9),
                                  "against": "host solve + bpmf_randn_stream (no oracle)", "seconds": time.perf_counter() - t_chk}
    if world == 1 and "algorithmic_bytes_per_iteration_this_rank" in mine:
        # HBM-side bytes per launch from the committed PMC pass of this record (profiles/r*_pmc_strong_10Mx1M.txt), if it was
        # taken with these kernel sources; algorithmic bytes per launch = half an iteration's
        p_traffic, _, pmc_file, pmc_sha = profiled("strong_10Mx1M")
        cur = pmc_file is not None and pmc_sha == kernel_source_sha()
        sides = profiled_by_grid("strong_10Mx1M")
        if sides and all(v.get("l2_memory_side_bytes") for v in sides.values()):
            # per launch = the mean of the two sides (the plain per-launch average of the file is over the kept dispatches, 2 + 1)
            p_traffic = 0.5 * sum(v["l2_memory_side_bytes"] for v in sides.values())
        per_launch = mine["algorithmic_bytes_per_iteration_this_rank"] / 2.0
        launch_s = 0.5 * sum(mine["sampler_ms"].values()) * 1e-3
        mine.update({"traffic": p_traffic if cur else None,
                     # what the counter is (VERDICT r5 "weak" 8): FETCH_SIZE / WRITE_SIZE sit on L2's MEMORY SIDE -- they count the requests
                     # L2 sends towards the fabric, Infinity-Cache (MALL, 256 MB) hits included, not DRAM reads.  The items factor of this
                     # shape is exactly 256 MB and the users side walks ascending row ids: part of this traffic is served by the MALL, and a
                     # rate above the ~6.3 TB/s a DRAM copy sustains is no contradiction.  The kernel is at the fabric-side roofline.
                     "traffic_is": "L2 memory-side requests (2 x FETCH_SIZE + WRITE_SIZE) incl. Infinity-Cache hits; not DRAM bytes",
                     "per_side_counters": sides if cur else None,
                     "algorithmic_bytes_per_launch": per_launch,
                     "hbm_traffic_over_algorithmic": (p_traffic / per_launch) if (cur and p_traffic) else None,
                     # the same fraction from the counters instead of the algorithmic bytes: HBM-side bytes per launch / launch time / 8 TB/s
                     "hbm_frac_counter": (p_traffic / launch_s / 1e9 / HBM_PEAK_GBS) if (cur and p_traffic and launch_s > 0) else None,
                     "profiled": {"source": pmc_file, "kernel_source_sha": pmc_sha, "current": bool(cur), "traffic": p_traffic}})
    ranks = R.gather(mine)
    out.update({k: v for k, v in ranks[0].items() if k != "rank"})          # rank 0's figures at top level (as before)
    out["model"] = strong_model(big.NU, big.NI, K, world, ranks, dt / steps * 1e3)
    if world > 1:
        out["per_rank"] = ranks
        errs = [r.get("spot_check", {}).get("max_err") for r in ranks]
        if all(e is not None for e in errs):
            out["spot_check"] = dict(ranks[0]["spot_check"], max_err=max(errs), ok=bool(max(errs) < 1e-9))
    eng.close()
    return out


def bpmf_exe_record(M, T, nusers, nmovies, K, nsims=25, burnin=5):
    """The C++ host the north star names: the `bpmf` executable (bpmf_amd/csrc/bpmf_main.cpp -> C ABI -> the same kernels) on
    the matrices of this run, written as .sdm: `bpmf -i 25 -b 5 -d K`, its own `Average items/sec` and `Final Avg RMSE`
    (c++/bpmf.cpp:246-252) parsed from stdout.  The first iterations carry start-up (clock ramp, first launches): the
    steady-state figure is the mean of the per-iteration items/sec of the second half of the run."""
    import re
    from bpmf_amd import io as bio
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    d = tempfile.mkdtemp(prefix="bpmf_exe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        bio.write_sparse(os.path.join(d, "train.sdm"), nusers, nmovies, M)
        bio.write_sparse(os.path.join(d, "test.sdm"), nusers, nmovies, T)
        t0 = time.perf_counter()
        r = subprocess.run([exe, "-n", "train.sdm", "-p", "test.sdm", "-i", str(nsims), "-b", str(burnin), "-d", str(K)], cwd=d,
                           capture_output=True, text=True, timeout=300)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            return {"error": "bpmf exited with %d: %s" % (r.returncode, r.stderr[-300:])}
        per_iter = [float(m.group(1)) for l in r.stdout.splitlines() if " iteration " in l for m in [re.search(r"\titems/sec:\s*([0-9.eE+]+)", l)] if m]
        avg = float(re.search(r"Average items/sec: (\S+)", r.stdout).group(1))
        final = float(re.search(r"Final Avg RMSE: (\S+)", r.stdout).group(1))
        steady = per_iter[len(per_iter) // 2:]
        return {"command": "bpmf -n train.sdm -p test.sdm -i %d -b %d -d %d" % (nsims, burnin, K), "average_items_per_s": avg,
                "steady_items_per_s": float(np.mean(steady)) if steady else None, "final_avg_rmse": final, "iterations": len(per_iter),
                "wall_s": wall, "unit": "samples/s (the reference's items/sec: users + movies per iteration time)",
                "host": "C++ (bpmf_amd/csrc/bpmf_main.cpp) over the C ABI of include/bpmf_hip.h"}
    except Exception as e:
        return {"error": repr(e)[:300]}
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)


# The other single-GPU configurations BASELINE.json names, in the order they are run after the headline (configs[2], configs[4],
# then the two the same kernels' fp64 / K = 64 forms give for free).  Each is THIS script, run as a child with the workload
# named, the same --steps / --warmup, its own >= 2 s timed window and the parity chain against the oracle (no CPU timing
# sweep, no strong-scaling record): a leg that fails or outlives its limit becomes {"value": null, "error": ...} and the
# headline survives.
CONFIG_LEGS = [("chembl", "BASELINE configs[2]: ChEMBL-20 shape, K = 64 fp64"),
               ("ml1m_k128", "BASELINE configs[4]: ML-1M shape, K = 128, fp32 factors (opt-in)"),
               ("ml1m_k64", "ML-1M shape, K = 64 fp64"),
               ("ml1m_k128_f64", "ML-1M shape, K = 128 in the reference's fp64 (`bpmf -d 128`)")]


def config_leg(name, what, steps, warmup, limit_s):
    """One entry of the line's `configs` object: ms_per_step / value / dtype / kernels / per-side launch times / roofline /
    parity of workload `name`, measured by a child run of this script through the same `step_block` and `timed_blocks`."""
    t0 = time.perf_counter()
    cmd = [sys.executable, os.path.abspath(__file__), "--workload", name, "--steps", str(steps), "--warmup", str(warmup), "--full",
           "--no-strong", "--no-bpmf-exe", "--no-configs", "--cpu-parity-only", "--repeats", "0", "--window-s", "2.0"]
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit_s)
    except subprocess.TimeoutExpired:
        return {"what": what, "value": None, "error": "no line within %.0f s (killed)" % limit_s, "wall_s": time.perf_counter() - t0}
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    if not lines:
        tail = " | ".join([l for l in (r.stderr or r.stdout).strip().splitlines() if l.strip()][-3:])
        return {"what": what, "value": None, "error": "exit code %d, no line: %s" % (r.returncode, tail[-400:]), "wall_s": time.perf_counter() - t0}
    c = json.loads(lines[-1])
    if c.get("value") is None:
        return {"what": what, "value": None, "error": c.get("error", "the child reported no value"), "wall_s": time.perf_counter() - t0}
    rf, par = c.get("roofline", {}), c.get("parity", {})
    out = {"what": what, "command": "bench.py " + " ".join(cmd[2:]),
           "ms_per_step": c["ms_per_step"], "value": c["value"], "unit": c["unit"], "dtype": c["dtype"], "steps": c["steps"],
           "repeats": c.get("repeats"), "timed_window_s": c.get("timed_window_s"),
           "ms_per_step_min": c.get("ms_per_step_min"), "ms_per_step_max": c.get("ms_per_step_max"),
           "kernel_per_side": rf.get("kernel_per_side"),
           "launch_us_per_side": {k: v * 1e3 for k, v in (rf.get("launch_ms_per_side") or {}).items()},
           "roofline": {k: rf.get(k) for k in ("bound", "frac", "achieved", "peak", "unit", "traffic", "hbm_frac", "hbm_frac_per_side",
                                               "executed_flops_per_launch", "algorithmic_bytes_per_launch", "issue_bound", "mfma_shape") if k in rf},
           "rmse": c.get("rmse"), "workload": c.get("config", {}).get("workload"),
           "wall_s": time.perf_counter() - t0}
    if par.get("ok") is not None:
        out["parity"] = {k: par.get(k) for k in ("ok", "iterations", "burnin", "d_rmse_max", "d_final_avg_rmse", "d_items_rel", "d_norm_rel",
                                                 "rmse_gpu", "rmse_cpu", "tolerance", "oracle_pinned")}
    else:
        out["parity"] = {"ok": None, "reason": par.get("reason")}
    return out


def strong_model(NU, NI, K, world, ranks, ms_per_step):
    """The predicted 1 -> 8 curve of the strong-scaling record, so that the first measured SCALE record can be read against
    it.  Ingredients: the sampler time of the whole matrix (sum over the ranks of their two launches -- at N = 1 the measured
    launches themselves), divided by N (columns are cut at equal work); the fresh columns every rank must receive per
    iteration, (NU + NI) K 8 (N - 1) / N bytes, arriving over N - 1 point-to-point xGMI links at 153 GB/s each (the mesh
    exchange puts one peer on one link: per-link bytes = (NU + NI) K 8 / N), of which only the last of 4 parts is not
    hidden behind sampling; two all-reduces of K^2 + K + 1 doubles (~30 us each); and what one iteration spends outside
    the samplers on one GPU (statistics, host draws, RMSE; measured at N = 1, else the 0.7 ms of the round-3 N = 1 record)."""
    link_gbs, allreduce_ms, parts = 153.0, 0.03, 4
    samp = [sum(r["sampler_ms"].values()) for r in ranks if r.get("sampler_ms")]
    if len(samp) != len(ranks):
        return {"error": "no sampler times"}
    s_total = float(sum(samp))
    # (N = 1: the HIP-event sample -- every 8th launch of a side -- and the wall mean over all steps come from different launches,
    # so their difference can come out slightly negative when the samplers are all there is: clamped at 0)
    rest = max(0.0, ms_per_step - s_total) if world == 1 else float(os.environ.get("BPMF_BENCH_MODEL_REST_MS", "0.7"))
    per_n, base = {}, None
    for n in (1, 2, 4, 8):
        link_bytes = (NU + NI) * K * 8.0 / n if n > 1 else 0.0
        ex = link_bytes / (link_gbs * 1e9) * 1e3
        ms = s_total / n + rest + (ex / parts if n > 1 else 0.0) + (2 * allreduce_ms if n > 1 else 0.0)
        base = ms if n == 1 else base
        per_n[str(n)] = {"sampler_ms": s_total / n, "exchange_bytes_per_link": link_bytes, "exchange_ms_if_exposed": ex,
                         "exchange_ms_exposed_with_%d_parts" % parts: ex / parts if n > 1 else 0.0, "allreduce_ms": 2 * allreduce_ms if n > 1 else 0.0,
                         "ms_per_step": ms, "samples_per_s": (NU + NI) / ms * 1e3, "speedup_vs_1": base / ms}
    return {"sampler_ms_whole_matrix": s_total, "rest_ms": rest,
            "rest_is": "measured at N = 1: wall mean per step - HIP-event mean of the sampled launches (every 8th of a side), clamped at 0" if world == 1 else "assumed (BPMF_BENCH_MODEL_REST_MS)",
            "xgmi_link_gbs": link_gbs, "per_n": per_n, "this_run": {"n_gpus": world, "ms_per_step": ms_per_step,
                                                                   "over_model": ms_per_step / per_n[str(world)]["ms_per_step"] if str(world) in per_n else None}}


def visible_devices():
    """HIP devices this process can see -- from the HIP runtime directly (the launcher has no other use for torch, whose import is
    seconds), torch as the fall-back."""
    try:
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_int(0)
        if hip.hipGetDeviceCount(ctypes.byref(n)) == 0:
            return int(n.value)
        return 0
    except OSError:
        import torch
        return torch.cuda.device_count() if torch.cuda.is_available() else 0


def self_launch(n):
    """`bench.py --gpus N` without a launcher: start the N ranks (one process per GPU) and relay their exit code."""
    import socket
    shared = os.environ.get("BPMF_BENCH_SHARED_GPU") == "1"
    have = None if shared else visible_devices()         # (the shared-GPU set-up: this process does not open the device at all)
    if not shared and have < n:
        raise SystemExit("bench.py: --gpus %d asked for, %d HIP device(s) visible: refusing to report fewer ranks as %d GPUs "
                         "(one rank per GPU; a launcher may set WORLD_SIZE / RANK / LOCAL_RANK instead)" % (n, have, n))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(n), BPMF_BENCH_SELF_LAUNCHED="1")
    procs = []
    for r in range(n):
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                                      env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE if r == 0 else None, text=True))
    # Reap with a wall-clock limit: a rank that dies takes the others down (they would wait for it in a collective), a job
    # that outlives BPMF_BENCH_TOTAL_TIMEOUT_S is killed, and if rank 0 never printed its line this process prints one.
    import threading
    seen = {"line": False}

    def relay():
        for line in procs[0].stdout:
            if line.startswith('{"metric"'):
                seen["line"] = True
            sys.stdout.write(line); sys.stdout.flush()
    th = threading.Thread(target=relay, daemon=True); th.start()
    limit = float(os.environ.get("BPMF_BENCH_TOTAL_TIMEOUT_S", "1500"))
    t0, rc, why = time.time(), 0, None
    while True:
        codes = [pr.poll() for pr in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            rc, why = bad[0][1], "rank %d exited with code %d" % bad[0]
            time.sleep(2.0)                                             # (its peers' watchdogs / error paths get to print first)
            break
        if all(c == 0 for c in codes):
            break
        if time.time() - t0 > limit:
            rc, why = 124, "the job did not finish within %.0f s" % limit
            break
        time.sleep(0.2)
    for pr in procs:
        if pr.poll() is None:
            pr.kill()
    for pr in procs:
        try:
            pr.wait(timeout=15)
        except subprocess.TimeoutExpired:
            pass
    th.join(timeout=5)
    if rc and not seen["line"]:
        print(error_line("bench.py --gpus %d: %s" % (n, why), launcher="self"), flush=True)
    raise SystemExit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS))
    ap.add_argument("--K", type=int, default=None, help="shorthand: ML-1M shape with this K (32, 64, 128)")
    ap.add_argument("--full", action="store_true", help="also the records that take runs of their own: parity chain, strong_10Mx1M, bpmf_exe, "
                                                         "configs, cpu_baseline (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the timed path computed in its last step as DIR/<name>.npy")
    ap.add_argument("--repeats", type=int, default=1, help="timed blocks of --steps steps, the median block is reported (0 = auto: as many as fill "
                                                           "--window-s of timed time, at least 5)")
    ap.add_argument("--window-s", type=float, default=2.5, help="timed time the blocks must add up to when --repeats is 0 (the median block is reported)")
    ap.add_argument("--no-configs", action="store_true", help="skip the `configs` object (the other single-GPU BASELINE configurations, one child run each)")
    ap.add_argument("--cpu-parity-only", action="store_true", help="the CPU leg runs the oracle's parity chain only (no timing sweep): what the `configs` children use")
    ap.add_argument("--prewarm-steps", type=int, default=256, help="untimed steps after the W warm-up steps (a fixed count: the timed chain "
                                                                   "does not depend on the speed)")
    ap.add_argument("--prewarm-ms", type=float, default=0.0, help="then untimed steps until this much time has passed since the warm-up began "
                                                                "(the timed chain then depends on the speed)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the `parity` object (the -i N -b B chain through the timed pipeline against the oracle's chain)")
    ap.add_argument("--no-bpmf-exe", action="store_true", help="skip the bpmf_exe sub-record (the `bpmf` executable on the same matrices)")
    ap.add_argument("--no-strong", action="store_true", help="skip the strong_10Mx1M sub-record")
    ap.add_argument("--strong-steps", type=int, default=8, help="timed steps of the strong_10Mx1M record (>= 8: the library times every 8th launch of a side)")
    ap.add_argument("--strong-scale", type=float, default=float(os.environ.get("BPMF_BENCH_STRONG_SCALE", "1.0")))
    ap.add_argument("--no-users-predict", action="store_true", help="A/B: leave users.predict(movies) (c++/bpmf.cpp:190) out of the step; the line says so")
    ap.add_argument("--preflight-child", action="store_true", help="internal: one rank of a 4-iteration trial of an exchange configuration")
    ap.add_argument("--ablate", type=int, default=None, help="profiling only: run with BPMF_HIP_ABLATE=<bits> (phases of the sampler skipped, samples WRONG); the line is marked invalid")
    args = ap.parse_args()
    if args.preflight_child:
        preflight_child()
        return
    wl = args.workload or {None: "ml1m", 32: "ml1m", 64: "ml1m_k64", 128: "ml1m_k128"}.get(args.K)
    if wl is None:
        raise SystemExit("bench.py: --K must be 32, 64 or 128 (or use --workload)")
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    # BPMF_HIP_ABLATE makes the sampler skip the Gram or the factorisation (tools/gpu_ablate.sh): a number measured
    # that way is not a throughput.  Only behind --ablate, and then the line says so.
    env_ablate = os.environ.get("BPMF_HIP_ABLATE", "0") or "0"
    if args.ablate is not None:
        os.environ["BPMF_HIP_ABLATE"] = str(args.ablate)
        # the phase switches exist only in the profiling build of the library (bpmf_amd/csrc/Makefile: `make prof`)
        prof = os.path.join(ROOT, "bpmf_amd", "libbpmf_hip_prof.so")
        if "BPMF_HIP_LIBRARY" not in os.environ:
            if not os.path.exists(prof):
                raise SystemExit("bench.py --ablate needs the profiling build: make -C bpmf_amd/csrc prof")
            os.environ["BPMF_HIP_LIBRARY"] = prof
    elif env_ablate not in ("0", ""):
        raise SystemExit("bench.py: BPMF_HIP_ABLATE=%s is set (the sampler would skip work and return wrong samples); "
                         "unset it, or ask for it with --ablate N" % env_ablate)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        self_launch(args.gpus)                                         # (does not return)
    R = Ranks()
    wd = Watchdog(R.rank, {"steps": args.steps, "warmup": args.warmup})
    try:
        run(args, wl, R, wd)
    except SystemExit:
        raise
    except BaseException as e:                                        # a rank that fails says so in the line's own format
        import traceback
        traceback.print_exc()
        if R.rank == 0:
            print(error_line("rank 0: %r" % (e,), stage=wd.name, steps=args.steps, warmup=args.warmup), flush=True)
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(4)                                                   # (not sys.exit: worker threads / a wedged collective must not hold the exit)
    wd.stop()


def run(args, wl, R, wd):
    if R.world != args.gpus and not R.force_dist:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s) (WORLD_SIZE): the two must agree" % (args.gpus, R.world))
    K, dtype, lds_wg, wg_per_cu = WORKLOADS[wl]
    t_process = time.perf_counter()

    import torch
    import bpmf_amd
    from bpmf_amd import synth
    from bpmf_amd.sys import Sys

    world, rank, local_rank = R.world, R.rank, R.local_rank

    def open_device():
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a HIP device (bpmf_amd has no CPU fallback)")
        if torch.cuda.device_count() <= local_rank:
            raise SystemExit("bench.py: rank %d wants device %d, %d visible" % (rank, local_rank, torch.cuda.device_count()))
    # The shared-GPU test set-up (BPMF_BENCH_SHARED_GPU=1: every rank on device 0, gloo for the launcher's collectives) opens the
    # device only after the preflight ladder, so that N ranks and their N preflight children never hold the one GPU all at once.
    if not R.shared_gpu:
        open_device()
    wd.stage("process group", max(wd.default, 300.0))
    R.init()
    comm = None
    force_dist = R.force_dist
    exchange_config = None
    if world > 1:
        exchange_config, err = preflight_ladder(R, wd)
        if err:
            if rank == 0:
                print(error_line(err, exchange_config=exchange_config, steps=args.steps, warmup=args.warmup), flush=True)
            R.finish()
            raise SystemExit(2)
        wd.extra["exchange_config"] = exchange_config
    if R.shared_gpu:
        open_device()
        torch.cuda.set_device(local_rank)
    wd.stage("matrices + engine + communicator", max(wd.default, 300.0))

    mult = world if (world > 1 or force_dist) else 1
    if wl == "chembl":
        M, Mt, T, Tt, nusers, nmovies = synth.ratings(483500 * mult, 5775, 1_023_952 * mult, seed=42, real_valued=True)
        shape_note = "ChEMBL-shaped synthetic R (%d compounds x %d targets, %d real-valued activities, 90/10 split)"
    elif mult == 1:
        M, Mt, T, Tt, nusers, nmovies = synth.ml1m_shaped(seed=42)
        shape_note = "ML-1M-shaped synthetic R (%d users x %d movies, %d ratings, 90/10 split)"
    else:
        M, Mt, T, Tt, nusers, nmovies = synth.ratings(6040 * mult, 3706, 1_000_209 * mult, seed=42)
        shape_note = "ML-1M-shaped synthetic R (%d users x %d movies, %d ratings, 90/10 split)"
    nnz = int(M[0][-1])
    mean = float(np.sum(M[2])) / nnz

    esz = 4 if dtype == "f32" else 8
    eng = bpmf_amd.HipEngine(K, device=local_rank, dtype=dtype)
    if world > 1 or force_dist:
        from bpmf_amd.dist import NativeComm, TorchComm
        # default: RCCL inside the library (exchange + all-reduce behind the sampling call);
        # BPMF_DIST=torch keeps the collectives in torch.distributed (same results, slower host path)
        comm = TorchComm(torch.device("cuda", local_rank)) if os.environ.get("BPMF_DIST") == "torch" else NativeComm(eng)
    Sys.nsims, Sys.burnin, Sys.alpha = 10 ** 6, 5, 2.0
    handover_ms = None
    if comm is None:
        # the boundary takes HOST buffers (bpmf_hip_side_create: the reference's SparseMatrixD in CSC form, c++/bpmf.h:130-137):
        # the one-time hand-over -- both orientations of R and of the test set over PCIe, the static schedule, the initial
        # factors -- is timed here and reported beside the steady-state value (`handover`), never inside it
        torch.cuda.synchronize()
        t_h = time.perf_counter()
        movies = Sys("movs", eng, M, nmovies, nusers, T=T, mean_rating=mean)
        users = Sys("users", eng, Mt, nusers, nmovies, T=Tt, mean_rating=mean)
        eng.sync(); torch.cuda.synchronize()
        handover_ms = (time.perf_counter() - t_h) * 1e3
        dom_m, dom_u = (0, nmovies), (0, nusers)
    else:
        from bpmf_amd.dist import build_sharded
        movies, users = build_sharded(eng, comm, M, Mt, T, nusers, nmovies, mean_rating=mean, Tt=Tt)
        dom_m, dom_u = movies.dom, users.dom
    # users.predict(movies) (c++/bpmf.cpp:190: inside the reference's timed region, its results never read) rides with
    # every movies.predict(users) as the twin evaluation of the library
    both_predicts = users.test is not None and getattr(comm, "native", True) and not args.no_users_predict
    if both_predicts:
        movies.set_twin(users)
    rccl_nranks = eng.comm_nranks() if getattr(comm, "native", False) else (world if comm is not None else 1)
    rccl_comm_streams = eng.comm_streams() if getattr(comm, "native", False) else 0     # 2: second communicator split off (ncclCommSplit)
    if world > 1 and getattr(comm, "native", False) and rccl_nranks != world:
        raise SystemExit("bench.py: the communicator has %d rank(s), the launcher started %d" % (rccl_nranks, world))

    def fence():
        eng.sync()
        torch.cuda.synchronize()
        R.barrier()
        torch.cuda.synchronize()

    dist_max = R.max
    pipelined = comm is None or getattr(comm, "native", False)

    def step_block(n):
        if not pipelined:
            for _ in range(n):
                movies.sample(users); users.sample(movies); movies.predict(users)
                if both_predicts:
                    users.predict(movies)
            return
        # the same n iterations, software-pipelined the way the `bpmf` executable runs them: the RMSE
        # of iteration i is collected after iteration i+1 has been enqueued (the evaluation runs on
        # its own stream beside those samplers, which write the other copy of the factors)
        for i in range(n):
            movies.sample(users)
            users.sample(movies)
            if i > 0:
                movies.predict_finish()
                if both_predicts:
                    users.predict_finish()
            movies.predict_launch(users)
        movies.predict_finish()
        if both_predicts:
            users.predict_finish()

    wd.stage("warm-up")
    # warm-up: W steps, then P more untimed steps on the same chain -- a fresh pair of sides needs ~250 steps to reach its steady
    # rate even on a warm GPU (ML-1M shape: 0.116 ms per step in the first 20, 0.100 from ~240 on), and a 20-step timed region
    # straight after start-up also sits on the clock ramp (round 1: 0.122 against 0.102).  P is a fixed count, so the timed chain
    # runs the same W + P + K steps on every run; --prewarm-ms T adds untimed steps until T ms have gone by (speed-dependent).
    t_warm = time.perf_counter()
    if args.warmup + args.prewarm_steps > 0:
        step_block(args.warmup + args.prewarm_steps)
    fence()
    extra = args.prewarm_steps
    while dist_max(time.perf_counter() - t_warm) < args.prewarm_ms * 1e-3:
        step_block(max(1, min(args.steps, 50))); extra += max(1, min(args.steps, 50))
        fence()
    prewarm_ms = (time.perf_counter() - t_warm) * 1e3
    base = {sd.name: eng.kernel_ms_sum(sd.side) for sd in (movies, users)}
    wd.stage("timed blocks", wd.default + 30)
    if args.repeats > 0:
        times = timed_blocks(step_block, fence, args.steps, dist_max, min_blocks=args.repeats, max_blocks=args.repeats)
    else:
        times = timed_blocks(step_block, fence, args.steps, dist_max, window_s=args.window_s)
    fence()
    dt = float(np.median(times))
    dumped = None
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path holds after its last step: both factor matrices, the test set's running average
        # prediction and the step's RMSE pair (before the extra predict below, which is not part of a step)
        dumped = dump_outputs(args.dump_outputs, {"U": users.items(), "V": movies.items(),
                                                  "test_pred_avg": eng.test_get(movies.test)[0] if movies.test is not None else np.zeros(0),
                                                  "rmse": np.array([movies.rmse, movies.rmse_avg])})

    # roofline of the dominant kernel (the sampler), per launch, this rank's shard
    nnz_m = movies.local_nnz; nnz_u = users.local_nnz
    info_m, info_u = eng.schedule_info(movies.side), eng.schedule_info(users.side)
    bytes_launch = 0.5 * (algorithmic_bytes(nnz_m, dom_m[1] - dom_m[0], K, esz) + algorithmic_bytes(nnz_u, dom_u[1] - dom_u[0], K, esz))
    flops_alg = 0.5 * (algorithmic_flops(nnz_m, dom_m[1] - dom_m[0], K) + algorithmic_flops(nnz_u, dom_u[1] - dom_u[0], K))
    # what the launches execute: differs from the algorithmic count where columns take the product form (ChEMBL shape)
    flops_launch = 0.5 * (executed_flops(info_m, nnz_m, dom_m[1] - dom_m[0], K) + executed_flops(info_u, nnz_u, dom_u[1] - dom_u[0], K))
    # HIP-event times of the sampler / statistics kernels on their streams, summed by the library
    # over the timed steps (events ride on every 8th launch of a side, every 32nd after its first 64: BPMF_HIP_TIMING_EVERY)
    kern_ms, red_ms, nl, per_side = 0.0, 0.0, 0, {}
    for sd in (movies, users):
        a1 = eng.kernel_ms_sum(sd.side); a0 = base[sd.name]
        if a1[2] > a0[2]:
            kern_ms += a1[0] - a0[0]; red_ms += a1[1] - a0[1]; nl += a1[2] - a0[2]
            per_side[sd.name] = (a1[0] - a0[0]) / (a1[2] - a0[2])
        else:
            a, b = eng.last_kernel_ms(sd.side); kern_ms += a; red_ms += b; nl += 1
            per_side[sd.name] = a
    launch_s = kern_ms / max(nl, 1) * 1e-3
    hbm_gbs = bytes_launch / launch_s / 1e9 if launch_s > 0 else 0.0
    tflops = flops_launch / launch_s / 1e12 if launch_s > 0 else 0.0
    flop_peak = FP32_PEAK_TFLOPS if dtype == "f32" else FP64_PEAK_TFLOPS
    # HBM-side bytes and LDS bank conflicts need rocprofv3 --pmc passes (not available inside a plain run): they come
    # from the committed profile of this command IF that profile was taken with these very kernel sources
    p_traffic, p_conflict, pmc_file, pmc_sha = profiled(wl) if world == 1 else (None, None, None, None)
    src_sha = kernel_source_sha()
    pmc_current = pmc_file is not None and pmc_sha == src_sha
    traffic = p_traffic if pmc_current else None
    kernel_names = {"movs": eng.kernel_name(movies.side), "users": eng.kernel_name(users.side)}
    kernel_name = kernel_names["movs"] if kernel_names["movs"] == kernel_names["users"] else "%s | %s" % (kernel_names["movs"], kernel_names["users"])

    movies.predict(users, True)
    if both_predicts:
        users.predict(movies)
    # Which resource binds?  K = 32 on this matrix: the factors (1.5 + 0.95 MB) live in L2 / MALL -- HBM-side
    # traffic is ~0.2 x the algorithmic bytes -- and the launch is bound by instruction issue: the fp64 MFMA
    # Gram and the VALU factorisation share the SIMD.  K >= 64: the dense contraction / factorisation.
    roofline = {"bound": "mfma", "bound_detail": ("fp64 issue: the MFMA Gram and the VALU/MFMA factorisation share the SIMD; "
                                                  "the factor matrices sit in L2/MALL at this size, HBM is secondary")
                if dtype == "f64" else "fp32 MFMA Gram + blocked factorisation",
                "achieved": tflops, "peak": flop_peak, "unit": "TFLOP/s", "frac": tflops / flop_peak,
                "traffic": traffic, "kernel": kernel_name, "kernel_per_side": kernel_names, "launch_ms": launch_s * 1e3,
                "launch_ms_per_side": per_side, "executed_flops_per_launch": flops_launch,
                "algorithmic_flops_per_launch": flops_alg, "algorithmic_bytes_per_launch": bytes_launch,
                "hbm_achieved_gbs": hbm_gbs, "hbm_frac": hbm_gbs / HBM_PEAK_GBS,
                "hbm_traffic_over_algorithmic": (traffic / bytes_launch) if traffic else None,
                "colstats_ms": red_ms / max(nl, 1),
                # the committed PMC passes these two figures come from, the kernel sources they were taken with, and
                # whether those are the sources of this run (if not: `traffic` stays null, the figures are history)
                "profiled": {"source": pmc_file, "kernel_source_sha": pmc_sha, "current": bool(pmc_current),
                             "traffic": p_traffic, "bank_conflict_rate": p_conflict},
                "kernel_source_sha": src_sha}
    if world == 1:
        roofline["issue_bound"] = issue_bound(wl, launch_s, getattr(eng, "num_cu", 256))
    # The ceiling of the MFMA SHAPE the sampler's Gram is built from, measured chip-wide on this hardware
    # (tools/probes/mfma_shapes_probe.hip -> profiles/r05_mfma_shapes_probe.txt): the data-sheet peak (78.6 / 157.3 TF) is what `frac`
    # is quoted against, but v_mfma_f64_16x16x4 sustains 48.4 TF and v_mfma_f32_16x16x4 138.7 TF whatever feeds them
    shape = {"ml1m": ("v_mfma_f64_4x4x4_4b_f64", 68.9), "ml1m_k64": ("v_mfma_f64_4x4x4_4b_f64", 68.9), "chembl": ("v_mfma_f64_4x4x4_4b_f64", 68.9),
             "ml1m_k128": ("v_mfma_f32_16x16x4_f32", 138.7), "ml1m_k128_f64": ("v_mfma_f64_16x16x4_f64", 48.4), "ml1m_k100": ("v_mfma_f64_16x16x4_f64", 48.4)}[wl]
    roofline["mfma_shape"] = {"instruction": shape[0], "measured_peak_tflops": shape[1], "frac_of_shape_peak": tflops / shape[1],
                              "source": "profiles/r05_mfma_shapes_probe.txt"}
    if abs(flops_launch - flops_alg) > 1e-6 * flops_alg:
        # Columns in the product form (ChEMBL shape) are never factorised, so neither flop count is a SURVEY 8(d) quantity of
        # what runs: the roofline of this workload is stated in 8(d) BYTES (the compounds side streams Q rows, ratings and
        # samples; the targets side gathers from a 247 MB factor matrix) -- achieved = algorithmic bytes per launch / launch
        # time against 8 TB/s -- and the two flop figures stay beside it, labelled for what they are.
        eff = flops_alg / launch_s / 1e12 if launch_s > 0 else 0.0
        roofline.update({"bound": "hbm", "bound_detail": "SURVEY 8(d) algorithmic bytes per launch / HIP-event launch time; the product-form kernels are VALU-issue "
                                                         "bound (Philox / polar draw + scans), not bandwidth bound: the fraction says how far from the stream rate they are",
                         "achieved": hbm_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": hbm_gbs / HBM_PEAK_GBS,
                         "executed_flop_model": {"tflops": tflops, "frac_of_fp64_peak": tflops / flop_peak,
                                                 "note": "a hand model of what the product form executes per column (bench.py::executed_flops): not a SURVEY 8(d) quantity, "
                                                         "not reproducible from a profile"},
                         "reference_algorithm_flops": {"tflops": eff, "over_fp64_peak": eff / flop_peak,
                                                       "note": "algorithmic flops of the reference's per-column factorisation (K^3/3 ...) / launch time: an algorithmic "
                                                               "speed-up figure (the product form never executes them), may exceed 1, not a roofline fraction"}})
        per_side_bytes = {"movs": algorithmic_bytes(nnz_m, dom_m[1] - dom_m[0], K, esz), "users": algorithmic_bytes(nnz_u, dom_u[1] - dom_u[0], K, esz)}
        roofline["hbm_frac_per_side"] = {k: (per_side_bytes[k] / (per_side[k] * 1e-3) / 1e9 / HBM_PEAK_GBS) if per_side.get(k) else None for k in per_side_bytes}
    # LDS occupancy of the kernels that hold the factorisation (north star: "LDS occupancy on the Cholesky"): static LDS per
    # workgroup and workgroups resident per CU as the LIBRARY reports them for the kernels this side launches
    # (bpmf_hip_side_kernel_resources: the runtime's occupancy query), for every workload; the bank-conflict rate from the
    # sha-matched PMC pass (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE over the sampler kernels of the run)
    try:
        lds = {}
        for sd in (movies, users):
            ks = eng.kernel_resources(sd.side)
            for k in ks:
                k["lds_bytes_per_cu"] = k["lds_bytes_per_workgroup"] * k["workgroups_per_cu"]
                k["lds_occupancy"] = k["lds_bytes_per_cu"] / LDS_PER_CU
                k["waves_per_simd"] = k["workgroups_per_cu"] * k["threads_per_workgroup"] / 64.0 / 4.0
            lds[sd.name] = ks
        roofline["lds"] = {"per_side": lds, "lds_per_cu": LDS_PER_CU, "bank_conflict_rate": p_conflict if pmc_current else None,
                           "bank_conflict_rate_of_committed_profile": p_conflict}
    except Exception as e:
        roofline["lds"] = {"error": repr(e)[:200]}
    bpmf_env = {k: v for k, v in sorted(os.environ.items()) if k.startswith("BPMF_") and k != "BPMF_BENCH_SELF_LAUNCHED"}
    out = {
        "metric": METRIC,
        "value": (nusers + nmovies) * args.steps / dt,
        "unit": "samples/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": dtype,
        "data": "synthetic",
        "config": {"workload": (shape_note + ", K=%d, alpha=2, full Gibbs iteration of c++/bpmf.cpp:182-195: both half-iterations incl. host "
                                "Normal-Wishart draws, movies.predict(users)" + (" and users.predict(movies)" if both_predicts else
                                                                                 "; users.predict(movies) of c++/bpmf.cpp:190 is not run"))
                               % (nusers, nmovies, nnz + int(T[0][-1]), K),
                   "both_predicts": bool(both_predicts),
                   "name": wl, "nnz_train": nnz, "nnz_test": int(T[0][-1]), "K": K,
                   "parallelism": "columns of U and V sharded over %d GPU(s)" % world},
        "exchange_config": exchange_config,
        "rccl_nranks": rccl_nranks, "rccl_comm_streams": rccl_comm_streams, "launcher": "self" if os.environ.get("BPMF_BENCH_SELF_LAUNCHED") else ("external" if "WORLD_SIZE" in os.environ else "none"),
        "repeats": len(times), "timed_window_s": float(sum(times)), "prewarm_ms": prewarm_ms, "prewarm_extra_steps": extra,
        "ms_per_step_median": dt / args.steps * 1e3, "ms_per_step_min": min(times) / args.steps * 1e3,
        "ms_per_step_max": max(times) / args.steps * 1e3, "ms_per_step_first_block": times[0] / args.steps * 1e3,
        "roofline": roofline,
        # PCIe-inclusive figure: the hand-over of the host matrices (once per run) + N iterations at the measured rate, for the
        # reference's own default run length (`Sys::nsims = 20`, c++/bpmf.cpp:78) and for the 1 000 iterations a converged chain takes
        "handover": None if handover_ms is None else {
            "ms": handover_ms, "host_bytes": int(2 * (nnz * 12 + len(T[2]) * 12) + 8 * (nusers + nmovies + 2) * 2),
            "what": "bpmf_hip_side_create x 2 + test sets from host CSC arrays: PCIe upload, static schedule, initial factors",
            "value_incl_handover": {str(n): (nusers + nmovies) * n / (handover_ms * 1e-3 + n * dt / args.steps) for n in (20, 1000)}},
        "rmse": movies.rmse, "rmse_avg": movies.rmse_avg,
        # secondary figures of SURVEY 8(d): the reference's ratings/s (nnz / t_iter, bpmf.cpp:195) and
        # the sampling-only rate (columns of both sides / the two sampler launches of one iteration)
        "ratings_per_s": nnz * args.steps / dt,
        "sampling_only_samples_per_s": (nusers + nmovies) / (2.0 * launch_s) if (launch_s > 0 and world == 1) else None,
        # every BPMF_* variable of the environment this line was measured under (switches of the library included)
        "env": bpmf_env,
        # true iff the oracle has been diffed against dumps of the real reference build (oracle/build_ref.sh +
        # tests/test_oracle_vs_ref.py, which leaves the marker); false: "parity unpinned" 
        "oracle_pinned": os.path.exists(os.path.join(ROOT, "oracle", "_ref", "PINNED")),
        "full": bool(args.full),
    }
    if dumped is not None:
        out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
    if args.ablate is not None:
        out["ablate"] = args.ablate
        out["invalid"] = "BPMF_HIP_ABLATE=%d: phases of the sampler were skipped, the samples are wrong; a profiling run, not a throughput" % args.ablate
    if world > 1:
        out["per_rank"] = R.gather({"rank": rank, "device": local_rank, "columns": {"movs": dom_m[1] - dom_m[0], "users": dom_u[1] - dom_u[0]},
                                    "launch_ms_per_side": per_side, "hbm_frac": hbm_gbs / HBM_PEAK_GBS,
                                    "exchange_and_rest_ms": dt / args.steps * 1e3 - sum(per_side.values())})
    # "test RMSE vs reference": the default run of the reference (-i 20 -b 5, c++/bpmf.cpp:30-31; -i 6 -b 2 on the K >= 64 workloads,
    # whose CPU chain costs seconds per iteration) through the SAME pipelined stateful path that was just timed, from the
    # reference's start; compared below with the oracle's chain, which the cpu_baseline child computes on the same matrix
    gpu_chain, parity_cfg, parity_skip = None, ((20, 5) if K <= 32 else (6, 2)), None
    if world != 1:
        parity_skip = "N > 1: the chain parity of the sharded path is tests/test_gpu_multirank.py's; this object is the N = 1 record's"
    elif not args.full:
        parity_skip = "not run (a plain run times the headline only; bench.py --full runs the chain against the oracle's)"
    elif args.no_parity or args.no_cpu_baseline:
        parity_skip = "skipped (--no-parity / --no-cpu-baseline: no oracle chain to compare with)"
    elif args.ablate is not None:
        parity_skip = "skipped (--ablate: the samples are wrong by construction)"
    else:
        wd.stage("parity chain", wd.default + 60)
        try:
            t_par = time.perf_counter()
            movies.refresh(); users.refresh()
            res = bpmf_amd.gibbs(eng, M, Mt, T, nusers, nmovies, nsims=parity_cfg[0], burnin=parity_cfg[1], Tt=Tt if both_predicts else None,
                                 pipelined=True)
            gpu_chain = {k: res[k] for k in ("rmse", "rmse_avg", "norm_u", "norm_m", "final_rmse_avg", "num_predict", "U", "V")}
            gpu_chain["info"] = {"gpu_chain_s": time.perf_counter() - t_par,
                                 "kernel_per_side": {"movs": eng.kernel_name(res["movies"].side), "users": eng.kernel_name(res["users"].side)}}
            del res
        except Exception as e:
            parity_skip = "the chain through the timed pipeline failed: %r" % (e,)
    try:
        eng.close()                      # sides, collector threads, streams, (RCCL communicator)
    except Exception:
        pass
    del movies, users

    if args.full and not args.no_strong and wl == "ml1m":
        wd.stage("strong_10Mx1M record", wd.default + 120)
        try:
            out["strong_10Mx1M"] = strong_10Mx1M(R, args.strong_steps, args.strong_scale)
        except Exception as e:               # the headline must still be reported -- with the failure in it, not instead of it
            out["strong_10Mx1M"] = {"error": repr(e)[:400], "n_gpus": world}
            if world > 1:                    # (the other ranks may be inside a collective of the record: no further collective here)
                if rank == 0:
                    out["wall_s"] = time.perf_counter() - t_process
                    print(json.dumps(out), flush=True)
                sys.stdout.flush()
                os._exit(5 if rank == 0 else 0)
    if args.full and rank == 0 and world == 1 and wl == "ml1m" and not args.no_bpmf_exe:
        wd.stage("bpmf executable", 330)
        out["bpmf_exe"] = bpmf_exe_record(M, T, nusers, nmovies, K, nsims=400)      # (0.1 ms per iteration: a 25-iteration run is all start-up)
        if out["bpmf_exe"].get("steady_items_per_s"):
            out["bpmf_exe"]["over_python_host"] = out["bpmf_exe"]["steady_items_per_s"] / out["value"]
    # (a run without the CPU leg is a development / test run: no configs legs either -- their parity objects need the oracle's chain)
    if args.full and rank == 0 and world == 1 and wl == "ml1m" and not args.no_configs and not args.no_cpu_baseline and args.ablate is None:
        # every other single-GPU configuration of BASELINE.json in the SAME line: driver-timed, not builder-run
        out["configs"] = {}
        leg_limit = float(os.environ.get("BPMF_BENCH_CONFIG_LEG_TIMEOUT_S", "150"))
        for name, what in CONFIG_LEGS:
            wd.stage("configs leg '%s'" % name, leg_limit + 30)
            try:
                out["configs"][name] = config_leg(name, what, args.steps, args.warmup, leg_limit)
            except Exception as e:
                out["configs"][name] = {"what": what, "value": None, "error": repr(e)[:400]}
    if rank == 0:
        wd.stage("cpu baseline", 700)
        if args.full and not args.no_cpu_baseline and world == 1:
            try:
                out["cpu_baseline"] = cpu_baseline(M, Mt, T, Tt, K, nusers, nmovies, parity=parity_cfg if gpu_chain else None,
                                                   parity_only=args.cpu_parity_only)
            except Exception as e:  # the GPU number must still be reported
                out["cpu_baseline"] = {"value": None, "unit": "samples/s", "cores": os.cpu_count(), "kind": "port",
                                       "sample": "failed: %r" % (e,)}
                parity_skip = parity_skip or "the CPU leg failed: %r" % (e,)
        ref_chain = out.get("cpu_baseline", {}).pop("parity_ref", None) if isinstance(out.get("cpu_baseline"), dict) else None
        if gpu_chain is not None and ref_chain is not None:
            info = dict(gpu_chain.pop("info"), cpu_chain=out["cpu_baseline"].get("parity_chain"))
            out["parity"] = parity_record(gpu_chain, ref_chain, dtype, parity_cfg[0], parity_cfg[1], info)
        else:
            out["parity"] = {"value": None, "reason": parity_skip or "the CPU leg returned no chain",
                             "oracle_pinned": os.path.exists(os.path.join(ROOT, "oracle", "_ref", "PINNED"))}
        out["wall_s"] = time.perf_counter() - t_process
        print(json.dumps(out), flush=True)
    R.finish()


if __name__ == "__main__":
    main()
