"""The library's OWN multi-rank path with nranks >= 2 on the one GPU there is.

RCCL refuses two ranks per device, so the ranks load the tests' RCCL double (tests/rccl_double: the nccl* entry points
for processes / threads that share a GPU, a shared-memory rendez-vous underneath) through BPMF_HIP_RCCL_LIBRARY.
Everything above those entry points is the product: bpmf_hip_ctx_comm_init, the ranges, the mesh all-gather-v of
launch_impl.h (never executed with a peer before round 3), parts, the second communicator, the connectivity-aware
lists, BPMF_REDUCE's grouped reduce, the fp32 context, `bpmf -g 2` and `bench.py --gpus 2`.  Reference behaviour being
matched: c++/mpi_isendirecv.h:222-260 (items travel while others are sampled), c++/mpi_common.h:44-50 (all-reduce of
the sums), c++/mpi_reduce.h:24-47.  Every run is compared with the ORACLE's single-process chain: the samples do not
depend on the rank count beyond the order of the all-reduced sums."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

DOUBLE = os.path.join(ROOT, "tests", "rccl_double", "librccl_double.so")


@pytest.fixture(params=["sync", "async"], autouse=True)
def double_mode(request, monkeypatch):
    """Every test of this module twice: with the double completing an operation before the call returns, and with its
    ASYNCHRONOUS mode (BPMF_RCCL_DOUBLE_ASYNC=1): calls only enqueue, a gate kernel holds the operation's stream the way
    an NCCL kernel does, a helper thread per communicator completes the operations after random, rank-dependent delays --
    so that the two communicators and the exchange stream of a rank interleave differently from its peers' (VERDICT r3:
    what the synchronous double serialises away).  Same assertions in both modes."""
    if request.param == "async":
        monkeypatch.setenv("BPMF_RCCL_DOUBLE_ASYNC", "1")
        # The double's helper threads move the data with HIP copies on streams of their own, and HIP maps the streams of a
        # process onto 4 hardware queues by default: a helper's copy can land in the queue of a stream that a LATER gate
        # kernel holds, which only that helper can release -- a deadlock of the double's making (RCCL's kernels move their
        # data themselves).  One hardware queue per stream for these runs.
        monkeypatch.setenv("GPU_MAX_HW_QUEUES", "24")
    else:
        monkeypatch.delenv("BPMF_RCCL_DOUBLE_ASYNC", raising=False)
    return request.param


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def run_ranks(tmp_path, nranks, case, dataset, K, nsims, burnin, env_extra=None):
    assert os.path.exists(DOUBLE), "tests/rccl_double/librccl_double.so is missing: __graft_entry__.build() makes it"
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / ("res_%s" % case))
    procs = []
    for rank in range(nranks):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(nranks), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   BPMF_HIP_RCCL_LIBRARY=DOUBLE, BPMF_RCCL_DOUBLE_TIMEOUT_S="40")
        env.update(env_extra or {})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_mr_worker.py"), case, dataset, str(K), str(nsims),
                                       str(burnin), out], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    errs = []
    for p in procs:
        try:
            so, se = p.communicate(timeout=420)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        errs.append((p.returncode, so[-500:], se[-3000:]))
    for rc, so, se in errs:
        assert rc == 0 and "MR-OK" in so, (so, se)
    return [np.load(out + ".rank%d.npz" % r) for r in range(nranks)]


def check_against_oracle(oracle, res, dataset, K, nsims, burnin, tol=1e-7, owned_only=False):
    data = {"ml100k": util.ml100k, "blocks": util.blocks, "heavy": lambda: util.synthetic(700, 500, 30000, seed=3, heavy=(7, 650))}[dataset]
    M, Mt, T, Tt, nu, nm = data()
    ref = oracle.gibbs(K, M, Mt, T, Tt, nsims=nsims, burnin=burnin)
    for r in res:
        assert int(r["nranks"]) == len(res)
        assert np.allclose(r["rmse"], ref["rmse"], atol=tol) and np.allclose(r["rmse_avg"], ref["rmse_avg"], atol=tol)
        assert np.allclose(r["norm_u"], ref["norm_u"], rtol=10 * tol) and np.allclose(r["norm_m"], ref["norm_m"], rtol=10 * tol)
        if owned_only:
            for X, Xref, dom in ((r["U"], ref["U"], r["dom_u"]), (r["V"], ref["V"], r["dom_m"])):
                assert rel_err(X[dom[0]:dom[1]], Xref[dom[0]:dom[1]]) < tol
        else:
            assert rel_err(r["U"], ref["U"]) < tol and rel_err(r["V"], ref["V"]) < tol
            assert np.array_equal(r["U"], res[0]["U"]) and np.array_equal(r["V"], res[0]["V"])       # every replica holds the same bits
    return ref


@pytest.mark.parametrize("nranks,K,env", [
    (2, 32, {}),                                           # the default: mesh of grouped send / recv, second communicator
    (3, 16, {}),                                           # three uneven ranges
    (2, 32, {"BPMF_HIP_EXCHANGE": "bcast"}),              # one broadcast per owner
    (2, 32, {"BPMF_HIP_COMM_STREAMS": "1"}),              # one communicator: statistics all-reduce on the main stream
    (2, 64, {}),                                           # slab form, unfused (sharded) launch
])
def test_mesh_exchange_between_two_ranks(oracle, tmp_path, nranks, K, env, double_mode):
    nsims, burnin = 4, 1
    res = run_ranks(tmp_path, nranks, "mesh", "ml100k", K, nsims, burnin, env)
    check_against_oracle(oracle, res, "ml100k", K, nsims, burnin)


@pytest.mark.parametrize("nranks,parts", [(2, 2), (2, 4), (3, 3)])
def test_parts_overlap_between_ranks(oracle, tmp_path, nranks, parts, double_mode):
    """bpmf_hip_side_set_overlap with a peer: the per-part sub-ranges of every rank are all-gathered once, part c travels
    on the exchange stream while part c + 1 is sampled; `heavy`: a 650-rating column that is cut into chunks."""
    nsims, burnin = 4, 1
    res = run_ranks(tmp_path, nranks, "parts", "heavy", 32, nsims, burnin, {"BPMF_HIP_OVERLAP": str(parts)})
    check_against_oracle(oracle, res, "heavy", 32, nsims, burnin)


def test_auto_overlap_decision_is_rank_invariant(oracle, tmp_path):
    """the automatic switch to parts must be taken from data every rank holds (a rank-local width near the
    threshold made some ranks enter the collective set_overlap and others not: a hang).  Threshold lowered so that the
    narrowest-range rule flips on for ml100k's users (3 uneven ranges) and stays off for its movies."""
    nsims, burnin = 3, 1
    res = run_ranks(tmp_path, 3, "auto", "ml100k", 16, nsims, burnin, {"BPMF_HIP_OVERLAP_MIN_KB": "100"})
    check_against_oracle(oracle, res, "ml100k", 16, nsims, burnin)


@pytest.mark.parametrize("parts", [1, 3])
def test_connectivity_lists_between_ranks(oracle, tmp_path, parts):
    """k_pack_cols -> grouped send / recv per peer -> k_unpack_cols between DIFFERENT ranks (c++/assign.cpp:204-241).
    parts = 3 (round 6): the side is ALSO sampled in three parts -- the packed lists are not cut, they must travel behind the
    last part (until round 6 they went with part 0: the peers received the previous iteration's columns of parts 1, 2)."""
    nsims, burnin = 4, 1
    res = run_ranks(tmp_path, 2, "conn", "blocks", 32, nsims, burnin, {"BPMF_HIP_OVERLAP": str(parts)} if parts > 1 else None)
    for r in res:
        assert r["conn_used"].all()
    check_against_oracle(oracle, res, "blocks", 32, nsims, burnin, owned_only=True)


def test_fp32_context_between_ranks(tmp_path, hip_engine_factory):
    """K = 128 fp32 sharded over two ranks == the same context on one rank, up to the order of the all-reduced sums."""
    import bpmf_amd
    nsims, burnin = 3, 1
    res = run_ranks(tmp_path, 2, "f32", "ml100k", 128, nsims, burnin)
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = bpmf_amd.HipEngine(128, dtype="f32")
    one = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin)
    for r in res:
        assert np.allclose(r["rmse"], one["rmse"], atol=1e-4)
        assert rel_err(r["U"], one["U"]) < 2e-3 and rel_err(r["V"], one["V"]) < 2e-3
        assert np.array_equal(r["U"], res[0]["U"])
    eng.close()


@pytest.mark.parametrize("K", [16, 64])
def test_reduce_formulation_between_ranks(oracle, tmp_path, K):
    """BPMF_REDUCE with two ranks: every rank precomputes the parts of ALL columns of the other side from its own fresh
    columns, the grouped ncclReduce sums them onto the owners (c++/mpi_reduce.h:24-47): against the oracle's restatement
    of that build with two simulated ranks and the same ranges."""
    from bpmf_amd import synth
    nsims, burnin = 3, 1
    res = run_ranks(tmp_path, 2, "reduce", "heavy", K, nsims, burnin)
    M, Mt, T, Tt, nu, nm = util.synthetic(700, 500, 30000, seed=3, heavy=(7, 650))
    bm, bu = synth.balanced_ranges(M[0], 2), synth.balanced_ranges(Mt[0], 2)
    ref = oracle.gibbs_reduce(K, M, Mt, T, alpha=2.0, nsims=nsims, burnin=burnin, bounds_m=bm, bounds_u=bu)
    for r in res:
        assert int(r["dom_m"][0]) in bm and int(r["dom_u"][0]) in bu
        assert rel_err(r["U"], ref["U"]) < 1e-8 and rel_err(r["V"], ref["V"]) < 1e-8
        assert np.allclose(r["rmse"], ref["rmse"], atol=1e-9)
        assert np.array_equal(r["U"], res[0]["U"]) and np.array_equal(r["V"], res[0]["V"])


@pytest.mark.parametrize("k,parts,tol", [(2, 3, 1e-2), (1, 2, 6e-2)])
def test_bounded_staleness_exchange_is_a_mild_relaxation(oracle, tmp_path, k, parts, tol):
    """SURVEY 8 f4, third variant (c++/bpmf_gaspi.h:91-104 send throttling, c++/mpi_allreduce.h:134-175 stale blocks):
    BPMF_HIP_STALE=k lets a part of a side travel every (k + 1)-th half-iteration only.  Property test, as the reference's
    own relaxations have no exact answer: the chain still converges -- final averaged RMSE of a 40-iteration run on
    MovieLens-100K (20 burn-in) close to the exact chain's 0.9397 (measured: 0.9415 with k = 2 over three parts, 0.980
    with k = 1 over two: staleness costs accuracy per iteration, as the reference's authors found) and far below the
    mean predictor's 1.1537 -- it is a different chain (the switch did something), and after the closing full
    exchange every replica holds the same bits."""
    nsims, burnin, K = 40, 20, 16
    res = run_ranks(tmp_path, 2, "stale", "ml100k", K, nsims, burnin, {"BPMF_HIP_STALE": str(k), "BPMF_HIP_OVERLAP": str(parts)})
    M, Mt, T, Tt, nu, nm = util.ml100k()
    ref = oracle.gibbs(K, M, Mt, T, Tt, nsims=nsims, burnin=burnin)
    for r in res:
        assert abs(float(r["final"]) - ref["final_rmse_avg"]) < tol
        assert float(r["final"]) < 1.0
        assert rel_err(r["U"], ref["U"]) > 1e-6                     # not the exact chain
        assert np.array_equal(r["U"], res[0]["U"]) and np.array_equal(r["V"], res[0]["V"])
    # k = 0 through the same switch is the exact chain
    res0 = run_ranks(tmp_path, 2, "stale0", "ml100k", K, 4, 1, {"BPMF_HIP_STALE": "0", "BPMF_HIP_OVERLAP": str(parts)})
    check_against_oracle(oracle, res0, "ml100k", K, 4, 1)


@pytest.mark.parametrize("k,parts", [(1, 2), (2, 3), (1, 1)])
def test_bounded_staleness_replica_age(tmp_path, k, parts):
    """the bound itself, observed.  After every iteration each rank's replica of a PEER's column must equal
    the value the owner held after one of its last k + 1 half-iterations of that side (k = 1, two parts: with two factor
    copies a skipped part fell back to what the other copy held -- zeros or the initial upload, for the whole run); own
    columns are always current; and the first half-iteration of a side exchanges everything."""
    nsims, K = 9, 16
    res = run_ranks(tmp_path, 2, "stale_age", "ml100k", K, nsims, 2, {"BPMF_TEST_STALE_K": str(k), "BPMF_HIP_OVERLAP": str(parts)})
    for name, dom in (("snaps_u", "dom_u"), ("snaps_v", "dom_m")):
        own = {}
        for r in res:                                               # the owner's history of its own range
            lo, hi = int(r[dom][0]), int(r[dom][1])
            own[(lo, hi)] = r[name][:, lo:hi]
        for r in res:
            mine = (int(r[dom][0]), int(r[dom][1]))
            for (lo, hi), hist in own.items():
                rep = r[name][:, lo:hi]
                if (lo, hi) == mine:
                    continue
                assert np.array_equal(rep[0], hist[0]), "%s: the first half-iteration must exchange every part" % name
                stale_seen = False
                for it in range(nsims):
                    # every column equals the owner's value of iteration it, it - 1, ... or it - k
                    ok = np.zeros(hi - lo, bool)
                    for back in range(0, k + 1):
                        if it - back >= 0:
                            ok |= (rep[it] == hist[it - back]).all(axis=1)
                    assert ok.all(), "%s: iteration %d: %d column(s) of a peer's range are older than k = %d half-iterations" % (name, it, int((~ok).sum()), k)
                    stale_seen = stale_seen or not np.array_equal(rep[it], hist[it])
                assert stale_seen, "k = %d did not skip any exchange" % k


def test_bpmf_g2_rank_threads_share_the_gpu(tmp_path):
    """`bpmf -g 2`: two rank THREADS of one process, both on device 0 (BPMF_HIP_DEVICES=0,0), the double as the
    communication library.  With BPMF_ASSIGN=contiguous the column ids -- hence the RNG streams -- are those of the
    single-GPU run: every sample, Pavg / Pm2 and the posterior files must agree with plain `bpmf` up to the order of the
    all-reduced sums; both rank logs carry the same RMSE lines and `nprocs: 2`."""
    from bpmf_amd import io as bio
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    train, test = os.path.join(util.GOLDEN, "ml100k-train.mtx.gz"), os.path.join(util.GOLDEN, "ml100k-test.mtx.gz")
    runs = {}
    for name, extra_args, extra_env in (("plain", [], {}), ("g2", ["-g", "2"], {"BPMF_HIP_DEVICES": "0,0", "BPMF_HIP_RCCL_LIBRARY": DOUBLE,
                                                                                 "BPMF_ASSIGN": "contiguous"})):
        d = tmp_path / name
        (d / "out").mkdir(parents=True)
        r = subprocess.run([exe, "-n", train, "-p", test, "-i", "6", "-b", "2", "-d", "16", "-v", "-o", str(d / "out")] + extra_args,
                           cwd=str(d), env=dict(os.environ, **extra_env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        runs[name] = d
        if name == "plain":
            plain_stdout = r.stdout
    log0, log1 = open(runs["g2"] / "bpmf_0.out").read(), open(runs["g2"] / "bpmf_1.out").read()
    assert "nprocs: 2" in log0 and "nprocs: 2" in log1
    import re
    pick = lambda text: re.findall(r"RMSE: ([0-9.]+)\s+avg RMSE: ([0-9.]+)", text)
    assert pick(log0) == pick(log1) and len(pick(log0)) == 6
    assert pick(log0) == pick(plain_stdout)                          # (4 printed decimals)
    for f in ["U-%d.ddm" % i for i in range(6)] + ["V-%d.ddm" % i for i in range(6)] + ["U-mu.ddm", "V-mu.ddm"]:
        a = bio.read_dense(str(runs["plain"] / "out" / f)); b = bio.read_dense(str(runs["g2"] / "out" / f))
        assert a.shape == b.shape and rel_err(b, a) < 1e-8, f
    a = bio.read_sparse(str(runs["plain"] / "out" / "Pavg.sdm"))[2]; b = bio.read_sparse(str(runs["g2"] / "out" / "Pavg.sdm"))[2]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.allclose(a[2], b[2], atol=1e-8)


def test_bench_self_launches_two_ranks_on_the_shared_gpu():
    """bench.py --gpus 2 without a launcher: it starts the two ranks itself; on this one-GPU box that is only allowed in
    the declared test set-up (BPMF_BENCH_SHARED_GPU=1 + the double); the line says n_gpus 2, rccl_nranks 2."""
    env = dict(os.environ, BPMF_BENCH_SHARED_GPU="1", BPMF_HIP_RCCL_LIBRARY=DOUBLE, BPMF_BENCH_STRONG_SCALE="0.01")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "4", "--warmup", "1", "--repeats", "1",
                        "--prewarm-ms", "0", "--prewarm-steps", "0", "--strong-steps", "8"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1200)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"metric"')][-1])
    assert j["n_gpus"] == 2 and j["rccl_nranks"] == 2 and j["launcher"] == "self" and len(j["per_rank"]) == 2
    assert j["env"].get("BPMF_BENCH_SHARED_GPU") == "1"
    s = j["strong_10Mx1M"]
    assert s["n_gpus"] == 2 and s["rccl_nranks"] == 2 and s["spot_check"]["ok"], s
    # (the chain's independence of N: test_mesh_exchange_between_two_ranks / tests/test_gpu_ranks8.py against the oracle's single-process chain)


def test_bench_refuses_more_ranks_than_devices():
    """`bench.py --gpus 2` on a one-GPU box exits non-zero with a clear message instead of printing n_gpus: 1."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two devices present")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BPMF_BENCH_SHARED_GPU"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "0"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode != 0 and "--gpus 2" in r.stderr and "device" in r.stderr
    assert '{"metric"' not in r.stdout


def test_bench_refuses_ablate_in_the_environment():
    env = dict(os.environ, BPMF_HIP_ABLATE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "0", "--no-strong", "--no-cpu-baseline"], cwd=ROOT,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode != 0 and "BPMF_HIP_ABLATE" in r.stderr and '{"metric"' not in r.stdout


def _bench_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith('{"metric"')]
    return json.loads(lines[-1]) if lines else None


def test_bench_stalled_rank_is_an_error_record_not_a_hang(double_mode):
    """a rank that stalls (BPMF_HIP_TEST_STALL_RANK: rank 1 sleeps 40 s before it enqueues iteration 3
    of a side) must not cost the lease: its peer's host-side wait on the stream that carries the collective is bounded
    (BPMF_HIP_COMM_TIMEOUT_MS), the communicators are aborted, and bench.py prints a line with "error" and exits non-zero
    -- inside the time the stall lasts, not after it."""
    import time
    env = dict(os.environ, BPMF_BENCH_SHARED_GPU="1", BPMF_HIP_RCCL_LIBRARY=DOUBLE, BPMF_HIP_TEST_STALL_RANK="1:40000:3",
               BPMF_HIP_COMM_TIMEOUT_MS="4000", BPMF_RCCL_DOUBLE_TIMEOUT_S="8", BPMF_BENCH_PREFLIGHT="0", BPMF_BENCH_WATCHDOG_S="60")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "8", "--warmup", "0", "--repeats", "1", "--prewarm-ms", "0", "--prewarm-steps", "0",
                        "--no-strong"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    took = time.time() - t0
    j = _bench_line(r.stdout)
    assert r.returncode != 0 and j is not None and j["value"] is None and j.get("error"), (r.returncode, r.stdout[-800:], r.stderr[-2000:])
    assert took < 38, "the error must come from the bounded wait, not from the end of the stall (%.1f s)" % took
    assert "timed out" in j["error"] or "watchdog" in j["error"] or "exited" in j["error"] or "waited for its peers" in r.stderr, j["error"]


# (The 2-rank version of "a rank's trial of the first rung hangs -> killed -> the ranks agree -> the second rung runs" lived here until
#  round 6; tests/test_gpu_ranks8.py::test_bench_gpus8_preflight_ladder_and_per_rank_record is the same scenario with eight ranks.)


def test_bench_under_the_drivers_launcher(double_mode):
    """The way the driver starts N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...` (here N = 2 on the shared GPU with the double).  The preflight children must find
    their own rendez-vous (not the elastic agent's store), and the line must say launcher: external, n_gpus 2, the exchange
    configuration that was chosen, and carry the strong-scaling record with its model."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, BPMF_BENCH_SHARED_GPU="1", BPMF_HIP_RCCL_LIBRARY=DOUBLE, BPMF_BENCH_STRONG_SCALE="0.01", BPMF_RCCL_DOUBLE_TIMEOUT_S="40")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "4", "--warmup", "1", "--repeats", "1", "--prewarm-ms", "0", "--prewarm-steps", "0",
                        "--strong-steps", "8"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    j = _bench_line(r.stdout)
    assert r.returncode == 0 and j is not None and j["value"] and not j.get("error"), (r.stdout[-800:], r.stderr[-3000:])
    assert j["n_gpus"] == 2 and j["rccl_nranks"] == 2 and j["launcher"] == "external"
    assert j["exchange_config"]["chosen"] == "mesh+parts+2comms" and j["exchange_config"]["ladder"][0]["ok"]
    st = j["strong_10Mx1M"]
    assert st["n_gpus"] == 2 and st["spot_check"]["ok"] and set(st["model"]["per_n"]) == {"1", "2", "4", "8"}
