"""The `bpmf` executable: the reference's command line and outputs (c++/bpmf.cpp) on the HIP path.
CPU part: usage / error exits (the conda recipe's test: no arguments => non-zero exit,
ci/conda-recipes/bpmf-0.2/run_test.sh:3-6).  GPU part: the reference's own two tests --
data/tiny/run_test.sh and the CTest run on MovieLens-100K (CMakeLists.txt:174-182) -- plus the
output files against the oracle."""
import os
import re
import subprocess

import numpy as np
import pytest

from bpmf_amd import io as bio
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
G = util.GOLDEN


def run(args, cwd):
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


def test_no_arguments_prints_usage_and_fails(tmp_path):
    r = run([], tmp_path)
    assert r.returncode != 0 and "Usage: bpmf -n <MTX> -p <MTX>" in r.stdout
    r = run(["-n", os.path.join(G, "tiny-train.mtx")], tmp_path)              # -p missing
    assert r.returncode != 0 and "Usage" in r.stdout
    r = run(["-x"], tmp_path)
    assert r.returncode != 0


def test_missing_file_and_bad_k(tmp_path):
    r = run(["-n", "nope.mtx", "-p", os.path.join(G, "tiny-test.mtx")], tmp_path)
    assert r.returncode != 0 and "File 'nope.mtx' not found" in r.stderr
    for bad in (["-d", "0"], ["-d", "129"], ["-d", "32", "--fp32"]):          # (every 1 .. 128 runs, in fp64; fp32 is for K > 64 and opt-in)
        r = run(["-n", os.path.join(G, "tiny-train.mtx"), "-p", os.path.join(G, "tiny-test.mtx")] + bad, tmp_path)
        assert r.returncode != 0 and "unsupported number of latent dimensions" in r.stderr, bad


@pytest.mark.gpu
def test_tiny_run_test_sh(oracle, tmp_path):
    """data/tiny/run_test.sh: bpmf -r -k -i 9 -b 0 -v -n train.mtx -p test.mtx -o output/ ; RMSE < 3."""
    (tmp_path / "output").mkdir()
    r = run(["-r", "-k", "-i", "9", "-b", "0", "-v", "-d", "8", "-n", os.path.join(G, "tiny-train.mtx"),
             "-p", os.path.join(G, "tiny-test.mtx"), "-o", "output/"], tmp_path)
    assert r.returncode == 0, r.stderr
    out = (tmp_path / "bpmf_0.out").read_text()
    final = float(re.search(r"Final Avg RMSE: (\S+)", out).group(1))
    assert final < 3.0
    M, Mt, T, Tt, nu, nm = util.tiny()
    ref = oracle.gibbs(8, M, Mt, T, Tt, nsims=9, burnin=0)
    assert abs(final - ref["final_rmse_avg"]) < 1e-4                          # printed with 6 significant digits
    lines = [l for l in out.splitlines() if "iteration" in l]
    assert len(lines) == 9 and lines[0].startswith("0: Sampling iteration 0:")
    rm = [float(re.search(r"\t RMSE: (\S+)", l).group(1)) for l in lines]
    assert np.allclose(rm, ref["rmse"], atol=1e-4)
    for needle in ("mean rating: 3.66667", "total number of ratings in train: 6", "num movs: 2", "num users: 4",
                   "num_latent: 8", "nsims: 9", "burnin: 0", "alpha: 2", "computed on 2 items (100% of total items in test set)"):
        assert needle in out, needle
    # -v: every sample; the last one equals the oracle's final factors (K x N column-major on disk)
    U8 = bio.read_dense(tmp_path / "output" / "U-8.ddm"); V8 = bio.read_dense(tmp_path / "output" / "V-8.ddm")
    assert U8.shape == (8, nu) and V8.shape == (8, nm)
    assert np.allclose(U8.T, ref["U"], rtol=1e-8, atol=1e-10) and np.allclose(V8.T, ref["V"], rtol=1e-8, atol=1e-10)
    # -o: predictions in the sparsity of the test matrix, posterior means of the 9 samples
    nr, nc, pavg = bio.read_sparse(tmp_path / "output" / "Pavg.sdm")
    assert (nr, nc) == (nu, nm) and np.array_equal(pavg[1], T[1]) and np.allclose(pavg[2], ref["Pavg"], rtol=1e-9)
    nr, nc, pm2 = bio.read_sparse(tmp_path / "output" / "Pm2.sdm")
    assert np.allclose(pm2[2], ref["Pm2"], rtol=1e-7, atol=1e-9)
    samples = np.stack([bio.read_dense(tmp_path / "output" / ("U-%d.ddm" % i)) for i in range(9)])
    assert np.allclose(bio.read_dense(tmp_path / "output" / "U-mu.ddm"), samples.mean(0), rtol=1e-10, atol=1e-12)
    lam = bio.read_dense(tmp_path / "output" / "U-Lambda.ddm")
    assert lam.shape == (64, nu)
    cov0 = np.cov(samples[:, :, 0].T)                                          # 9 samples of an 8-vector: invertible
    assert np.allclose(lam[:, 0].reshape(8, 8, order="F"), np.linalg.inv(cov0), rtol=1e-6, atol=1e-8)
    # ... and every column at the bar of tests/test_gpu_posterior_outputs.py: the .ddm files are binary, so neither the samples
    # nor Lambda lost a digit in print -- the error against the longdouble inverse may be 8 x that of numpy's fp64 inverse of
    # the one-pass covariance of the same samples (which scales with the condition number of this matrix; no constant does)
    from tests.test_gpu_posterior_outputs import LAMBDA_FACTOR, lambda_err, lambda_reference, lambda_restatement
    X = samples.transpose(0, 2, 1)                                             # [sample, column, K]
    mu_ref, lam_ref = lambda_reference(X)
    err, err_np = lambda_err(lam.T.reshape(nu, 8, 8).transpose(0, 2, 1), lam_ref), lambda_err(lambda_restatement(X)[1], lam_ref)
    print("bpmf -o U-Lambda.ddm: err %s, numpy's %s" % (err, err_np))
    assert np.all(err <= LAMBDA_FACTOR * err_np), (err, err_np)


@pytest.mark.gpu
@pytest.mark.parametrize("suffix", [".mtx.gz"])
def test_movielens_ctest(tmp_path, suffix):
    """CTest `bpmf_compressed`: ./bpmf -i 4 -n ml-train.mtx.gz -p ml-test.mtx.gz must exit 0."""
    r = run(["-i", "4", "-n", os.path.join(G, "ml100k-train" + suffix), "-p", os.path.join(G, "ml100k-test" + suffix)], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "num_latent: 32" in r.stdout and "total number of ratings in train: 80000" in r.stdout
    assert "mean rating: 3.52835" in r.stdout and "num movs: 1682" in r.stdout and "num users: 943" in r.stdout
    lines = [l for l in r.stdout.splitlines() if "iteration" in l]
    assert len(lines) == 4 and all("Burnin" in l for l in lines)
    assert abs(float(re.search(r"\t RMSE: (\S+)", lines[0]).group(1)) - 1.1537) < 2e-3
    assert re.search(r"Average items/sec: \S+", r.stdout) and re.search(r"Final Avg RMSE: 1\.15", r.stdout)


@pytest.mark.gpu
def test_propagated_posterior_workflow(hip_engine_factory, tmp_path):
    """The workflow -m / -l exist for (c++/bpmf.cpp:134-135): a first run writes U/V-mu.ddm and
    U/V-Lambda.ddm with -o, a second run takes them as per-column priors.  The second run's chain
    must be the one the library gives when the same Lambda matrices are set through the C ABI."""
    import bpmf_amd
    from bpmf_amd.sys import Sys
    K = 8
    train, test = os.path.join(G, "ml100k-train.mtx.gz"), os.path.join(G, "ml100k-test.mtx.gz")
    (tmp_path / "o1").mkdir()
    r = run(["-i", "14", "-b", "2", "-d", str(K), "-n", train, "-p", test, "-o", "o1/"], tmp_path)
    assert r.returncode == 0, r.stderr
    lam_u = bio.read_dense(tmp_path / "o1" / "U-Lambda.ddm"); lam_v = bio.read_dense(tmp_path / "o1" / "V-Lambda.ddm")
    assert np.all(np.isfinite(lam_u)) and np.all(np.isfinite(lam_v))
    r = run(["-i", "5", "-b", "1", "-d", str(K), "-n", train, "-p", test,
             "-m", "o1/V-mu.ddm,o1/V-Lambda.ddm", "-l", "o1/U-mu.ddm,o1/U-Lambda.ddm"], tmp_path)
    assert r.returncode == 0, r.stderr
    final = float(re.search(r"Final Avg RMSE: (\S+)", r.stdout).group(1))
    # the same through the Python mirror
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)
    Sys.nsims, Sys.burnin, Sys.alpha = 5, 1, 2.0
    movies = Sys("movs", eng, M, nm, nu, T=T); users = Sys("users", eng, Mt, nu, nm)
    eng.set_prop_posterior(movies.side, lam_v.T); eng.set_prop_posterior(users.side, lam_u.T)
    for _ in range(5):
        movies.sample(users); users.sample(movies); movies.predict(users)
    movies.predict(users, True)
    assert abs(final - movies.rmse_avg) < 1e-4
    # malformed argument / wrong shape
    r = run(["-i", "1", "-d", str(K), "-n", train, "-p", test, "-m", "o1/V-mu.ddm"], tmp_path)
    assert r.returncode != 0 and "MU_FILE,LAMBDA_FILE" in r.stderr
    r = run(["-i", "1", "-d", str(K), "-n", train, "-p", test, "-m", "o1/U-mu.ddm,o1/U-Lambda.ddm"], tmp_path)
    assert r.returncode != 0 and "expected" in r.stderr


@pytest.mark.gpu
def test_d128_is_fp64_and_fp32_is_an_explicit_opt_in(oracle, tmp_path):
    """-d 128 means what it means in the reference (`bpmf-128` of ci/multilatent.sh:5: fp64, c++/bpmf.h:55-58): the chain of
    the oracle to the printed digits.  --fp32 / BPMF_HIP_F32=1 select the mixed-precision path and say so on stdout."""
    args = ["-i", "4", "-b", "1", "-d", "128", "-n", os.path.join(G, "ml100k-train.mtx.gz"), "-p", os.path.join(G, "ml100k-test.mtx.gz")]
    r = run(args, tmp_path)
    assert r.returncode == 0, r.stderr
    assert "num_latent: 128" in r.stdout and "fp32" not in r.stdout
    M, Mt, T, Tt, nu, nm = util.ml100k()
    ref = oracle.gibbs(128, M, Mt, T, Tt, nsims=4, burnin=1, nthreads=8)
    pick = lambda text: [float(m.group(1)) for m in re.finditer(r"\t RMSE: (\S+)", text)]
    assert np.allclose(pick(r.stdout), ref["rmse"], atol=1e-4)                # (4 printed decimals)
    assert abs(float(re.search(r"Final Avg RMSE: (\S+)", r.stdout).group(1)) - ref["final_rmse_avg"]) < 1e-5
    for extra, env in ((["--fp32"], {}), ([], {"BPMF_HIP_F32": "1"})):
        r32 = subprocess.run([BPMF] + args + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=dict(os.environ, **env))
        assert r32.returncode == 0, r32.stderr
        assert "arithmetic: fp32" in r32.stdout
        assert np.allclose(pick(r32.stdout), ref["rmse"], atol=2e-3)          # the fp32 study's tolerance (tests/test_gpu_f32.py)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [10, 100])
def test_d_any_num_latent_of_the_reference_builds(oracle, tmp_path, K):
    """ci/multilatent.sh:5 ships bpmf-10 ... bpmf-100; BASELINE.md's "industrial" run is K = 100.  `bpmf -d K` runs them on
    the next instantiated kernel size, with the RNG streams and the sizes of every output taken from the true K: RMSE lines and
    the -o / -v files against the oracle at that K."""
    (tmp_path / "o").mkdir()
    r = run(["-i", "5", "-b", "2", "-d", str(K), "-v", "-o", "o/", "-n", os.path.join(G, "ml100k-train.mtx.gz"), "-p", os.path.join(G, "ml100k-test.mtx.gz")], tmp_path)
    assert r.returncode == 0, r.stderr
    assert ("num_latent: %d" % K) in r.stdout and "padded dimensions" in r.stdout
    M, Mt, T, Tt, nu, nm = util.ml100k()
    ref = oracle.gibbs(K, M, Mt, T, Tt, nsims=5, burnin=2, nthreads=8)
    pick = lambda text: [float(m.group(1)) for m in re.finditer(r"\t RMSE: (\S+)", text)]
    assert np.allclose(pick(r.stdout), ref["rmse"], atol=1e-4)
    assert abs(float(re.search(r"Final Avg RMSE: (\S+)", r.stdout).group(1)) - ref["final_rmse_avg"]) < 1e-5
    U = bio.read_dense(tmp_path / "o" / "U-4.ddm"); V = bio.read_dense(tmp_path / "o" / "V-4.ddm")
    assert U.shape == (K, nu) and V.shape == (K, nm)
    assert np.allclose(U.T, ref["U"], rtol=1e-7, atol=1e-9) and np.allclose(V.T, ref["V"], rtol=1e-7, atol=1e-9)
    samples = np.stack([bio.read_dense(tmp_path / "o" / ("U-%d.ddm" % i)) for i in range(2, 5)])
    assert np.allclose(bio.read_dense(tmp_path / "o" / "U-mu.ddm"), samples.mean(0), rtol=1e-10, atol=1e-12)
    assert bio.read_dense(tmp_path / "o" / "U-Lambda.ddm").shape == (K * K, nu)
    assert np.allclose(bio.read_sparse(tmp_path / "o" / "Pavg.sdm")[2][2], ref["Pavg"], rtol=1e-8)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 128])
def test_g1_runs_the_sharded_path_and_equals_the_plain_run(tmp_path, K):
    """bpmf -g N: the reference's `mpirun -np N bpmf` (c++/bpmf.cpp:111-117) as N rank threads in one process, RCCL id
    shared in memory.  -g 1 drives everything but a second GPU -- communicator, ranges, the sharded sys_sample /
    predict with their all-reduces, per-rank bpmf_<rank>.out -- and must print the chain of the plain run.
    The ADVICE finding of round 1: nprocs was hard-wired to 1 and the sharded path unreachable from the CLI."""
    args = ["-i", "6", "-b", "2", "-d", str(K), "-n", os.path.join(G, "ml100k-train.mtx.gz"), "-p", os.path.join(G, "ml100k-test.mtx.gz")]
    # (one run each, with -o: the stdout chain AND the output files of the same two runs are compared)
    (tmp_path / "o_plain").mkdir(); (tmp_path / "o_g1").mkdir(); (tmp_path / "g").mkdir()
    plain = run(args + ["-o", "o_plain/"], tmp_path)
    assert plain.returncode == 0, plain.stderr
    sharded = run(args + ["-g", "1", "-r", "-o", "../o_g1/"], tmp_path / "g")
    assert sharded.returncode == 0, sharded.stderr
    out = (tmp_path / "g" / "bpmf_0.out").read_text()
    assert "nprocs: 1" in out and "movs domain: [0, 1682)" in out
    pick = lambda text: [(m.group(1), m.group(2)) for m in re.finditer(r"\t RMSE: (\S+)\tavg RMSE: (\S+)", text)]
    assert len(pick(out)) == 6 and pick(out) == pick(plain.stdout)
    assert re.search(r"Final Avg RMSE: (\S+)", out).group(1) == re.search(r"Final Avg RMSE: (\S+)", plain.stdout).group(1)
    # with outputs: Pavg / U-mu of the sharded run equal the plain run's
    a = bio.read_sparse(tmp_path / "o_plain" / "Pavg.sdm"); b = bio.read_sparse(tmp_path / "o_g1" / "Pavg.sdm")
    assert np.array_equal(a[2][2], b[2][2])
    assert np.array_equal(bio.read_dense(tmp_path / "o_plain" / "U-mu.ddm"), bio.read_dense(tmp_path / "o_g1" / "U-mu.ddm"))


def test_more_gpus_than_devices_fails_cleanly(tmp_path):
    """-g 2 on a box without two GPUs (here: none): an error message, not a hang or a crash."""
    r = run(["-i", "1", "-g", "2", "-n", os.path.join(G, "tiny-train.mtx"), "-p", os.path.join(G, "tiny-test.mtx")], tmp_path)
    assert r.returncode != 0 and "bpmf:" in r.stderr


@pytest.mark.gpu
def test_bpmf_reduce_env_runs_the_reduce_build(tmp_path):
    """BPMF_REDUCE=1: the reference's BPMF_REDUCE build (c++/bpmf.h:30-42, sample.cpp:289-291) as a run-time switch of
    `bpmf`; its chain equals the default one up to the order of the floating-point sums (RMSE printed with 5 digits),
    also over the one-rank communicator of -g 1 (grouped ncclReduce onto the owner)."""
    args = ["-i", "6", "-b", "2", "-n", os.path.join(G, "ml100k-train.mtx.gz"), "-p", os.path.join(G, "ml100k-test.mtx.gz")]
    plain = run(args, tmp_path)
    assert plain.returncode == 0, plain.stderr
    pick = lambda text: [(float(m.group(1)), float(m.group(2))) for m in re.finditer(r"\t RMSE: (\S+)\tavg RMSE: (\S+)", text)]
    env = dict(os.environ, BPMF_REDUCE="1")
    for extra in ([], ["-g", "1"]):
        r = subprocess.run([BPMF] + args + extra, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr
        got, want = pick(r.stdout), pick(plain.stdout)
        assert len(got) == 6 and np.allclose(got, want, atol=2e-4), (got, want)


@pytest.mark.gpu
def test_cpp_host_keeps_up_with_the_python_host():
    """north_star: "C++ host code calls through a thin C-ABI".  bench.py's `bpmf_exe` sub-record runs the `bpmf` executable on the
    very matrices of the timed Python loop (written as .sdm) and parses its own `Average items/sec` / `Final Avg RMSE`
    (c++/bpmf.cpp:246-252): the steady-state rate of the C++ host must be within 10 % of the Python host's (round 4 found it
    17 % behind: a bpmf_hip_sys_state per iteration drained the pipeline; bpmf_hip_sys_norm does not)."""
    import json
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "200", "--warmup", "20", "--repeats", "5", "--no-strong", "--no-cpu-baseline"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"metric"')][-1])
    x = j["bpmf_exe"]
    assert "error" not in x, x
    assert x["iterations"] == 400 and 0.5 < x["final_avg_rmse"] < 3.0          # (bpmf -i 400 whatever --steps says: a short run is all start-up)
    h = j["handover"]                                                   # the host matrices' one-time hand-over, beside the value and never in it
    assert 0.5 < h["ms"] < 500 and h["host_bytes"] > 2 * 12 * 1_000_000 and h["value_incl_handover"]["20"] < h["value_incl_handover"]["1000"] < j["value"]
    assert 0.85 <= x["over_python_host"] <= 1.25, x                     # (clean runs: 1.01 - 1.05, profiles/r05_bench*.json; inside a busy suite run 0.90 was seen)
