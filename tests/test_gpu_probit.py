"""Probit likelihood (`gibbs(..., probit=True)`, `bpmf --probit`) on the GPU.

  * the latent draw (k_probit_latent) against the CPU restatement of tests/probit_ref.py, every rating: K = 8, 10, 16, 32, 64, 100,
    128 fp64 and 128 fp32 on a matrix with a 50 000-rating column, empty columns and a side of 1-2 ratings per column;
    bit-identical between two calls and between BPMF_HIP_DBUF=0/1; the ratings themselves are never written
  * one half-iteration through each sampler family with the latent scores in place of the ratings, against oracle.sample_side fed
    the restatement's scores
  * the coupled chain against the restated chain (K = 32, 64; pipelined and plain loop; K = 32 with BPMF_HIP_FUSED=0): factors,
    traces, prob, auc
  * probit_add / probit_get against numpy
  * recovery of a planted rank-4 probit model (AUC against the restatement's recorded value and the ceiling of the true model)
  * `bpmf --probit` end to end, and a guard that a probit run leaves nothing behind in the fixed path

tests/test_probit_host.py asserts on the CPU that no accept / reject decision of the restatement is within 1e-9 of its threshold
for the inputs of the first test: a mismatch here is never a flipped branch.
"""
import csv
import os
import re
import subprocess

import numpy as np
import pytest

from tests import probit_ref as ref
from tests import util
from tests.conftest import ROOT
from tests.test_gpu_parity import RTOL, rel_err

pytestmark = pytest.mark.gpu

NT = ref.NT


def _hyper(K, ncols, it, seed):
    import bpmf_amd
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, 3 * K))
    return bpmf_amd.engine.hyper_sample(K, ncols, A @ A.T / (3 * K), it)


def _pair(eng, A, nrows, X, Y, threshold, tag):
    """A probit side over the ratings A holding the factors X, and a partner without ratings holding Y."""
    ncols = len(A[0]) - 1
    me = eng.side_create(ncols, nrows, *A, 0.0)
    ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_probit(me, threshold, tag)
    eng.set_items(me, X)
    eng.set_items(ot, Y)
    return me, ot


@pytest.mark.parametrize("K,dtype", ref.LATENT_CASES)
def test_latent_against_restatement(K, dtype):
    import bpmf_amd
    M, Mt, nu, nm = ref.skewed()
    U, V = ref.latent_factors(K, dtype, nu, nm)
    it, thr = ref.LATENT_ITER, ref.LATENT_THRESHOLD
    old = os.environ.get("BPMF_HIP_DBUF")
    eng = bpmf_amd.HipEngine(K, dtype=dtype)
    try:
        for A, nrows, X, Y, tag in ((M, nu, V, U, ref.TAG_MOVIES), (Mt, nm, U, V, ref.TAG_USERS)):
            ncols = len(A[0]) - 1
            z_ref, m, attempts, margin, bmargin = ref.latent(A, X, Y, it, tag, thr, full=True)
            mu, LU, LF = _hyper(K, ncols, it, 70 + K)
            got = []
            for dbuf in ("1", "0"):
                os.environ["BPMF_HIP_DBUF"] = dbuf                   # (read when a side is created)
                me, ot = _pair(eng, A, nrows, X, Y, thr, tag)
                assert np.array_equal(eng.get_items(me), X) and np.array_equal(eng.get_items(ot), Y)     # fp32: representable values
                eng.sample_side(me, ot, it, 1.0, mu, LF)
                got.append(eng.probit_latent(me, len(A[2])))
                if dbuf == "1":                                      # a second call from the same state: the same bits
                    eng.set_items(me, X)
                    eng.sample_side(me, ot, it, 1.0, mu, LF)
                    got.append(eng.probit_latent(me, len(A[2])))
                eng.side_destroy(me); eng.side_destroy(ot)
            z = got[0]
            err = np.abs(z - z_ref) / (1.0 + np.abs(m))
            print("K %d %s tag %d: %d ratings, |m| <= %.2f, attempts mean %.3f max %d, worst error %.3g, closest decision %.3g"
                  % (K, dtype, tag, len(z), np.abs(m).max(), attempts.mean(), attempts.max(), err.max(), min(margin, bmargin)))
            assert np.all(z * ref.labels(A[2], thr) > 0)
            assert err.max() <= 1e-12, (K, dtype, tag, int(err.argmax()), float(err.max()))
            assert got[1].tobytes() == z.tobytes() and got[2].tobytes() == z.tobytes()
    finally:
        eng.close()
        if old is None:
            os.environ.pop("BPMF_HIP_DBUF", None)
        else:
            os.environ["BPMF_HIP_DBUF"] = old


def _hip_runtime():
    """Raw hipMalloc / hipMemcpy through ctypes, as tests/test_gpu_latent.py does: the HIP runtime the library itself is linked
    against, for a device buffer of the test's own (the caller-owned ratings of side_create_dev)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def _to_device(hip, a):
    import ctypes as C
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
    assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0          # hipMemcpyHostToDevice
    return p


def _from_device(hip, p, like):
    import ctypes as C
    out = np.empty_like(like)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, out.nbytes, 2) == 0        # hipMemcpyDeviceToHost
    return out


def test_latent_leaves_the_ratings_alone_and_checks_its_arguments():
    import bpmf_amd
    from bpmf_amd import BpmfHipError
    K = 32
    M, Mt, T, Tt, nu, nm = util.ml100k()
    rng = np.random.default_rng(4)
    V, U = 0.4 * rng.standard_normal((nm, K)), 0.4 * rng.standard_normal((nu, K))
    eng = bpmf_amd.HipEngine(K)
    try:
        hip = _hip_runtime()
        d_rows, d_vals = _to_device(hip, M[1]), _to_device(hip, M[2])
        me = eng.side_create_dev(nm, nu, M[0], d_rows.value, d_vals.value, 0.0)
        ot = eng.side_create(nu, nm, np.zeros(nu + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
        eng.set_probit(me, 3.0, 1)
        eng.set_items(me, V); eng.set_items(ot, U)
        mu, LU, LF = _hyper(K, nm, 2, 5)
        eng.sample_side(me, ot, 2, 1.0, mu, LF)
        z = eng.probit_latent(me, len(M[2]))
        assert np.all(np.abs(z - ref.latent(M, V, U, 2, 1, 3.0)) <= 1e-12 * (1.0 + np.abs(ref.dots(M, V, U))))
        assert np.array_equal(_from_device(hip, d_vals, M[2]), M[2]) and np.array_equal(_from_device(hip, d_rows, M[1]), M[1])
        with pytest.raises(BpmfHipError, match="alpha = 1"):
            eng.sample_side(me, ot, 3, 2.0, mu, LF)
        with pytest.raises(BpmfHipError, match="already"):
            eng.set_probit(me, 3.0, 1)
        with pytest.raises(BpmfHipError, match="not a probit side"):
            eng.probit_latent(ot, 0)
        plain = eng.side_create(nm, nu, *M, util.mean_rating(M))
        with pytest.raises(BpmfHipError, match="mean_rating = 0"):
            eng.set_probit(plain, 3.0, 1)
        zero = eng.side_create(nm, nu, *M, 0.0)
        with pytest.raises(BpmfHipError, match="tag"):
            eng.set_probit(zero, 3.0, 0)
        with pytest.raises(BpmfHipError, match="finite"):
            eng.set_probit(zero, float("inf"), 1)
        part = eng.side_create(nm, nu, M[0][:11] - M[0][0], M[1][:M[0][10]], M[2][:M[0][10]], 0.0, 0, 10)
        with pytest.raises(BpmfHipError, match="whole"):
            eng.set_probit(part, 3.0, 1)
        eng.set_probit(zero, 3.0, 1)
        zu = eng.side_create(nu, nm, *Mt, 0.0)
        with pytest.raises(BpmfHipError, match="probit"):
            eng.sys_set_reduce(zero, zu)
        eng.sys_set_reduce(plain, zu)
        with pytest.raises(BpmfHipError, match="BPMF_REDUCE"):
            eng.set_probit(zu, 3.0, 2)
    finally:
        eng.close()
    hip.hipFree(d_rows); hip.hipFree(d_vals)


def _half_iteration(oracle, eng, K, A, nrows, X, Y, it, tag, thr, tol, stat_tol, expect_kernel):
    ncols = len(A[0]) - 1
    me, ot = _pair(eng, A, nrows, X, Y, thr, tag)
    assert re.search(expect_kernel, eng.kernel_name(me)), eng.kernel_name(me)
    info = eng.schedule_info(me)
    X, Y = eng.get_items(me), eng.get_items(ot)                      # (fp32: the stored values, widened)
    z = ref.latent(A, X, Y, it, tag, thr)
    mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, it)
    want = X.copy()
    s_ref, p_ref, n_ref = oracle.sample_side(K, (A[0], A[1], z), 0.0, 1.0, Y, want, it, mu, LF, nthreads=NT)
    s, p, n = eng.sample_side(me, ot, it, 1.0, mu, LF)
    items = eng.get_items(me)
    eng.side_destroy(me); eng.side_destroy(ot)
    assert np.all(np.isfinite(items))
    err = rel_err(items, want)
    print("K %d %s: %.3g" % (K, eng.dtype, err))
    assert err < tol, err
    assert rel_err(s, s_ref) < stat_tol and rel_err(p, p_ref) < stat_tol and abs(n - n_ref) <= stat_tol * abs(n_ref)
    return info


@pytest.mark.parametrize("mode", [1, 3])
def test_half_iteration_k8(oracle, mode):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    old = os.environ.get("BPMF_HIP_MODE")
    os.environ["BPMF_HIP_MODE"] = str(mode)
    eng = bpmf_amd.HipEngine(8)
    try:
        rng = np.random.default_rng(80 + mode)
        _half_iteration(oracle, eng, 8, M, nu, 0.7 * rng.standard_normal((nm, 8)), 0.7 * rng.standard_normal((nu, 8)), 3, 1, 3.0,
                        RTOL, 1e-8, {1: r"k_sample1", 3: r"k_sample4"}[mode])
    finally:
        eng.close()
        if old is None:
            os.environ.pop("BPMF_HIP_MODE", None)
        else:
            os.environ["BPMF_HIP_MODE"] = old


def _product_form_side(rng, nrows=400):
    """A side with columns of 0 .. 16 ratings in every product-form class, a few of 30 and 300 for the slab launch, ratings 1 .. 5
    (the column counts of tests/test_gpu_alpha.py::test_alpha_k64_product_form)."""
    counts = np.concatenate([np.full(301, 0), np.full(203, 1), np.full(97, 2), np.full(250, 3), np.full(333, 4), np.full(334, 5),
                             np.full(335, 6)] + [np.full(33, n) for n in range(7, 17)] + [np.full(9, 30), np.full(3, 300)])
    rng.shuffle(counts)
    colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rowidx = np.concatenate([np.sort(rng.choice(nrows, size=c, replace=False)) for c in counts]).astype(np.int32)
    return (colptr, rowidx, rng.integers(1, 6, len(rowidx)).astype(np.float64)), nrows


@pytest.mark.parametrize("K,dtype", [(32, "f64"), (64, "f64"), (128, "f64"), (128, "f32")])
def test_half_iteration_families(oracle, K, dtype):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = bpmf_amd.HipEngine(K, dtype=dtype)
    try:
        rng = np.random.default_rng(800 + K)
        sigma = (2.0 / K) ** 0.25
        tol, stat_tol = (2e-3, 1e-3) if dtype == "f32" else (RTOL, 1e-8)
        if K == 64:                                                  # product-form columns + the slab launch of the heavier ones
            A, nrows = _product_form_side(rng)
            ncols = len(A[0]) - 1
            info = _half_iteration(oracle, eng, K, A, nrows, sigma * rng.standard_normal((ncols, K)), sigma * rng.standard_normal((nrows, K)),
                                   4, 1, 3.0, tol, stat_tol, r"k_sample_pf")
            assert info["pf_le3"] > 0 and info["pf_4to6"] > 0 and info["pf_7to16"] > 0 and info["other_items"] > 0, info
        else:
            V, U = sigma * rng.standard_normal((nm, K)), sigma * rng.standard_normal((nu, K))
            _half_iteration(oracle, eng, K, M, nu, V, U, 4, 1, 3.0, tol, stat_tol, {32: r"k_sample", 128: r"k_sample_wg2"}[K])
    finally:
        eng.close()


@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("pipelined", [True, False])
def test_probit_chain_against_cpu(oracle, K, pipelined):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    nsims, burnin, thr = 8, 3, 3.0
    want = ref.restate_chain(oracle, K, M, Mt, T, nsims, burnin, thr)
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, Tt=Tt, pipelined=pipelined, probit=True, threshold=thr)
    finally:
        eng.close()
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(res["U"] - want["U"]).max() / scale, np.abs(res["V"] - want["V"]).max() / scale
    ep = np.abs(res["prob"] - want["prob"]).max()
    print("K %d pipelined %s: U %.3g V %.3g prob %.3g auc %.6f / %.6f brier %.4f, closest decision of the restatement %.3g"
          % (K, pipelined, eu, ev, ep, res["auc"], want["auc"], res["brier"], want["margin"]))
    assert eu < 1e-6 and ev < 1e-6
    assert np.abs(np.array(res["rmse"]) - want["rmse"]).max() < 1e-6
    assert np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max() < 1e-6
    assert ep < 1e-6 and abs(res["auc"] - want["auc"]) < 1e-6 and abs(res["brier"] - want["brier"]) < 1e-6
    assert len(res["prob"]) == len(T[2])


def test_probit_chain_with_the_gate_on_its_own_stream(oracle):
    """BPMF_HIP_FUSED=0: the gate kernel runs on the side's second stream and the samplers' stream waits for its event; the
    latent kernel is enqueued ahead of that wait (bpmf_hip_sys_sample), not by launch_sampler.  Same chain as the fused form."""
    import bpmf_amd
    K, nsims, burnin, thr = 32, 6, 2, 3.0
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want = ref.restate_chain(oracle, K, M, Mt, T, nsims, burnin, thr)
    old = os.environ.get("BPMF_HIP_FUSED")
    os.environ["BPMF_HIP_FUSED"] = "0"
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, Tt=Tt, pipelined=True, probit=True, threshold=thr)
    finally:
        eng.close()
        if old is None:
            os.environ.pop("BPMF_HIP_FUSED", None)
        else:
            os.environ["BPMF_HIP_FUSED"] = old
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    assert np.abs(res["U"] - want["U"]).max() < 1e-6 * scale and np.abs(res["V"] - want["V"]).max() < 1e-6 * scale
    assert np.abs(res["prob"] - want["prob"]).max() < 1e-6 and abs(res["auc"] - want["auc"]) < 1e-6


@pytest.mark.parametrize("K,dtype", [(10, "f64"), (16, "f64"), (64, "f64"), (128, "f32")])
def test_probit_add_against_numpy(K, dtype):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    S = 5
    rng = np.random.default_rng(K)
    eng = bpmf_amd.HipEngine(K, dtype=dtype)
    try:
        movies = eng.side_create(nm, nu, *M, 0.0)
        users = eng.side_create(nu, nm, *Mt, 0.0)
        test = eng.test_create(movies, *T)
        with pytest.raises(bpmf_amd.BpmfHipError, match="nothing added"):
            eng.probit_get(test)
        acc = np.zeros(len(T[2]))
        sigma = (3.0 / K) ** 0.25
        for _ in range(S):
            eng.set_items(movies, sigma * rng.standard_normal((nm, K)))
            eng.set_items(users, sigma * rng.standard_normal((nu, K)))
            eng.probit_add(test, movies, users)
            acc += ref.phi(ref.dots(T, eng.get_items(movies), eng.get_items(users)))
        prob, n = eng.probit_get(test)
        assert n == S
        assert prob.min() >= 0.0 and prob.max() <= 1.0 and prob.min() < 0.2 and prob.max() > 0.8      # (the mean of S samples: not the extremes of one)
        assert np.abs(prob - acc / S).max() <= 1e-12
    finally:
        eng.close()


# python -c "from tests import probit_ref as R; from oracle.oracle import Oracle; P = R.RECOVERY; d = R.recovery_data(**P);
#            print(d[6], R.restate_chain(Oracle(), P['K'], d[0], d[1], d[2], P['nsims'], P['burnin'])['auc'])"
RECOVERY_CEILING = 0.9160968039851615        # AUC of the true Phi(u . v) on the test pairs
RECOVERY_RESTATED = 0.9064184095341258       # AUC of the restated CPU chain (40 iterations, 20 kept; the midpoint is 0.7080)


def test_probit_recovers_a_planted_model():
    import bpmf_amd
    P = ref.RECOVERY
    M, Mt, T, Tt, nu, nm, ceiling = ref.recovery_data(**P)
    assert abs(ceiling - RECOVERY_CEILING) < 1e-12
    assert RECOVERY_RESTATED > 0.5 + 0.5 * (RECOVERY_CEILING - 0.5)      # above the midpoint between chance and the ceiling
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=P["nsims"], burnin=P["burnin"], Tt=Tt, pipelined=True, probit=True)
    finally:
        eng.close()
    print("AUC: ceiling %.6f, restated chain %.6f, GPU %.6f; Brier %.4f" % (RECOVERY_CEILING, RECOVERY_RESTATED, res["auc"], res["brier"]))
    assert abs(res["auc"] - RECOVERY_RESTATED) < 1e-6


def _write_mtx(path, nrows, ncols, r, c, v):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (nrows, ncols, len(v)))
        for i in range(len(v)):
            f.write("%d %d %g\n" % (r[i] + 1, c[i] + 1, v[i]))


def _csc01(nrows, ncols, r, c, v):
    import scipy.sparse as sp
    m = sp.coo_matrix((v + 1.0, (r, c)), shape=(nrows, ncols)).tocsc()   # (+ 1: explicit zeros survive the containers)
    A, At = util.csc_arrays(m), util.csc_arrays(m.T)
    return (A[0], A[1], A[2] - 1.0), (At[0], At[1], At[2] - 1.0)


def test_cli_probit_end_to_end(tmp_path):
    import bpmf_amd
    rng = np.random.default_rng(77)
    nu, nm, n = 300, 200, 14000
    pos = rng.permutation(nu * nm)[:n]
    r, c = pos // nm, pos % nm
    Ut, Vt = rng.standard_normal((nu, 2)), rng.standard_normal((nm, 2))
    v = (np.einsum("ij,ij->i", Ut[r], Vt[c]) + rng.standard_normal(n) > 0).astype(np.float64)
    tr, te = np.arange(n) < 12500, np.arange(n) >= 12500
    _write_mtx(tmp_path / "train.mtx", nu, nm, r[tr], c[tr], v[tr])
    _write_mtx(tmp_path / "test.mtx", nu, nm, r[te], c[te], v[te])
    M, Mt = _csc01(nu, nm, r[tr], c[tr], v[tr])
    T, Tt = _csc01(nu, nm, r[te], c[te], v[te])
    eng = bpmf_amd.HipEngine(16)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=12, burnin=4, Tt=Tt, probit=True, topn=5)
    finally:
        eng.close()
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    args = [exe, "-n", str(tmp_path / "train.mtx"), "-p", str(tmp_path / "test.mtx"), "-i", "12", "-b", "4", "-d", "16", "--probit"]
    (tmp_path / "o").mkdir()
    runs = [subprocess.run(args + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
            for extra in (["-o", str(tmp_path / "o"), "--topn", "5"], [])]        # -o: the plain loop; without: the pipelined one
    for run in runs:
        assert run.returncode == 0, run.stderr
        assert re.search(r"^likelihood: probit, a rating > 0\.5 is a positive label; the RMSE columns compare the latent score with "
                         r"the raw label and are not an error measure$", run.stdout, re.M), run.stdout
        assert re.search(r"^mean rating: 0$", run.stdout, re.M) and re.search(r"^alpha: 1$", run.stdout, re.M)
        assert len(re.findall(r"iteration \d+:\t RMSE: \S+\tavg RMSE: \S+\tFU\(", run.stdout)) == 12
        auc = re.search(r"^Final Avg RMSE: \S+\nFinal AUC: (\S+)\nFinal Brier: (\S+)$", run.stdout, re.M)
        assert auc, run.stdout
        assert auc.group(1) == "%g" % res["auc"] and auc.group(2) == "%g" % res["brier"], (auc.groups(), res["auc"], res["brier"])
    with open(tmp_path / "o" / "probit.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["row", "col", "label", "prob"] and len(rows) == 1 + len(T[2])
    tcols = np.repeat(np.arange(nm), np.diff(T[0]))
    assert [int(x[0]) - 1 for x in rows[1:]] == list(T[1]) and [int(x[1]) - 1 for x in rows[1:]] == list(tcols)      # test-set order
    assert [int(x[2]) for x in rows[1:]] == list(T[2].astype(int))
    assert np.abs(np.array([float(x[3]) for x in rows[1:]]) - res["prob"]).max() <= 1e-9
    with open(tmp_path / "o" / "topn.csv") as f:
        top = list(csv.reader(f))
    assert top[0] == ["query", "rank", "candidate", "mean", "std"] and len(top) > 1 + 4 * nu
    idx = res["topn"][0]
    first = [int(x[2]) - 1 for x in top[1:6]]
    assert [int(x[0]) for x in top[1:6]] == [1] * 5 and first == list(idx[0])
    assert not (tmp_path / "probit.csv").exists()


def test_fixed_path_is_untouched_by_a_probit_run():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = bpmf_amd.HipEngine(16)
    try:
        before = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
        pr = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True, probit=True, threshold=3.0)
        after = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
    finally:
        eng.close()
    assert before["U"].tobytes() == after["U"].tobytes() and before["V"].tobytes() == after["V"].tobytes()
    assert before["rmse"] == after["rmse"] and before["rmse_avg"] == after["rmse_avg"]
    assert "prob" not in before and "auc" not in after and len(pr["prob"]) == len(T[2])
    assert not np.array_equal(pr["U"], before["U"])
