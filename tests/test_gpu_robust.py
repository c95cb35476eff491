"""Student-t noise (`gibbs(..., robust=NU)`, `bpmf --robust NU`) on the GPU.

  1. the weights k_robust_weights leaves behind one half-iteration against the restatement of tests/robust_ref.py: the edge side
     (tiles of 256 ratings end inside columns and on column boundaries) and sides of 0, 1, 255, 256, 257 ratings; K = 8, 10, 32, 64,
     100, 128, nu = 1, 4, 30, alpha = 0.5, 2, 3
  2. two launches with the same (iteration, tag, factors) are bit-equal; another iteration gives other weights
  3. one half-iteration through every sampler family: the factors against the weighted reference fed the restated weights
  4. the coupled chain against the restated chain (K = 32, 64; pipelined and plain loop; BPMF_HIP_FUSED=0 with topn once)
  5. planted outliers: the Student-t run beats the best single alpha; a small posterior-mean weight finds the planted cells
  6. `bpmf --robust 4 -o DIR` end to end, and a run without the flag
  7. arguments, mutual refusals in both orders, device memory, a plain side beside a robust one
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import robust_ref as ref
from tests import util
from tests import weights_ref
from tests.conftest import ROOT
from tests.test_gpu_parity import RTOL, rel_err
from tests.test_gpu_weights import FAMILIES, STAT_TOL, _env, _mask

pytestmark = pytest.mark.gpu

EINVAL = -1
LATENT_BAR = 1e-12          # the bar of the probit and censored latent tests (test_gpu_probit.py, test_gpu_censored.py)


def _pair(eng, A, nrows, X, Y, nu, tag, mean=None):
    """A robust side over the ratings A holding the factors X, and a partner without ratings holding Y."""
    ncols = len(A[0]) - 1
    me = eng.side_create(ncols, nrows, *A, util.mean_rating(A) if mean is None else mean)
    ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    if nu is not None:
        eng.set_robust(me, nu, tag)
    eng.set_items(me, X)
    eng.set_items(ot, Y)
    return me, ot


def _mean(A):
    return util.mean_rating(A) if len(A[2]) else 0.0


# ---- 1. the weights against the restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", ref.KS)
def test_weights_against_the_restatement(oracle, K):
    import bpmf_amd
    edge, nrows = ref.edge_side()
    sides = [(edge, nrows, ref.TAG_MOVIES)] + [ref.small_side(n) + (ref.TAG_USERS,) for n in ref.SMALL_NNZ]
    assert [len(s[0][2]) for s in sides] == [894, 0, 1, 255, 256, 257]
    assert len(edge[0]) - 1 == 15 and 256 not in edge[0] and 512 not in edge[0]     # the edge side: tiles end inside columns ...
    assert 256 in sides[5][0][0][1:-1] and sides[4][0][0][-1] == 256                # ... 257: on a column boundary; 256: on the side's end
    worst_sw = worst_zw = 0.0
    eng = bpmf_amd.HipEngine(K)
    try:
        for A, nr, tag in sides:
            ncols, nnz, mean = len(A[0]) - 1, len(A[2]), _mean(A)
            X, Y = ref.factors(K, ncols, nr)
            mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, ref.ITER)
            for nu in ref.NUS:
                for alpha in ref.ALPHAS:
                    me, ot = _pair(eng, A, nr, X, Y, nu, tag, mean)
                    sw0, zw0 = eng.weights_get(me)                       # before the first launch: w = 1
                    assert np.all(sw0 == 1.0) and zw0.tobytes() == (A[2] - mean).tobytes()
                    eng.sample_side(me, ot, ref.ITER, alpha, mu, LF)
                    sw, zw = eng.weights_get(me)
                    eng.side_destroy(me); eng.side_destroy(ot)
                    sw_ref, zw_ref, m, attempts, margin = ref.weights(A, X, Y, ref.ITER, tag, alpha, nu, mean, full=True)
                    assert sw.shape == (nnz,) and zw.shape == (nnz,)
                    if nnz == 0:
                        continue
                    assert margin >= ref.MARGIN
                    esw = float(np.max(np.abs(sw - sw_ref) / (1.0 + sw_ref)))
                    ezw = float(np.max(np.abs(zw - zw_ref) / (1.0 + np.abs(zw_ref))))
                    worst_sw, worst_zw = max(worst_sw, esw), max(worst_zw, ezw)
                    assert esw <= LATENT_BAR and ezw <= LATENT_BAR, (K, nnz, nu, alpha, esw, ezw)
    finally:
        eng.close()
    print("K %d: max |sw - ref| / (1 + ref) = %.3g, max |zw - ref| / (1 + |ref|) = %.3g" % (K, worst_sw, worst_zw))


# ---- 2. grid independence ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [8, 128])
def test_weights_depend_on_rating_iteration_tag_and_factors_only(oracle, K):
    import bpmf_amd
    A, nrows = ref.edge_side()
    ncols = len(A[0]) - 1
    X, Y = ref.factors(K, ncols, nrows)
    mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, ref.ITER)

    def launch(eng, it, tag):
        me, ot = _pair(eng, A, nrows, X, Y, 4.0, tag)
        eng.sample_side(me, ot, it, 2.0, mu, LF)
        sw, zw = eng.weights_get(me)
        out = (sw.tobytes(), zw.tobytes(), eng.get_items(me).tobytes())
        eng.side_destroy(me); eng.side_destroy(ot)
        return out, sw
    eng = bpmf_amd.HipEngine(K)
    try:
        a, sw_a = launch(eng, ref.ITER, ref.TAG_MOVIES)
        b, _ = launch(eng, ref.ITER, ref.TAG_MOVIES)
        c, sw_c = launch(eng, ref.ITER + 1, ref.TAG_MOVIES)
        d, sw_d = launch(eng, ref.ITER, ref.TAG_USERS)
    finally:
        eng.close()
    assert a == b
    assert np.count_nonzero(sw_a != sw_c) == len(sw_a) and np.count_nonzero(sw_a != sw_d) == len(sw_a)


# ---- 3. one half-iteration per family ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [16, None])
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_half_iteration_edge_side(oracle, fam, chunk):
    import bpmf_amd
    _, K, env, kern, _ = fam
    nu, alpha, it = 4.0, 2.0, ref.ITER
    A, nrows = ref.edge_side()
    ncols, mean = len(A[0]) - 1, util.mean_rating(A)
    X, Y = ref.factors(K, ncols, nrows, seed=3)
    mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, it)
    sw_ref, _ = ref.weights(A, X, Y, it, ref.TAG_MOVIES, alpha, nu, mean)
    want = X.copy()
    s_ref, p_ref, n_ref = weights_ref.sample_side_weighted(oracle, K, A, sw_ref * sw_ref, mean, alpha, Y, want, it, mu, LF)
    with _env(**dict(env, **({"BPMF_HIP_CHUNK": chunk} if chunk else {}))):
        eng = bpmf_amd.HipEngine(K)
        try:
            me, ot = _pair(eng, A, nrows, X, Y, nu, ref.TAG_MOVIES)
            assert re.search(kern, eng.kernel_name(me)), eng.kernel_name(me)
            info = eng.schedule_info(me)
            s, p, n = eng.sample_side(me, ot, it, alpha, mu, LF)
            items = eng.get_items(me)
        finally:
            eng.close()
    if chunk:
        assert info["chunk"] == 16 and info["chunked_columns"] == 8, info
    err = rel_err(items, want)
    print("K %d: factors %.3g, sum %.3g, prod %.3g" % (K, err, rel_err(s, s_ref), rel_err(p, p_ref)))
    assert np.all(np.isfinite(items)) and err < RTOL, err
    assert rel_err(s, s_ref) < STAT_TOL and rel_err(p, p_ref) < STAT_TOL and abs(n - n_ref) <= STAT_TOL * abs(n_ref)


# ---- 4. chains against the CPU restatement ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _restated_ml100k(K):
    from oracle.oracle import Oracle
    M, Mt, T, Tt, nu, nm = util.ml100k()
    C = ref.CHAIN
    return ref.restate_chain(Oracle(), K, M, Mt, T, C["nu"], C["nsims"], C["burnin"], C["alpha"])


def _check_chain(res, want, label):
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(res["U"] - want["U"]).max() / scale, np.abs(res["V"] - want["V"]).max() / scale
    et = max(np.abs(np.array(res["rmse"]) - want["rmse"]).max(), np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max())
    ef = abs(res["final_rmse_avg"] - want["final_rmse_avg"])
    print("%s: U %.3g V %.3g traces %.3g final %.3g" % (label, eu, ev, et, ef))
    assert eu < 1e-6 and ev < 1e-6 and et < 1e-6 and ef < 1e-6, (label, eu, ev, et, ef)
    rb = res["robust"]
    ew = float(np.max(np.abs(rb["weight_mean"] - want["weight_mean"]) / want["weight_mean"]))
    print("%s: weight_mean %.3g relative, closest decision of the restated chain %.3g" % (label, ew, want["margin"]))
    assert want["margin"] >= ref.MARGIN
    assert rb["kept"] == want["kept"] and ew < 1e-9, ew


@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("pipelined", [True, False])
def test_robust_chain_against_cpu(K, pipelined):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want = _restated_ml100k(K)
    C = ref.CHAIN
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, pipelined=pipelined, robust=C["nu"], nsims=C["nsims"], burnin=C["burnin"],
                             alpha=C["alpha"])
    finally:
        eng.close()
    assert res["robust"]["nu"] == C["nu"]
    _check_chain(res, want, "K %d pipelined %s" % (K, pipelined))


def test_robust_chain_with_the_gate_on_its_own_stream():
    """BPMF_HIP_FUSED=0: the weight kernel goes ahead of the wait for the gate kernel, and the sample rings on top.  Same chain."""
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want = _restated_ml100k(32)
    C = ref.CHAIN
    with _env(BPMF_HIP_FUSED=0):
        eng = bpmf_amd.HipEngine(32)
        try:
            res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, pipelined=True, robust=C["nu"], topn=5, nsims=C["nsims"],
                                 burnin=C["burnin"], alpha=C["alpha"])
        finally:
            eng.close()
    _check_chain(res, want, "K 32 unfused")
    assert res["topn"][0].shape == (nu, 5)


# ---- 5. planted outliers ----------------------------------------------------------------------------------------------------------------

def test_planted_outliers(oracle):
    """600 x 300, rank 4, 40 training cells per user with noise sd 0.25, 6000 noise-free test cells; a seeded 5 % of the training cells
    replaced by the truth + 10 or - 10.  Restated CPU chains, test RMSE of the posterior-mean prediction (robust_ref.PLANTED_MEASURED;
    tests/test_robust_host.py re-measures all three):
        Student-t noise, nu = 4, alpha = 16             0.1201
        Gaussian noise, alpha = 16                      4.1025
        Gaussian noise, alpha = 1 / mean variance       0.9837   (the best single alpha)
    and a small posterior-mean weight separates the planted cells from the others with an AUC of 1.0000.
    Asserted: the GPU's Student-t chain beats the best single alpha by at least half the recorded margin (0.4318), its AUC is within
    0.02 of the recorded one -- and it is the restated chain at the chain bars."""
    import bpmf_amd
    P = ref.PLANTED
    d = ref.planted_data(**P)
    want = ref.restate_chain(oracle, P["K"], d["M"], d["Mt"], d["T"], P["nu"], P["nsims"], P["burnin"], P["alpha"])
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, d["M"], d["Mt"], d["T"], P["nusers"], P["nmovies"], nsims=P["nsims"], burnin=P["burnin"], Tt=d["Tt"],
                             pipelined=True, alpha=P["alpha"], robust=P["nu"])
    finally:
        eng.close()
    rg = res["final_rmse_avg"]              # (the running-mean prediction of the last line; the closing evaluation counts the last sample twice)
    auc = ref.planted_auc(res["robust"]["weight_mean"], d["planted"])
    print("test RMSE: GPU Student-t %.4f, restated %.4f, recorded best single alpha %.4f; AUC of the weights: GPU %.4f, recorded %.4f"
          % (rg, weights_ref.planted_rmse(want["pred"], d["T"][2]), ref.PLANTED_MEASURED[2], auc, ref.PLANTED_AUC))
    assert ref.PLANTED_MEASURED[2] - rg >= ref.PLANTED_HALF_MARGIN, (rg, ref.PLANTED_MEASURED)
    assert abs(auc - ref.PLANTED_AUC) <= 0.02
    assert abs(weights_ref.planted_rmse(want["pred"], d["T"][2]) - ref.PLANTED_MEASURED[0]) < 1e-6
    _check_chain(res, want, "planted outliers")


# ---- 6. the executable ------------------------------------------------------------------------------------------------------------------

def test_cli_robust_end_to_end(tmp_path, oracle):
    from bpmf_amd import io as bio
    M, Mt, T, Tt, nu, nm = util.tiny()
    C = ref.CLI
    want = ref.restate_chain(oracle, C["K"], M, Mt, T, C["nu"], C["nsims"], C["burnin"], C["alpha"])
    assert want["margin"] >= ref.MARGIN
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    base = [exe, "-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx"), "-a", str(C["alpha"]),
            "-i", str(C["nsims"]), "-b", str(C["burnin"]), "-d", str(C["K"])]
    (tmp_path / "o").mkdir(); (tmp_path / "p").mkdir()

    def run(extra):
        return subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    plain_before = run(["-o", str(tmp_path / "p")])
    runs = [run(["--robust", "4", "-v", "-o", str(tmp_path / "o")]),       # -o: the plain loop
            run(["--robust", "4"])]                                        # without: the pipelined one
    plain_after = run(["-o", str(tmp_path / "p")])
    for out in runs:
        assert out.returncode == 0, out.stderr
        assert re.search(r"^robust: Student-t noise, nu = 4$", out.stdout, re.M), out.stdout
        lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", out.stdout)
        assert len(lines) == C["nsims"]
        got = np.array([[float(a), float(b)] for a, b in lines])
        assert np.abs(got[:, 0] - want["rmse"]).max() <= 1e-6 + 5e-5 and np.abs(got[:, 1] - want["rmse_avg"]).max() <= 1e-6 + 5e-5
        final = re.search(r"^Final Avg RMSE: (\S+)$", out.stdout, re.M)
        assert final and abs(float(final.group(1)) - want["final_rmse_avg"]) <= 1e-6 + 5e-6 * max(1.0, want["final_rmse_avg"])
    # every sample (-v) at the bar of the chain tests: the last one against the restated chain
    last = C["nsims"] - 1
    U, V = bio.read_dense(tmp_path / "o" / ("U-%d.ddm" % last)).T, bio.read_dense(tmp_path / "o" / ("V-%d.ddm" % last)).T
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(U - want["U"]).max() / scale, np.abs(V - want["V"]).max() / scale
    print("bpmf --robust: U %.3g V %.3g of max|U|" % (eu, ev))
    assert eu < 1e-6 and ev < 1e-6, (eu, ev)
    # robust-weights.sdm: the posterior-mean weight of every training cell, in the cells of the training matrix
    nr, nc, W = bio.read_sparse(tmp_path / "o" / "robust-weights.sdm")
    assert (nr, nc) == (nu, nm) and np.array_equal(W[0], M[0]) and np.array_equal(W[1], M[1])
    ew = float(np.max(np.abs(W[2] - want["weight_mean"]) / want["weight_mean"]))
    print("robust-weights.sdm: %.3g relative" % ew)
    assert ew < 1e-9
    assert not (tmp_path / "p" / "robust-weights.sdm").exists()
    # without the flag: the same stdout before and after, no robust line, and the lines of the plain chain
    assert plain_before.returncode == 0 and plain_after.returncode == 0, plain_before.stderr + plain_after.stderr
    assert _mask(plain_before.stdout) == _mask(plain_after.stdout) and "robust" not in plain_before.stdout
    plain_want = ref.restate_chain(oracle, C["K"], M, Mt, T, None, C["nsims"], C["burnin"], C["alpha"])
    lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", plain_before.stdout)
    got = np.array([[float(a), float(b)] for a, b in lines])
    assert np.abs(got[:, 0] - plain_want["rmse"]).max() <= 1e-6 + 5e-5
    assert _mask(plain_before.stdout) != _mask(runs[0].stdout)


# ---- 7. arguments, mutual refusals, device memory, a plain side beside a robust one ------------------------------------------------------

def test_arguments_and_mutual_refusals():
    import ctypes as C
    import scipy.sparse as sp
    import bpmf_amd
    from bpmf_amd import BpmfHipError
    K = 32
    M, Mt, T, Tt, nu, nm = util.ml100k()
    nnz, mean = len(M[2]), util.mean_rating(M)
    rng = np.random.default_rng(4)
    eng = bpmf_amd.HipEngine(K)
    try:
        lib = eng.lib
        plain = eng.side_create(nm, nu, *M, mean)
        with pytest.raises(BpmfHipError, match="side_set_robust: NULL") as e:
            bpmf_amd._lib.check(lib.bpmf_hip_side_set_robust(None, 4.0, 9))
        assert e.value.code == EINVAL
        for bad in (0.5, 0.0, -2.0, float("nan"), float("inf")):
            with pytest.raises(BpmfHipError, match=r"side_set_robust: nu = .* is not finite and >= 1") as e:
                eng.set_robust(plain, bad, 9)
            assert e.value.code == EINVAL
        with pytest.raises(BpmfHipError, match="side_set_robust: tag must be >= 1"):
            eng.set_robust(plain, 4.0, 0)
        for call in (eng.robust_add, eng.robust_get):
            with pytest.raises(BpmfHipError, match="not a robust side"):
                call(plain)
        # set_robust refuses a side that has another add-on
        ws = eng.side_create(nm, nu, *M, mean)
        eng.set_weights(ws, np.ones(nnz))
        with pytest.raises(BpmfHipError, match="side_set_robust: not on a side with per-rating weights"):
            eng.set_robust(ws, 4.0, 9)
        pb = eng.side_create(nm, nu, *M, 0.0)
        eng.set_probit(pb, 3.0, 1)
        with pytest.raises(BpmfHipError, match="side_set_robust: not on a probit side"):
            eng.set_robust(pb, 4.0, 9)
        cs = eng.side_create(nm, nu, *M, mean)
        eng.set_censored(cs, np.zeros(nnz, np.int8), 5)
        with pytest.raises(BpmfHipError, match="side_set_robust: not on a censored side"):
            eng.set_robust(cs, 4.0, 9)
        ft = eng.side_create(nm, nu, *M, mean)
        eng.set_features(ft, rng.standard_normal((nm, 3)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="side_set_robust: not together with features"):
            eng.set_robust(ft, 4.0, 9)
        pp = eng.side_create(nm, nu, *M, mean)
        eng.set_prop_posterior(pp, np.tile(np.eye(K).ravel(), (nm, 1)))
        with pytest.raises(BpmfHipError, match="side_set_robust: not together with propagated priors"):
            eng.set_robust(pp, 4.0, 9)
        part = eng.side_create(nm, nu, M[0][:11] - M[0][0], M[1][:M[0][10]], M[2][:M[0][10]], mean, 0, 10)
        with pytest.raises(BpmfHipError, match="side_set_robust: .*whole"):
            eng.set_robust(part, 4.0, 9)
        ru, rm = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt)), eng.side_create(nm, nu, *M, mean)
        eng.sys_set_reduce(rm, ru)
        with pytest.raises(BpmfHipError, match="side_set_robust: .*BPMF_REDUCE"):
            eng.set_robust(rm, 4.0, 9)
        # ... and the other add-ons refuse a robust side
        me = eng.side_create(nm, nu, *M, mean)
        eng.set_robust(me, 4.0, 9)
        assert eng.kernel_name(me) == "k_sample1w<32>"
        with pytest.raises(BpmfHipError, match="side_set_robust: the side is a robust side already"):
            eng.set_robust(me, 4.0, 9)
        with pytest.raises(BpmfHipError, match="side_set_weights: not on a side with Student-t noise"):
            eng.set_weights(me, np.ones(nnz))
        with pytest.raises(BpmfHipError, match="side_set_probit: not on a side with Student-t noise"):
            eng.set_probit(me, 3.0, 1)
        with pytest.raises(BpmfHipError, match="side_set_censored: not on a side with Student-t noise"):
            eng.set_censored(me, np.zeros(nnz, np.int8), 5)
        with pytest.raises(BpmfHipError, match="not on a side with Student-t noise"):
            eng.set_features(me, rng.standard_normal((nm, 3)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="not on a side with Student-t noise"):
            eng.set_features(me, sp.random(nm, 9, density=0.3, random_state=1, format="csr"), 5.0, 3)
        with pytest.raises(BpmfHipError, match="set_prop_posterior: not on a side with Student-t noise"):
            eng.set_prop_posterior(me, np.tile(np.eye(K).ravel(), (nm, 1)))
        cu = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt))
        with pytest.raises(BpmfHipError, match="sys_set_reduce: not together with Student-t noise"):
            eng.sys_set_reduce(me, cu)
        with pytest.raises(BpmfHipError, match="train_sse: not with a side with per-rating weights"):
            eng.train_sse(me, cu)
        # nothing added yet: the count and nu come back, the mean is refused
        n, got_nu = C.c_int(-1), C.c_double()
        bpmf_amd._lib.check(lib.bpmf_hip_side_robust_get(me.handle, None, C.byref(n), C.byref(got_nu)))
        assert (n.value, got_nu.value) == (0, 4.0)
        with pytest.raises(BpmfHipError, match="side_robust_get: nothing added"):
            eng.robust_get(me)
        # a launch with an alpha that is not finite and > 0
        eng.set_items(me, 0.3 * rng.standard_normal((nm, K))); eng.set_items(cu, 0.3 * rng.standard_normal((nu, K)))
        mu, LF = np.zeros(K), np.eye(K)
        for bad in (0.0, -1.0, float("inf")):
            with pytest.raises(BpmfHipError, match="robust: a robust side is sampled with a finite alpha > 0"):
                eng.sample_side(me, cu, 0, bad, mu, LF)
    finally:
        eng.close()


def test_set_robust_refuses_an_fp32_context():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = bpmf_amd.HipEngine(128, dtype="f32")
    try:
        side = eng.side_create(nm, nu, *M, util.mean_rating(M))
        with pytest.raises(bpmf_amd.BpmfHipError, match="side_set_robust: not on an fp32 context") as e:
            eng.set_robust(side, 4.0, 9)
        assert e.value.code == EINVAL
        with pytest.raises(ValueError, match="fp64"):
            bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=0, robust=4)
    finally:
        eng.close()


_COMM_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bpmf_amd
eng = bpmf_amd.HipEngine(8)
eng.comm_init(1, 0, eng.comm_unique_id())
side = eng.side_create(2, 4, np.array([0, 4, 6], np.int64), np.array([0, 1, 2, 3, 0, 2], np.int32), np.array([2., 3., 7., 4., 5., 1.]), 3.0)
try:
    eng.set_robust(side, 4.0, 9)
    print("ACCEPTED")
except bpmf_amd.BpmfHipError as e:
    print("REFUSED %d %s" % (e.code, e))
eng.close()
"""


def test_set_robust_refuses_a_context_with_a_communicator():
    """The other branch of the single-GPU check: a whole side on a context that has a communicator.  In a process of its own: a
    communicator is process-wide state of the communication library."""
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("BPMF_HIP_RCCL_LIBRARY", None)
    r = subprocess.run([sys.executable, "-c", _COMM_CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert re.search(r"^REFUSED -1 .*side_set_robust: .*communicator", r.stdout, re.M), r.stdout


def test_device_memory_returns_and_the_plain_path_is_untouched():
    import bpmf_amd

    def live():
        return int(bpmf_amd.load_library().bpmf_hip_live_device_bytes())
    M, Mt, T, Tt, nu, nm = util.tiny()
    base = live()
    eng = bpmf_amd.HipEngine(16)
    try:
        before_run = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
        movies = eng.side_create(nm, nu, *M, util.mean_rating(M))
        users = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt))
        before = live()
        with pytest.raises(bpmf_amd.BpmfHipError, match="not finite and >= 1"):     # a refused call leaves nothing
            eng.set_robust(movies, 0.5, 9)
        assert live() == before
        eng.set_robust(movies, 4.0, 9)
        assert live() - before == (3 * len(M[2]) + len(M[0])) * 8    # sw, zw, wsum and the column pointers
        eng.set_robust(users, 4.0, 10)
        held = live()
        for _ in range(3):
            eng.sys_sample(movies, users, 2.0)
            eng.sys_sample(users, movies, 2.0)
            eng.robust_add(movies)
        wm, n, got_nu = eng.robust_get(movies)
        assert n == 3 and got_nu == 4.0 and np.all(wm > 0) and np.all(np.isfinite(wm))
        sw, _ = eng.weights_get(movies)                              # the arrays the newest launch read
        assert np.all(sw > 0) and np.any(sw != 1.0)
        assert live() == held
        eng.side_destroy(movies)
        assert live() < held
        eng.side_destroy(users)
        assert live() == before
        after_run = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
        robust_run = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True, robust=4)
        again = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
    finally:
        eng.close()
    assert live() == base
    # a plain side in the same context samples bit for bit as before a robust side existed
    for r in (after_run, again):
        assert before_run["U"].tobytes() == r["U"].tobytes() and before_run["V"].tobytes() == r["V"].tobytes()
        assert before_run["rmse"] == r["rmse"] and before_run["rmse_avg"] == r["rmse_avg"] and "robust" not in r
    assert robust_run["robust"]["kept"] == 4 and not np.array_equal(robust_run["U"], before_run["U"])
