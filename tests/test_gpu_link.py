"""Side information (`gibbs(..., row_features=, col_features=)`, bpmf_hip_link_sample) on the GPU.  DESIGN.md section 13.

  1. the two dense products (k_link_gemm_tn / k_link_gemm_nn) against numpy, entry by entry within the summation bound
     2 gamma_k |A|^T |B|; bit-identical between two calls and -- the implementation claims grid independence -- with the grid of the
     long-dimension product forced to another shape (BPMF_LINK_WG_CHUNKS)
  2. the residual and shift kernels on the skewed matrix of the probit latent test (a 50 000-rating column, empty columns,
     1-2-rating columns), K = 8 .. 128 incl. the padded 10 / 100
  3. one half-iteration from random state through every sampler family against tests/link_ref.py
  4. chains on MovieLens-100K with row features, column features and both, K = 8 and 64, and their repeatability bit for bit
  5. no effect without features: gibbs(row_features=None, col_features=None) returns the bits of gibbs() without the arguments
  6. the planted experiment: the GPU chain equals the restatement, and in the restatement the features lower the RMSE of cold rows
  7. refusals on the device
  8. `bpmf --row-features ... -o DIR` end to end against gibbs(), and `bpmf` without the flags against the pipelined gibbs()

Every test of this file fails on the commit before the feature (missing entry points / arguments), except
test_cli_without_the_flags_prints_no_new_line, which guards the unchanged path.
"""
import math
import os

import numpy as np
import pytest

from tests import link_ref as ref
from tests import probit_ref
from tests import util

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


def gamma(k):
    return k * U53 / (1.0 - k * U53)


class _Env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = str(self.value)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


# ---- 1. the products -----------------------------------------------------------------------------------------------------------------

# (N, D, n or "D" for A^T A, subtract a vector from B)
TN_CASES = [(1, 1, 8, False), (63, 16, 10, True), (1000, 100, 32, True), (60000, 16, 64, True), (1000, 1024, 128, False),
            (60000, 100, 100, True), (63, 100, "D", False), (1000, 1024, "D", False), (60000, 16, "D", False), (1, 16, 128, True)]
NN_CASES = [(1, 1, 8), (63, 16, 10), (1000, 100, 32), (60000, 16, 64), (1000, 1024, 128), (60000, 100, 100), (63, 1024, 10)]


@pytest.mark.parametrize("N,D,n,sub", TN_CASES)
def test_gemm_tn_against_numpy(N, D, n, sub):
    from bpmf_amd import engine
    rng = np.random.default_rng(N + 7 * D)
    A = rng.standard_normal((N, D))
    B = None if n == "D" else rng.standard_normal((N, n))
    v = rng.standard_normal(n) if sub else None
    got = engine.link_gemm_tn(A, B, v)
    Bp = A if B is None else (B - v if sub else B)
    want = A.T @ Bp
    bound = 2.0 * gamma(N) * (np.abs(A).T @ np.abs(Bp))
    worst = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print("tn N %d D %d n %s: max |err| / bound %.3g" % (N, D, n, worst))
    assert got.shape == want.shape and np.all(np.abs(got - want) <= bound)
    assert np.array_equal(got, engine.link_gemm_tn(A, B, v))                     # call to call: bits
    with _Env("BPMF_LINK_WG_CHUNKS", 3):                                         # another grid, the same chunks: bits
        assert np.array_equal(got, engine.link_gemm_tn(A, B, v))


@pytest.mark.parametrize("N,D,n", NN_CASES)
def test_gemm_nn_against_numpy(N, D, n):
    from bpmf_amd import engine
    rng = np.random.default_rng(N + 11 * D)
    A = rng.standard_normal((N, D))
    B = rng.standard_normal((D, n))
    got = engine.link_gemm_nn(A, B)
    want = A @ B
    bound = 2.0 * gamma(D) * (np.abs(A) @ np.abs(B))
    worst = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print("nn N %d D %d n %d: max |err| / bound %.3g" % (N, D, n, worst))
    assert got.shape == want.shape and np.all(np.abs(got - want) <= bound)
    assert np.array_equal(got, engine.link_gemm_nn(A, B))


# ---- 2. residuals and shift ----------------------------------------------------------------------------------------------------------

def _pair(eng, A, nrows, X, Y, F, lam=5.0, tag=3):
    """A side over the ratings A with features F holding the factors X, and a partner without ratings holding Y."""
    ncols = len(A[0]) - 1
    me = eng.side_create(ncols, nrows, *A, util.mean_rating(A))
    ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_features(me, F, lam, tag)
    eng.set_items(me, X)
    eng.set_items(ot, Y)
    return me, ot


@pytest.mark.parametrize("K", [K for K, dt in probit_ref.LATENT_CASES if dt == "f64"])
def test_residual_and_shift(K):
    import bpmf_amd
    M, Mt, nu, nm = probit_ref.skewed()
    U, V = probit_ref.latent_factors(K, "f64", nu, nm)
    rng = np.random.default_rng(50 + K)
    for A, X, Y, D in ((M, V, U, 5), (Mt, U, V, 3)):
        ncols, nrows = len(A[0]) - 1, len(Y)
        F = rng.standard_normal((ncols, D))
        beta = rng.standard_normal((D, K)) / math.sqrt(D)
        eng = bpmf_amd.HipEngine(K)
        try:
            me, ot = _pair(eng, A, nrows, X, Y, F)
            eng.link_set(me, beta)
            b, offs = eng.link_get(me)
            assert np.array_equal(b, beta)
            want_offs = F @ beta
            assert np.all(np.abs(offs - want_offs) <= 2.0 * gamma(D) * (np.abs(F) @ np.abs(beta)))
            r = eng.link_residual(me, ot, len(A[2]))
            want = ref.residuals(A, offs, Y)
            err = float((np.abs(r - want) / (1.0 + np.abs(A[2]))).max())
            print("K %d, %d columns: residuals max err / (1 + |r|) %.3g" % (K, ncols, err))
            assert err <= 1e-12
            assert np.array_equal(r, eng.link_residual(me, ot, len(A[2])))
            nrm = eng.link_shift(me)
            got = eng.get_items(me)
            assert np.array_equal(got, X + offs)                                 # one addition: bits
            assert abs(nrm - float((got ** 2).sum())) <= 1e-12 * nrm
            if K in (10, 100):                                                   # the pad slots of a padded num_latent stay zero
                assert np.array_equal(eng.link_get(me)[1], offs)
        finally:
            eng.close()


# ---- 3. one half-iteration from random state -----------------------------------------------------------------------------------------

def _half_iteration(oracle, K, A, nrows, D, seed, pattern=None):
    import bpmf_amd
    rng = np.random.default_rng(seed)
    ncols = len(A[0]) - 1
    sigma = (2.0 / K) ** 0.25
    X, Y = sigma * rng.standard_normal((ncols, K)), sigma * rng.standard_normal((nrows, K))
    F = rng.standard_normal((ncols, D))
    beta = 0.3 * rng.standard_normal((D, K))
    link = ref.Link(F, 5.0)
    assert link.cond <= 1e3, link.cond
    mean = util.mean_rating(A)
    st = dict(U=X.copy(), cov=np.zeros((K, K)), beta=beta.copy(), M=F @ beta)
    ref.half_iteration(oracle, K, A, mean, 2.0, st, Y, 0, ref.TAG_MOVIES, link)
    eng = bpmf_amd.HipEngine(K)
    try:
        me, ot = _pair(eng, A, nrows, X, Y, F, 5.0, ref.TAG_MOVIES)
        eng.link_set(me, beta)
        if pattern is not None:
            import re
            assert re.search(pattern, eng.kernel_name(me)), eng.kernel_name(me)
        info = eng.schedule_info(me)
        eng.link_sample(me, ot, 2.0)
        got_beta, got_m = eng.link_get(me)
        got_u = eng.get_items(me)
        it, nrm, cov, mu, LF, LU = eng.sys_state(me)
    finally:
        eng.close()
    eb = np.abs(got_beta - st["beta"]).max() / np.abs(st["beta"]).max()
    eu = np.abs(got_u - st["U"]).max() / np.abs(st["U"]).max()
    ec = np.abs(cov - st["cov"]).max() / np.abs(st["cov"]).max()
    print("K %d (%s): beta %.3g factors %.3g cov %.3g, cond(G) %.3g" % (K, pattern, eb, eu, ec, link.cond))
    assert it == 0
    assert eb <= 1e-9 and eu <= 1e-9
    assert np.abs(mu - st["mu"]).max() <= 1e-9 * max(1.0, np.abs(st["mu"]).max())
    assert ec <= 1e-8
    assert abs(nrm - float((st["U"] ** 2).sum())) <= 1e-9 * nrm
    return info


@pytest.mark.parametrize("K", [8, 16, 32])
@pytest.mark.parametrize("mode", [1, 3])
def test_half_iteration_small_k(oracle, K, mode):
    M, Mt, T, Tt, nu, nm = util.ml100k()
    with _Env("BPMF_HIP_MODE", mode):
        _half_iteration(oracle, K, M, nu, 16, 300 + K + mode, {1: r"k_sample1", 3: r"k_sample4"}[mode])


def test_half_iteration_k64_product_form_and_slab(oracle):
    from tests.test_gpu_probit import _product_form_side
    A, nrows = _product_form_side(np.random.default_rng(864))
    info = _half_iteration(oracle, 64, A, nrows, 16, 364, r"k_sample_pf")
    assert info["pf_le3"] > 0 and info["pf_4to6"] > 0 and info["pf_7to16"] > 0 and info["other_items"] > 0, info


def test_half_iteration_k64_chunked_column(oracle):
    M, Mt, nu, nm = probit_ref.skewed()                                  # movie 0 has 50 000 ratings
    info = _half_iteration(oracle, 64, M, nu, 16, 365)
    assert info["chunked_columns"] > 0, info


@pytest.mark.parametrize("K", [128, 10, 100])
def test_half_iteration_large_and_padded_k(oracle, K):
    M, Mt, T, Tt, nu, nm = util.ml100k()
    _half_iteration(oracle, K, M, nu, 16, 400 + K)


# ---- 4. chains -----------------------------------------------------------------------------------------------------------------------

def _compare_chain(res, want, rows, cols):
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(res["U"] - want["U"]).max() / scale, np.abs(res["V"] - want["V"]).max() / scale
    er = np.abs(np.array(res["rmse"]) - want["rmse"]).max()
    ea = np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max()
    en = max(np.abs(np.array(res["norm_u"]) / want["norm_u"] - 1).max(), np.abs(np.array(res["norm_m"]) / want["norm_m"] - 1).max())
    eb = 0.0
    for key, have in (("beta_rows", rows), ("beta_cols", cols)):
        if have:
            eb = max(eb, np.abs(res[key] - want[key]).max() / np.abs(want[key]).max())
        else:
            assert res[key] is None
    print("U %.3g V %.3g rmse %.3g avg %.3g norms %.3g beta %.3g; final %.6f / %.6f" % (eu, ev, er, ea, en, eb, res["final_rmse_avg"],
                                                                                       want["final_rmse_avg"]))
    assert eu <= 1e-6 and ev <= 1e-6 and eb <= 1e-6
    assert er <= 1e-6 and ea <= 1e-6 and en <= 1e-6
    assert abs(res["final_rmse_avg"] - want["final_rmse_avg"]) <= 1e-6


@pytest.mark.parametrize("K", [8, 64])
@pytest.mark.parametrize("rows,cols", [(True, False), (False, True), (True, True)])
def test_chain_against_restatement(oracle, K, rows, cols):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    Fr = ref.features(nu, 16, 1) if rows else None
    Fc = ref.features(nm, 16, 2) if cols else None
    nsims, burnin = 8, 3
    want = ref.restate_chain(oracle, K, M, Mt, T, nsims, burnin, row_features=Fr, col_features=Fc, lam=5.0)
    assert want["cond"] <= 1e3
    runs = []
    for _ in range(2 if K == 8 else 1):
        eng = bpmf_amd.HipEngine(K)
        try:
            runs.append(bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, Tt=Tt, row_features=Fr, col_features=Fc,
                                       lambda_beta=5.0))
        finally:
            eng.close()
    _compare_chain(runs[0], want, rows, cols)
    if len(runs) == 2:                                                       # the same call twice: bits
        assert np.array_equal(runs[0]["U"], runs[1]["U"]) and np.array_equal(runs[0]["V"], runs[1]["V"])
        for key, have in (("beta_rows", rows), ("beta_cols", cols)):
            if have:
                assert np.array_equal(runs[0][key], runs[1][key])


# ---- 5. no effect without features ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pipelined", [False, True])
def test_no_features_is_the_plain_chain(pipelined):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    out = []
    for kw in ({}, dict(row_features=None, col_features=None)):
        eng = bpmf_amd.HipEngine(16)
        try:
            out.append(bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=5, burnin=2, Tt=Tt, pipelined=pipelined, **kw))
        finally:
            eng.close()
    a, b = out
    assert np.array_equal(a["U"], b["U"]) and np.array_equal(a["V"], b["V"])
    assert a["rmse"] == b["rmse"] and a["rmse_avg"] == b["rmse_avg"] and a["norm_u"] == b["norm_u"] and a["norm_m"] == b["norm_m"]
    assert "beta_rows" not in b and "beta_cols" not in b


def test_link_sample_without_features_is_the_stateless_half_iteration(oracle):
    """Both sides of a model step through link_sample; for a side without features that is Sys.sample's stateless branch."""
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want = oracle.gibbs(16, M, Mt, T, Tt, nsims=3, burnin=0)
    eng = bpmf_amd.HipEngine(16)
    try:
        movies = eng.side_create(nm, nu, *M, util.mean_rating(M))
        users = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt))
        for _ in range(3):
            eng.link_sample(movies, users, 2.0)
            eng.link_sample(users, movies, 2.0)
        U, V = eng.get_items(users), eng.get_items(movies)
        assert eng.sys_state(users)[0] == 2
    finally:
        eng.close()
    err = max(np.abs(U - want["U"]).max(), np.abs(V - want["V"]).max())
    assert err < 1e-8 * max(1.0, np.abs(want["U"]).max())


# ---- 6. the planted experiment -------------------------------------------------------------------------------------------------------

def test_planted_features_help_cold_rows(oracle):
    """600 users x 300 movies, rank 4, 16 user features that explain the users' factors up to noise 0.2, 12 ratings per user,
    alpha = 4; 30 % of the warm users' ratings and every rating of the last 100 users are the test set (2 992 entries, 1 200 of
    them on cold rows); K = 8, lambda_beta = 5, 60 iterations, 30 of them burn-in.

    (i) the GPU chain with features equals the restatement at the chain bars (1e-6).
    (ii) in the restatement, measured on the CPU before this test was written: cold-row RMSE 0.7930 with features against 2.3191
    without (the mean predictor: 2.2714); warm rows 0.7395 against 2.1894.  The margin on cold rows, 1.5261, is asserted at half
    its size.  Every test entry is scored."""
    import bpmf_amd
    P = ref.PLANTED
    M, Mt, T, Tt, F, cold = ref.planted_data(**P)
    assert len(T[2]) == 2992 and int(cold.sum()) == 1200
    kw = dict(lam=P["lam"], alpha=P["alpha"], predictions=True)
    with_f = ref.restate_chain(oracle, P["K"], M, Mt, T, P["nsims"], P["burnin"], row_features=F, **kw)
    without = ref.restate_chain(oracle, P["K"], M, Mt, T, P["nsims"], P["burnin"], **kw)
    assert with_f["cond"] <= 1e3
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, P["nusers"], P["nmovies"], nsims=P["nsims"], burnin=P["burnin"], alpha=P["alpha"], Tt=Tt,
                             row_features=F, lambda_beta=P["lam"])
    finally:
        eng.close()
    _compare_chain(res, with_f, True, False)
    warm_f, cold_f = ref.split_rmse(with_f["pred"], T, cold)
    warm_0, cold_0 = ref.split_rmse(without["pred"], T, cold)
    print("restatement: with features warm %.4f cold %.4f; without warm %.4f cold %.4f" % (warm_f, cold_f, warm_0, cold_0))
    assert len(with_f["pred"]) == len(T[2]) == len(without["pred"])
    assert cold_0 - cold_f >= 0.5 * 1.5261


# ---- 7. refusals on the device -------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    F = ref.features(nm, 4, 9)

    def refused(fn, code=-1):
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        return str(e.value)

    eng = bpmf_amd.HipEngine(128, dtype="f32")
    try:
        s = eng.side_create(nm, nu, *M, 0.0)
        assert "fp32" in refused(lambda: eng.set_features(s, F))
    finally:
        eng.close()
    eng = bpmf_amd.HipEngine(8)
    try:
        movies = eng.side_create(nm, nu, *M, 0.0)
        users = eng.side_create(nu, nm, *Mt, 0.0)
        eng.set_probit(movies, 3.0, 1)
        assert "probit" in refused(lambda: eng.set_features(movies, F))
        shard = eng.side_create(nm, nu, M[0][:101], M[1][:M[0][100]], M[2][:M[0][100]], 0.0, 0, 100)
        assert "whole" in refused(lambda: eng.set_features(shard, F))
        Fu = ref.features(nu, 4, 10)
        refused(lambda: eng.set_features(users, np.zeros((nu, 1025))))
        refused(lambda: eng.set_features(users, Fu, 0.0))
        refused(lambda: eng.set_features(users, Fu, 5.0, 0))
        bad = Fu.copy(); bad[5, 1] = np.inf
        refused(lambda: eng.set_features(users, bad))
        refused(lambda: eng.link_get(users))
        eng.set_features(users, Fu, 5.0, 4)
        refused(lambda: eng.set_features(users, Fu, 5.0, 4))
        assert "bpmf_hip_link_sample" in refused(lambda: eng.sys_sample(users, movies, 2.0))
        refused(lambda: eng.sample_side(users, movies, 0, 2.0, np.zeros(8), np.eye(8)))
        refused(lambda: eng.set_probit(users, 3.0, 2))
        refused(lambda: eng.link_mean(users))
    finally:
        eng.close()
    eng = bpmf_amd.HipEngine(8)
    try:
        with pytest.raises(ValueError, match="pipelined"):
            bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=0, pipelined=True, col_features=F)
        with pytest.raises(ValueError, match="probit"):
            bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=0, probit=True, col_features=F)
        with pytest.raises(ValueError, match="adaptive"):
            bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=0, noise="adaptive", col_features=F)
    finally:
        eng.close()


# ---- the executable ------------------------------------------------------------------------------------------------------------------

def _bpmf(args, cwd):
    import subprocess
    from tests.conftest import ROOT
    return subprocess.run([os.path.join(ROOT, "bpmf_amd", "bpmf")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=300)


def _fields(line):
    """An iteration line without its timing fields (items/sec, ratings/sec)"""
    return [f for f in line.split("\t") if not f.startswith(("items/sec", "ratings/sec"))]


def test_cli_planted_end_to_end(tmp_path):
    """`bpmf --row-features F.ddm -o DIR` on the planted experiment: the header names the mode, the iteration lines are gibbs's, and
    DIR/U-link.ddm is res["beta_rows"]."""
    import io as _io
    import bpmf_amd
    from bpmf_amd import io
    P = ref.PLANTED
    M, Mt, T, Tt, F, cold = ref.planted_data(**P)
    nu, nm = P["nusers"], P["nmovies"]
    io.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    io.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    io.write_dense(tmp_path / "F.ddm", F)
    (tmp_path / "out").mkdir()
    nsims, burnin = 12, 4
    r = _bpmf(["-n", "train.sdm", "-p", "test.sdm", "-d", str(P["K"]), "-i", str(nsims), "-b", str(burnin), "-a", str(P["alpha"]),
               "--row-features", "F.ddm", "--lambda-beta", str(P["lam"]), "-o", "out"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "side information: row features D = 16, lambda_beta = 5; blocking loop" in r.stdout
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        buf = _io.StringIO()
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, alpha=P["alpha"], Tt=Tt, row_features=F,
                             lambda_beta=P["lam"], out=buf)
    finally:
        eng.close()
    mine = [l for l in r.stdout.splitlines() if "iteration" in l]
    theirs = [l for l in buf.getvalue().splitlines() if "iteration" in l]
    assert len(mine) == nsims and [_fields(l) for l in mine] == [_fields(l) for l in theirs]
    beta = io.read_dense(tmp_path / "out" / "U-link.ddm")
    assert beta.shape == (16, P["K"]) and not (tmp_path / "out" / "V-link.ddm").exists()
    assert np.abs(beta - res["beta_rows"]).max() <= 1e-12
    assert io.read_dense(tmp_path / "out" / "U-mu.ddm").shape == (P["K"], nu)


def test_cli_without_the_flags_prints_no_new_line(tmp_path):
    import io as _io
    import bpmf_amd
    G = util.GOLDEN
    M, Mt, T, Tt, nu, nm = util.ml100k()
    r = _bpmf(["-i", "4", "-b", "2", "-d", "16", "-n", os.path.join(G, "ml100k-train.mtx.gz"), "-p", os.path.join(G, "ml100k-test.mtx.gz")], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "side information" not in r.stdout and "link" not in r.stdout and "lambda_beta" not in r.stdout
    head = [l.split(":")[0] for l in r.stdout.splitlines()[:r.stdout.splitlines().index("update_freq: 1") + 1] if ":" in l and not l.startswith(" ")]
    assert head[-8:] == ["hostname", "pid", "num_latent", "nprocs", "nthrds", "nsims", "burnin", "alpha", "update_freq"][-8:], head
    eng = bpmf_amd.HipEngine(16)
    try:
        buf = _io.StringIO()
        bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=4, burnin=2, Tt=Tt, pipelined=True, out=buf)
    finally:
        eng.close()
    mine = [l for l in r.stdout.splitlines() if "iteration" in l]
    theirs = [l for l in buf.getvalue().splitlines() if "iteration" in l]
    assert len(mine) == 4 and [_fields(l) for l in mine] == [_fields(l) for l in theirs]
