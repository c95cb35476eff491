"""A sampled link precision lambda_beta (`gibbs(..., lambda_beta_prior=)`, bpmf_hip_side_link_lambda_prior) and the device
factorisation of G(lambda_beta) it needs on the dense path (bpmf_hip_link_chol_solve), on the GPU.  DESIGN.md section 15.

  1. link_chol_solve over the shapes at which the blocked code can go wrong (D below, at and above a block, several blocks, the
     largest D; n below a tile, padded, the largest n): the residual of X = L^-T (L^-1 P + E) against numpy's LAPACK on the same
     input, the structure of the factor, bits from call to call, an indefinite matrix
  2. a dense side at a fixed lambda_beta through the device factorisation against the plain dense side (G^-1 from the host), one
     half-iteration per sampler family
  3. chains on MovieLens-100K against tests/link_lambda_ref.py: dense rows, dense columns, both, sparse rows; the lambda_beta traces
  4. the planted experiment, 120 iterations, lambda_beta sampled from a start of 500
  5. refusals on the device
  6. `bpmf --lambda-beta-prior` end to end

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import math
import os

import numpy as np
import pytest

from tests import link_lambda_ref as lref
from tests import link_ref as ref
from tests import link_sparse_ref as sref
from tests import util
from tests.test_gpu_link import _Env, _bpmf, _compare_chain, _fields, _pair

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
ENUM = -5


# ---- 1. the factorisation and the solves -----------------------------------------------------------------------------------------------

def _spd(D, kind):
    if kind == "features":                                               # A = F^T F + lambda I, F: 2 D + 3 rows of N(0, 1)
        F = ref.features(2 * D + 3, D, 100 + D)
        return F.T @ F + 5.0 * np.eye(D)
    rng = np.random.default_rng(7 * D)                                   # "cond1e6": eigenvalues 1 .. 1e-6, a random basis
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    A = (Q * np.logspace(0, -6, D)) @ Q.T
    return 0.5 * (A + A.T)


def _lapack(A, P, E):
    from scipy.linalg import solve_triangular
    L = np.linalg.cholesky(A)
    Y = solve_triangular(L, P, lower=True)
    if E is not None:
        Y = Y + E
    return solve_triangular(L.T, Y, lower=False), L


def _residual(A, X, L, P, E):
    rhs = P if E is None else P + L @ E
    return float(np.linalg.norm(A @ X - rhs) / (np.linalg.norm(A) * np.linalg.norm(X) + np.linalg.norm(rhs)))


# (D, n, with E, matrix)
CHOL_CASES = [(1, 1, True, "features"), (5, 8, True, "features"), (63, 10, True, "features"), (64, 128, True, "features"),
              (65, 100, False, "features"), (130, 1, True, "features"), (200, 128, True, "features"), (200, 100, True, "cond1e6"),
              (1024, 128, True, "features"), (1024, 10, False, "features")]


@pytest.mark.parametrize("D,n,with_e,kind", CHOL_CASES)
def test_chol_solve_against_lapack(D, n, with_e, kind):
    from bpmf_amd import engine
    A = _spd(D, kind)
    rng = np.random.default_rng(1000 + D + n)
    P = rng.standard_normal((D, n))
    E = rng.standard_normal((D, n)) if with_e else None
    X, L = engine.link_chol_solve(A, P, E, want_factor=True)
    Xl, Ll = _lapack(A, P, E)
    floor = D * U53
    r_dev, r_lap = _residual(A, X, L, P, E), _residual(A, Xl, Ll, P, E)
    f_dev = float(np.linalg.norm(L @ L.T - A) / np.linalg.norm(A))
    f_lap = float(np.linalg.norm(Ll @ Ll.T - A) / np.linalg.norm(A))
    print("D %d n %d %s: residual %.3g (LAPACK %.3g, ratio %.3g), |L L^T - A| / |A| %.3g (LAPACK %.3g, ratio %.3g), floor %.3g, cond %.3g"
          % (D, n, kind, r_dev, r_lap, r_dev / max(r_lap, 1e-300), f_dev, f_lap, f_dev / max(f_lap, 1e-300), floor, np.linalg.cond(A)))
    assert X.shape == (D, n) and np.all(np.isfinite(X))
    assert r_dev <= max(8.0 * r_lap, floor)
    # structure: lower triangular, a positive diagonal, L L^T = A to the same kind of bound
    assert np.array_equal(L, np.tril(L)) and np.all(np.diag(L) > 0.0)
    assert f_dev <= max(8.0 * f_lap, floor)
    # the same bits from call to call
    X2, L2 = engine.link_chol_solve(A, P, E, want_factor=True)
    assert np.array_equal(X, X2) and np.array_equal(L, L2)
    if D == 200 and kind == "features":                                  # without the factor: the same solution
        assert np.array_equal(X, engine.link_chol_solve(A, P, E))


@pytest.mark.parametrize("D,bad", [(5, 2), (130, 0), (130, 70), (130, 129)])
def test_chol_solve_indefinite_matrix_is_reported_not_trapped(D, bad):
    import bpmf_amd
    from bpmf_amd import engine
    A = _spd(D, "features")
    P = np.ones((D, 3))
    good = engine.link_chol_solve(A, P)
    B = A.copy()
    B[bad, bad] = -1.0                                                   # a negative pivot in the first / a later diagonal block
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        engine.link_chol_solve(B, P)
    assert e.value.code == ENUM and "positive definite" in str(e.value)
    B[bad, bad] = np.nan
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        engine.link_chol_solve(B, P)
    assert e.value.code == ENUM
    assert np.array_equal(good, engine.link_chol_solve(A, P))           # the next call on a good matrix succeeds


# ---- 2. the old path against the new one at a fixed lambda_beta -----------------------------------------------------------------------

def _one_half_iteration(K, A, nrows, D, seed, devfac):
    import bpmf_amd
    rng = np.random.default_rng(seed)
    ncols = len(A[0]) - 1
    sigma = (2.0 / K) ** 0.25
    X, Y = sigma * rng.standard_normal((ncols, K)), sigma * rng.standard_normal((nrows, K))
    F = rng.standard_normal((ncols, D))
    beta = 0.3 * rng.standard_normal((D, K))
    eng = bpmf_amd.HipEngine(K)
    try:
        me, ot = _pair(eng, A, nrows, X, Y, F, 5.0, ref.TAG_MOVIES)
        eng.link_set(me, beta)
        if devfac:
            eng.link_lambda_set(me, 5.0)
            assert eng.link_lambda_get(me)[0] == 5.0 and not eng.link_lambda_get(me)[2]
        name = eng.kernel_name(me)
        eng.link_sample(me, ot, 2.0)
        got_beta, got_m = eng.link_get(me)
        got_u = eng.get_items(me)
        state = eng.sys_state(me)
        if devfac:                                                       # a second half-iteration at the same lambda: the factor is kept
            eng.link_sample(me, ot, 2.0)
            assert np.all(np.isfinite(eng.link_get(me)[0]))
    finally:
        eng.close()
    return dict(beta=got_beta, M=got_m, U=got_u, cov=state[2], mu=state[3], name=name, cond=float(np.linalg.cond(F.T @ F + 5.0 * np.eye(D))))


@pytest.mark.parametrize("D", [16, 200])
@pytest.mark.parametrize("K,mode", [(8, 1), (8, 3), (32, 1), (32, 3), (64, None), (100, None)])
def test_device_factor_path_equals_the_plain_dense_path(K, mode, D):
    M, Mt, T, Tt, nu, nm = util.ml100k()
    with _Env("BPMF_HIP_MODE", mode):
        old = _one_half_iteration(K, M, nu, D, 500 + K + D, False)
        new = _one_half_iteration(K, M, nu, D, 500 + K + D, True)
    if mode is not None:
        import re
        assert re.search({1: r"k_sample1", 3: r"k_sample4"}[mode], new["name"]), new["name"]
    err = {k: float(np.abs(new[k] - old[k]).max() / np.abs(old[k]).max()) for k in ("beta", "M", "U", "mu", "cov")}
    print("K %d mode %s D %d: %s, cond(G) %.3g" % (K, mode, D, " ".join("%s %.3g" % kv for kv in err.items()), old["cond"]))
    assert old["cond"] <= 10.0
    assert err["beta"] <= 1e-9 and err["M"] <= 1e-9 and err["U"] <= 1e-9
    assert err["mu"] == 0.0                                              # (the hyper-parameters do not depend on the path)


# ---- 3. chains ---------------------------------------------------------------------------------------------------------------------------

def _compare_lambda(res, want):
    worst = 0.0
    for mine, theirs in (("lambda_beta_rows", "lambda_rows"), ("lambda_beta_cols", "lambda_cols")):
        if want[theirs] is None:
            assert res[mine] is None
            continue
        a, b = np.array(res[mine]), np.array(want[theirs])
        assert a.shape == b.shape
        worst = max(worst, float(np.abs(a / b - 1.0).max()))
    print("lambda_beta traces: max relative difference %.3g" % worst)
    assert worst <= 1e-9


def _sparse_rows(nu):
    return sref.random_sparse(nu, 40, 0.1, 5)


@pytest.mark.parametrize("K,rows,cols", [(8, "dense", None), (8, None, "dense"), (8, "dense", "dense"), (64, "dense", "dense"),
                                         (8, "sparse", None)])
def test_chain_against_restatement(oracle, K, rows, cols):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    Fr = {"dense": ref.features(nu, 16, 1), "sparse": _sparse_rows(nu), None: None}[rows]
    Fc = ref.features(nm, 16, 2) if cols else None
    nsims, burnin = 8, 3
    tol = dict(tol=1e-12, max_iter=1000)
    want = lref.restate_chain(oracle, K, M, Mt, T, nsims, burnin, row_features=Fr, col_features=Fc, lam=5.0, prior=lref.DEFAULT_PRIOR, **tol)
    assert want["cond"] <= 1e3
    runs = []
    for _ in range(2 if K == 8 and rows == "dense" and cols else 1):
        eng = bpmf_amd.HipEngine(K)
        try:
            runs.append(bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, Tt=Tt, row_features=Fr, col_features=Fc,
                                       lambda_beta=5.0, lambda_beta_prior=lref.DEFAULT_PRIOR, link_tol=1e-12, link_max_iter=1000))
        finally:
            eng.close()
    res = runs[0]
    print("lambda rows %s cols %s" % (res["lambda_beta_rows"], res["lambda_beta_cols"]))
    _compare_chain(res, want, rows is not None, cols is not None)
    _compare_lambda(res, want)
    for key, have in (("lambda_beta_rows", rows), ("lambda_beta_cols", cols)):
        if have:
            assert len(res[key]) == nsims and res[key][0] == 5.0 and res[key][1] != 5.0   # no draw at the first half-iteration
    if len(runs) == 2:                                                   # the same call twice: bits
        assert np.array_equal(runs[0]["U"], runs[1]["U"]) and np.array_equal(runs[0]["V"], runs[1]["V"])
        assert runs[0]["lambda_beta_rows"] == runs[1]["lambda_beta_rows"] and runs[0]["lambda_beta_cols"] == runs[1]["lambda_beta_cols"]


def test_without_the_prior_nothing_changes():
    """gibbs(lambda_beta_prior=None) returns the bits of gibbs() without the argument, and no lambda traces."""
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    Fr = ref.features(nu, 16, 1)
    out = []
    for kw in ({}, dict(lambda_beta_prior=None)):
        eng = bpmf_amd.HipEngine(16)
        try:
            out.append(bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=4, burnin=2, Tt=Tt, row_features=Fr, **kw))
        finally:
            eng.close()
    a, b = out
    assert np.array_equal(a["U"], b["U"]) and np.array_equal(a["V"], b["V"]) and np.array_equal(a["beta_rows"], b["beta_rows"])
    assert "lambda_beta_rows" not in b and "lambda_beta_cols" not in b


# ---- 4. the planted experiment ---------------------------------------------------------------------------------------------------------

def test_planted_chain_sampled_from_500(oracle):
    """tests/link_ref.py::PLANTED with 120 iterations, 60 of them burn-in, lambda_beta sampled from a start of 500 under the default
    prior: the GPU chain equals the restatement at the chain bars (1e-6) and the lambda_beta trace to 1e-9."""
    import bpmf_amd
    P = lref.PLANTED
    runs = lref.planted_runs(oracle, ("sampled",))
    M, Mt, T, Tt, F, cold = runs["data"]
    want = runs["sampled"]
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, P["nusers"], P["nmovies"], nsims=P["nsims"], burnin=P["burnin"], alpha=P["alpha"], Tt=Tt,
                             row_features=F, lambda_beta=500.0, lambda_beta_prior=lref.DEFAULT_PRIOR)
    finally:
        eng.close()
    lam = res["lambda_beta_rows"]
    print("lambda_beta: first %s, at 40 %.3g, at 60 %.3g, 60 .. 119 in [%.3g, %.3g]" % (["%.4g" % v for v in lam[:4]], lam[40], lam[60],
                                                                                       min(lam[60:]), max(lam[60:])))
    _compare_chain(res, want, True, False)
    _compare_lambda(res, want)


# ---- 5. refusals on the device ---------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    Fm, Fu = ref.features(nm, 4, 9), ref.features(nu, 4, 10)

    def refused(fn, code=-1):
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        return str(e.value)

    eng = bpmf_amd.HipEngine(8)
    try:
        movies = eng.side_create(nm, nu, *M, 0.0)
        users = eng.side_create(nu, nm, *Mt, 0.0)
        assert "no features" in refused(lambda: eng.link_lambda_prior(movies))
        assert "no features" in refused(lambda: eng.link_lambda_set(movies, 5.0))
        assert "no features" in refused(lambda: eng.link_lambda_get(movies))
        eng.set_features(movies, Fm, 5.0, 3)
        for a0, b0 in ((0.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (math.nan, 1.0), (1.0, math.inf), (math.inf, 1.0)):
            refused(lambda: eng.link_lambda_prior(movies, a0, b0))
        for lam in (0.0, -1.0, math.nan, math.inf):
            refused(lambda: eng.link_lambda_set(movies, lam))
        assert eng.link_lambda_get(movies)[0] == 5.0 and math.isnan(eng.link_lambda_get(movies)[1]) and not eng.link_lambda_get(movies)[2]
        eng.set_features(users, Fu, 5.0, 16)                             # a tag above 15 has no lambda_beta stream
        assert "1 .. 15" in refused(lambda: eng.link_lambda_prior(users))
        eng.link_lambda_prior(movies, 1.0, 0.0)
        assert eng.link_lambda_get(movies)[2]
        eng.link_sample(movies, users, 2.0)
        eng.link_sample(users, movies, 2.0)
        assert "first half-iteration" in refused(lambda: eng.link_lambda_prior(movies, 1.0, 1.0))
        eng.link_set(movies, np.zeros((4, 8)))                           # B0 = 0 and beta = 0: the posterior has no rate
        assert "without a rate" in refused(lambda: eng.link_sample(movies, users, 2.0))
    finally:
        eng.close()
    eng = bpmf_amd.HipEngine(8)
    try:
        users = eng.side_create(nu, nm, *Mt, 0.0)
        eng.set_features(users, _sparse_rows(nu), 5.0, 4)                # a side with sparse features takes the prior too
        eng.link_lambda_prior(users, 5e-4, 5e-4)
        assert eng.link_lambda_get(users)[2]
        with pytest.raises(ValueError, match="lambda_beta_prior"):
            bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=0, lambda_beta_prior=(1.0, 1.0))
        with pytest.raises(ValueError, match="lambda_beta_prior"):
            bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=0, row_features=Fu, lambda_beta_prior=(0.0, 1.0))
    finally:
        eng.close()


# ---- 6. the executable -----------------------------------------------------------------------------------------------------------------

def test_cli_planted_end_to_end(tmp_path):
    """`bpmf --row-features F.ddm --lambda-beta-prior A0,B0 -o DIR --topn 3` on the planted experiment: the old header line stays, one
    more names the prior, the iteration lines are gibbs's, DIR/lambda_beta.csv is res["lambda_beta_rows"] with an empty column for the
    side without features, and top-N rides on top.  Without the flag the output has neither the line nor the file."""
    import io as _io
    import bpmf_amd
    from bpmf_amd import io
    P = ref.PLANTED
    M, Mt, T, Tt, F, cold = ref.planted_data(**P)
    nu, nm = P["nusers"], P["nmovies"]
    io.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    io.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    io.write_dense(tmp_path / "F.ddm", F)
    (tmp_path / "out").mkdir(); (tmp_path / "plain").mkdir()
    nsims, burnin = 12, 4
    base = ["-n", "train.sdm", "-p", "test.sdm", "-d", str(P["K"]), "-i", str(nsims), "-b", str(burnin), "-a", str(P["alpha"]),
            "--row-features", "F.ddm", "--lambda-beta", "500"]
    r = _bpmf(base + ["--lambda-beta-prior", "5e-4,5e-4", "-o", "out", "--topn", "3"], tmp_path)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    old = "side information: row features D = 16, lambda_beta = 500; blocking loop (bpmf_hip_link_sample)"
    assert old in lines
    assert lines[lines.index(old) + 1] == "lambda_beta: sampled per side, prior Gamma(shape 0.0005, rate 0.0005), initial value 500"
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        buf = _io.StringIO()
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, alpha=P["alpha"], Tt=Tt, row_features=F,
                             lambda_beta=500.0, lambda_beta_prior=(5e-4, 5e-4), out=buf, topn=3)
    finally:
        eng.close()
    mine = [l for l in lines if "iteration" in l]
    theirs = [l for l in buf.getvalue().splitlines() if "iteration" in l]
    assert len(mine) == nsims and [_fields(l) for l in mine] == [_fields(l) for l in theirs]
    rows = (tmp_path / "out" / "lambda_beta.csv").read_text().splitlines()
    assert rows[0] == "iteration,lambda_rows,lambda_cols" and len(rows) == nsims + 1
    for i, row in enumerate(rows[1:]):
        it, lr, lc = row.split(",")
        assert int(it) == i and lc == "" and abs(float(lr) / res["lambda_beta_rows"][i] - 1.0) <= 1e-9   # (two processes: the trace bar, not bits)
    beta = io.read_dense(tmp_path / "out" / "U-link.ddm")
    assert np.abs(beta - res["beta_rows"]).max() <= 1e-12
    top = (tmp_path / "out" / "topn.csv").read_text().splitlines()
    assert top[0] == "query,rank,candidate,mean,std" and len(top) > nu
    first = [l.split(",") for l in top[1:4]]
    assert [int(f[2]) - 1 for f in first] == [int(v) for v in res["topn"][0][0]]
    # without the flag: the fixed-lambda output, no new line, no file
    r0 = _bpmf(base + ["-o", "plain"], tmp_path)
    assert r0.returncode == 0, r0.stderr
    assert old in r0.stdout and "lambda_beta: sampled" not in r0.stdout and not (tmp_path / "plain" / "lambda_beta.csv").exists()
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        buf = _io.StringIO()
        bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, alpha=P["alpha"], Tt=Tt, row_features=F, lambda_beta=500.0, out=buf)
    finally:
        eng.close()
    mine = [l for l in r0.stdout.splitlines() if "iteration" in l]
    theirs = [l for l in buf.getvalue().splitlines() if "iteration" in l]
    assert len(mine) == nsims and [_fields(l) for l in mine] == [_fields(l) for l in theirs]
