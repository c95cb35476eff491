"""Sparse side information (`gibbs(..., row_features=<scipy.sparse>)`, bpmf_hip_side_set_features_sparse) on the GPU.  DESIGN.md
section 14.

  1. the two sparse products (k_sp_rows and the chunk kernels) against scipy.sparse @ dense, entry by entry within the summation
     bound 2 gamma_k |F| |V| (k: the longest row / column); bit-identical between two calls and with another grid
     (BPMF_LINK_WG_CHUNKS)
  2. the noise rows against tests/link_sparse_ref.py::randn_rows at the tolerance of the device-vs-oracle normal test (8 ulp:
     tests/test_gpu_parity.py), which also shows that the accept / reject decisions are the same
  3. the stand-alone CG solve at tol = 1e-12 against numpy.linalg.solve on the dense G; a zero column; the host's look-ahead
     (BPMF_LINK_CG_CHECK); max_iter
  4. one half-iteration per sampler family against the restatement, both at tol = 1e-12
  5. chains on MovieLens-100K and their repeatability bit for bit
  6. the planted experiment with D = 2048 binary features
  7. refusals on the device
  8. `bpmf --row-features F.sbm -o DIR --topn N` end to end against gibbs()

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import link_ref as ref
from tests import link_sparse_ref as sref
from tests import probit_ref
from tests import util
from tests.test_gpu_link import _Env, _bpmf, _compare_chain, _fields, _pair, gamma

pytestmark = pytest.mark.gpu

TOL = 1e-12


# ---- 1. the products -----------------------------------------------------------------------------------------------------------------

def _with_full_column(F, col=0):
    """F with feature `col` present in every row"""
    F = sp.lil_matrix(F)
    F[:, col] = 1.0
    return F.tocsr()


def _product_cases():
    cases = {
        "N1": lambda: sp.csr_matrix(np.array([[0.0, 2.0, 0.0, -1.0]])),
        "D1": lambda: sp.csr_matrix((np.arange(700) % 3 == 0).astype(np.float64).reshape(-1, 1)),                 # a 234-entry column, empty rows
        "tiny_all_zero": lambda: sp.csr_matrix((5, 7)),
        "empty_rows_and_columns": lambda: sp.hstack([sp.csr_matrix((340, 10)), sp.vstack([sref.random_sparse(300, 90, 0.05, 1),
                                                                                           sp.csr_matrix((40, 90))])]).tocsr(),
        "values": lambda: sref.random_sparse(5000, 700, 0.01, 2),
        "bits_full_column": lambda: sref.skewed_bits(3000, 400, 16, 3),                                               # column 0 in all 3000 rows: chunked
        "values_full_column": lambda: (_with_full_column(sref.random_sparse(2500, 300, 0.02, 4), 17)).multiply(1.5).tocsr(),
        "long_row": lambda: sp.vstack([sref.random_sparse(50, 2000, 0.01, 5), sp.csr_matrix(np.ones((1, 2000))),
                                       sref.random_sparse(50, 2000, 0.5, 6)]).tocsr(),                                 # rows of 2000 and ~1000 nonzeros
        "D200000": lambda: _with_full_column(sref.random_sparse(4000, 200000, 1e-4, 7, binary=True), 199999),
    }
    return cases


PRODUCT_N = {"N1": [8, 128], "D1": [10, 64], "tiny_all_zero": [8], "empty_rows_and_columns": [8, 10, 32, 64, 100, 128], "values": [32, 100],
             "bits_full_column": [8, 10, 32, 64, 100, 128], "values_full_column": [10, 64, 128], "long_row": [8, 100], "D200000": [8, 64]}


@pytest.mark.parametrize("name,n", [(name, n) for name in PRODUCT_N for n in PRODUCT_N[name]])
def test_sparse_products_against_scipy(name, n):
    from bpmf_amd import engine
    F = _product_cases()[name]()
    N, D = F.shape
    rng = np.random.default_rng(N + 7 * n)
    V, X, P = rng.standard_normal((D, n)), rng.standard_normal((N, n)), rng.standard_normal((D, n))
    absF = abs(F)
    krow = int(np.diff(F.indptr).max()) if F.nnz else 0
    kcol = int(np.diff(F.tocsc().indptr).max()) if F.nnz else 0
    # F V: k = the longest row
    got = engine.link_spmm_nn(F, V)
    want = F @ V
    bound = 2.0 * gamma(max(krow, 1)) * (absF @ np.abs(V))
    assert got.shape == want.shape and np.all(np.abs(got - want) <= bound)
    worst_nn = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    assert np.array_equal(got, engine.link_spmm_nn(F, V))
    with _Env("BPMF_LINK_WG_CHUNKS", 3):
        assert np.array_equal(got, engine.link_spmm_nn(F, V))
    # F^T X and F^T X + lambda P: k = the longest column (+ 1 term)
    got_t = engine.link_spmm_tn(F, X)
    want_t = F.T @ X
    bound_t = 2.0 * gamma(max(kcol, 1)) * (absF.T @ np.abs(X))
    assert got_t.shape == want_t.shape and np.all(np.abs(got_t - want_t) <= bound_t)
    worst_tn = float((np.abs(got_t - want_t) / np.maximum(bound_t, 1e-300)).max())
    got_p = engine.link_spmm_tn(F, X, 2.5, P)
    assert np.all(np.abs(got_p - (want_t + 2.5 * P)) <= 2.0 * gamma(kcol + 1) * (absF.T @ np.abs(X) + 2.5 * np.abs(P)))
    assert np.array_equal(got_t, engine.link_spmm_tn(F, X)) and np.array_equal(got_p, engine.link_spmm_tn(F, X, 2.5, P))
    with _Env("BPMF_LINK_WG_CHUNKS", 3):
        assert np.array_equal(got_t, engine.link_spmm_tn(F, X)) and np.array_equal(got_p, engine.link_spmm_tn(F, X, 2.5, P))
    print("%s n %d (%d x %d, nnz %d, longest row %d column %d): max |err| / bound nn %.3g tn %.3g" % (name, n, N, D, F.nnz, krow, kcol,
                                                                                                       worst_nn, worst_tn))


def test_product_cases_cover_the_chunked_paths():
    """the shapes above do reach the chunk kernels: a column and a row longer than the 512 nonzeros of a chunk"""
    cases = _product_cases()
    assert int(np.diff(cases["bits_full_column"]().tocsc().indptr).max()) == 3000
    assert int(np.diff(cases["long_row"]().indptr).max()) == 2000
    assert cases["D200000"]().shape[1] == 200000 and int(np.diff(cases["D200000"]().tocsc().indptr).max()) == 4000


# ---- 2. the noise rows ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 8, 20, 64, 100, 128])
def test_noise_rows_against_restatement(K):
    from bpmf_amd import engine
    nrows, it, key = 203, 7, ref.TAG_USERS + sref.KEY_Z2
    want = sref.randn_rows(nrows, K, it, key)
    got = engine.link_noise_rows(nrows, K, it, key)
    # identical accept / reject decisions (a different decision shifts every later normal of the row); log / sqrt may differ in the last ulps
    assert np.allclose(got, want, rtol=4e-16 * 8, atol=0)
    assert np.array_equal(got, engine.link_noise_rows(nrows, K, it, key))
    assert np.array_equal(got[:50], engine.link_noise_rows(50, K, it, key))                  # a row does not depend on the grid
    assert not np.any(got == engine.link_noise_rows(nrows, K, it + 1, key))
    # times R^-T: K terms per entry, each normal within 8 ulp
    rng = np.random.default_rng(K)
    Rinv = np.triu(rng.standard_normal((K, K))) + 3.0 * np.eye(K)
    got_r = engine.link_noise_rows(nrows, K, it, key, Rinv)
    bound = (8 * 4e-16 + 2.0 * gamma(K)) * (np.abs(want) @ np.abs(Rinv).T)
    assert np.all(np.abs(got_r - want @ Rinv.T) <= bound)


# ---- 3. the CG solve -----------------------------------------------------------------------------------------------------------------

CG_CASES = [("values", 2000, 300, 0.02, 1.0, 8), ("values", 500, 3000, 0.004, 0.5, 20), ("bits", 3000, 1000, 12, 5.0, 64),
            ("bits", 1500, 200, 8, 2.0, 128), ("values", 400, 1, 0.5, 1.0, 10)]


def _cg_input(kind, N, D, dens, seed):
    return sref.skewed_bits(N, D, dens, seed) if kind == "bits" else sref.random_sparse(N, D, dens, seed)


@pytest.mark.parametrize("kind,N,D,dens,lam,n", CG_CASES)
def test_cg_solve_against_dense_solve(kind, N, D, dens, lam, n):
    """|x - x*| <= kappa |r| / |b| |x*| for the true residual r; the recursion residual the solve stops on may differ from the true
    one, hence the factor 4 on kappa tol."""
    from bpmf_amd import engine
    F = _cg_input(kind, N, D, dens, 11 + n)
    rng = np.random.default_rng(n)
    RHS = rng.standard_normal((D, n))
    RHS[:, n // 2] = 0.0
    G = (F.T @ F).toarray() + lam * np.eye(D)
    kappa = float(np.linalg.cond(G))
    want = np.linalg.solve(G, RHS)
    x, iters, hit = engine.link_cg_solve(F, lam, RHS, TOL, 5000)
    err = [np.linalg.norm(x[:, k] - want[:, k]) / max(np.linalg.norm(want[:, k]), 1e-300) for k in range(n) if k != n // 2]
    print("%s %d x %d n %d: kappa %.3g, iterations %d..%d, max |x - x*| / |x*| %.3g (bound %.3g)" % (kind, N, D, n, kappa, iters.min(), iters.max(),
                                                                                                   max(err), 4 * kappa * TOL))
    assert not hit
    assert max(err) <= 4.0 * kappa * TOL
    assert iters[n // 2] == 0 and np.all(x[:, n // 2] == 0.0) and not np.any(np.signbit(x[:, n // 2]))
    assert np.all(np.delete(iters, n // 2) > 0)
    # the host's look-ahead changes nothing: a converged column is frozen on the device
    for check in (1, 8):
        with _Env("BPMF_LINK_CG_CHECK", check):
            x2, it2, _ = engine.link_cg_solve(F, lam, RHS, TOL, 5000)
        assert np.array_equal(x, x2) and np.array_equal(iters, it2), check
    with _Env("BPMF_LINK_WG_CHUNKS", 3):
        x3, it3, _ = engine.link_cg_solve(F, lam, RHS, TOL, 5000)
    assert np.array_equal(x, x3) and np.array_equal(iters, it3)


def test_cg_solve_stopped_at_max_iter_is_the_restatement():
    """Three iterations of the same recurrence.  The device and numpy add the D (N) terms of a scalar (product) in different orders:
    each alpha, beta differs by at most sqrt(kappa) gamma relative (p . q = p^T G p may cancel down to |p| |q| / sqrt(kappa)), and x
    is a sum of three alpha p: bound 16 kappa gamma_max(N, D) |x| per column."""
    from bpmf_amd import engine
    F = sref.skewed_bits(3000, 1000, 12, 5)
    N, D = F.shape
    rng = np.random.default_rng(2)
    RHS = rng.standard_normal((D, 20))
    RHS[:, 3] = 0.0
    kappa = float(np.linalg.cond((F.T @ F).toarray() + 5.0 * np.eye(D)))
    want, wit, whit = sref.cg_lockstep(F, F.T.tocsr(), 5.0, RHS, 1e-6, 3)
    for check in (1, 8):
        with _Env("BPMF_LINK_CG_CHECK", check):
            x, iters, hit = engine.link_cg_solve(F, 5.0, RHS, 1e-6, 3)
        assert hit and whit and np.array_equal(iters, wit) and iters.max() == 3 and iters[3] == 0
        err = np.linalg.norm(x - want, axis=0) / np.maximum(np.linalg.norm(want, axis=0), 1e-300)
        print("check %d: max |x - restatement| / |x| %.3g (bound %.3g, kappa %.3g)" % (check, err.max(), 16 * kappa * gamma(max(N, D)), kappa))
        assert err.max() <= 16.0 * kappa * gamma(max(N, D))


# ---- 4. one half-iteration from random state -----------------------------------------------------------------------------------------

def _half_iteration(oracle, K, A, nrows, D, seed, pattern=None):
    import bpmf_amd
    rng = np.random.default_rng(seed)
    ncols = len(A[0]) - 1
    sigma = (2.0 / K) ** 0.25
    X, Y = sigma * rng.standard_normal((ncols, K)), sigma * rng.standard_normal((nrows, K))
    F = sref.skewed_bits(ncols, D, 6, seed)
    beta = 0.3 * rng.standard_normal((D, K))
    link = sref.SparseLink(F, 5.0, TOL, 1000)
    kappa = link.cond
    bound = 4.0 * kappa * TOL
    assert bound <= 1e-9, kappa
    mean = util.mean_rating(A)
    st = dict(U=X.copy(), cov=np.zeros((K, K)), beta=beta.copy(), M=F @ beta)
    sref.half_iteration(oracle, K, A, mean, 2.0, st, Y, 0, ref.TAG_MOVIES, link)
    eng = bpmf_amd.HipEngine(K)
    try:
        me, ot = _pair(eng, A, nrows, X, Y, F, 5.0, ref.TAG_MOVIES)
        eng.link_cg_set(me, TOL, 1000)
        eng.link_set(me, beta)
        assert np.array_equal(eng.link_get(me)[0], beta)
        if pattern is not None:
            import re
            assert re.search(pattern, eng.kernel_name(me)), eng.kernel_name(me)
        info = eng.schedule_info(me)
        eng.link_sample(me, ot, 2.0)
        got_beta, got_m = eng.link_get(me)
        got_u = eng.get_items(me)
        it, nrm, cov, mu, LF, LU = eng.sys_state(me)
        stats = eng.link_cg_stats(me)
    finally:
        eng.close()
    eb = np.abs(got_beta - st["beta"]).max() / np.abs(st["beta"]).max()
    eu = np.abs(got_u - st["U"]).max() / np.abs(st["U"]).max()
    em = np.abs(got_m - st["M"]).max() / np.abs(st["M"]).max()
    ec = np.abs(cov - st["cov"]).max() / np.abs(st["cov"]).max()
    print("K %d (%s): beta %.3g factors %.3g offsets %.3g cov %.3g; cond(G) %.3g bound %.3g; CG iterations %d / %d" % (
        K, pattern, eb, eu, em, ec, kappa, bound, stats["iters_last"], link.iters[-1]))
    assert it == 0 and not stats["hit_max_iter"] and stats["relres_max_last"] <= TOL
    assert 0 < stats["iters_last"] < 1000 and stats["iters_total"] == stats["iters_last"]
    assert eb <= bound and eu <= bound and em <= bound
    assert np.abs(mu - st["mu"]).max() <= 1e-9 * max(1.0, np.abs(st["mu"]).max())
    assert ec <= 1e-8
    assert abs(nrm - float((st["U"] ** 2).sum())) <= 1e-9 * nrm
    return info


@pytest.mark.parametrize("K", [8, 16, 32])
@pytest.mark.parametrize("mode", [1, 3])
def test_half_iteration_small_k(oracle, K, mode):
    M, Mt, T, Tt, nu, nm = util.ml100k()
    with _Env("BPMF_HIP_MODE", mode):
        _half_iteration(oracle, K, M, nu, 48, 300 + K + mode, {1: r"k_sample1", 3: r"k_sample4"}[mode])


def test_half_iteration_k64_product_form_and_slab(oracle):
    from tests.test_gpu_probit import _product_form_side
    A, nrows = _product_form_side(np.random.default_rng(864))
    info = _half_iteration(oracle, 64, A, nrows, 48, 364, r"k_sample_pf")
    assert info["pf_le3"] > 0 and info["pf_4to6"] > 0 and info["pf_7to16"] > 0 and info["other_items"] > 0, info


def test_half_iteration_k64_chunked_column(oracle):
    M, Mt, nu, nm = probit_ref.skewed()
    info = _half_iteration(oracle, 64, M, nu, 48, 365)
    assert info["chunked_columns"] > 0, info


@pytest.mark.parametrize("K", [128, 20, 100])
def test_half_iteration_large_and_padded_k(oracle, K):
    M, Mt, T, Tt, nu, nm = util.ml100k()
    _half_iteration(oracle, K, M, nu, 48, 400 + K)


# ---- 5. chains -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,rows,cols", [(8, True, False), (8, False, True), (8, True, True), (64, True, True)])
def test_chain_against_restatement(oracle, K, rows, cols):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    Fr = sref.skewed_bits(nu, 256, 16, 1) if rows else None
    Fc = sref.random_sparse(nm, 1500, 0.01, 2) if cols else None                              # D = 1500: past the dense limit
    nsims, burnin = 8, 3
    want = sref.restate_chain(oracle, K, M, Mt, T, nsims, burnin, row_features=Fr, col_features=Fc, lam=5.0, tol=TOL)
    assert not want["hit_max_iter"]
    runs = []
    for _ in range(2 if K == 8 else 1):
        eng = bpmf_amd.HipEngine(K)
        try:
            runs.append(bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, Tt=Tt, row_features=Fr, col_features=Fc,
                                       lambda_beta=5.0, link_tol=TOL))
        finally:
            eng.close()
    res = runs[0]
    _compare_chain(res, want, rows, cols)
    assert len(res["link_cg_iters"]) == nsims and not res["link_cg_hit_max_iter"]
    for i, (im, iu) in enumerate(res["link_cg_iters"]):
        assert (im is None) == (not cols) and (iu is None) == (not rows)
        # (the counts are reported, not compared: at tol = 1e-12 the residual crosses the threshold near its rounding floor, where
        #  two summation orders may differ by a few iterations)
        assert (im is None or 0 < im < 1000) and (iu is None or 0 < iu < 1000)
    print("CG iterations (movies, users): device %s, restatement %s" % (res["link_cg_iters"], list(zip(want["cg_iters"]["movies"] or [None] * nsims,
                                                                                                      want["cg_iters"]["users"] or [None] * nsims))))
    if len(runs) == 2:                                                       # the same call twice: bits
        assert np.array_equal(runs[0]["U"], runs[1]["U"]) and np.array_equal(runs[0]["V"], runs[1]["V"])
        assert runs[0]["link_cg_iters"] == runs[1]["link_cg_iters"]
        for key, have in (("beta_rows", rows), ("beta_cols", cols)):
            if have:
                assert np.array_equal(runs[0][key], runs[1][key])


# ---- 6. the planted experiment -------------------------------------------------------------------------------------------------------

def test_planted_sparse_features_help_cold_rows(oracle):
    """3000 users x 300 movies, rank 4, D = 2048 binary user features (column d on with probability ~ 1 / (d + 1), 32 bits per user
    on average, feature 0 on for everyone: 95 416 nonzeros), true U = F B + 0.2 noise, B ~ N(0, 1 / 32), 12 ratings per user,
    alpha = 4; 30 % of the warm users' ratings and every rating of the last 500 users are the test set (14 979 entries, 6 000 of
    them on cold rows); K = 8, lambda_beta = 5, 60 iterations, 30 of them burn-in.  The dense path refuses D = 2048.

    (i) the GPU chain equals the restatement at the chain bars (1e-6), both with CG at tol = 1e-12.
    (ii) in the restatement at the default tol = 1e-6, measured on the CPU before this test was written: cold-row RMSE 1.0775 with
    features against 2.0907 without (the mean predictor: 2.0731); warm rows 0.7046 against 0.8299; 83 .. 93 CG iterations per
    draw, cond(G) = 5.2e3.  The margin on cold rows, 1.0132, is asserted at half its size.  (The restatement with CG at 1e-12
    against the restatement with numpy.linalg.solve on the dense G: the per-iteration RMSEs differ by at most 3.9e-13, the factors
    by 4.2e-11 relative -- the chain bar holds under CG.)"""
    import bpmf_amd
    P = sref.PLANTED
    M, Mt, T, Tt, F, cold = sref.planted_data(**P)
    assert F.shape == (3000, 2048) and F.nnz == 95416 and F[:, 0].nnz == 3000
    assert len(T[2]) == 14979 and int(cold.sum()) == 6000
    kw = dict(lam=P["lam"], alpha=P["alpha"], predictions=True)
    with_f = sref.restate_chain(oracle, P["K"], M, Mt, T, P["nsims"], P["burnin"], row_features=F, tol=P["tol"], **kw)
    without = sref.restate_chain(oracle, P["K"], M, Mt, T, P["nsims"], P["burnin"], **kw)
    tight = sref.restate_chain(oracle, P["K"], M, Mt, T, P["nsims"], P["burnin"], row_features=F, tol=TOL, **kw)
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        with pytest.raises(bpmf_amd.BpmfHipError):
            bpmf_amd.gibbs(eng, M, Mt, T, P["nusers"], P["nmovies"], nsims=1, burnin=0, row_features=F.toarray())
    finally:
        eng.close()
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, P["nusers"], P["nmovies"], nsims=P["nsims"], burnin=P["burnin"], alpha=P["alpha"], Tt=Tt,
                             row_features=F, lambda_beta=P["lam"], link_tol=TOL)
    finally:
        eng.close()
    _compare_chain(res, tight, True, False)
    its = [iu for _, iu in res["link_cg_iters"]]
    print("CG iterations per draw at 1e-12: device %d..%d, restatement %d..%d; at 1e-6 restatement %d..%d" % (
        min(its), max(its), min(tight["cg_iters"]["users"]), max(tight["cg_iters"]["users"]), min(with_f["cg_iters"]["users"]),
        max(with_f["cg_iters"]["users"])))
    warm_f, cold_f = sref.split_rmse(with_f["pred"], T, cold)
    warm_0, cold_0 = sref.split_rmse(without["pred"], T, cold)
    print("restatement: with features warm %.4f cold %.4f; without warm %.4f cold %.4f" % (warm_f, cold_f, warm_0, cold_0))
    assert len(with_f["pred"]) == len(T[2]) == len(without["pred"])
    assert cold_0 - cold_f >= 0.5 * 1.0132


# ---- 7. refusals on the device -------------------------------------------------------------------------------------------------------

def test_sparse_refusals_on_the_device():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    F = sref.skewed_bits(nm, 30, 4, 9)

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
        Fu = sref.skewed_bits(nu, 30, 4, 10)
        refused(lambda: eng.set_features(users, Fu, 0.0))
        refused(lambda: eng.set_features(users, Fu, 5.0, 0))
        assert "0x10000" in refused(lambda: eng.set_features(users, Fu, 5.0, 0x10000))
        bad = Fu.copy().astype(np.float64); bad.data[5] = np.inf
        refused(lambda: eng.set_features(users, bad))
        # bad CSR straight through the C ABI: unsorted, duplicate, out of range, rowptr not starting at 0
        rowptr, colidx, _ = bpmf_amd.engine.csr_arrays(Fu)
        first = int(np.nonzero(np.diff(rowptr) >= 2)[0][0])
        lib, ptr = eng.lib, lambda a: a.ctypes.data

        def raw(rp, ci, D=30):
            return lib.bpmf_hip_side_set_features_sparse(users.handle, D, ptr(rp), ptr(ci), None, 5.0, 4)
        swapped = colidx.copy(); p = rowptr[first]; swapped[p], swapped[p + 1] = colidx[p + 1], colidx[p]
        dup = colidx.copy(); dup[p + 1] = dup[p]
        assert raw(rowptr, swapped) == -1 and "sorted" in lib.bpmf_hip_last_error().decode()
        assert raw(rowptr, dup) == -1
        assert raw(rowptr, colidx, D=int(colidx.max())) == -1 and "outside" in lib.bpmf_hip_last_error().decode()
        shifted = rowptr.copy(); shifted[0] = 1
        assert raw(shifted, colidx) == -1
        refused(lambda: eng.link_get(users))
        refused(lambda: eng.link_cg_stats(users))
        eng.set_features(users, Fu, 5.0, 4)
        refused(lambda: eng.set_features(users, Fu, 5.0, 4))                                  # twice
        refused(lambda: eng.set_features(users, Fu.toarray(), 5.0, 4))                        # and not a dense one on top
        refused(lambda: eng.link_cg_set(users, 0.0, 10))
        refused(lambda: eng.link_cg_set(users, 1e-6, 0))
        assert "bpmf_hip_link_sample" in refused(lambda: eng.sys_sample(users, movies, 2.0))
        refused(lambda: eng.set_probit(users, 3.0, 2))
        refused(lambda: eng.link_mean(users))
        assert eng.link_cg_stats(users) == dict(iters_last=0, iters_total=0, relres_max_last=0.0, hit_max_iter=False)
    finally:
        eng.close()
    eng = bpmf_amd.HipEngine(8)
    try:
        dense_side = eng.side_create(nu, nm, *Mt, 0.0)
        eng.set_features(dense_side, ref.features(nu, 4, 1), 5.0, 4)
        assert "sparse" in refused(lambda: eng.link_cg_set(dense_side, 1e-6, 10))
        assert "sparse" in refused(lambda: eng.link_cg_stats(dense_side))
        refused(lambda: eng.set_features(dense_side, sref.skewed_bits(nu, 30, 4, 10), 5.0, 4))
    finally:
        eng.close()


def test_max_iter_is_reported_not_an_error():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    F = sref.skewed_bits(nu, 256, 16, 1)
    eng = bpmf_amd.HipEngine(8)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=3, burnin=1, Tt=Tt, row_features=F, link_tol=TOL, link_max_iter=4)
        st = eng.link_cg_stats(res["users"].side)
    finally:
        eng.close()
    assert res["link_cg_hit_max_iter"] and [iu for _, iu in res["link_cg_iters"]][1:] == [4, 4]
    assert st["hit_max_iter"] and st["iters_last"] == 4 and st["relres_max_last"] > TOL
    assert np.all(np.isfinite(res["U"])) and res["beta_rows"].shape == (256, 8)


# ---- 8. the executable ---------------------------------------------------------------------------------------------------------------

def test_cli_sparse_features_end_to_end(tmp_path):
    """`bpmf --row-features F.sbm -o DIR --topn 5` on the planted experiment: the header names the sparse mode, D and nnz, the
    iteration lines are gibbs's, DIR/U-link.ddm is res["beta_rows"], and the top-N file is written on top."""
    import io as _io
    import bpmf_amd
    from bpmf_amd import io
    P = sref.PLANTED
    M, Mt, T, Tt, F, cold = sref.planted_data(**P)
    # ratings on a grid of 1 / 1024: their sum is exact in any order, so the mean rating `bpmf` computes (a sequential sum) and the
    # one gibbs computes (numpy's pairwise sum) are the same double and the two runs see the same input to the last bit
    M, Mt, T, Tt = ((A[0], A[1], np.round(A[2] * 1024.0) / 1024.0) for A in (M, Mt, T, Tt))
    nu, nm = P["nusers"], P["nmovies"]
    io.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    io.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    Fc = F.tocsc(); Fc.sort_indices()
    io.write_sparse(tmp_path / "F.sbm", nu, F.shape[1], (Fc.indptr, Fc.indices, Fc.data))
    (tmp_path / "out").mkdir()
    nsims, burnin = 12, 4
    r = _bpmf(["-n", "train.sdm", "-p", "test.sdm", "-d", str(P["K"]), "-i", str(nsims), "-b", str(burnin), "-a", str(P["alpha"]),
               "--row-features", "F.sbm", "--lambda-beta", str(P["lam"]), "--link-tol", "1e-8", "--link-max-iter", "500", "--topn", "5",
               "-o", "out"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "side information: row features sparse D = 2048 nnz = 95416, CG tol = 1e-08 max_iter = 500, lambda_beta = 5; blocking loop" in r.stdout
    assert "warning" not in r.stderr
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        buf = _io.StringIO()
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, alpha=P["alpha"], Tt=Tt, row_features=F,
                             lambda_beta=P["lam"], link_tol=1e-8, link_max_iter=500, out=buf)
    finally:
        eng.close()
    mine = [l for l in r.stdout.splitlines() if "iteration" in l]
    theirs = [l for l in buf.getvalue().splitlines() if "iteration" in l]
    assert len(mine) == nsims and [_fields(l) for l in mine] == [_fields(l) for l in theirs]
    beta = io.read_dense(tmp_path / "out" / "U-link.ddm")
    assert beta.shape == (2048, P["K"]) and not (tmp_path / "out" / "V-link.ddm").exists()
    assert np.abs(beta - res["beta_rows"]).max() <= 1e-12
    assert (tmp_path / "out" / "topn.csv").stat().st_size > 0
    # max_iter too small: one warning line, the run goes on
    r = _bpmf(["-n", "train.sdm", "-p", "test.sdm", "-d", str(P["K"]), "-i", "3", "-b", "1", "--row-features", "F.sbm", "--link-max-iter", "2"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("warning: the CG draw of the link matrix reached --link-max-iter 2") == 1
