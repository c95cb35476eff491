"""Rows unseen in training, predicted from their features on the device: k_predict_block, the projection of
new feature rows, w[c] = (1/S) sum_s v^T Lambda_s^-1 v, bpmf_hip_newrows_*, gibbs(new_row_features=, new_col_features=) and
`bpmf --new-row-features / --new-col-features`.

Every reference is tests/newrows_ref.py in numpy longdouble, fed with values READ BACK from the device (ring contents through
get_items per kept sample, newrows_get, link_get, sys_state), so each stage is judged on its own inputs; u = 2^-53.

  1. predict_block on rings filled through set_items + samples_add: Kt in {3, 10, 32, 64, 128} (Kp 4, 12, 32, 64, 128), S in
     {1, 2, 5} in rings reserved for 7, (nq, nc) in {(1, 1), (15, 63), (17, 65), (65, 130)}, one fp32 context at Kt = 128.
     mean: |dev - ref| <= 2 (S Kp + 3) u (|mean_rating| + (1/S) sum_s sum_k |e_sk v_sk|), the forward bound of a dot product in
     any order.  std^2: with e_p = (Kp + 2) u max_s sum_k |e_sk v_sk|,
     |dev - ref| <= 4 [4 e_p sum_s |p_s - mean| + (S + 3) u sum_s (p_s - mean)^2] / (S - 1) + 4 u ref, the first-order
     perturbation of a two-pass variance (the 4 covers second-order terms and a one-pass scheme's constant).  S = 1: exactly 0.
  2. (65, 130) whole, as four quadrants cut at (17, 65), and twice over: the same bits; predict_block_device refuses
     host memory
  3. cancellation: p_s = P + delta_s, |delta_s| ~ 1e-7 |P|, P carried by the factors: the naive sum p / sum p^2 form of the
     reference breaks the bound of (1) on this input (asserted first), the device keeps it
  4. projection: dense D in {1, 7, 64, 65} x n_new in {1, 63, 130}, a sparse case (D = 300, 0 .. 9 ones per row, an empty row);
     E within 2 (D + 2) u (|mu_k| + sum_d |F_id beta_dk|).  The pad rows of the ring (Kt = 10: components 10, 11 of every sample,
     dense and sparse) are read back as stored (newrows_get(padded=True)) and are exactly 0; the stored components below Kt are
     the bits newrows_get returns.
  5. w[c] against longdouble v^T Lambda_s^-1 v from sys_state's LambdaF, relative error <= 8 Kp u max_s kappa_2(Lambda_s), over a
     chain of three kept samples at K = 8 and K = 64
  6. newrows_topn in both directions: the lists are numpy's top-N of newrows_predict's own mean matrix in the order (mean
     descending, id ascending); n = 1 and n = 32, with 20 candidates once (empty slots -1 / 0 / 0).  The ranking kernels and the
     block kernel sum the same products in different orders, so means within twice the bound of (1) and std^2 within twice that
     of (1) stand in for "equal"; two means closer than that may swap, which the test allows for (DESIGN.md section 17 records
     this as a decision).
  7. the chain: gibbs(..., new_row_features=) at K = 8, dense D = 16, and a sparse run.  (a) res["new_rows"] against the
     restatement fed the device's own per-sample state (newrows_get and the kept factors) within the bounds of (1); (b) against
     tests/newrows_ref.py::restate_newrows, which drives link_ref.half_iteration on the CPU, within the bounds of (1), (4) and (5)
     combined to first order (newrows_ref.chain_bounds; measured: 0.02 and 0.09 of it, 1.4e-16 and 1.2e-15 of
     the scale).  The sparse run's CPU chain draws beta by tests/link_sparse_ref.py's conjugate gradients, which agree with the
     device's to the solver's tolerance and not to round-off, so no bound of (1), (4), (5) applies to it: that run is held to
     what every device chain is held to against that restatement (tests/test_gpu_link.py::_compare_chain), 1e-6 of the scale (measured: 1.4e-16 and 7.6e-16);
     (c) a run without the new arguments gives the same trace bit for bit
  8. refusals on the device: no features, wrong D, wrong kind, full ring, unequal counts, a communicator
  9. `bpmf --new-row-features / --new-col-features -o DIR` on the planted data: header line, the four .ddm shapes, the csv format,
     values equal to gibbs()'s; without the flags no new line and no new file
 10. the planted experiment with its 100 cold users taken OUT of the matrix (see its docstring for the ten numbers)

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from bpmf_amd import _lib
from tests import link_ref as ref
from tests import newrows_ref as nr
from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
f64 = lambda a: np.asarray(a, np.float64)


def kp_of(K):
    return (K + 3) // 4 * 4


def pair_of_sides(eng, nq, nc):
    """a side of nq columns and its partner of nc columns with one rating between them"""
    A = sp.coo_matrix((np.array([3.0]), (np.array([0]), np.array([0]))), shape=(nc, nq)).tocsc()      # nc x nq: one column per query
    return eng.side_create(nq, nc, *util.csc_arrays(A), 0.0), eng.side_create(nc, nq, *util.csc_arrays(A.T.tocsc()), 0.0)


def fill_rings(eng, sq, sc, Es, Vs, cap_q=7, cap_c=7):
    """the samples through set_items + samples_add; returns what the device holds (get_items: fp32 contexts round)"""
    eng.samples_reserve(sq, cap_q); eng.samples_reserve(sc, cap_c)
    Eb, Vb = [], []
    for E, V in zip(Es, Vs):
        eng.set_items(sq, E); eng.set_items(sc, V)
        Eb.append(eng.get_items(sq)); Vb.append(eng.get_items(sc))
        eng.samples_add(sq); eng.samples_add(sc)
    return np.stack(Eb), np.stack(Vb)


def check_block(mean, std, good, Kp, mr, tag, scale=1.0):
    em = np.abs(mean - f64(good["mean"])); bm = scale * f64(nr.mean_bound(good, Kp, mr))
    ev = np.abs(std * std - f64(good["var"])); bv = scale * f64(nr.var_bound(good, Kp))
    print("%s: mean err / bound %.3g, var err / bound %.3g" % (tag, (em / bm).max(), (ev / np.maximum(bv, 1e-300)).max() if good["S"] > 1 else 0.0))
    assert (em <= bm).all(), tag
    if good["S"] == 1 and good["var"].max() == 0:
        assert (std == 0.0).all(), tag
    else:
        assert (ev <= bv).all(), tag


# ---- 1. the block kernel ---------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (15, 63), (17, 65), (65, 130)]


@pytest.mark.parametrize("K,dtype", [(3, "f64"), (10, "f64"), (32, "f64"), (64, "f64"), (128, "f64"), (128, "f32")])
def test_predict_block_against_longdouble(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    mr = 3.5
    for nq, nc in SHAPES:
        sq, sc = pair_of_sides(eng, nq, nc)
        try:
            for S in (1, 2, 5):
                rng = np.random.default_rng(1000 * K + 10 * nq + S)
                Es, Vs = fill_rings(eng, sq, sc, rng.standard_normal((S, nq, K)), rng.standard_normal((S, nc, K)), 7, 7 if S != 2 else 6)
                mean, std = eng.predict_block(sq, sc, mr)
                assert mean.shape == (nq, nc) and std.shape == (nq, nc)
                check_block(mean, std, nr.predict(Es, Vs, mr), kp_of(K), mr, (K, dtype, nq, nc, S))
        finally:
            eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 2. ranges and repeats -------------------------------------------------------------------------------------------------------------

def test_predict_block_bits_do_not_depend_on_the_ranges(hip_engine_factory):
    K, nq, nc, S = 10, 65, 130, 5
    eng = hip_engine_factory(K)
    sq, sc = pair_of_sides(eng, nq, nc)
    try:
        rng = np.random.default_rng(5)
        fill_rings(eng, sq, sc, rng.standard_normal((S, nq, K)), rng.standard_normal((S, nc, K)))
        whole = eng.predict_block(sq, sc, 1.25)
        again = eng.predict_block(sq, sc, 1.25)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
        for q0, q1 in ((0, 17), (17, 65)):
            for c0, c1 in ((0, 65), (65, 130)):
                part = eng.predict_block(sq, sc, 1.25, q0, q1, c0, c1)
                assert part[0].shape == (q1 - q0, c1 - c0)
                assert np.array_equal(part[0], whole[0][q0:q1, c0:c1]) and np.array_equal(part[1], whole[1][q0:q1, c0:c1]), (q0, c0)
        empty = eng.predict_block(sq, sc, 1.25, 5, 5, 0, 130)
        assert empty[0].shape == (0, 130)
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_predict_block_device_refuses_host_memory(hip_engine_factory):
    """bpmf_hip_predict_block_device takes device memory of the context's device alone (tools/predblock_bench.py runs it on device
    tensors and compares the block with a composition of library calls); host arrays are refused and left as they were"""
    import bpmf_amd
    K, nq, nc, S = 10, 17, 65, 2
    eng = hip_engine_factory(K)
    sq, sc = pair_of_sides(eng, nq, nc)
    try:
        rng = np.random.default_rng(6)
        fill_rings(eng, sq, sc, rng.standard_normal((S, nq, K)), rng.standard_normal((S, nc, K)))
        host = np.zeros((2, nq, nc))
        with pytest.raises(bpmf_amd.BpmfHipError, match="device memory") as e:
            eng.predict_block_device(sq, sc, 1.25, host[0].ctypes.data, host[1].ctypes.data)
        assert e.value.code == -1 and not host.any()
        mean, std = eng.predict_block(sq, sc, 1.25)                          # and the context goes on working
        assert np.isfinite(mean).all() and np.isfinite(std).all()
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 3. cancellation -------------------------------------------------------------------------------------------------------------------

def test_predict_block_survives_cancellation(hip_engine_factory):
    from tests.test_newrows_host import cancelling_case
    K, nq, nc, S = 8, 17, 65, 5
    eng = hip_engine_factory(K)
    sq, sc = pair_of_sides(eng, nq, nc)
    try:
        Es, Vs = cancelling_case(nq, nc, K, S, 3)
        Es, Vs = fill_rings(eng, sq, sc, Es, Vs)
        good = nr.predict(Es, Vs, 0.0)
        P = f64(good["mean"]); spread = np.sqrt(f64(good["var"]))
        assert (np.abs(P) > 800).all() and (spread / np.abs(P) < 1e-6).all() and (spread / np.abs(P) > 1e-9).all()
        _, naive = nr.predict_naive(Es, Vs, 0.0)
        assert (np.abs(naive - f64(good["var"])) > f64(nr.var_bound(good, 8))).any()      # the input discriminates
        mean, std = eng.predict_block(sq, sc, 0.0)
        check_block(mean, std, good, 8, 0.0, "cancellation")
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 4. / 5. projection and w ----------------------------------------------------------------------------------------------------------

def linked_pair(eng, nu, nm, F, seed, iters=2, alpha=2.0):
    """users (with features F) and movies on a small random matrix, `iters` iterations of the blocking loop"""
    M, Mt, T, Tt, nu, nm = util.synthetic(nu, nm, 12 * nu, seed=seed)
    movies = eng.side_create(nm, nu, *M, util.mean_rating(M))
    users = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt))
    eng.set_features(users, F, 5.0, 4)
    for _ in range(iters):
        eng.link_sample(movies, users, alpha)
        eng.link_sample(users, movies, alpha)
    return users, movies


def check_projection(eng, users, movies, Fnew, K, D, tag):
    """two kept samples with a beta set through link_set each; E against mu + F beta in longdouble; the prediction is finite"""
    rng = np.random.default_rng(D)
    eng.newrows_set(users, Fnew, 3)
    eng.samples_reserve(movies, 3)
    want = []
    for s in range(2):
        eng.link_set(users, rng.standard_normal((D, K)))
        beta = eng.link_get(users)[0]
        mu = eng.sys_state(users)[3]
        eng.newrows_add(users, movies); eng.samples_add(movies)
        want.append(nr.project(Fnew, beta, mu))
    assert eng.newrows_count(users) == 2
    E, w = eng.newrows_get(users)
    n = Fnew.shape[0]
    assert E.shape == (n, 2, K) and w.shape == (movies.ncols,)
    worst = 0.0
    for s in range(2):
        err = np.abs(E[:, s, :] - f64(want[s][0])); bound = f64(nr.project_bound(D, want[s][1]))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (tag, s)
    print("%s: projection err / bound %.3g" % (tag, worst))
    Ep = eng.newrows_get(users, padded=True)                                   # the slots as the ring stores them
    assert Ep.shape == (n, 2, kp_of(K)) and np.array_equal(Ep[:, :, :K], E), tag
    assert (Ep[:, :, K:] == 0.0).all(), tag                                     # pad rows: exactly 0
    mean, std = eng.newrows_predict(users, movies, 0.0)
    assert mean.shape == (n, movies.ncols) and np.isfinite(mean).all() and np.isfinite(std).all() and (std > 0).all()
    return E, w


@pytest.mark.parametrize("D", [1, 7, 64, 65])
def test_projection_dense(D):
    import bpmf_amd
    K, nu, nm = 10, 80, 60                                                    # Kt = 10: the ring has two pad rows per sample
    eng = bpmf_amd.HipEngine(K)
    try:
        users, movies = linked_pair(eng, nu, nm, ref.features(nu, D, 1), seed=D)
        for n in (1, 63, 130):
            E, w = check_projection(eng, users, movies, ref.features(n, D, 100 + n), K, D, ("dense", D, n))
            # the block against the restatement on the device's own E, V, w
            V = eng.get_items(movies)
            good = nr.predict(np.transpose(E, (1, 0, 2)), np.stack([V, V]), 0.0, w)
            mean, std = eng.newrows_predict(users, movies, 0.0)
            check_block(mean, std, good, kp_of(K), 0.0, ("dense block", D, n))
    finally:
        eng.close()


@pytest.mark.parametrize("K", [8, 10])                                         # Kt = 10: two pad rows per sample
def test_projection_sparse(K):
    import bpmf_amd
    nu, nm, D, n = 80, 60, 300, 70
    rng = np.random.default_rng(9)

    def bits(rows, empty):
        A = sp.lil_matrix((rows, D))
        for i in range(rows):
            k = 0 if i == empty else int(rng.integers(0, 10))
            A[i, rng.choice(D, k, replace=False)] = 1.0
        return A.tocsr()
    eng = bpmf_amd.HipEngine(K)
    try:
        users, movies = linked_pair(eng, nu, nm, bits(nu, 3), seed=2)
        Fnew = bits(n, 5)
        assert Fnew[5].nnz == 0 and Fnew.nnz > 0
        E, w = check_projection(eng, users, movies, Fnew, K, D, ("sparse", D, n))
        mu_rows = E[5]                                                        # the empty row projects to mu itself
        assert np.array_equal(mu_rows[1], eng.sys_state(users)[3])
    finally:
        eng.close()


@pytest.mark.parametrize("K", [8, 64])
def test_w_against_longdouble(K):
    import bpmf_amd
    nu, nm, D = 300, 200, 6
    eng = bpmf_amd.HipEngine(K)
    try:
        M, Mt, T, Tt, nu, nm = util.synthetic(nu, nm, 20 * nu, seed=K)
        movies = eng.side_create(nm, nu, *M, util.mean_rating(M))
        users = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt))
        eng.set_features(users, ref.features(nu, D, 1), 5.0, 4)
        eng.newrows_set(users, ref.features(4, D, 2), 3)
        Vs, Lams, kappa = [], [], 0.0
        for it in range(5):
            eng.link_sample(movies, users, 2.0)
            eng.link_sample(users, movies, 2.0)
            if it >= 2:
                eng.newrows_add(users, movies)
                Vs.append(eng.get_items(movies)); Lams.append(np.array(eng.sys_state(users)[4]))
                kappa = max(kappa, float(np.linalg.cond(Lams[-1])))
        w = eng.newrows_get(users)[1]
        want = nr.w_of(Vs, Lams)
        rel = np.abs(w - f64(want)) / f64(want)
        bound = 8.0 * kp_of(K) * nr.U53 * kappa
        print("K %d: w rel err %.3g, bound %.3g (kappa %.3g)" % (K, rel.max(), bound, kappa))
        assert (f64(want) > 0).all() and (rel <= bound).all()
    finally:
        eng.close()


# ---- 6. top-N --------------------------------------------------------------------------------------------------------------------------

def test_newrows_topn_both_directions():
    import bpmf_amd
    K, nu, nm, D, n_new = 8, 90, 70, 5, 20
    eng = bpmf_amd.HipEngine(K)
    try:
        users, movies = linked_pair(eng, nu, nm, ref.features(nu, D, 1), seed=4, iters=3)
        eng.newrows_set(users, ref.features(n_new, D, 2), 3)
        eng.samples_reserve(movies, 4)
        Vs = []
        for _ in range(3):
            eng.link_sample(movies, users, 2.0); eng.link_sample(users, movies, 2.0)
            eng.newrows_add(users, movies); eng.samples_add(movies); Vs.append(eng.get_items(movies))
        mr = 2.75
        mean, std = eng.newrows_predict(users, movies, mr)
        E, w = eng.newrows_get(users)
        good = nr.predict(np.transpose(E, (1, 0, 2)), np.stack(Vs), mr, w)
        bm, bv = 2.0 * f64(nr.mean_bound(good, 8, mr)), 2.0 * f64(nr.var_bound(good, 8))
        for new_q, Mn, Sd, Bm, Bv in ((True, mean, std, bm, bv), (False, mean.T, std.T, bm.T, bv.T)):
            nq, nc = Mn.shape
            for n in (1, 32):
                idx, tm, ts = eng.newrows_topn(users, movies, mr, n, new_are_queries=new_q)
                assert idx.shape == (nq, n)
                want = nr.topn_of(Mn, n)
                filled = min(n, nc)
                assert (idx[:, filled:] == -1).all() and (tm[:, filled:] == 0).all() and (ts[:, filled:] == 0).all()
                assert (idx[:, :filled] >= 0).all()
                rows = np.arange(nq)[:, None]
                got = idx[:, :filled]
                assert (np.abs(tm[:, :filled] - Mn[rows, got]) <= Bm[rows, got]).all()
                assert (np.abs(ts[:, :filled] ** 2 - Sd[rows, got] ** 2) <= Bv[rows, got]).all()
                for i in range(nq):                                           # the same list, up to swaps of means closer than the bound
                    for r in np.nonzero(got[i] != want[i, :filled])[0]:
                        assert abs(Mn[i, got[i, r]] - Mn[i, want[i, r]]) <= 2 * Bm[i, got[i, r]], (new_q, n, i, r)
                    assert len(set(got[i].tolist())) == filled
                assert (np.diff(tm[:, :filled], axis=1) <= 0).all()
            if not new_q:
                assert nc == n_new < 32                                       # fewer candidates than n: the empty slots were seen
    finally:
        eng.close()


# ---- 7. the chain ----------------------------------------------------------------------------------------------------------------------

def chain_case(oracle, sparse):
    import bpmf_amd
    K, D, n_new, nsims, burnin = 8, 16, 37, 8, 4
    M, Mt, T, Tt, nu, nm = util.synthetic(300, 200, 6000, seed=11)
    if sparse:
        rng = np.random.default_rng(3)
        F = sp.csr_matrix((rng.random((nu, 40)) < 0.1).astype(float)); Fnew = sp.csr_matrix((rng.random((n_new, 40)) < 0.1).astype(float))
    else:
        F, Fnew = ref.features(nu, D, 1), ref.features(n_new, D, 2)
    eng = bpmf_amd.HipEngine(K)
    try:
        kw = dict(nsims=nsims, burnin=burnin, Tt=Tt, row_features=F, lambda_beta=5.0, link_tol=1e-13)
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, new_row_features=Fnew, keep_samples=True, **kw)
        mean, std = res["new_rows"]["mean"], res["new_rows"]["std"]
        assert mean.shape == (n_new, nm) and std.shape == (n_new, nm) and "new_cols" not in res and "new_rows_topn" not in res
        # (a) the device's own per-sample state
        E, w = eng.newrows_get(res["users"].side)
        Vs = np.stack([v for _, v in res["samples"][burnin:]])
        mr = res["movies"].mean_rating
        check_block(mean, std, nr.predict(np.transpose(E, (1, 0, 2)), Vs, mr, w), 8, mr, ("chain, device state", sparse))
        # (c) without the new arguments: the same trace, bit for bit
        plain = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, **kw)
        assert np.array_equal(plain["U"], res["U"]) and np.array_equal(plain["V"], res["V"])
        assert plain["rmse"] == res["rmse"] and plain["rmse_avg"] == res["rmse_avg"] and plain["norm_u"] == res["norm_u"]
        assert np.array_equal(plain["beta_rows"], res["beta_rows"]) and "new_rows" not in plain
    finally:
        eng.close()
    want = nr.restate_newrows(oracle, K, M, Mt, nsims, burnin, F, Fnew, lam=5.0, alpha=2.0, tol=1e-13)      # (b) the CPU chain
    scale = np.abs(want["mean"]).max()
    em, es = np.abs(mean - want["mean"]).max() / scale, np.abs(std - want["std"]).max() / want["std"].max()
    if sparse:                                                                # beta by CG on both sides: the solver's tolerance, not round-off
        print("sparse chain against the CPU restatement: mean %.3g std %.3g of the scale" % (em, es))
        assert em <= 1e-6 and es <= 1e-6
    else:
        mb, vb = nr.chain_bounds(want, Fnew, D, 8)
        rm = (np.abs(mean - f64(want["good"]["mean"])) / f64(mb)).max()
        rv = (np.abs(std * std - f64(want["good"]["var"])) / f64(vb)).max()
        print("chain against the CPU restatement: mean %.3g std %.3g of the scale; err / combined bound: mean %.3g var %.3g" % (em, es, rm, rv))
        assert rm <= 1.0 and rv <= 1.0


def test_chain_dense(oracle):
    chain_case(oracle, False)


def test_chain_sparse(oracle):
    chain_case(oracle, True)


def test_gibbs_new_cols_and_topn():
    import bpmf_amd
    K, D, n_new = 8, 6, 11
    M, Mt, T, Tt, nu, nm = util.synthetic(120, 90, 2400, seed=12)
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=3, Tt=Tt, col_features=ref.features(nm, D, 1), row_features=ref.features(nu, D, 2),
                             new_col_features=ref.features(n_new, D, 3), new_row_features=ref.features(n_new + 1, D, 4), topn=5)
        assert res["new_cols"]["mean"].shape == (nu, n_new) and res["new_cols"]["std"].shape == (nu, n_new)
        assert res["new_rows"]["mean"].shape == (n_new + 1, nm)
        idx, tm, ts = res["new_cols_topn"]
        assert idx.shape == (n_new, 5) and (idx >= 0).all() and (idx < nu).all()
        rows = np.arange(n_new)[:, None]
        # (the ranking kernels and the block kernel add the same S Kp = 24 products of size O(1) in different orders)
        np.testing.assert_allclose(tm, res["new_cols"]["mean"].T[rows, idx], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ts, res["new_cols"]["std"].T[rows, idx], rtol=1e-9, atol=1e-12)
        assert res["new_rows_topn"][0].shape == (n_new + 1, 5) and res["topn"][0].shape == (nu, 5)
    finally:
        eng.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device():
    import bpmf_amd
    K, nu, nm, D = 8, 60, 40, 4
    eng = bpmf_amd.HipEngine(K)

    def refused(fn, code=-1):
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        return str(e.value)
    try:
        M, Mt, T, Tt, nu, nm = util.synthetic(nu, nm, 600, seed=1)
        movies = eng.side_create(nm, nu, *M, util.mean_rating(M))
        users = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt))
        Fn = ref.features(5, D, 2)
        with pytest.raises(ValueError, match="no features"):
            eng.newrows_set(users, Fn, 2)
        assert "no features" in refused(lambda: _lib.check(eng.lib.bpmf_hip_side_newrows_set(users.handle, 5, Fn.ctypes.data_as(C.c_void_p), 2)))
        assert "no new rows" in refused(lambda: eng.newrows_add(users, movies))
        eng.set_features(users, ref.features(nu, D, 1), 5.0, 4)
        with pytest.raises(ValueError, match="D = 4"):
            eng.newrows_set(users, ref.features(5, D + 1, 2), 2)                # wrong D
        with pytest.raises(ValueError, match="same kind"):
            eng.newrows_set(users, sp.csr_matrix(Fn), 2)                       # wrong kind
        bad = Fn.copy(); bad[1, 1] = np.nan
        assert "not finite" in refused(lambda: eng.newrows_set(users, bad, 2))
        eng.newrows_set(users, Fn, 2)
        assert "hyper-parameters" in refused(lambda: eng.newrows_add(users, movies))      # before the first half-iteration
        eng.link_sample(movies, users, 2.0); eng.link_sample(users, movies, 2.0)
        assert "sample ring" in refused(lambda: eng.newrows_predict(users, movies, 0.0))
        eng.samples_reserve(movies, 3)
        assert "same number" in refused(lambda: eng.newrows_predict(users, movies, 0.0))  # 0 and 0
        eng.newrows_add(users, movies)
        assert "same number" in refused(lambda: eng.newrows_topn(users, movies, 0.0, 3))  # 1 against 0
        eng.samples_add(movies)
        eng.newrows_predict(users, movies, 0.0)
        assert "wrong number of columns" in refused(lambda: eng.newrows_predict(users, users, 0.0))
        assert "out of bounds" in refused(lambda: eng.newrows_predict(users, movies, 0.0, 0, 6))
        assert "out of bounds" in refused(lambda: eng.newrows_predict(users, movies, 0.0, 0, 5, 0, nm + 1))
        refused(lambda: eng.newrows_topn(users, movies, 0.0, 33))
        eng.newrows_add(users, movies)
        assert "full" in refused(lambda: eng.newrows_add(users, movies))         # full ring
        assert "same number" in refused(lambda: eng.newrows_predict(users, movies, 0.0))  # 2 against 1
        assert "sample ring" in refused(lambda: eng.predict_block(users, movies, 0.0))    # predict_block: no ring on the queries
        eng.samples_reserve(users, 2); eng.samples_add(users)
        eng.predict_block(users, movies, 0.0)
        eng.samples_add(users)
        assert "same number" in refused(lambda: eng.predict_block(users, movies, 0.0))    # 2 against 1
        eng.newrows_set(users, None, 0)                                        # freed
        assert eng.newrows_count(users) == 0
        assert "no new rows" in refused(lambda: eng.newrows_predict(users, movies, 0.0))
    finally:
        eng.close()


_COMM_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bpmf_amd
eng = bpmf_amd.HipEngine(8)
eng.comm_init(1, 0, eng.comm_unique_id())
a = eng.side_create(2, 4, np.array([0, 4, 6], np.int64), np.array([0, 1, 2, 3, 0, 2], np.int32), np.array([2., 3., 7., 4., 5., 1.]), 3.0)
b = eng.side_create(4, 2, np.array([0, 2, 3, 5, 6], np.int64), np.array([0, 1, 0, 0, 1, 0], np.int32), np.array([2., 5., 3., 7., 1., 4.]), 3.0)
eng.samples_reserve(a, 1); eng.samples_reserve(b, 1); eng.samples_add(a); eng.samples_add(b)
try:
    eng.predict_block(a, b, 0.0)
    print("ACCEPTED")
except bpmf_amd.BpmfHipError as e:
    print("REFUSED %d %s" % (e.code, e))
eng.close()
"""


def test_predict_block_refuses_a_context_with_a_communicator():
    """In a process of its own: a communicator is process-wide state of the communication library."""
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("BPMF_HIP_RCCL_LIBRARY", None)
    r = subprocess.run([sys.executable, "-c", _COMM_CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert re.search(r"^REFUSED -1 .*predict_block: .*communicator", r.stdout, re.M), r.stdout


# ---- 9. the executable -----------------------------------------------------------------------------------------------------------------

def _bpmf(args, cwd):
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def _csv(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "query,rank,candidate,mean,std"
    return np.array([l.split(",") for l in lines[1:]], dtype=float)


def test_cli_planted_end_to_end(tmp_path):
    import bpmf_amd
    from bpmf_amd import io
    P = ref.PLANTED
    sp_ = nr.planted_split(P)
    M, Mt = sp_["Mw"], sp_["Mtw"]
    nu, nm, K = sp_["nw"], P["nmovies"], P["K"]
    Fm, Fm_new = ref.features(nm, 5, 7), ref.features(9, 5, 8)
    T, Tt = sp_["Tw"], sp_["Ttw"]                                            # the test entries of the warm users
    io.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    io.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    io.write_dense(tmp_path / "F.ddm", sp_["F_warm"]); io.write_dense(tmp_path / "Fnew.ddm", sp_["F_cold"])
    io.write_dense(tmp_path / "G.ddm", Fm); io.write_dense(tmp_path / "Gnew.ddm", Fm_new)
    (tmp_path / "out").mkdir(); (tmp_path / "plain").mkdir()
    nsims, burnin, N = 10, 4, 7
    base = ["-n", "train.sdm", "-p", "test.sdm", "-d", str(K), "-i", str(nsims), "-b", str(burnin), "-a", str(P["alpha"]),
            "--row-features", "F.ddm", "--col-features", "G.ddm", "--lambda-beta", str(P["lam"])]
    r = _bpmf(base + ["--new-row-features", "Fnew.ddm", "--new-col-features", "Gnew.ddm", "--topn", str(N), "-o", "out"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "new rows: 100 (--new-row-features)" in r.stdout and "new columns: 9 (--new-col-features)" in r.stdout
    r0 = _bpmf(base + ["-o", "plain"], tmp_path)
    assert r0.returncode == 0, r0.stderr
    assert "new rows" not in r0.stdout and "new columns" not in r0.stdout and not list((tmp_path / "plain").glob("new-*"))
    strip = lambda text: [[f for f in l.split("\t") if not f.startswith(("items/sec", "ratings/sec"))] for l in text.splitlines() if "iteration" in l]
    assert strip(r.stdout) == strip(r0.stdout) and len(strip(r.stdout)) == nsims
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=nsims, burnin=burnin, alpha=P["alpha"], Tt=Tt, row_features=sp_["F_warm"],
                             col_features=Fm, lambda_beta=P["lam"], new_row_features=sp_["F_cold"], new_col_features=Fm_new, topn=N)
    finally:
        eng.close()
    for name, want in (("new-rows-mean", res["new_rows"]["mean"]), ("new-rows-std", res["new_rows"]["std"]),
                       ("new-cols-mean", res["new_cols"]["mean"]), ("new-cols-std", res["new_cols"]["std"])):
        got = io.read_dense(tmp_path / "out" / (name + ".ddm"))
        assert got.shape == want.shape == ((100, nm) if "rows" in name else (nu, 9)), name
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12, err_msg=name)
    for name, key, nq in (("new-rows-topn.csv", "new_rows_topn", 100), ("new-cols-topn.csv", "new_cols_topn", nu)):
        rec = _csv(tmp_path / "out" / name)
        assert rec.shape == (nq * N, 5)
        assert (rec[:, 0].reshape(nq, N) == np.arange(1, nq + 1)[:, None]).all() and (rec[:, 1].reshape(nq, N) == np.arange(1, N + 1)).all()
        if key == "new_rows_topn":                                            # --topn-by rows: the new rows are the queries, as in gibbs()
            idx, tm, ts = res[key]
            assert np.array_equal(rec[:, 2].reshape(nq, N) - 1, idx)
            np.testing.assert_allclose(rec[:, 3].reshape(nq, N), tm, rtol=1e-10); np.testing.assert_allclose(rec[:, 4].reshape(nq, N), ts, rtol=1e-10)
        else:                                                                 # ... and every existing row gets its best new columns
            cand = rec[:, 2].reshape(nq, N).astype(int) - 1
            assert (cand >= 0).all() and (cand < 9).all()
            # (the ranking kernel and the block kernel add the same S Kp = 48 products of size O(1) in different orders: 1e-12 absolute)
            np.testing.assert_allclose(rec[:, 3].reshape(nq, N), res["new_cols"]["mean"][np.arange(nq)[:, None], cand], rtol=1e-12, atol=1e-12)
    assert (tmp_path / "out" / "topn.csv").exists()


# ---- 10. the planted experiment --------------------------------------------------------------------------------------------------------

def test_planted_cold_users_out_of_the_matrix():
    """link_ref.PLANTED with its 100 cold users removed from the training matrix altogether (500 x 300) and their features passed
    as new rows; the statistic is the RMSE of res["new_rows"]["mean"] at their 1 200 held-out cells, against the in-matrix cold-row
    RMSE of the same data (the 100 users present as empty rows; 0.7930 in tests/test_gpu_link.py): the same estimator on two chains.

    Measured on the CPU restatement (tests/newrows_ref.py::restate_newrows, link_ref.restate_chain) before this test was written,
    data seeds 31 .. 35, (in-matrix, out-of-matrix): (0.7930, 0.7856), (0.8038, 0.8019), (0.7568, 0.7541), (0.8337, 0.8255),
    (0.7789, 0.7726).  Out minus in: -0.0074, -0.0019, -0.0027, -0.0082, -0.0063; the largest in size is 0.0082, three times it
    is the margin, 0.0246: the GPU run (seed 31) must stay within 0.7930 + 0.0246.
    The share of the cells with |r - mean| <= 2 sqrt(std^2 + 1 / alpha) in the same five out-of-matrix runs: 0.9717, 0.9650,
    0.9817, 0.9675, 0.9817: the band [0.9650, 0.9817], widened by its own width 0.0167 on either side: [0.9483, 0.9984]."""
    import bpmf_amd
    P = ref.PLANTED
    s = nr.planted_split(P)
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, s["Mw"], s["Mtw"], s["Tw"], s["nw"], P["nmovies"], nsims=P["nsims"], burnin=P["burnin"], alpha=P["alpha"], Tt=s["Ttw"],
                             row_features=s["F_warm"], lambda_beta=P["lam"], new_row_features=s["F_cold"])
    finally:
        eng.close()
    i, c, r = s["cells"]
    assert len(r) == 1200
    mean, std = res["new_rows"]["mean"][i, c], res["new_rows"]["std"][i, c]
    rmse, cover = nr.rmse(r, mean), nr.coverage(r, mean, std, P["alpha"])
    print("out-of-matrix cold rows: RMSE %.4f, coverage %.4f, mean std %.4f" % (rmse, cover, std.mean()))
    assert rmse <= 0.7930 + 0.0246
    assert 0.9483 <= cover <= 0.9984
