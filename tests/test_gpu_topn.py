"""Posterior top-N ranking on the device (bpmf_hip_topn, engine.topn, gibbs(topn=N), bpmf --topn).

Exact cases: the factors are small dyadic rationals (k / 8, |k| <= 4), so every fp64 sum of the product is exact in any
order and the kernel's means and its full ordered lists must equal a numpy restatement bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import util
from bpmf_amd import io as bio
from bpmf_amd.sys import gibbs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")


def ratings(nu, nm, per_user, seed):
    """users side (columns = users, rows = items) and items side of a random pattern, as CSC arrays"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for u in range(nu):
        k = min(nm, int(rng.integers(0, per_user + 1)))
        for m in rng.choice(nm, size=k, replace=False):
            rows.append(int(m)); cols.append(u)
    A = sp.coo_matrix((np.ones(len(rows)) * 3.0, (rows, cols)), shape=(nm, nu)).tocsc()       # nm x nu: one column per user
    return util.csc_arrays(A), util.csc_arrays(A.T.tocsc())


def expected(Us, Vs, mean_rating, n, rated, q_from, q_to):
    """numpy restatement: Us [S, nq_all, K], Vs [S, nc, K]; rated: list of sets per query column (or None)"""
    S = Us.shape[0]
    P = np.einsum("sqk,sck->sqc", Us[:, q_from:q_to], Vs)                 # per-sample dot products
    mean = mean_rating + P.sum(0) / S
    nq, nc = mean.shape
    idx = np.full((nq, n), -1, np.int32); mo = np.zeros((nq, n)); so = np.zeros((nq, n))
    for i in range(nq):
        ok = np.ones(nc, bool)
        if rated is not None:
            ok[list(rated[q_from + i])] = False
        cand = np.nonzero(ok)[0]
        order = cand[np.lexsort((cand, -mean[i, cand]))][:n]
        idx[i, :len(order)] = order
        mo[i, :len(order)] = mean[i, order]
        if S > 1:
            p = mean_rating + P[:, i, order]
            so[i, :len(order)] = np.sqrt(((p - mean[i, order]) ** 2).sum(0) / (S - 1))
    return idx, mo, so


def dyadic(rng, shape):
    return rng.integers(-4, 5, size=shape) / 8.0


def run_case(eng, K, nu, nm, S, per_user, seed, dup=True, cases=None):
    U_side, M_side = ratings(nu, nm, per_user, seed)
    su = eng.side_create(nu, nm, *U_side, 0.0)
    sm = eng.side_create(nm, nu, *M_side, 0.0)
    try:
        rng = np.random.default_rng(seed)
        eng.samples_reserve(su, S + 1); eng.samples_reserve(sm, S)           # (rings of different capacity: strides differ)
        Us = dyadic(rng, (S, nu, K)); Vs = dyadic(rng, (S, nm, K))
        if dup:                                                           # duplicate columns: equal means, lower index first
            Vs[:, 1::5] = Vs[:, 0:-1:5][:, :Vs[:, 1::5].shape[1]]
            Us[:, 1::7] = Us[:, 0:-1:7][:, :Us[:, 1::7].shape[1]]
        for s in range(S):
            eng.set_items(su, Us[s]); eng.set_items(sm, Vs[s])
            eng.samples_add(su); eng.samples_add(sm)
        assert eng.samples_count(su) == S and eng.samples_count(sm) == S
        rated_u = [set(U_side[1][U_side[0][u]:U_side[0][u + 1]].tolist()) for u in range(nu)]
        rated_m = [set(M_side[1][M_side[0][m]:M_side[0][m + 1]].tolist()) for m in range(nm)]
        mr = 0.5
        for n, excl, by_cols, q_from, q_to in cases:
            q, c, Q, C_, rated = (sm, su, Vs, Us, rated_m) if by_cols else (su, sm, Us, Vs, rated_u)
            q_to = q.ncols if q_to is None else q_to
            idx, mean, std = eng.topn(q, c, mr, n, q_from, q_to, exclude_rated=excl)
            ei, em, es = expected(Q, C_, mr, n, rated if excl else None, q_from, q_to)
            tag = (K, S, n, excl, by_cols, q_from, q_to)
            assert np.array_equal(idx, ei), tag
            assert np.array_equal(mean, em), tag
            np.testing.assert_allclose(std, es, rtol=1e-12, atol=1e-12, err_msg=str(tag))
    finally:
        eng.side_destroy(su); eng.side_destroy(sm)


CASES = [(n, excl, by_cols, 0, None) for n in (1, 10) for excl in (True, False) for by_cols in (False, True)]


@pytest.mark.parametrize("K,dtype", [(8, "f64"), (10, "f64"), (32, "f64"), (64, "f64"), (128, "f64"), (128, "f32")])
def test_topn_exact(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    for S in (1, 4):
        run_case(eng, K, 150, 110, S, 40, seed=K + S, cases=CASES + [(10, True, False, 3, 140)])


def test_topn_padding_and_errors(hip_engine_factory):
    eng = hip_engine_factory(8)
    # 6 candidates, N = 10: everything eligible is listed, the rest are padding slots (idx -1, mean 0, std 0)
    run_case(eng, 8, 30, 6, 4, 5, seed=3, dup=False, cases=[(10, True, False, 0, None), (10, False, False, 0, None),
                                                            (10, True, True, 0, None)])
    U_side, M_side = ratings(20, 12, 4, 1)
    su = eng.side_create(20, 12, *U_side, 0.0)
    sm = eng.side_create(12, 20, *M_side, 0.0)
    try:
        with pytest.raises(RuntimeError):
            eng.topn(su, sm, 0.0, 5)                                       # no rings
        eng.samples_reserve(su, 2); eng.samples_reserve(sm, 2)
        with pytest.raises(RuntimeError):
            eng.topn(su, sm, 0.0, 5)                                       # no samples
        eng.samples_add(su); eng.samples_add(su); eng.samples_add(sm)
        with pytest.raises(RuntimeError):
            eng.samples_add(su)                                            # full
        with pytest.raises(RuntimeError):
            eng.topn(su, sm, 0.0, 5)                                       # 2 against 1 samples
        eng.samples_add(sm)
        with pytest.raises(RuntimeError):
            eng.topn(su, sm, 0.0, 33)                                      # n out of range
        idx, mean, std = eng.topn(su, sm, 0.0, 5)
        assert idx.shape == (20, 5) and (idx < 12).all()
        eng.samples_reserve(su, 0)
        assert eng.samples_count(su) == 0
    finally:
        eng.side_destroy(su); eng.side_destroy(sm)


def test_topn_few_queries_many_candidates(hip_engine_factory):
    """20 queries x 200 000 candidates: the candidates are split over workgroups and merged"""
    eng = hip_engine_factory(8)
    run_case(eng, 8, 20, 200000, 2, 3000, seed=11, cases=[(10, True, False, 0, None), (1, False, False, 0, None)])


# ---- the real chain ---------------------------------------------------------------------------------------------------
def chain_data():
    return util.synthetic(600, 400, 12000, seed=5)


def test_gibbs_topn_against_kept_samples(hip_engine_factory):
    M, Mt, T, Tt, nu, nm = chain_data()
    eng = hip_engine_factory(32)
    res = gibbs(eng, M, Mt, T, nu, nm, nsims=8, burnin=4, keep_samples=True, topn=10)
    idx, mean, std = res["topn"]
    assert idx.shape == (nu, 10) and (idx >= 0).all()
    Us = np.stack([u for u, _ in res["samples"][4:]]); Vs = np.stack([v for _, v in res["samples"][4:]])
    mr = res["movies"].mean_rating
    S = Us.shape[0]
    P = mr + np.einsum("sqk,sck->sqc", Us, Vs)
    full = P.mean(0)
    rows = np.arange(nu)[:, None]
    np.testing.assert_allclose(mean, full[rows, idx], rtol=1e-12, atol=0)
    np.testing.assert_allclose(std, np.sqrt(((P[:, rows, idx] - full[rows, idx]) ** 2).sum(0) / (S - 1)), rtol=1e-12, atol=1e-14)
    # no training pair; the set is numpy's top 10 except where its 10th and 11th means are within 1e-12
    train = sp.csc_matrix((M[2], M[1], M[0]), shape=(nu, nm)).toarray() != 0
    assert not train[rows, idx].any()
    masked = np.where(train, -np.inf, full)
    srt = -np.sort(-masked, axis=1)
    for u in range(nu):
        if abs(srt[u, 9] - srt[u, 10]) <= 1e-12 * abs(srt[u, 9]):
            continue
        assert set(idx[u].tolist()) == set(np.argsort(-masked[u], kind="stable")[:10].tolist()), u
    # pipelined loop: the same lists; two calls: byte-identical
    res2 = gibbs(eng, M, Mt, T, nu, nm, nsims=8, burnin=4, pipelined=True, topn=10)
    assert all(np.array_equal(a, b) for a, b in zip(res["topn"], res2["topn"]))
    again = eng.topn(res["users"].side, res["movies"].side, mr, 10)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res["topn"], again))


def test_cli_topn(tmp_path):
    args = ["-d", "16", "-i", "8", "-b", "4", "-n", os.path.join(util.GOLDEN, "ml100k-train.mtx.gz"),
            "-p", os.path.join(util.GOLDEN, "ml100k-test.mtx.gz")]
    os.makedirs(tmp_path / "a")
    r0 = subprocess.run([BPMF] + args + ["-o", str(tmp_path / "a"), "-v"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    os.makedirs(tmp_path / "b")
    r1 = subprocess.run([BPMF] + args + ["-o", str(tmp_path / "b"), "-v", "--topn", "10"], cwd=tmp_path, capture_output=True, text=True,
                        timeout=300)
    assert r0.returncode == 0 and r1.returncode == 0, r1.stderr
    pick = lambda text: [re.search(r"\t RMSE: (\S+)\tavg RMSE: (\S+)\t", l).groups() for l in text.splitlines() if "iteration" in l]
    assert pick(r0.stdout) == pick(r1.stdout) and len(pick(r1.stdout)) == 8
    lines = open(tmp_path / "b" / "topn.csv").read().splitlines()
    assert lines[0] == "query,rank,candidate,mean,std"
    rec = np.array([l.split(",") for l in lines[1:]], dtype=float)
    assert rec.shape == (943 * 10, 5)
    q = rec[:, 0].astype(int) - 1; c = rec[:, 2].astype(int) - 1
    assert (rec[:, 1].reshape(943, 10) == np.arange(1, 11)).all() and (q.reshape(943, 10) == np.arange(943)[:, None]).all()
    M, Mt, T, Tt, nu, nm = util.ml100k()
    train = sp.csc_matrix((M[2], M[1], M[0]), shape=(nu, nm)).toarray() != 0
    assert not train[q, c].any()
    mr = float(M[2].sum()) / len(M[2])
    P = np.stack([mr + (bio.read_dense(tmp_path / "b" / ("U-%d.ddm" % i))[:, q] * bio.read_dense(tmp_path / "b" / ("V-%d.ddm" % i))[:, c]).sum(0)
                  for i in range(4, 8)])
    mean = P.mean(0)
    np.testing.assert_allclose(rec[:, 3], mean, rtol=1e-12, atol=0)
    np.testing.assert_allclose(rec[:, 4], np.sqrt(((P - mean) ** 2).sum(0) / 3), rtol=1e-12, atol=1e-14)
    assert (np.diff(rec[:, 3].reshape(943, 10), axis=1) <= 0).all()
