"""Top-N by an acquisition score on the device (bpmf_hip_topn_scored, engine.topn_scored, gibbs(topn_score=), bpmf --topn-score;
DESIGN.md section 18).

  1. exact cases: dyadic factors, the sigma = 0 forms and ucb with kappa = 0 equal a numpy restatement / engine.topn bit for bit
  2. the mean and std of every pick are predict_block's, bit for bit, for every kind
  3. the selection is VERIFIED against a longdouble reference with the bounds of tests/topn_score_ref.py, not compared with a
     second ranking: near ties cannot flake and nothing is skipped
  4. the bits of an element do not depend on the query range or the candidate splits
  5. padding slots and every refusal of the entry point
  6. the chain (gibbs) and the executable
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from bpmf_amd import _lib
from bpmf_amd import io as bio
from bpmf_amd.sys import gibbs
from tests import newrows_ref as nr
from tests import topn_score_ref as tr
from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")


def kp_of(K):
    return (K + 3) // 4 * 4


def ratings(nq, nc, per_query, seed):
    """(query side, candidate side) CSC arrays of a random pattern in which pair (0, 0) is always rated, and the rated set of every
    query"""
    rng = np.random.default_rng(seed)
    rated = [set() for _ in range(nq)]
    rated[0].add(0)
    for q in range(nq):
        k = min(nc, int(rng.integers(0, per_query + 1)))
        rated[q].update(int(c) for c in rng.choice(nc, size=k, replace=False))
    rows = [c for q in range(nq) for c in sorted(rated[q])]
    cols = [q for q in range(nq) for _ in rated[q]]
    A = sp.coo_matrix((np.full(len(rows), 3.0), (rows, cols)), shape=(nc, nq)).tocsc()          # nc x nq: one column per query
    return util.csc_arrays(A), util.csc_arrays(A.T.tocsc()), rated


def make_sides(eng, nq, nc, per_query, seed):
    Q, Cs, rated = ratings(nq, nc, per_query, seed)
    rated_c = [set() for _ in range(nc)]
    for q, rs in enumerate(rated):
        for c in rs:
            rated_c[c].add(q)
    return eng.side_create(nq, nc, *Q, 0.0), eng.side_create(nc, nq, *Cs, 0.0), rated, rated_c


def fill_rings(eng, sq, sc, Es, Vs, cap_q=7, cap_c=6):
    """the samples through set_items + samples_add; returns what the device holds (get_items: fp32 contexts round)"""
    eng.samples_reserve(sq, cap_q); eng.samples_reserve(sc, cap_c)             # (rings of different capacity: the strides differ)
    Eb, Vb = [], []
    for E, V in zip(Es, Vs):
        eng.set_items(sq, E); eng.set_items(sc, V)
        Eb.append(eng.get_items(sq)); Vb.append(eng.get_items(sc))
        eng.samples_add(sq); eng.samples_add(sc)
    return np.stack(Eb), np.stack(Vb)


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------------------

def dyadic(rng, shape):
    return rng.integers(-4, 5, size=shape) / 8.0


EXACT_CASES = [(n, excl, by_cols, 0, None) for n in (1, 10) for excl in (True, False) for by_cols in (False, True)] + [(10, True, False, 3, 140)]


@pytest.mark.parametrize("K,dtype", [(8, "f64"), (10, "f64"), (32, "f64"), (64, "f64"), (128, "f64"), (128, "f32")])
def test_exact(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    nu, nm, mr, t = 150, 110, 0.5, 0.5
    for S in (1, 4):
        su, sm, rated_u, rated_m = make_sides(eng, nu, nm, 40, seed=K + S)
        try:
            rng = np.random.default_rng(K + S)
            Us = dyadic(rng, (S, nu, K)); Vs = dyadic(rng, (S, nm, K))
            Vs[:, 1::5] = Vs[:, 0:-1:5][:, :Vs[:, 1::5].shape[1]]              # duplicated columns: equal scores, lower index first
            Us[:, 1::7] = Us[:, 0:-1:7][:, :Us[:, 1::7].shape[1]]
            fill_rings(eng, su, sm, Us, Vs, S + 1, S)
            hit = 0
            for n, excl, by_cols, q_from, q_to in EXACT_CASES:
                q, c, Q, Cn, rated = (sm, su, Vs, Us, rated_m) if by_cols else (su, sm, Us, Vs, rated_u)
                q_to = q.ncols if q_to is None else q_to
                tag = (K, dtype, S, n, excl, by_cols, q_from, q_to)
                hit += int((mr + np.einsum("sqk,sck->sqc", Q, Cn) == t).sum())
                for kind in ("prob", "ei"):
                    want = tr.exact_scores(Q[:, q_from:q_to], Cn, mr, kind, t)
                    wi, ws = tr.ranked(want, n, rated if excl else None, q_from)
                    idx, score, mean, std = eng.topn_scored(q, c, mr, n, kind, t, 0.0, q_from, q_to, exclude_rated=excl)
                    assert np.array_equal(idx, wi), (kind,) + tag
                    assert score.tobytes() == ws.tobytes(), (kind,) + tag
                idx, score, mean, std = eng.topn_scored(q, c, mr, n, "ucb", 0.0, 0.0, q_from, q_to, exclude_rated=excl)
                ti, tm, ts = eng.topn(q, c, mr, n, q_from, q_to, exclude_rated=excl)
                assert np.array_equal(idx, ti) and mean.tobytes() == tm.tobytes() and score.tobytes() == tm.tobytes(), ("ucb",) + tag
            assert hit > 0                                                     # p_s == t occurs: the strict inequality is exercised
        finally:
            eng.side_destroy(su); eng.side_destroy(sm)


# ---- 2 and 3. the moments are predict_block's; the selection against longdouble --------------------------------------------------------

SHAPES = [(1, 1), (15, 63), (17, 65), (65, 130)]
SCORED = [("ucb", 2.0, 0.0), ("ucb", -1.0, 0.0), ("prob", 3.75, 0.5), ("prob", 3.75, 1.0), ("ei", 3.75, 0.5), ("ei", 3.75, 1.0)]


@pytest.mark.parametrize("K", [3, 10, 32, 64, 128])
def test_moments_and_selection(hip_engine_factory, K):
    eng = hip_engine_factory(K)
    mr, Kp = 3.5, kp_of(K)
    worst = {k: 0.0 for k in tr.KINDS}
    for nq, nc in SHAPES:
        sq, sc, rated, _ = make_sides(eng, nq, nc, 5, seed=nq)
        excl = nq * nc > 1                                                     # (the single pair of 1 x 1 is rated: nothing would be left)
        n = min(10, nc)
        try:
            for S in (1, 2, 5):
                rng = np.random.default_rng(1000 * K + 10 * nq + S)
                Es, Vs = fill_rings(eng, sq, sc, rng.standard_normal((S, nq, K)), rng.standard_normal((S, nc, K)))
                bm, bs = eng.predict_block(sq, sc, mr)
                rows = np.arange(nq)[:, None]
                for kind, param, sigma in SCORED:
                    tag = (K, nq, nc, S, kind, param, sigma)
                    idx, score, mean, std = eng.topn_scored(sq, sc, mr, n, kind, param, sigma, exclude_rated=excl)
                    listed = idx >= 0
                    safe = np.where(listed, idx, 0)
                    # 2. mean and std of every pick: the bits of predict_block
                    assert np.array_equal(mean[listed], bm[rows, safe][listed]) and np.array_equal(std[listed], bs[rows, safe][listed]), tag
                    assert (mean[~listed] == 0).all() and (std[~listed] == 0).all(), tag
                    if kind == "ucb":
                        plain = mean + param * std
                        assert (np.abs(score - plain) <= 2.0 * np.spacing(np.abs(plain))).all(), tag
                    # 3. the selection, verified
                    ref = tr.reference(Es, Vs, mr, Kp, kind, param, sigma)
                    worst[kind] = max(worst[kind], tr.check_lists(idx, score, ref, n, rated if excl else None, tag=tag))
        finally:
            eng.side_destroy(sq); eng.side_destroy(sc)
    print("K = %d: max err / bound  " % K + "  ".join("%s %.3g" % (k, worst[k]) for k in tr.KINDS))


# ---- 4. ranges and splits --------------------------------------------------------------------------------------------------------------

def test_bits_do_not_depend_on_ranges_or_splits(hip_engine_factory):
    K, nq, nc, S, n = 10, 40, 600, 3, 32                                       # 40 x 600: three splits of 256 candidates
    eng = hip_engine_factory(K)
    sq, sc, rated, _ = make_sides(eng, nq, nc, 30, seed=9)
    try:
        rng = np.random.default_rng(9)
        Vs = rng.standard_normal((S, nc, K))
        Vs[:, 1::5] = Vs[:, 0::5]                                              # columns 5 i and 5 i + 1 are twins, across tiles and splits
        fill_rings(eng, sq, sc, rng.standard_normal((S, nq, K)), Vs)
        bm, bs = eng.predict_block(sq, sc, 1.25)
        for kind, param, sigma in (("ucb", 1.0, 0.0), ("prob", 1.5, 1.0), ("ei", 1.5, 0.5), ("prob", 1.5, 0.0)):
            whole = eng.topn_scored(sq, sc, 1.25, n, kind, param, sigma, exclude_rated=False)
            again = eng.topn_scored(sq, sc, 1.25, n, kind, param, sigma, exclude_rated=False)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again)), kind
            parts = [eng.topn_scored(sq, sc, 1.25, n, kind, param, sigma, q0, q1, exclude_rated=False) for q0, q1 in ((0, 17), (17, 40))]
            for f in range(4):
                assert np.concatenate([p[f] for p in parts]).tobytes() == whole[f].tobytes(), (kind, f)
            idx, score, mean, std = whole
            rows = np.arange(nq)[:, None]
            assert np.array_equal(mean, bm[rows, idx]) and np.array_equal(std, bs[rows, idx]), kind   # across the splits too
            twins = 0
            for q in range(nq):
                for r in range(n):
                    c = int(idx[q, r])
                    if c % 5 == 1:                                             # the higher twin is listed: the lower one stands right before it
                        assert r > 0 and idx[q, r - 1] == c - 1 and score[q, r - 1] == score[q, r], (kind, q, r)
                        twins += 1
            assert twins > 0, kind
            # with the rated candidates excluded: the same elements, the same bits
            ex = eng.topn_scored(sq, sc, 1.25, n, kind, param, sigma)
            for q in range(nq):
                keep = [r for r in range(n) if int(idx[q, r]) not in rated[q]]
                assert ex[0][q, :len(keep)].tolist() == idx[q, keep].tolist() and ex[1][q, :len(keep)].tobytes() == score[q, keep].tobytes(), (kind, q)
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 5. padding and errors -------------------------------------------------------------------------------------------------------------

def test_padding_and_errors(hip_engine_factory):
    eng = hip_engine_factory(8)
    other = hip_engine_factory(10)
    lib = _lib.load_library()
    sq, sc, rated, _ = make_sides(eng, 30, 6, 3, seed=3)
    oq, oc, _, _ = make_sides(other, 30, 6, 3, seed=3)
    try:
        def refused(f):
            with pytest.raises(RuntimeError) as e:
                f()
            return str(e.value)
        assert "sample ring" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 5, "ucb", 1.0))
        eng.samples_reserve(sq, 3); eng.samples_reserve(sc, 3)
        assert "same number" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 5, "ucb", 1.0))          # no samples
        rng = np.random.default_rng(3)
        eng.set_items(sq, rng.standard_normal((30, 8))); eng.set_items(sc, rng.standard_normal((6, 8)))
        eng.samples_add(sq); eng.samples_add(sq); eng.samples_add(sc)
        assert "same number" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 5, "ucb", 1.0))          # 2 against 1
        eng.samples_add(sc)
        assert "n = 33" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 33, "ucb", 1.0))
        assert "n = 0" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 0, "ucb", 1.0))
        assert "range" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 5, "ucb", 1.0, q_from=0, q_to=31))
        assert "range" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 5, "ucb", 1.0, q_from=4, q_to=3))
        assert "kappa is not finite" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 5, "ucb", float("inf")))
        assert "threshold is not finite" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 5, "prob", float("nan"), 1.0))
        for kind in ("prob", "ei"):
            for bad in (-1.0, float("nan"), float("inf")):
                assert "sigma" in refused(lambda: eng.topn_scored(sq, sc, 0.0, 5, kind, 1.0, bad))
        eng.topn_scored(sq, sc, 0.0, 5, "ucb", 1.0, float("nan"))                                      # sigma is ignored for ucb
        assert "different contexts" in refused(lambda: eng.topn_scored(sq, oc, 0.0, 5, "ucb", 1.0))
        with pytest.raises(ValueError):
            eng.topn_scored(sq, sc, 0.0, 5, "mean", 1.0)
        out = np.zeros(30 * 5); idx = np.zeros(30 * 5, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.bpmf_hip_topn_scored(sq.handle, sc.handle, 0.0, 5, 0, 30, 1, 7, 1.0, 0.0, p(idx), p(out), p(out), p(out)) == -1
        assert b"unknown score kind 7" in lib.bpmf_hip_last_error()
        assert lib.bpmf_hip_topn_scored(sq.handle, sc.handle, 0.0, 5, 0, 30, 1, 0, 1.0, 0.0, p(idx), None, p(out), p(out)) == -1
        assert b"NULL output" in lib.bpmf_hip_last_error()
        # a side whose rows are not the candidates' columns cannot exclude
        assert "exclude_rated" in refused(lambda: eng.topn_scored(sq, sq, 0.0, 5, "ucb", 1.0))
        # the context keeps working: 6 candidates, N = 10 -> padding slots with id -1 and zeros in all four outputs
        Es = np.stack([eng.get_items(sq)] * 2); Vs = np.stack([eng.get_items(sc)] * 2)
        for kind, param, sigma in (("ucb", 1.0, 0.0), ("prob", 0.0, 1.0), ("ei", 0.0, 1.0)):
            for excl in (True, False):
                idx, score, mean, std = eng.topn_scored(sq, sc, 0.0, 10, kind, param, sigma, exclude_rated=excl)
                tr.check_lists(idx, score, tr.reference(Es, Vs, 0.0, 8, kind, param, sigma), 10, rated if excl else None, tag=(kind, excl))
                pad = idx < 0
                assert pad[:, 6:].all() and (pad.sum(1) == 4 + np.array([len(r) if excl else 0 for r in rated])).all()
                assert (score[pad] == 0).all() and (mean[pad] == 0).all() and (std[pad] == 0).all()
                assert (std[~pad] == 0).all()                                  # two equal samples: no spread
        assert eng.topn_scored(sq, sc, 0.0, 3, "ucb", 1.0, q_from=5, q_to=5)[0].shape == (0, 3)
        # a sigma below the smallest normal double (1 / sigma would overflow) is the sigma = 0 form
        t = float(Es[0, 3] @ Vs[0, 2])
        for kind in ("prob", "ei"):
            zero = eng.topn_scored(sq, sc, 0.0, 6, kind, t, 0.0, exclude_rated=False)
            tiny = eng.topn_scored(sq, sc, 0.0, 6, kind, t, 5e-324, exclude_rated=False)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(zero, tiny)), kind
            assert (tiny[0] >= 0).all() and np.isfinite(tiny[1]).all(), kind
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc); other.side_destroy(oq); other.side_destroy(oc)


# ---- 6. the chain and the executable ---------------------------------------------------------------------------------------------------

def test_gibbs_topn_score(hip_engine_factory):
    M, Mt, T, Tt, nu, nm = util.synthetic(600, 400, 12000, seed=5)
    eng = hip_engine_factory(32)
    res = gibbs(eng, M, Mt, T, nu, nm, nsims=8, burnin=4, keep_samples=True, topn=10, topn_score=("ucb", 1.0))
    assert len(res["topn"]) == 4
    idx, score, mean, std = res["topn"]
    assert idx.shape == (nu, 10) and (idx >= 0).all()
    Us = np.stack([u for u, _ in res["samples"][4:]]); Vs = np.stack([v for _, v in res["samples"][4:]])
    mr = res["movies"].mean_rating
    train = sp.csc_matrix((M[2], M[1], M[0]), shape=(nu, nm)).toarray() != 0
    rated = [set(np.nonzero(train[u])[0].tolist()) for u in range(nu)]
    ref = tr.reference(Us, Vs, mr, 32, "ucb", 1.0)
    print("gibbs ucb: max err / bound %.3g" % tr.check_lists(idx, score, ref, 10, rated, tag="gibbs"))
    bm, bs = eng.predict_block(res["users"].side, res["movies"].side, mr)
    rows = np.arange(nu)[:, None]
    assert np.array_equal(mean, bm[rows, idx]) and np.array_equal(std, bs[rows, idx])
    # the pipelined loop: the same bytes; without topn_score: the 3-tuple of the mean ranking, as before
    res2 = gibbs(eng, M, Mt, T, nu, nm, nsims=8, burnin=4, pipelined=True, topn=10, topn_score=("ucb", 1.0))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res["topn"], res2["topn"]))
    res3 = gibbs(eng, M, Mt, T, nu, nm, nsims=8, burnin=4, topn=10)
    assert len(res3["topn"]) == 3
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res3["topn"], eng.topn(res3["users"].side, res3["movies"].side, mr, 10)))


def test_cli_topn_score(tmp_path):
    args = ["-d", "16", "-i", "8", "-b", "4", "-n", os.path.join(util.GOLDEN, "ml100k-train.mtx.gz"),
            "-p", os.path.join(util.GOLDEN, "ml100k-test.mtx.gz")]
    os.makedirs(tmp_path / "a"); os.makedirs(tmp_path / "b")
    r0 = subprocess.run([BPMF] + args + ["-o", str(tmp_path / "a"), "-v"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    r1 = subprocess.run([BPMF] + args + ["-o", str(tmp_path / "b"), "-v", "--topn", "10", "--topn-score", "prob", "--topn-threshold", "4"],
                        cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r1.returncode == 0, r1.stderr
    pick = lambda text: [l for l in text.splitlines() if "iteration" in l]
    untimed = lambda text: [re.sub(r"\titems/sec:.*$", "", l) for l in pick(text)]     # the whole line but its two throughput fields
    assert untimed(r0.stdout) == untimed(r1.stdout) and len(untimed(r1.stdout)) == 8
    assert all(re.search(r"\t RMSE: \S+\tavg RMSE: \S+\tFU\(", l) for l in untimed(r1.stdout))
    assert "topn score: prob, threshold = 4, sigma = " in r1.stderr
    lines = open(tmp_path / "b" / "topn.csv").read().splitlines()
    assert lines[0] == "query,rank,candidate,score,mean,std"
    rec = np.array([l.split(",") for l in lines[1:]], dtype=float)
    assert rec.shape == (943 * 10, 6)
    q = rec[:, 0].astype(int) - 1; c = rec[:, 2].astype(int) - 1
    assert (rec[:, 1].reshape(943, 10) == np.arange(1, 11)).all() and (q.reshape(943, 10) == np.arange(943)[:, None]).all()
    M, Mt, T, Tt, nu, nm = util.ml100k()
    train = sp.csc_matrix((M[2], M[1], M[0]), shape=(nu, nm)).toarray() != 0
    assert not train[q, c].any()
    mr = float(M[2].sum()) / len(M[2])
    Us = np.stack([bio.read_dense(tmp_path / "b" / ("U-%d.ddm" % i)).T for i in range(4, 8)])          # [S, nu, K]
    Vs = np.stack([bio.read_dense(tmp_path / "b" / ("V-%d.ddm" % i)).T for i in range(4, 8)])
    assert Us.shape == (4, nu, 16) and Vs.shape == (4, nm, 16)
    sigma = 1.0 / np.sqrt(2.0)                                                 # the default -a 2
    ref = tr.reference(Us, Vs, mr, 16, "prob", 4.0, sigma)
    err = np.abs(tr.LD(1) * rec[:, 3] - ref["score"][q, c])
    print("cli prob: max err / bound %.3g" % float((err / ref["bound"][q, c]).max()))
    assert (err <= ref["bound"][q, c]).all()
    good = nr.predict(Us, Vs, mr)
    np.testing.assert_allclose(rec[:, 4], np.asarray(good["mean"], float)[q, c], rtol=1e-12, atol=0)
    assert (np.diff(rec[:, 3].reshape(943, 10), axis=1) <= 0).all()
