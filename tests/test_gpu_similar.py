"""Similar columns of one side by posterior cosine / distance on the device (bpmf_hip_similar, bpmf_hip_similar_block, engine.similar,
gibbs(similar=), bpmf --similar).

  1. exact: dyadic factors with duplicated columns; for euclid every sum is exact, so lists and values equal a plain numpy restatement
     bit for bit, duplicates list the lower index first and a duplicate's distance is exactly 0
  2. similar_block against the longdouble reference within the bounds of tests/similar_ref.py, both kinds, with an all-zero column and
     columns scaled by 2^+-300 (cosine) / 2^+-200 (euclid); block[q, c] and block[c, q] have equal bytes
  3. the lists equal the top-N of the device's own block by the stated order, bit for bit, for kappa in {0, 1}, with and without a
     mask, at one, two and three candidate splits; and pass check_lists against longdouble
  4. the bytes of a pair do not depend on the ranges or the call
  5. the cosine lists agree with topn_scored("ucb", -kappa) over a normalised copy of the ring in a scratch pair of sides whose
     exclusion list is the query's own column, to the sum of both routes' bounds
  6. padding slots and every refusal of the entry points
  7. a loaded model gives byte-identical results, also from an fp32 run
  8. gibbs(similar=) and the executable; bpmf --model reproduces the file byte for byte
  9. the planted experiment

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import bpmf_amd
from bpmf_amd import _lib
from bpmf_amd import io as bio
from tests import model_ref as mr
from tests import similar_ref as sr
from tests import topn_score_ref as tr
from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
LD = sr.LD


def kp_of(K):
    return (K + 3) // 4 * 4


def empty_side(eng, nc):
    return eng.side_create(nc, 1, np.zeros(nc + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)


def load_ring(eng, side, Vs, spare=2):
    """Vs [S, nc, K] into slots 0 .. S - 1 of a ring reserved for S + spare samples"""
    eng.samples_reserve(side, Vs.shape[0] + spare)
    eng.samples_set(side, np.ascontiguousarray(np.transpose(Vs, (1, 0, 2))))


def masks(nc):
    ok = np.ones(nc, bool)
    ok[::3] = False
    return (None, ok)


# ---- 1. exact ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [3, 10, 32, 64, 128])
def test_exact_euclid(hip_engine_factory, K):
    eng = hip_engine_factory(K)
    nc, n = 130, 10
    side = empty_side(eng, nc)
    try:
        for S in (1, 2, 5):
            rng = np.random.default_rng(K + S)
            Vs = rng.integers(-4, 5, size=(S, nc, K)) / 8.0
            Vs[:, 1::5] = Vs[:, 0::5]                                          # columns 5 i and 5 i + 1 are twins, across the tiles
            load_ring(eng, side, Vs)
            want_mean, want_std = sr.plain(Vs, "euclid")
            bm, bs = eng.similar_block(side, "euclid")
            assert bm.tobytes() == want_mean.tobytes(), (K, S)
            if S == 1:
                assert (bs == 0).all()
            for ok in masks(nc):
                idx, score, mean, std = eng.similar(side, n, "euclid", 0.0, cand_ok=ok)
                wi = sr.ranked(want_mean, n, ok)
                rows = np.arange(nc)[:, None]
                assert np.array_equal(idx, wi), (K, S)
                assert score.tobytes() == want_mean[rows, wi].tobytes() and mean.tobytes() == score.tobytes(), (K, S)
                assert std.tobytes() == bs[rows, wi].tobytes(), (K, S)
                twins = 0
                for q in range(nc):
                    for r in range(n):
                        c = int(idx[q, r])
                        if c % 5 == 1 and c - 1 != q and (ok is None or ok[c - 1]):   # the higher twin is listed: the lower one right before it
                            assert r > 0 and idx[q, r - 1] == c - 1 and score[q, r - 1] == score[q, r], (K, S, q, r)
                            twins += 1
                    if q % 5 == 0 and (ok is None or ok[q + 1]):               # a duplicate's distance is exactly 0: nothing is nearer
                        at = np.nonzero(idx[q] == q + 1)[0]
                        assert len(at) == 1 and score[q, at[0]] == 0.0 and std[q, at[0]] == 0.0 and (score[q, :at[0]] == 0.0).all(), (K, S, q)
                assert twins > 0
    finally:
        eng.side_destroy(side)


# ---- 2. the block against longdouble; symmetry --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc,K,S", [s for s in sr.SHAPES if s[0] <= 130])
def test_block_against_longdouble(hip_engine_factory, nc, K, S):
    eng = hip_engine_factory(K)
    side = empty_side(eng, nc)
    try:
        for kind in sr.KINDS:
            Vs = sr.inputs(nc, K, S, seed=1000 * K + 10 * nc + S, big=sr.BIG[kind])
            load_ring(eng, side, Vs)
            ref = sr.reference(Vs, kp_of(K), kind)
            bm, bs = eng.similar_block(side, kind)
            assert np.isfinite(bm).all() and np.isfinite(bs).all()
            em, es = np.abs(LD(1) * bm - ref["mean"]), np.abs(LD(1) * bs - ref["std"])
            nzm, nzs = ref["mean_bound"] > 0, ref["std_bound"] > 0
            print("%s nc = %d K = %d S = %d: max err / bound  mean %.3g  std %.3g" % (
                kind, nc, K, S, float((em[nzm] / ref["mean_bound"][nzm]).max()) if nzm.any() else 0.0,
                float((es[nzs] / ref["std_bound"][nzs]).max()) if nzs.any() else 0.0))
            assert (ref["mean_bound"] <= ref["cap"]).all()
            assert (em <= ref["mean_bound"]).all(), (kind, float((em - ref["mean_bound"]).max()))
            assert (es <= ref["std_bound"]).all(), (kind, float((es - ref["std_bound"]).max()))
            assert bm.tobytes() == np.ascontiguousarray(bm.T).tobytes() and bs.tobytes() == np.ascontiguousarray(bs.T).tobytes(), kind
            if kind == "cosine" and nc > 1:
                assert (bm[1] == 0).all() and (bs[1] == 0).all()               # the all-zero column: cosine 0 with everything
                assert (np.abs(bm) <= 1).all()
            if kind == "euclid":
                assert (bm <= 0).all()
    finally:
        eng.side_destroy(side)


# ---- 3. the lists equal the block ----------------------------------------------------------------------------------------------------------

def lists_against_block(eng, side, Vs, K, kind, kappa, ok, n, q_from=0, q_to=None, block=None, ref=None):
    nc = Vs.shape[1]
    q_to = nc if q_to is None else q_to
    bm, bs = block if block is not None else eng.similar_block(side, kind)
    idx, score, mean, std = eng.similar(side, n, kind, kappa, q_from, q_to, cand_ok=ok)
    bscore = bm - kappa * bs                                                   # the product rounded, then the difference: the device's order
    wi = sr.ranked(bscore[q_from:q_to], n, ok, q_from)
    tag = (kind, kappa, ok is not None, n, q_from, q_to)
    assert np.array_equal(idx, wi), tag
    listed = idx >= 0
    rows = np.arange(q_from, q_to)[:, None]
    safe = np.where(listed, idx, 0)
    for got, want in ((score, bscore), (mean, bm), (std, bs)):
        assert np.where(listed, got, 0.0).tobytes() == np.where(listed, want[rows, safe], 0.0).tobytes(), tag
        assert (got[~listed] == 0).all(), tag
    if ref is None:
        ref = sr.reference(Vs, kp_of(K), kind, kappa, q_from, q_to)
    return sr.check_lists(idx, score, mean, std, ref, n, ok, q_from, tag=tag)


@pytest.mark.parametrize("nc,K,S", sr.SHAPES)
def test_lists_equal_block(hip_engine_factory, nc, K, S):
    eng = hip_engine_factory(K)
    side = empty_side(eng, nc)
    try:
        for kind in sr.KINDS:
            Vs = sr.inputs(nc, K, S, seed=1000 * K + 10 * nc + S, big=sr.BIG[kind])
            load_ring(eng, side, Vs)
            block = eng.similar_block(side, kind)
            worst = 0.0
            for kappa in (0.0, 1.0):
                ref = sr.reference(Vs, kp_of(K), kind, kappa)
                for ok in masks(nc):
                    worst = max(worst, lists_against_block(eng, side, Vs, K, kind, kappa, ok, 10, block=block, ref=ref))
            worst = max(worst, lists_against_block(eng, side, Vs, K, kind, 1.0, None, 32, block=block, ref=ref))   # the larger LDS
            print("%s nc = %d K = %d S = %d: lists, max score err / bound %.3g" % (kind, nc, K, S, worst))
    finally:
        eng.side_destroy(side)


# ---- 4. ranges and calls -------------------------------------------------------------------------------------------------------------------

def test_bits_do_not_depend_on_ranges_or_calls(hip_engine_factory):
    K, nc, S, n = 10, 600, 3, 10                                               # 600 columns: three splits of 256 candidates
    eng = hip_engine_factory(K)
    side = empty_side(eng, nc)
    try:
        for kind in sr.KINDS:
            Vs = sr.inputs(nc, K, S, seed=9, big=sr.BIG[kind])
            Vs[:, 11::50] = Vs[:, 10::50]                                      # twins across tiles and splits
            load_ring(eng, side, Vs)
            bm, bs = eng.similar_block(side, kind)
            again = eng.similar_block(side, kind)
            assert bm.tobytes() == again[0].tobytes() and bs.tobytes() == again[1].tobytes(), kind
            for q0, q1, c0, c1 in ((17, 230, 100, 555), (0, 1, 599, 600), (63, 65, 0, 600), (300, 600, 0, 64)):
                pm, pstd = eng.similar_block(side, kind, q0, q1, c0, c1)
                assert pm.tobytes() == np.ascontiguousarray(bm[q0:q1, c0:c1]).tobytes(), (kind, q0, q1, c0, c1)
                assert pstd.tobytes() == np.ascontiguousarray(bs[q0:q1, c0:c1]).tobytes(), (kind, q0, q1, c0, c1)
            whole = eng.similar(side, n, kind, 1.0)
            second = eng.similar(side, n, kind, 1.0)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, second)), kind
            parts = [eng.similar(side, n, kind, 1.0, q0, q1) for q0, q1 in ((0, 17), (17, 300), (300, 600))]
            for f in range(4):
                assert np.concatenate([p[f] for p in parts]).tobytes() == whole[f].tobytes(), (kind, f)
            # twins: x_s(q, 50 i + 10) and x_s(q, 50 i + 11) have equal bits, so the lower index stands right before the higher
            idx, score = whole[0], whole[1]
            twins = 0
            for q in range(nc):
                for r in range(n):
                    c = int(idx[q, r])
                    if c % 50 == 11 and c - 1 != q:
                        assert r > 0 and idx[q, r - 1] == c - 1 and score[q, r - 1] == score[q, r], (kind, q, r)
                        twins += 1
            assert twins > 0, kind
            assert eng.similar(side, 3, kind, 0.0, 5, 5)[0].shape == (0, 3)
            assert eng.similar_block(side, kind, 5, 5, 0, 9)[0].shape == (0, 9)
            assert eng.similar_last_ms(side) > 0
    finally:
        eng.side_destroy(side)


# ---- 5. the cross-check through topn_scored ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc,K,S", [(65, 10, 5), (130, 32, 2), (300, 10, 2)])
def test_cosine_agrees_with_topn_scored_over_a_normalised_copy(hip_engine_factory, nc, K, S):
    eng = hip_engine_factory(K)
    n = 10
    Vs = sr.inputs(nc, K, S, seed=77 + nc)
    side = empty_side(eng, nc)
    eye = util.csc_arrays(sp.identity(nc, format="csc"))                       # query q has rated candidate q: its exclusion list
    sq, sc = eng.side_create(nc, nc, *eye, 0.0), eng.side_create(nc, nc, *eye, 0.0)
    try:
        load_ring(eng, side, Vs)
        N = sr.normalised(Vs)
        load_ring(eng, sq, N, 1); load_ring(eng, sc, N, 3)
        for kappa in (0.0, 1.0):
            ref = sr.reference(Vs, kp_of(K), "cosine", kappa)
            other = tr.reference(N, N, 0.0, kp_of(K), "ucb", -kappa)
            assert (np.abs(other["score"] - ref["score"]) <= ref["bound"] + other["bound"])[~np.eye(nc, dtype=bool)].all()   # the copy's rounding is inside
            both = dict(ref, bound=2 * ref["bound"] + other["bound"])
            mine = eng.similar(side, n, "cosine", kappa)
            theirs = eng.topn_scored(sq, sc, 0.0, n, "ucb", -kappa)
            sr.check_lists(*mine, ref, n, tag=("similar", kappa))
            worst = sr.check_lists(theirs[0], theirs[1], None, None, both, n, tag=("copy", kappa), moments=False)
            # the two lists name the same columns except where the scores are within both bounds of the other list's last
            for q in range(nc):
                for a, b in ((mine, theirs), (theirs, mine)):
                    last = LD(1) * b[1][q, n - 1]
                    for c in set(a[0][q].tolist()) - set(b[0][q].tolist()):
                        assert ref["score"][q, c] <= last + both["bound"][q, c], (kappa, q, c)
            print("nc = %d K = %d S = %d kappa = %g: normalised-copy route, max err / (sum of bounds) %.3g" % (nc, K, S, kappa, worst))
    finally:
        eng.side_destroy(side); eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 6. padding and refusals ---------------------------------------------------------------------------------------------------------------

def test_padding_and_errors(hip_engine_factory):
    eng = hip_engine_factory(8)
    lib = _lib.load_library()
    nc = 6
    side = empty_side(eng, nc)
    half = eng.side_create(nc, 1, np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0, col_from=0, col_to=3)
    try:
        def refused(f):
            with pytest.raises(RuntimeError) as e:
                f()
            return str(e.value)
        assert "no sample ring" in refused(lambda: eng.similar(side, 5))
        assert "no sample ring" in refused(lambda: eng.similar_block(side))
        eng.samples_reserve(side, 3)
        assert "ring is empty" in refused(lambda: eng.similar(side, 5))
        assert "ring is empty" in refused(lambda: eng.similar_block(side))
        assert "no ranking of the side has been timed" in refused(lambda: eng.similar_last_ms(side))
        Vs = sr.inputs(nc, 8, 2, seed=3)
        load_ring(eng, side, Vs)
        assert "n = 33" in refused(lambda: eng.similar(side, 33))
        assert "n = 0" in refused(lambda: eng.similar(side, 0))
        assert "range" in refused(lambda: eng.similar(side, 5, q_from=0, q_to=7))
        assert "range" in refused(lambda: eng.similar(side, 5, q_from=4, q_to=3))
        assert "range" in refused(lambda: eng.similar(side, 5, q_from=-1, q_to=3))
        for bad in (-1.0, float("nan"), float("inf")):
            assert "kappa must be finite and >= 0" in refused(lambda: eng.similar(side, 5, kappa=bad))
        assert "query range" in refused(lambda: eng.similar_block(side, q_from=2, q_to=1))
        assert "candidate range" in refused(lambda: eng.similar_block(side, c_from=0, c_to=7))
        assert "whole on one GPU" in refused(lambda: eng.similar(half, 2))
        assert "whole on one GPU" in refused(lambda: eng.similar_block(half))
        with pytest.raises(ValueError):
            eng.similar(side, 5, "pearson")
        with pytest.raises(ValueError):
            eng.similar_block(side, "pearson")
        with pytest.raises(ValueError):
            eng.similar(side, 5, cand_ok=np.ones(nc + 1))
        out = np.zeros(nc * 5); idx = np.zeros(nc * 5, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.bpmf_hip_similar(side.handle, 7, 0.0, 5, 0, nc, None, p(idx), p(out), p(out), p(out)) == -1
        assert b"unknown kind 7" in lib.bpmf_hip_last_error()
        assert lib.bpmf_hip_similar_block(side.handle, 2, 0, nc, 0, nc, p(out), p(out)) == -1
        assert b"unknown kind 2" in lib.bpmf_hip_last_error()
        assert lib.bpmf_hip_similar(side.handle, 0, 0.0, 5, 0, nc, None, p(idx), None, p(out), p(out)) == -1
        assert b"NULL output" in lib.bpmf_hip_last_error()
        assert lib.bpmf_hip_similar(None, 0, 0.0, 5, 0, nc, None, p(idx), p(out), p(out), p(out)) == -1
        # the context keeps working: 6 columns, N = 10 -> 5 neighbours and 5 padding slots; a mask that leaves two columns
        ok = np.array([1, 0, 0, 1, 0, 0], bool)
        for kind in sr.KINDS:
            Vk = sr.inputs(nc, 8, 2, seed=3, big=sr.BIG[kind])
            load_ring(eng, side, Vk)
            ref = sr.reference(Vk, 8, kind, 0.5)
            for mask in (None, ok):
                idx, score, mean, std = eng.similar(side, 10, kind, 0.5, cand_ok=mask)
                sr.check_lists(idx, score, mean, std, ref, 10, mask, tag=(kind, mask is not None))
                left = np.array([(nc if mask is None else int(mask.sum())) - (1 if mask is None or mask[q] else 0) for q in range(nc)])
                assert ((idx >= 0).sum(1) == left).all(), (kind, idx)
                pad = idx < 0
                assert (score[pad] == 0).all() and (mean[pad] == 0).all() and (std[pad] == 0).all()
        load_ring(eng, side, Vs)
        # a mask that leaves nothing: only padding
        idx, score, mean, std = eng.similar(side, 3, "cosine", cand_ok=np.zeros(nc))
        assert (idx == -1).all() and (score == 0).all() and (mean == 0).all() and (std == 0).all()
        # a norm that overflows need only not trap
        big = Vs.copy(); big[:, 2] *= 2.0 ** 600
        load_ring(eng, side, big)
        for kind in sr.KINDS:
            idx, score, mean, std = eng.similar(side, 5, kind)
            assert ((idx >= -1) & (idx < nc)).all()
            eng.similar_block(side, kind)
        load_ring(eng, side, Vs)
        assert all(np.isfinite(a).all() for a in eng.similar(side, 5)[1:])
    finally:
        eng.side_destroy(side); eng.side_destroy(half)


# ---- 7. a loaded model ---------------------------------------------------------------------------------------------------------------------

def similar_products(engine, res):
    out = []
    for side in (res["movies"].side, res["users"].side):
        for kind in sr.KINDS:
            ok = np.arange(side.ncols) % 4 != 1
            out += list(engine.similar(side, 5, kind, 0.5)) + list(engine.similar(side, 7, kind, 0.0, 3, 29, cand_ok=ok))
            out += list(engine.similar_block(side, kind)) + list(engine.similar_block(side, kind, 2, 31, 5, 38))
    return out


@pytest.mark.parametrize("K,dtype", [(8, "f64"), (72, "f32")])
def test_loaded_model_gives_the_same_bytes(K, dtype, tmp_path):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    train = bpmf_amd.HipEngine(K, dtype=dtype)
    serve = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(train, M, Mt, T, nu, nm, nsims=8, burnin=3, save_model=str(tmp_path / "model"), Tt=Tt,
                             similar=5, similar_kind="euclid", similar_kappa=0.5)
        want = similar_products(train, res)
        sim = res["similar"]
        assert (sim["by"], sim["kind"], sim["kappa"]) == ("cols", "euclid", 0.5)
        assert all(sim[k].tobytes() == w.tobytes() for k, w in zip(("idx", "score", "mean", "std"), want[12:16]))
        loaded = bpmf_amd.load_model(serve, str(tmp_path / "model"))
        got = similar_products(serve, loaded)
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (K, dtype, i)
    finally:
        train.close(); serve.close()


# ---- 8. the chain and the executable -------------------------------------------------------------------------------------------------------

def test_gibbs_similar(hip_engine_factory):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    eng = hip_engine_factory(16)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=8, burnin=4, keep_samples=True, similar=6, similar_by="rows", similar_kappa=1.0,
                         similar_min_ratings=8)
    sim = res["similar"]
    assert sim["by"] == "rows" and sim["kind"] == "cosine" and sim["idx"].shape == (nu, 6)
    ok = np.diff(Mt[0]) >= 8
    assert 0 < ok.sum() < nu
    Us = np.stack([u for u, _ in res["samples"][4:]])
    ref = sr.reference(Us, 16, "cosine", 1.0)
    print("gibbs: max err / bound %.3g" % sr.check_lists(sim["idx"], sim["score"], sim["mean"], sim["std"], ref, 6, ok, tag="gibbs"))
    direct = eng.similar(res["users"].side, 6, "cosine", 1.0, cand_ok=ok)
    assert all(sim[k].tobytes() == d.tobytes() for k, d in zip(("idx", "score", "mean", "std"), direct))
    # independent of topn, and the pipelined loop gives the same bytes
    res2 = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=8, burnin=4, pipelined=True, topn=5, similar=6, similar_by="rows", similar_kappa=1.0,
                          similar_min_ratings=8)
    assert all(sim[k].tobytes() == res2["similar"][k].tobytes() for k in ("idx", "score", "mean", "std")) and "topn" in res2
    assert "similar" not in bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=3, burnin=1)


def run(args, cwd, env=None):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def read_similar(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# similar ") and lines[1] == "query,rank,neighbour,score,mean,std"
    return lines[0], np.array([ln.split(",") for ln in lines[2:]], dtype=float).reshape(-1, 6)


def test_cli_similar(tmp_path, hip_engine_factory):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    bio.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    bio.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    for d in ("A", "B", "C", "P"):
        os.mkdir(tmp_path / d)
    K, n, minr = 16, 5, 10
    chain = ["-n", "train.sdm", "-p", "test.sdm", "-d", K, "-i", 8, "-b", 4]
    ask = ["--similar", n, "--similar-kappa", 0.5, "--similar-min-ratings", minr]
    plain = run(chain + ["-o", "P"], tmp_path)
    a = run(chain + ask + ["--save-model", "model", "-o", "A"], tmp_path)
    final = lambda text: [ln for ln in text.splitlines() if ln.startswith("Final Avg RMSE: ")]
    assert final(a.stdout) == final(plain.stdout) and len(final(a.stdout)) == 1                                # the chain and stdout stay as they are
    assert len(a.stdout.replace("save-model: model\n", "").splitlines()) == len(plain.stdout.splitlines())
    assert "similar: 5 per column for %d queries, " % nm in a.stderr
    assert sorted(set(os.listdir(tmp_path / "A")) - set(os.listdir(tmp_path / "P"))) == ["similar-cols.csv"]
    # a saved model serves the same file, byte for byte
    b = run(["--model", "model", "-n", "train.sdm"] + ask + ["-o", "B"], tmp_path)
    assert "similar: 5 per column" in b.stderr
    assert (tmp_path / "A" / "similar-cols.csv").read_bytes() == (tmp_path / "B" / "similar-cols.csv").read_bytes()
    # a renumbered run (the assignment of two ranks on one GPU) with the samples written: original ids, and the Python result
    run(chain + ask + ["--similar-kind", "euclid", "-v", "-o", "C"], tmp_path, {"BPMF_TEST_ASSIGN_PARTS": "2"})
    head, rec = read_similar(tmp_path / "C" / "similar-cols.csv")
    assert head == "# similar 5 by cols kind euclid kappa 0.5 min-ratings 10"
    Vs = np.stack([bio.read_dense(tmp_path / "C" / ("V-%d.ddm" % i)).T for i in range(4, 8)])          # [S, nm, K], original numbering
    assert Vs.shape == (4, nm, K)
    ok = np.diff(M[0]) >= minr
    assert 0 < ok.sum() < nm
    eng = hip_engine_factory(K)
    side = empty_side(eng, nm)
    try:
        load_ring(eng, side, Vs)
        idx, score, mean, std = eng.similar(side, n, "euclid", 0.5, cand_ok=ok)
    finally:
        eng.side_destroy(side)
    listed = idx >= 0
    assert len(rec) == int(listed.sum())
    qs, rs = np.nonzero(listed)
    assert np.array_equal(rec[:, 0].astype(int) - 1, qs) and np.array_equal(rec[:, 1].astype(int) - 1, rs)
    assert np.array_equal(rec[:, 2].astype(int) - 1, idx[listed])
    assert rec[:, 3].tobytes() == score[listed].tobytes() and rec[:, 4].tobytes() == mean[listed].tobytes() and rec[:, 5].tobytes() == std[listed].tobytes()


# ---- 9. the planted experiment -------------------------------------------------------------------------------------------------------------

def test_planted_groups(hip_engine_factory):
    """Items in groups that share a factor centre (similar_ref.PLANTED): after a short chain the neighbours by posterior cosine are of
    the query's group far more often than the neighbours by the cosine between raw rating columns."""
    P = sr.PLANTED
    M, Mt, T, Tt, group = sr.planted_data(**P)
    eng = hip_engine_factory(P["K"])
    res = bpmf_amd.gibbs(eng, M, Mt, T, P["nusers"], P["nitems"], similar=10, **sr.PLANTED_CHAIN)
    post = sr.same_group_share(res["similar"]["idx"], group)
    raw = sr.same_group_share(sr.raw_column_neighbours(M, P["nusers"], 10), group)
    print("planted: same-group share among 10 neighbours: posterior cosine %.3f, raw rating columns %.3f" % (post, raw))
    assert post > raw
