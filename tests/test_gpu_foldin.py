"""Fold-in on the device: k_foldin, the hyper ring, bpmf_hip_foldin*, gibbs(foldin=True) + fold_in and
`bpmf --fold-in-rows`.

The reference is tests/foldin_ref.py (numpy / LAPACK; Philox and canonical53 of tests/probit_ref.py), fed with what the device holds
(the ring contents through get_items per kept sample, the hyper ring through hyper_get).  A candidate side of 300 columns, rings
filled by set_items + samples_add with seeded random factors, hyper-parameters through explicit hyper_add with Lambda_s = A^T A / K
+ I; the test computes cond(Lambda*) on the CPU and asserts it <= 1e4.

  1. conditional mean (draw=False) and draw against the restatement: K in {8, 10, 32, 64, 100, 128} in fp64 and one fp32 context at
     K = 128, S in {1, 3} with a different alpha per sample (rings reserved for S + 2), one batch of rows with 0, 1, K - 1, K, K + 1,
     chunk - 1, chunk, chunk + 1, 257 and all 300 ratings.  Bar: 1e-9 max|u|, the bar of the link half-iteration in
     tests/test_gpu_link.py.  Measured maxima (in units of max|u|): see DESIGN.md section 19.
  2. determinism: a repeated call and row 0 of [A, B, C] against row 0 of [A] give the same bits; the pad components are zeros
  3. foldin_predict against numpy over foldin_get at the bounds tests/test_gpu_newrows.py holds predict_block to; a sub-range has
     the full call's bits
  4. foldin_topn = the argsort of foldin_predict's mean (ties to the lower id), with and without the rows' own columns; a row
     without ratings and one that rated all 300 (every slot -1); n in {1, 5}
  5. a pivot that is not positive: BPMF_HIP_ECHOL names the row, its ring entry is zeros, the next valid call succeeds
  6. the refusals of the C ABI, each by its message
  7. the chain: gibbs(foldin=True) + fold_in on the planted data equals the restatement fed the chain's own samples and
     hyper-parameters; `bpmf --fold-in-rows --topn 5 -o DIR` writes what fold_in returns

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import foldin_ref as fr
from tests import newrows_ref as nr
from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
NC = fr.NCOLS
BAR = 1e-9                       # of max|u|
ECHOL, EINVAL = -4, -1


def pair_of_sides(eng, nq=2, nc=NC, mean=0.0):
    """the side new rows are folded into (nq columns of its own) and its partner of nc columns, one rating between them"""
    A = sp.coo_matrix((np.array([3.0]), (np.array([0]), np.array([0]))), shape=(nc, nq)).tocsc()
    return eng.side_create(nq, nc, *util.csc_arrays(A), mean), eng.side_create(nc, nq, *util.csc_arrays(A.T.tocsc()), mean)


def fill(eng, side, cand, K, S, seed, cap_extra=2):
    """the candidate ring through set_items + samples_add, the hyper ring through explicit hyper_add; returns what the device holds"""
    Vs = fr.factors(K, S, cand.ncols, seed)
    alphas, mus, Lams = fr.hypers(K, S, seed + 1)
    eng.samples_reserve(cand, S + cap_extra); eng.hyper_reserve(side, S)
    held = []
    for s in range(S):
        eng.set_items(cand, Vs[s]); held.append(eng.get_items(cand)); eng.samples_add(cand)
        eng.hyper_add(side, alphas[s], mus[s], Lams[s])
    assert eng.hyper_count(side) == S == eng.samples_count(cand)
    a, m, L = eng.hyper_get(side)
    assert np.array_equal(a, alphas) and np.array_equal(m, mus) and np.array_equal(L, Lams)
    return np.stack(held), alphas, mus, Lams


# ---- 1. against the restatement --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,dtype", [(8, "f64"), (10, "f64"), (32, "f64"), (64, "f64"), (100, "f64"), (128, "f64"), (128, "f32")])
def test_mean_and_draw_against_restatement(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    chunk = eng.foldin_chunk()
    counts = fr.edge_counts(K, chunk)
    R = fr.rows_with_counts(counts, NC, 100 + K)
    assert sorted(np.diff(R.indptr).tolist()) == sorted(counts) and max(counts) == NC
    mean = 3.25
    for S in (1, 3):
        side, cand = pair_of_sides(eng)
        try:
            Vs, alphas, mus, Lams = fill(eng, side, cand, K, S, 10 * K + S)
            u1 = fr.uniforms(len(counts), S, K, fr.TAG_ROWS)[0]
            assert u1.min() > 1e-300                                         # ln u1 is finite for every block the batch draws
            for draw in (False, True):
                want, cond = fr.fold_in(R, Vs, alphas, mus, Lams, mean, fr.TAG_ROWS if draw else None, want_cond=True)
                assert cond <= 1e4, cond
                eng.foldin(side, cand, mean, R, fr.TAG_ROWS, draw=draw)
                assert eng.foldin_count(side) == len(counts)
                got = eng.foldin_get(side)
                assert got.shape == want.shape == (len(counts), S, K) and np.isfinite(got).all()
                err = np.abs(got - want).max() / np.abs(want).max()
                print("K %d %s S %d %s: max|du| / max|u| = %.3g (cond <= %.3g)" % (K, dtype, S, "draw" if draw else "mean", err, cond))
                assert err <= BAR, (K, dtype, S, draw, err)
            # the draw moved every row off its mean, by something of the size of Lambda*^-1/2
            eng.foldin(side, cand, mean, R, fr.TAG_ROWS, draw=False)
            assert np.abs(got - eng.foldin_get(side)).max(axis=(1, 2)).min() > 1e-3
        finally:
            eng.side_destroy(side); eng.side_destroy(cand)


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------------

def test_bits_do_not_depend_on_the_call_or_the_batch(hip_engine_factory):
    K, S = 10, 3                                                             # Kt = 10: the ring has two pad components per sample
    eng = hip_engine_factory(K)
    side, cand = pair_of_sides(eng)
    try:
        fill(eng, side, cand, K, S, 7)
        R = fr.rows_with_counts([33, 0, 300, 9], NC, 5)
        eng.foldin(side, cand, 2.5, R, 7)
        first = eng.foldin_get(side, padded=True)
        eng.foldin(side, cand, 2.5, R, 7)
        again = eng.foldin_get(side, padded=True)
        assert first.shape == (4, S, 12) and first.tobytes() == again.tobytes()
        assert (first[:, :, K:] == 0.0).all() and np.array_equal(first[:, :, :K], eng.foldin_get(side))
        eng.foldin(side, cand, 2.5, R[:1], 7)                                # row 0 alone: its bits in the batch of four
        alone = eng.foldin_get(side, padded=True)
        assert alone.shape == (1, S, 12) and alone[0].tobytes() == first[0].tobytes()
        eng.foldin(side, cand, 2.5, R, 8)                                    # another tag: other normals
        assert not np.array_equal(eng.foldin_get(side), first[:, :, :K])
    finally:
        eng.side_destroy(side); eng.side_destroy(cand)


# ---- 3. / 4. prediction and ranking -----------------------------------------------------------------------------------------------------

def test_foldin_predict_and_topn(hip_engine_factory):
    from tests.test_gpu_newrows import check_block
    K, S, mr = 10, 3, 3.5
    eng = hip_engine_factory(K)
    side, cand = pair_of_sides(eng)
    try:
        Vs = fill(eng, side, cand, K, S, 21)[0]
        counts = [0, 5, NC, 40, 1, 17, 64, 65, 2, 8, 100, 12, 3, 30, 7, 6, 50, 9]      # 18 queries: more than one 16-query tile
        R = fr.rows_with_counts(counts, NC, 9)
        eng.foldin(side, cand, mr, R, 7)
        E = eng.foldin_get(side)
        mean, std = eng.foldin_predict(side, cand, mr)
        assert mean.shape == std.shape == (len(counts), NC)
        check_block(mean, std, nr.predict(np.transpose(E, (1, 0, 2)), Vs, mr), 12, mr, "foldin_predict")
        m2, s2 = fr.predict(E, Vs, mr)
        np.testing.assert_allclose(mean, m2, rtol=0, atol=1e-12 * np.abs(m2).max()); np.testing.assert_allclose(std, s2, rtol=1e-9, atol=1e-12)
        part = eng.foldin_predict(side, cand, mr, 3, 17, 65, 130)
        assert part[0].shape == (14, 65) and np.array_equal(part[0], mean[3:17, 65:130]) and np.array_equal(part[1], std[3:17, 65:130])
        own = [R.indices[R.indptr[i]:R.indptr[i + 1]] for i in range(len(counts))]
        rows = np.arange(len(counts))[:, None]
        for n in (1, 5):
            for excl in (False, True):
                idx, tm, ts = eng.foldin_topn(side, cand, mr, n, exclude_rated=excl)
                want = fr.topn_of(mean, n, own if excl else None)
                assert idx.shape == (len(counts), n) and np.array_equal(idx, want), (n, excl)
                filled = idx >= 0
                assert (tm[~filled] == 0).all() and (ts[~filled] == 0).all()
                np.testing.assert_allclose(tm[filled], mean[rows, np.maximum(idx, 0)][filled], rtol=0, atol=1e-12 * np.abs(mean).max())
                np.testing.assert_allclose(ts[filled], std[rows, np.maximum(idx, 0)][filled], rtol=1e-9, atol=1e-12)
                if excl:
                    assert (idx[2] == -1).all()                              # rated all 300: nothing left
                    assert (idx[0] >= 0).all()                               # rated nothing: a full list
                    assert all(not set(idx[i][idx[i] >= 0].tolist()) & set(own[i].tolist()) for i in range(len(counts)))
                else:
                    assert filled.all()
    finally:
        eng.side_destroy(side); eng.side_destroy(cand)


# ---- 5. a pivot that is not positive ----------------------------------------------------------------------------------------------------

def test_bad_pivot_is_an_error_return(hip_engine_factory):
    import bpmf_amd
    K = 8
    eng = hip_engine_factory(K)
    side, cand = pair_of_sides(eng)
    try:
        Vs = fr.factors(K, 1, NC, 3)
        eng.samples_reserve(cand, 1); eng.set_items(cand, Vs[0]); eng.samples_add(cand)
        eng.hyper_reserve(side, 1); eng.hyper_add(side, 2.0, np.zeros(K), -np.eye(K))
        R = fr.rows_with_counts([NC, 0, 200], NC, 4)                         # 300 and 200 ratings carry Lambda* over -I; none does not
        with pytest.raises(bpmf_amd.BpmfHipError, match=r"Cholesky failed for new row 1 ") as e:
            eng.foldin(side, cand, 3.0, R, 7)
        assert e.value.code == ECHOL
        E = eng.foldin_get(side, padded=True)
        assert E.shape == (3, 1, 8) and (E[1] == 0.0).all() and np.isfinite(E).all() and np.abs(E[0]).max() > 0 and np.abs(E[2]).max() > 0
        want = fr.fold_in(R[[0, 2]], Vs, [2.0], np.zeros((1, K)), -np.eye(K)[None], 3.0, 7)
        assert np.abs(E[0, :, :K] - want[0]).max() <= BAR * np.abs(want).max()      # the rows beside it are served
        eng.hyper_reserve(side, 1); eng.hyper_add(side, 2.0, np.zeros(K), np.eye(K))
        eng.foldin(side, cand, 3.0, R, 7)                                    # and the next valid call succeeds
        assert (np.abs(eng.foldin_get(side)).max(axis=(1, 2)) > 0).all() and np.isfinite(eng.foldin_predict(side, cand, 3.0)[0]).all()
    finally:
        eng.side_destroy(side); eng.side_destroy(cand)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_c_abi():
    import bpmf_amd
    K = 8
    eng = bpmf_amd.HipEngine(K)

    def refused(fn, code=EINVAL):
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        return str(e.value)
    try:
        side, cand = pair_of_sides(eng)
        R = fr.rows_with_counts([3, 0, 12], NC, 1)
        csr = lambda ptr, idx, val: (np.array(ptr, np.int64), np.array(idx, np.int32), np.array(val, float))
        assert "no hyper-parameters" in refused(lambda: eng.foldin(side, cand, 0.0, R, 7))
        fill(eng, side, cand, K, 2, 5)
        eng.foldin(side, cand, 0.0, R, 7)
        assert "row 1 rates column 4 twice" in refused(lambda: eng.foldin(side, cand, 0.0, csr([0, 1, 4], [9, 2, 4, 4], [1, 2, 3, 4]), 7))
        assert "out of order" in refused(lambda: eng.foldin(side, cand, 0.0, csr([0, 2], [5, 4], [1, 2]), 7))
        assert "row 0 rates column 300, out of range" in refused(lambda: eng.foldin(side, cand, 0.0, csr([0, 2], [5, 300], [1, 2]), 7))
        assert "out of range" in refused(lambda: eng.foldin(side, cand, 0.0, csr([0, 2], [-1, 4], [1, 2]), 7))
        assert "row 0, column 5 is not finite" in refused(lambda: eng.foldin(side, cand, 0.0, csr([0, 2], [4, 5], [1, np.inf]), 7))
        assert "not finite" in refused(lambda: eng.foldin(side, cand, 0.0, csr([0, 2], [4, 5], [np.nan, 1]), 7))
        assert "rowptr decreases at row 1" in refused(lambda: eng.foldin(side, cand, 0.0, csr([0, 2, 1], [4], [1]), 7))
        assert "tag must be >= 1" in refused(lambda: eng.foldin(side, cand, 0.0, R, 0))
        assert "wrong number of columns" in refused(lambda: eng.foldin(side, side, 0.0, csr([0, 0], [], []), 7))
        assert eng.foldin_count(side) == 3                                   # a refused call leaves the earlier set alone
        eng.samples_add(cand)                                                # ring 3, hyper ring 2
        assert "must be the same samples" in refused(lambda: eng.foldin(side, cand, 0.0, R, 7))
        assert "folded in against 2 samples" in refused(lambda: eng.foldin_predict(side, cand, 0.0))
        assert "full" in refused(lambda: eng.hyper_add(side, 2.0, np.zeros(K), np.eye(K)))
        assert "not finite" in refused(lambda: (eng.hyper_reserve(side, 1), eng.hyper_add(side, 2.0, np.full(K, np.nan), np.eye(K))))
        eng.foldin(side, None, 0.0, None, 7)                                 # freed
        assert eng.foldin_count(side) == 0
        assert "no folded-in rows" in refused(lambda: eng.foldin_predict(side, cand, 0.0))
        assert "no folded-in rows" in refused(lambda: eng.foldin_topn(side, cand, 0.0, 3))
        assert "no hyper-parameters yet" in refused(lambda: eng.hyper_add(side, 2.0))       # no half-iteration has run
        # a side with features; a probit side
        fs, fc = pair_of_sides(eng)
        eng.set_features(fs, np.ones((fs.ncols, 2)), 5.0, 4)
        assert "the side has features" in refused(lambda: eng.hyper_reserve(fs, 1))
        assert "the side has features" in refused(lambda: eng.foldin(fs, fc, 0.0, R, 7))
        ps, pc = pair_of_sides(eng)
        eng.set_probit(ps, 0.5, 1)
        assert "probit side" in refused(lambda: eng.foldin(ps, pc, 0.0, R, 7))
        assert "probit side" in refused(lambda: eng.hyper_reserve(ps, 1))
    finally:
        eng.close()


# ---- 7. the chain -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted_run():
    """gibbs(foldin=True) on the planted matrix without its 100 held-out users, then fold_in of what they arrive with"""
    import bpmf_amd
    P = fr.PLANTED
    d = fr.planted_data(**P)
    M, Mt, nu = fr.planted_matrices(d, False)
    R = fr.planted_new_rows(d)
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, None, nu, P["nmovies"], nsims=P["nsims"], burnin=P["burnin"], alpha=P["alpha"], foldin=True, keep_samples=True)
        out = bpmf_amd.fold_in(res, new_rows=R, topn=5)
        E = eng.foldin_get(res["users"].side)
        hyp = eng.hyper_get(res["users"].side)
        plain = bpmf_amd.gibbs(eng, M, Mt, None, nu, P["nmovies"], nsims=8, burnin=4, alpha=P["alpha"])
        with_ = bpmf_amd.gibbs(eng, M, Mt, None, nu, P["nmovies"], nsims=8, burnin=4, alpha=P["alpha"], foldin=True)
    finally:
        eng.close()
    return dict(d=d, M=M, Mt=Mt, nu=nu, R=R, res=res, out=out, E=E, hyp=hyp, plain=plain, with_=with_)


def test_chain_equals_restatement_on_its_own_samples(planted_run):
    P, run = fr.PLANTED, planted_run
    res, out = run["res"], run["out"]
    S = P["nsims"] - P["burnin"]
    alphas, mus, Lams = run["hyp"]
    assert alphas.shape == (S,) and (alphas == P["alpha"]).all() and mus.shape == (S, P["K"]) and Lams.shape == (S, P["K"], P["K"])
    assert np.abs(Lams - np.transpose(Lams, (0, 2, 1))).max() <= 1e-12 * np.abs(Lams).max()
    Vs = np.stack([v for _, v in res["samples"][P["burnin"]:]])
    mr = res["movies"].mean_rating
    want = fr.fold_in(run["R"], Vs, alphas, mus, Lams, mr, fr.TAG_ROWS)
    err = np.abs(run["E"] - want).max() / np.abs(want).max()
    print("chain: max|du| / max|u| = %.3g" % err)
    assert run["E"].shape == (P["held"], S, P["K"]) and err <= BAR
    i, c, r = fr.planted_cells(run["d"])
    assert len(r) == 1200
    got, ref = fr.rmse(r, out["rows"]["mean"][i, c]), fr.rmse(r, fr.predict(want, Vs, mr)[0][i, c])
    print("chain: RMSE at the held-out cells %.6f (restatement on the same samples %.6f; CPU chain %.6f, mean predictor %.6f)"
          % (got, ref, fr.PLANTED_MEASURED[0], fr.rmse(r, np.full(len(r), mr))))
    assert abs(got - ref) <= 1e-6
    assert got <= fr.rmse(r, np.full(len(r), mr)) - fr.PLANTED_HALF_MARGIN
    # the lists: the argsort of the block's mean without the users' own 12 movies
    idx = out["rows"]["topn"][0]
    own = [run["R"].indices[run["R"].indptr[q]:run["R"].indptr[q + 1]] for q in range(P["held"])]
    assert np.array_equal(idx, fr.topn_of(out["rows"]["mean"], 5, own))
    # and the chain itself does not notice: the same trace with and without foldin=True
    a, b = run["plain"], run["with_"]
    assert np.array_equal(a["U"], b["U"]) and np.array_equal(a["V"], b["V"]) and a["norm_u"] == b["norm_u"] and a["norm_m"] == b["norm_m"]
    assert "foldin" not in a and b["foldin"] is True


def test_fold_in_new_columns_and_adaptive_noise():
    """new movies against the users' ring (tag 8), on a chain with noise='adaptive': the hyper ring holds every iteration's own alpha"""
    import bpmf_amd
    K = 8
    M, Mt, T, Tt, nu, nm = util.synthetic(120, 90, 2400, seed=12)
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=7, burnin=3, Tt=Tt, noise="adaptive", foldin=True, keep_samples=True, pipelined=False)
        alphas, mus, Lams = eng.hyper_get(res["movies"].side)
        assert np.array_equal(alphas, np.array(res["alpha"][3:])) and len(set(alphas.tolist())) == 4
        C = fr.rows_with_counts([0, 4, 30], nu, 2).T.tocsc()                  # [nusers, 3 new movies]
        out = bpmf_amd.fold_in(res, new_cols=C, topn=3)
        assert out["cols"]["mean"].shape == (nu, 3) and out["cols"]["topn"][0].shape == (3, 3) and "rows" not in out
        Us = np.stack([u for u, _ in res["samples"][3:]])
        want = fr.fold_in(C.T.tocsr(), Us, alphas, mus, Lams, res["movies"].mean_rating, fr.TAG_COLS)
        E = eng.foldin_get(res["movies"].side)
        assert np.abs(E - want).max() <= BAR * np.abs(want).max()
        m2 = fr.predict(want, Us, res["movies"].mean_rating)[0]
        np.testing.assert_allclose(out["cols"]["mean"], m2.T, rtol=0, atol=1e-9 * np.abs(m2).max())
    finally:
        eng.close()


def _csv(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "query,rank,candidate,mean,std"
    return np.array([l.split(",") for l in lines[1:]], dtype=float)


def test_cli_fold_in_rows_end_to_end(planted_run, tmp_path):
    from bpmf_amd import io
    P, run = fr.PLANTED, planted_run
    nu, nm, N = run["nu"], P["nmovies"], 5
    io.write_sparse(tmp_path / "train.sdm", nu, nm, run["M"])
    Rc = run["R"].tocsc(); Rc.sort_indices()
    io.write_sparse(tmp_path / "new.sdm", P["held"], nm, (Rc.indptr.astype(np.int64), Rc.indices.astype(np.int32), Rc.data))
    (tmp_path / "out").mkdir(); (tmp_path / "plain").mkdir()
    base = ["-n", "train.sdm", "-p", "train.sdm", "-d", str(P["K"]), "-i", str(P["nsims"]), "-b", str(P["burnin"]), "-a", str(P["alpha"])]
    run_ = lambda a: subprocess.run([BPMF] + a, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    r = run_(base + ["--fold-in-rows", "new.sdm", "--topn", str(N), "-o", "out"])
    assert r.returncode == 0, r.stderr
    assert "fold-in rows: 100 (--fold-in-rows), 1200 ratings" in r.stdout
    r0 = run_(base + ["-o", "plain"])
    assert r0.returncode == 0 and "fold-in" not in r0.stdout and not list((tmp_path / "plain").glob("foldin-*"))
    strip = lambda text: [[f for f in l.split("\t") if not f.startswith(("items/sec", "ratings/sec"))] for l in text.splitlines() if "iteration" in l]
    assert strip(r.stdout) == strip(r0.stdout) and len(strip(r.stdout)) == P["nsims"]
    out = run["out"]["rows"]
    for name, want in (("foldin-rows-mean", out["mean"]), ("foldin-rows-std", out["std"])):
        got = io.read_dense(tmp_path / "out" / (name + ".ddm"))
        assert got.shape == want.shape == (P["held"], nm), name
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9, err_msg=name)
    rec = _csv(tmp_path / "out" / "foldin-rows-topn.csv")
    nq = P["held"]
    assert rec.shape == (nq * N, 5)
    assert (rec[:, 0].reshape(nq, N) == np.arange(1, nq + 1)[:, None]).all() and (rec[:, 1].reshape(nq, N) == np.arange(1, N + 1)).all()
    idx, tm, ts = out["topn"]
    assert np.array_equal(rec[:, 2].reshape(nq, N) - 1, idx)
    np.testing.assert_allclose(rec[:, 3].reshape(nq, N), tm, rtol=1e-9, atol=1e-9); np.testing.assert_allclose(rec[:, 4].reshape(nq, N), ts, rtol=1e-9, atol=1e-9)
    assert not (tmp_path / "out" / "foldin-cols-mean.ddm").exists()
