"""Implicit feedback on the GPU (`gibbs(..., implicit=w0)`, engine.set_implicit / implicit_sample).

  * one half-iteration of every sampler family against the DENSE reference of tests/implicit_ref.py -- every cell of a column an
    explicit weighted rating, G never formed -- on weights_ref.edge_side()'s pattern with values 1, w = w0 + 0.05 + Gamma(2, 0.5),
    w0 = 0.3, alpha = 1.7, at BPMF_HIP_CHUNK=16 and at the automatic chunk; the bars are the project's (RTOL, STAT_TOL).  The plain
    side is more than max|x| away from that reference, so a wrong w0, alpha or side in G fails it
  * bits: two launches; G across calls and across BPMF_LINK_WG_CHUNKS; an `other` whose columns have no ratings contributes to G;
    a padded num_latent (10, 100) leaves the extra dimensions exactly 0; weights_get is numpy's sqrt(w - w0) and w r / sqrt(w - w0)
  * refusals in both orders
  * the chain against the restated dense chain (60 x 40, K = 8 and 64)
  * the planted experiment: the implicit chain ranks the held-out ones better than the plain chain on the ones and than popularity
  * `bpmf --implicit W0 --rank-eval N -o DIR` end to end, --rank-eval on a plain run, and a run without the flags
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import implicit_ref as ref
from tests import util
from tests.test_gpu_parity import RTOL, rel_err
from tests.conftest import ROOT
from tests.test_gpu_probit import _from_device, _hip_runtime, _to_device, _write_mtx
from tests.test_gpu_weights import ALPHA, FAMILIES, STAT_TOL, _env, _factors

pytestmark = pytest.mark.gpu

W0 = 0.3


def _pair(eng, A, nrows, X, Y, w, w0=W0):
    """An implicit side over the ratings A holding the factors X, and an implicit partner WITHOUT ratings holding Y."""
    ncols = len(A[0]) - 1
    me = eng.side_create(ncols, nrows, *A, 0.0)
    ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_implicit(me, w0, w)
    eng.set_implicit(ot, w0)
    eng.set_items(me, X)
    eng.set_items(ot, Y)
    return me, ot


def _step(eng, A, nrows, X, Y, w):
    """the first half-iteration (counter 0, cov 0) of a fresh pair -> items, norm, cov, G, the kernel's name"""
    me, ot = _pair(eng, A, nrows, X, Y, w)
    name = eng.kernel_name(me)
    eng.implicit_sample(me, ot, ALPHA)
    it, norm, cov = eng.sys_state(me)[:3]
    assert it == 0
    out = eng.get_items(me), norm, np.array(cov), eng.implicit_gram(me), name
    eng.side_destroy(me); eng.side_destroy(ot)
    return out


@pytest.mark.parametrize("chunk", [16, None])
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_half_iteration_against_the_dense_reference(oracle, fam, chunk):
    import bpmf_amd
    _, K, env, kern, _ = fam
    A, nrows, w = ref.edge_implicit(W0)
    ncols = len(A[0]) - 1
    X, Y = _factors(K, ncols, nrows, 1200 + K)
    with _env(**dict(env, **({"BPMF_HIP_CHUNK": chunk} if chunk else {}))):
        eng = bpmf_amd.HipEngine(K)
        try:
            items, norm, cov, G, name = _step(eng, A, nrows, X, Y, w)
        finally:
            eng.close()
    assert re.search(kern, name), name
    mu, LU, LF = oracle.hyper_sample(K, ncols, np.zeros((K, K)), 0)
    want = X.copy()
    s_ref, p_ref, n_ref = ref.sample_side_dense(oracle, K, A, w, W0, ALPHA, Y, want, 0, mu, LF)
    plain = X.copy()
    oracle.sample_side(K, A, 0.0, ALPHA, Y, plain, 0, mu, LF, nthreads=ref.NT)
    err, away = rel_err(items, want), rel_err(plain, want)
    # the sums of a blocking half-iteration stay inside the library: what it forms from them (cov, norm) and the sums of its factors
    cov_ref = oracle.cov(K, ncols, s_ref, p_ref)
    e_cov, e_sum, e_prod = rel_err(cov, cov_ref), rel_err(items.sum(0), s_ref), rel_err(items.T @ items, np.asarray(p_ref).reshape(K, K))
    print("K %d chunk %s: factors %.3g (the plain side: %.3g), cov %.3g, sum %.3g, prod %.3g, norm %.3g"
          % (K, chunk, err, away, e_cov, e_sum, e_prod, abs(norm - n_ref) / abs(n_ref)))
    assert np.all(np.isfinite(items))
    assert away > 1.0                                                 # (what the test would see without the feature)
    assert err < RTOL, err
    assert e_cov < STAT_TOL and e_sum < STAT_TOL and e_prod < STAT_TOL and abs(norm - n_ref) <= STAT_TOL * abs(n_ref)
    assert rel_err(G, Y.T @ Y) < 1e-12                                # every column of the partner, none of which has a rating


@pytest.mark.parametrize("K", [8, 10, 64, 100])
def test_bits_gram_and_padding(K):
    import bpmf_amd
    A, nrows, w = ref.edge_implicit(W0)
    ncols = len(A[0]) - 1
    X, Y = _factors(K, ncols, nrows, 1300 + K)
    eng = bpmf_amd.HipEngine(K)
    try:
        a = _step(eng, A, nrows, X, Y, w)
        b = _step(eng, A, nrows, X, Y, w)
        with _env(BPMF_LINK_WG_CHUNKS=1):
            c = _step(eng, A, nrows, X, Y, w)
        with _env(BPMF_LINK_WG_CHUNKS=3):
            d = _step(eng, A, nrows, X, Y, w)
        for o in (b, c, d):
            assert o[0].tobytes() == a[0].tobytes() and o[1] == a[1] and o[2].tobytes() == a[2].tobytes() and o[3].tobytes() == a[3].tobytes()
        assert np.abs(a[3]).min() > 0 and np.array_equal(a[3], a[3].T)
        # a partner with other factors: another G, other factors
        e = _step(eng, A, nrows, X, 2.0 * Y, w)
        assert rel_err(e[3], 4.0 * a[3]) < 1e-14 and rel_err(e[0], a[0]) > 1e-3
        # the device's own leading dimension: the dimensions K .. ld - 1 stay exactly 0
        # (the side is bound to a buffer of the test's own, [ncols, ld]: its samplers then write in place)
        ld = eng.ld()
        me, ot = _pair(eng, A, nrows, X, Y, w)
        padded = np.zeros((ncols, ld)); padded[:, :K] = X
        hip = _hip_runtime()
        buf = _to_device(hip, padded)
        try:
            eng.bind_items(me, buf.value, ld=ld, nbytes=padded.nbytes)
            eng.implicit_sample(me, ot, ALPHA)
            eng.sync()
            got = _from_device(hip, buf, padded)
            assert got[:, :K].tobytes() == a[0].tobytes()
            if ld > K:
                assert np.count_nonzero(got[:, K:]) == 0 and not np.signbit(got[:, K:]).any()
            eng.side_destroy(me); eng.side_destroy(ot)
        finally:
            hip.hipFree(buf)
    finally:
        eng.close()


def test_weights_get_is_numpy_bit_for_bit():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    w = W0 + 0.05 + np.random.default_rng(7).gamma(2.0, 0.5, len(M[2]))
    eng = bpmf_amd.HipEngine(16)
    try:
        me = eng.side_create(nm, nu, *M, 0.0)
        eng.set_implicit(me, W0, w)
        sw, zw = eng.weights_get(me)
        assert sw.tobytes() == np.sqrt(w - W0).tobytes() and zw.tobytes() == (w * M[2] / np.sqrt(w - W0)).tobytes()
        assert eng.implicit_w0(me) == W0 and eng.weights_count(me) == (len(w), float(w.min()), float(w.max()))
        one = eng.side_create(nm, nu, *M, 0.0)
        eng.set_implicit(one, W0)                                    # no confidences: every one is 1
        sw, zw = eng.weights_get(one)
        assert sw.tobytes() == np.sqrt(np.ones(len(w)) - W0).tobytes() and zw.tobytes() == (M[2] / np.sqrt(np.ones(len(w)) - W0)).tobytes()
        assert eng.implicit_w0(eng.side_create(nm, nu, *M, 0.0)) == 0.0
    finally:
        eng.close()


def test_refusals_in_both_orders(oracle):
    import bpmf_amd
    from bpmf_amd import BpmfHipError
    K = 8
    M, Mt, T, Tt, nu, nm = util.tiny()
    nnz = len(M[2])
    w = np.full(nnz, 1.5)
    eng = bpmf_amd.HipEngine(K)
    try:
        new = lambda mean=0.0: eng.side_create(nm, nu, *M, mean)
        with pytest.raises(BpmfHipError, match="side_set_implicit: the side's mean rating is .* needs exactly 0"):
            eng.set_implicit(new(util.mean_rating(M)), W0, w)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(BpmfHipError, match="side_set_implicit: w0 must be finite and > 0"):
                eng.set_implicit(new(), bad, w)
        for v in (W0, 0.1, float("nan"), float("inf")):
            wrong = w.copy(); wrong[2] = v; wrong[4] = 0.0              # the first offender is named
            with pytest.raises(BpmfHipError, match=r"side_set_implicit: the confidence \S+ of rating 2 is not finite and > w0 = 0.3"):
                eng.set_implicit(new(), W0, wrong)
        with pytest.raises(BpmfHipError, match="needs w0 < 1"):
            eng.set_implicit(new(), 1.0)
        with pytest.raises(ValueError, match="confidences for a side of"):
            eng.set_implicit(new(), W0, w[:-1])
        # a side with another add-on refuses set_implicit ...
        s = new(); eng.set_weights(s, w)
        with pytest.raises(BpmfHipError, match="side_set_implicit: not on a side with per-rating weights"):
            eng.set_implicit(s, W0, w)
        s = new(); eng.set_robust(s, 4.0, 9)
        with pytest.raises(BpmfHipError, match="side_set_implicit: not on a side with Student-t noise"):
            eng.set_implicit(s, W0, w)
        s = new(); eng.set_probit(s, 3.0, 1)
        with pytest.raises(BpmfHipError, match="side_set_implicit: not on a probit side"):
            eng.set_implicit(s, W0, w)
        s = new(); eng.set_censored(s, np.zeros(nnz, np.int8), 5)
        with pytest.raises(BpmfHipError, match="side_set_implicit: not on a censored side"):
            eng.set_implicit(s, W0, w)
        s = new(); eng.set_features(s, np.random.default_rng(1).standard_normal((nm, 2)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="side_set_implicit: not together with features"):
            eng.set_implicit(s, W0, w)
        s = new(); eng.set_prop_posterior(s, np.tile(np.eye(K).ravel(), (nm, 1)))
        with pytest.raises(BpmfHipError, match="side_set_implicit: not together with propagated priors"):
            eng.set_implicit(s, W0, w)
        s = new(); eng.hyper_reserve(s, 2)
        with pytest.raises(BpmfHipError, match="side_set_implicit: not together with fold-in"):
            eng.set_implicit(s, W0, w)
        ru, rm = eng.side_create(nu, nm, *Mt, 0.0), new()
        eng.sys_set_reduce(rm, ru)
        with pytest.raises(BpmfHipError, match="side_set_implicit: .*BPMF_REDUCE"):
            eng.set_implicit(rm, W0, w)
        part = eng.side_create(nm, nu, M[0][:2] - M[0][0], M[1][:M[0][1]], M[2][:M[0][1]], 0.0, 0, 1)
        with pytest.raises(BpmfHipError, match="side_set_implicit: .*whole"):
            eng.set_implicit(part, W0)
        # ... and an implicit side refuses the others
        me, us = new(), eng.side_create(nu, nm, *Mt, 0.0)
        eng.set_implicit(me, W0, w)
        with pytest.raises(BpmfHipError, match="side_set_implicit: the side is an implicit side already"):
            eng.set_implicit(me, W0, w)
        with pytest.raises(BpmfHipError, match="side_set_weights: not on an implicit side"):
            eng.set_weights(me, w)
        with pytest.raises(BpmfHipError, match="side_set_robust: not on a side with per-rating weights"):
            eng.set_robust(me, 4.0, 9)
        with pytest.raises(BpmfHipError, match="side_set_probit: not on a side with per-rating weights"):
            eng.set_probit(me, 3.0, 1)
        with pytest.raises(BpmfHipError, match="side_set_censored: not on a side with per-rating weights"):
            eng.set_censored(me, np.zeros(nnz, np.int8), 5)
        with pytest.raises(BpmfHipError, match="not on a side with per-rating weights"):
            eng.set_features(me, np.random.default_rng(1).standard_normal((nm, 2)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="set_prop_posterior: not on a side with per-rating weights"):
            eng.set_prop_posterior(me, np.tile(np.eye(K).ravel(), (nm, 1)))
        with pytest.raises(BpmfHipError, match="side_hyper_reserve: not on an implicit side"):
            eng.hyper_reserve(me, 2)
        with pytest.raises(BpmfHipError, match="sys_set_reduce: not together with per-rating weights"):
            eng.sys_set_reduce(me, us)
        # one-sided models, and the other ways to step a side
        with pytest.raises(BpmfHipError, match="implicit_sample: the other side is not implicit: both sides"):
            eng.implicit_sample(me, us, 2.0)
        with pytest.raises(BpmfHipError, match="implicit_sample: the side is not implicit"):
            eng.implicit_sample(us, me, 2.0)
        for a, b in ((me, us), (us, me)):
            with pytest.raises(BpmfHipError, match="sys_sample: the model is implicit: step BOTH sides with bpmf_hip_implicit_sample"):
                eng.sys_sample(a, b, 2.0)
            with pytest.raises(BpmfHipError, match="link_sample: the model is implicit"):
                eng.link_sample(a, b, 2.0)
        mu, LU, LF = oracle.hyper_sample(K, nm, np.zeros((K, K)), 0)
        with pytest.raises(BpmfHipError, match="sample_side: the side is implicit: step it with bpmf_hip_implicit_sample"):
            eng.sample_side(me, us, 0, 2.0, mu, LF)
        eng.set_implicit(us, 0.2)
        with pytest.raises(BpmfHipError, match="implicit_sample: the two sides were given different w0"):
            eng.implicit_sample(me, us, 2.0)
        us2 = eng.side_create(nu, nm, *Mt, 0.0)
        eng.set_implicit(us2, W0)
        for bad in (0.0, float("nan")):
            with pytest.raises(BpmfHipError, match="implicit_sample: alpha must be finite and > 0"):
                eng.implicit_sample(me, us2, bad)
        assert eng.sys_state(me)[0] == -1                             # nothing above stepped the side
    finally:
        eng.close()
    e32 = bpmf_amd.HipEngine(128, dtype="f32")
    try:
        with pytest.raises(BpmfHipError, match="side_set_implicit: not on an fp32 context"):
            e32.set_implicit(e32.side_create(nm, nu, *M, 0.0), W0)
        with pytest.raises(ValueError, match="implicit does not go together with an fp32 engine"):
            bpmf_amd.gibbs(e32, M, Mt, T, nu, nm, nsims=2, burnin=0, implicit=W0)
    finally:
        e32.close()


# ---- the chain --------------------------------------------------------------------------------------------------------------------------

CHAIN = dict(nsims=6, burnin=2, alpha=1.5)


@functools.lru_cache(maxsize=None)
def _restated(K, weighted):
    from oracle.oracle import Oracle
    M, Mt, T, Tt, nu, nm = ref.small_ones()
    W = (M[0], M[1], 0.5 + np.random.default_rng(3).gamma(2.0, 0.5, len(M[2]))) if weighted else None
    return ref.restate_chain(Oracle(), K, M, Mt, T, W, W0, CHAIN["nsims"], CHAIN["burnin"], CHAIN["alpha"], keep=True), W


@pytest.mark.parametrize("K,weighted", [(8, False), (64, False), (8, True)])
def test_implicit_chain_against_the_dense_chain(K, weighted):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = ref.small_ones()
    assert 0.05 < len(M[2]) / (nu * nm) < 0.11
    want, W = _restated(K, weighted)
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, implicit=W0, weights=W, rank_eval=10, topn=32, **CHAIN)
        plain = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, **CHAIN)
    finally:
        eng.close()
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(res["U"] - want["U"]).max() / scale, np.abs(res["V"] - want["V"]).max() / scale
    et = max(np.abs(np.array(res["rmse"]) - want["rmse"]).max(), np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max())
    ef = abs(res["final_rmse_avg"] - want["final_rmse_avg"])
    print("K %d weighted %s: U %.3g V %.3g traces %.3g final %.3g" % (K, weighted, eu, ev, et, ef))
    assert eu < 1e-6 and ev < 1e-6 and et < 1e-6 and ef < 1e-6, (eu, ev, et, ef)
    im = res["implicit"]
    assert im["w0"] == W0 and im["observed"] == len(M[2]) and im["cells"] == nu * nm and "weights" not in res and "implicit" not in plain
    assert (im["weights"][0] > 0) == weighted
    assert np.abs(plain["U"] - res["U"]).max() / scale > 1e-2
    # the ranks of the test ones (value > 0 under implicit=), against the top-32 list of the same rings and against the restated chain
    rk = res["rank"]
    ones = np.asarray(T[2]) > 0
    assert rk["n"] == 10 and rk["by"] == "rows" and rk["entries"] == int(ones.sum()) and np.all((rk["rank"] > 0) == ones)
    users = np.asarray(T[1])
    movies = np.repeat(np.arange(nm), np.diff(T[0]))
    idx = res["topn"][0]
    for p in np.nonzero(ones)[0]:
        r = int(rk["rank"][p])
        assert (r <= 32 and idx[users[p], r - 1] == movies[p]) or (r > 32 and movies[p] not in idx[users[p]])
    tptr, tcand, cell = bpmf_amd.held_out_lists(T, nu, "rows", 0.0)
    score = ref.mean_scores(want["samples"])
    d = 4e-6 * scale * scale * K                                     # both factors of a pair within 1e-6 scale of the restated ones, K terms
    rated = ref.rated_sets(Mt, nu)
    for q in range(nu):
        ok = np.ones(nm, bool); ok[sorted(rated[q])] = False
        assert rk["ncand"][q] == ok.sum()
        for p in range(tptr[q], tptr[q + 1]):
            c = tcand[p]
            ok2 = ok.copy(); ok2[c] = False
            lo, hi = int((score[q, ok2] > score[q, c] + d).sum()), int((score[q, ok2] > score[q, c] - d).sum())
            assert lo <= rk["rank"][cell[p]] - 1 <= hi
    m = bpmf_amd.rank_metrics(rk["rank"][cell], tptr, rk["ncand"], 10)
    assert all(rk[k] == m[k] or (np.isnan(rk[k]) and np.isnan(m[k])) for k in m)
    # rank_eval on the plain Gaussian run: every test cell is a held-out item
    eng = bpmf_amd.HipEngine(K)
    try:
        g = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, rank_eval=5, rank_by="cols", **CHAIN)
    finally:
        eng.close()
    assert g["rank"]["entries"] == len(T[2]) and g["rank"]["rank"].min() >= 1 and len(g["rank"]["ncand"]) == nm
    assert plain["U"].tobytes() == g["U"].tobytes()                   # the evaluation leaves the chain alone


# ---- the planted experiment -------------------------------------------------------------------------------------------------------------

def test_planted_implicit_ranks_best():
    """200 x 120, rank 4, a cell is a one with the probability sigmoid(1.6 u . v - 2.6); 20 % of the ones held out (implicit_ref.PLANTED).
    Restated on the CPU (implicit_ref.PLANTED_MEASURED), (recall@10, MPR):
        the implicit chain, w0 = 0.3       (0.4249, 0.2173)
        the plain chain on the ones only   (0.1029, 0.5071)
        the popularity ranking             (0.1660, 0.4148)
    Asserted on the GPU: the implicit arm has the best recall@10 and the lowest MPR of the three."""
    import bpmf_amd
    P = ref.PLANTED
    d = ref.planted(**P)
    nu, nm = P["nusers"], P["nmovies"]
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        run = dict(nsims=P["nsims"], burnin=P["burnin"], alpha=P["alpha"], Tt=d["Tt"], rank_eval=P["n"])
        a = bpmf_amd.gibbs(eng, d["M"], d["Mt"], d["T"], nu, nm, implicit=P["w0"], **run)["rank"]
        b = bpmf_amd.gibbs(eng, d["M"], d["Mt"], d["T"], nu, nm, **run)["rank"]
    finally:
        eng.close()
    c = ref.score_arm(ref.popularity_scores(d), d, P["n"])
    print("(recall@%d, MPR): implicit (%.4f, %.4f), plain (%.4f, %.4f), popularity (%.4f, %.4f)"
          % (P["n"], a["recall"], a["mpr"], b["recall"], b["mpr"], c[0], c[1]))
    assert a["entries"] == len(d["T"][2]) == b["entries"]
    assert a["recall"] > max(b["recall"], c[0]) and a["mpr"] < min(b["mpr"], c[1])


# ---- the executable ---------------------------------------------------------------------------------------------------------------------

def _coords(A):
    return np.asarray(A[1]), np.repeat(np.arange(len(A[0]) - 1), np.diff(A[0])), np.asarray(A[2])


def _finals(stdout, n):
    out = {}
    for key, label in (("recall", "recall@%d" % n), ("ndcg", "NDCG@%d" % n), ("mrr", "MRR"), ("mpr", "MPR"), ("auc", "rank AUC")):
        m = re.search(r"^Final %s: (\S+)$" % re.escape(label), stdout, re.M)
        assert m, (label, stdout)
        out[key] = float(m.group(1))
    return out


def test_cli_implicit_and_rank_eval(tmp_path):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = ref.small_ones()
    _write_mtx(tmp_path / "train.mtx", nu, nm, *_coords(M))
    _write_mtx(tmp_path / "test.mtx", nu, nm, *_coords(T))
    run = dict(nsims=6, burnin=2, alpha=1.5, Tt=Tt)
    eng = bpmf_amd.HipEngine(8)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, implicit=W0, rank_eval=10, **run)
        plain = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, rank_eval=5, rank_by="cols", **run)
    finally:
        eng.close()
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    base = [exe, "-n", str(tmp_path / "train.mtx"), "-p", str(tmp_path / "test.mtx"), "-a", "1.5", "-i", "6", "-b", "2", "-d", "8"]
    for d in ("o", "p", "q"):
        (tmp_path / d).mkdir()

    def go(extra):
        out = subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        return out

    def check(out, want, n, by_cols, odir):
        lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", out.stdout)
        got = np.array([[float(a), float(b)] for a, b in lines])
        assert got.shape == (6, 2) and np.abs(got[:, 0] - want["rmse"]).max() <= 5e-5 and np.abs(got[:, 1] - want["rmse_avg"]).max() <= 5e-5
        fin = _finals(out.stdout, n)
        for k, v in fin.items():                                     # six significant digits are printed
            assert abs(v - want["rank"][k]) <= 5e-6 * max(1.0, abs(want["rank"][k])), (k, v, want["rank"][k])
        assert out.stdout.index("Final Avg RMSE:") < out.stdout.index("Final recall@")
        rows = np.loadtxt(tmp_path / odir / "ranks.csv", delimiter=",", skiprows=1, dtype=np.int64).reshape(-1, 4)
        assert open(tmp_path / odir / "ranks.csv").readline().strip() == "query,candidate,rank,ncand"
        users, movies, vals = _coords(T)
        cell = {((m, u) if by_cols else (u, m)): p for p, (u, m) in enumerate(zip(users.tolist(), movies.tolist()))}
        per_cell = np.zeros(len(vals), np.int64)
        for q, c, r, ncd in rows:
            per_cell[cell[(q - 1, c - 1)]] = r
            assert ncd == want["rank"]["ncand"][q - 1]
        assert np.array_equal(per_cell, want["rank"]["rank"]) and len(rows) == want["rank"]["entries"]

    a = go(["--implicit", "0.3", "--rank-eval", "10", "-o", "o"])
    assert re.search(r"^implicit: w0 0\.3, %d observed of %d x %d cells$" % (len(M[2]), nu, nm), a.stdout, re.M), a.stdout
    check(a, res, 10, False, "o")
    b = go(["--rank-eval", "5", "--rank-by", "cols", "-o", "p"])
    assert "implicit:" not in b.stdout
    check(b, plain, 5, True, "p")
    # without -o: the same five lines, no file; without the flags: nothing of either
    c = go(["--implicit", "0.3", "--rank-eval", "10"])
    assert _finals(c.stdout, 10) == _finals(a.stdout, 10) and not (tmp_path / "ranks.csv").exists()
    d = go(["-o", "q"])
    assert "implicit" not in d.stdout and "recall" not in d.stdout and "rank" not in d.stdout and not (tmp_path / "q" / "ranks.csv").exists()
    assert sorted(os.listdir(tmp_path / "q")) == sorted(f for f in os.listdir(tmp_path / "p") if f != "ranks.csv")
    lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", d.stdout)
    got = np.array([[float(x), float(y)] for x, y in lines])
    assert np.abs(got[:, 0] - plain["rmse"]).max() <= 5e-5 and np.abs(got[:, 1] - plain["rmse_avg"]).max() <= 5e-5
