"""Row and column bias terms (`gibbs(..., bias=True | LAMBDA)`) on the GPU.

  * the bias step (k_bias_resid, k_bias_piece_sums, k_bias_draw, k_bias_values) against the longdouble restatement of
    tests/bias_ref.py on the edge side (columns of 0, 1, 63, 64, 65, 255, 256, 257 and 3 x piece + 1 ratings: every piece boundary and
    a column of four parked partials), K = 8 (modes 1 and 3), 10, 32, 64, 100, 128, given factors and a given c.  The bar on a
    column's bias is derived (bias_ref.bar):
        |b - b_ref| <= 2 alpha (n + Kt + 8) 2^-53 M / (lambda + alpha n) + 8 2^-53 (|mean part| + |noise part|)
    z is checked bit for bit against (r - b_dev[col]) - c[row].
  * two launches of one iteration bit-equal; another iteration or another tag changes every bias
  * 2 000 empty columns draw from the prior: the restatement's values, and their sum of squares inside the chi-square 1e-6 interval
  * a fixed lambda is what bias_lambda reports, one step per launch and no k_bias_lambda launch
  * the lambda draw (k_bias_lambda) at N = 1, 255, 256, 257, 2 001 against the numpy restatement of the same Marsaglia-Tsang draw to the
    bar of the robust weight draw, the trace against bias_lambda, and a 20-iteration chain with a sampled lambda
  * the ring rows: predict_block, topn and predict_cells against numpy over the samples of mean + b_s + c_s + u_s . v_s at K = 8, 10,
    30, 32, 64; equal roles, unequal rows per sample, biases on one side only and num_latent > 126 refused
  * k_predict_bias against longdouble mean + b + c + u . v at 0, 1, 255, 256, 257 entries, with and without a twin, to the bars of
    tests/test_gpu_posterior_outputs.py; with b = c = 0 the bytes of k_predict
  * one half-iteration through each sampler family with z in place of the ratings, against oracle.sample_side
  * 20-iteration chains at K = 32 and 64 on ml-100k against bias_ref.restate_chain, to the bars of the censored chain test
  * a run without bias twice gives the same bytes, and the kernel of a side without biases is the one it was
  * every refusal of the C ABI and of gibbs; the failure word on non-finite factors
  * the planted experiment: the device's two final RMSEs against the recorded pair of tests/golden/bias_planted.json
"""
import functools
import re

import numpy as np
import pytest

from tests import bias_ref as ref
from tests import util
from tests.test_gpu_censored import _env, _hyper
from tests.test_gpu_parity import RTOL, rel_err
from tests.test_gpu_posterior_outputs import (LD, MEAN_M, MEAN_U, NS, PN, _check_predict, _empty_side, _same_bytes, predict_factors,
                                               predict_matrix, transpose_matrix)
from tests.test_gpu_probit import _product_form_side

pytestmark = pytest.mark.gpu

NT = ref.NT
ENUM, EINVAL = -5, -1
ALPHA, LAM = 1.7, 2.5       # neither a power of two


def _pair(eng, A, nrows, X, Y, c, lam=LAM, tag=ref.TAG_MOVIES, mean=None):
    """A side with biases over the ratings A holding the factors X, and a partner without ratings holding Y and the biases c."""
    ncols = len(A[0]) - 1
    me = eng.side_create(ncols, nrows, *A, util.mean_rating(A) if mean is None else mean)
    ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_bias(me, lam, tag, 0)
    eng.set_bias(ot, lam, ref.TAG_USERS if tag != ref.TAG_USERS else ref.TAG_MOVIES, 1)
    eng.bias_set(ot, c)
    eng.set_items(me, X)
    eng.set_items(ot, Y)
    return me, ot


@functools.lru_cache(maxsize=None)
def _edge():
    A, nrows = ref.edge_side()
    counts = np.diff(A[0])
    assert len(counts) == 33 + len(ref.EDGE_COUNTS) and tuple(counts[33:]) == ref.EDGE_COUNTS and counts[3] == 0
    return A, nrows


# ---- 1. the step against the restatement --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,mode", [(8, 1), (8, 3), (10, None), (32, None), (64, None), (100, None), (128, None)])
def test_step_against_restatement(K, mode):
    import bpmf_amd
    A, nrows = _edge()
    ncols, mean, it = len(A[0]) - 1, util.mean_rating(A), 5
    X, Y = ref.factors(K, ncols, nrows)
    c = np.random.default_rng(60 + K).standard_normal(nrows)
    mu, LU, LF = _hyper(K, ncols, it, 70 + K)
    r = ref.step(A, X, Y, c, it, ref.TAG_MOVIES, ALPHA, LAM, mean)
    bar = ref.bar(r, K, ALPHA, LAM)
    with _env(**({"BPMF_HIP_MODE": mode} if mode else {})):
        eng = bpmf_amd.HipEngine(K)
        try:
            me, ot = _pair(eng, A, nrows, X, Y, c)
            assert eng.bias_latent(me).tobytes() == A[2].tobytes() and not eng.bias_get(me).any()      # before any launch
            eng.sample_side(me, ot, it, ALPHA, mu, LF)
            b, z = eng.bias_get(me), eng.bias_latent(me)
            assert eng.bias_get(ot).tobytes() == c.tobytes()
            eng.side_destroy(me); eng.side_destroy(ot)
        finally:
            eng.close()
    err = np.abs(b.astype(LD) - r["b"]).astype(np.float64)
    worst = int(np.argmax(err / bar))
    print("K %d mode %s: worst |b - b_ref| / bar %.3g (column %d of %d ratings, |b - b_ref| %.3g, bar %.3g)" %
          (K, mode, err[worst] / bar[worst], worst, r["n"][worst], err[worst], bar[worst]))
    assert np.all(np.isfinite(b)) and np.all(err <= bar), (K, worst, err[worst], bar[worst])
    assert z.tobytes() == ref.values(A, b, c).tobytes()


# ---- 2. repeated launches -----------------------------------------------------------------------------------------------------------

def test_repeated_launches_and_streams():
    import bpmf_amd
    K = 32
    A, nrows = _edge()
    ncols = len(A[0]) - 1
    X, Y = ref.factors(K, ncols, nrows, 1)
    c = np.random.default_rng(3).standard_normal(nrows)
    mu, LU, LF = _hyper(K, ncols, 2, 9)
    eng = bpmf_amd.HipEngine(K)
    try:
        got = {}
        for key, it, tag in (("a", 2, 13), ("b", 2, 13), ("iter", 3, 13), ("tag", 2, 15)):
            me, ot = _pair(eng, A, nrows, X, Y, c, tag=tag)
            eng.sample_side(me, ot, it, ALPHA, mu, LF)
            got[key] = (eng.bias_get(me), eng.bias_latent(me))
            if key == "a":                                            # ... and a second launch on the same side
                eng.set_items(me, X)
                eng.sample_side(me, ot, it, ALPHA, mu, LF)
                assert eng.bias_get(me).tobytes() == got["a"][0].tobytes() and eng.bias_latent(me).tobytes() == got["a"][1].tobytes()
            eng.side_destroy(me); eng.side_destroy(ot)
    finally:
        eng.close()
    assert got["a"][0].tobytes() == got["b"][0].tobytes() and got["a"][1].tobytes() == got["b"][1].tobytes()
    assert np.all(got["iter"][0] != got["a"][0]) and np.all(got["tag"][0] != got["a"][0])


# ---- 3. empty columns draw from the prior -------------------------------------------------------------------------------------------

def test_empty_columns_draw_from_the_prior():
    import bpmf_amd
    from scipy.stats import chi2
    K, n_empty, nrows, it = 8, 2000, 40, 4
    rng = np.random.default_rng(12)
    rows = np.sort(rng.choice(nrows, size=7, replace=False)).astype(np.int32)
    counts = np.zeros(n_empty + 1, np.int64); counts[1000] = 7       # one rated column among 2 000 empty ones
    A = (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), rows, rng.integers(1, 6, 7).astype(np.float64))
    X, Y = ref.factors(K, n_empty + 1, nrows, 2)
    c = rng.standard_normal(nrows)
    mu, LU, LF = _hyper(K, n_empty + 1, it, 5)
    r = ref.step(A, X, Y, c, it, ref.TAG_MOVIES, ALPHA, LAM, util.mean_rating(A))
    eng = bpmf_amd.HipEngine(K)
    try:
        me, ot = _pair(eng, A, nrows, X, Y, c)
        eng.sample_side(me, ot, it, ALPHA, mu, LF)
        b = eng.bias_get(me)
    finally:
        eng.close()
    assert np.all(np.abs(b.astype(LD) - r["b"]).astype(np.float64) <= ref.bar(r, K, ALPHA, LAM))
    empty = np.delete(b, 1000)
    stat = float(LAM * np.sum(empty ** 2))                            # ~ chi-square with 2 000 degrees of freedom
    lo, hi = chi2.ppf(5e-7, n_empty), chi2.ppf(1.0 - 5e-7, n_empty)
    print("lambda sum b^2 over %d empty columns: %.1f, accepted (%.1f, %.1f)" % (n_empty, stat, lo, hi))
    assert lo < stat < hi


# ---- 4. a fixed lambda ------------------------------------------------------------------------------------------------------------------

def test_fixed_lambda_is_reported_and_steps_are_counted():
    import bpmf_amd
    K = 8
    A, nrows = _edge()
    ncols = len(A[0]) - 1
    X, Y = ref.factors(K, ncols, nrows, 3)
    mu, LU, LF = _hyper(K, ncols, 0, 2)
    eng = bpmf_amd.HipEngine(K)
    try:
        me, ot = _pair(eng, A, nrows, X, Y, np.zeros(nrows), lam=0.75)
        assert eng.bias_lambda(me)[0::2] == (0.75, 0)
        for it in range(3):
            eng.sample_side(me, ot, it, ALPHA, mu, LF)
        lam, trace, steps, draws = eng.bias_lambda(me, 5)
        assert (lam, steps, draws) == (0.75, 3, 0) and np.all(trace == 0.75)          # a fixed lambda launches no k_bias_lambda
        assert eng.bias_lambda(ot)[0::2] == (0.75, 0)
    finally:
        eng.close()


# ---- 4b. a sampled lambda -----------------------------------------------------------------------------------------------------------------

LAMBDA_BAR = 1e-12          # |lambda - lambda_ref| <= 1e-12 (1 + lambda_ref): the bar of the robust weight draw (tests/test_gpu_robust.py)
MARGIN = 1e-9               # no decision of the restated draw closer than this to its threshold (robust_ref.MARGIN)


@pytest.mark.parametrize("ncols", [1, 255, 256, 257, 2001])
def test_lambda_draw_against_restatement(ncols):
    """one rated column, the rest without ratings (the draw reads the biases only): one chunk less one, one chunk, one chunk plus one,
    eight chunks"""
    import bpmf_amd
    K, nrows, a0, b0, lam0 = 8, 16, 2.0, 1.5, 0.75
    rng = np.random.default_rng(40 + ncols)
    A = (np.concatenate([[0], np.full(ncols, 3)]).astype(np.int64), np.arange(3, dtype=np.int32), np.array([1.0, 4.0, 2.0]))
    X, Y = ref.factors(K, ncols, nrows, 4)
    mu, LU, LF = _hyper(K, ncols, 0, 2)
    eng = bpmf_amd.HipEngine(K)
    try:
        me, ot = _pair(eng, A, nrows, X, Y, np.zeros(nrows), lam=lam0, mean=0.0)
        eng.bias_prior(me, a0, b0)
        eng.sample_side(me, ot, 0, ALPHA, mu, LF)                      # the side's first half-iteration: no draw
        assert eng.bias_lambda(me)[0::2] == (lam0, 1) and eng.bias_lambda(me)[3] == 0
        worst = 0.0
        for it, scale in ((3, 1.0), (7, 0.05), (9, 30.0)):
            b = scale * rng.standard_normal(ncols)
            eng.bias_set(me, b)
            eng.set_items(me, X)
            eng.sample_side(me, ot, it, ALPHA, mu, LF)
            lam, trace, steps, draws = eng.bias_lambda(me, 12)
            want, attempts, margin = ref.lambda_draw(b, it, ref.TAG_MOVIES, a0, b0)
            assert margin >= MARGIN, margin
            err = abs(lam - float(want)) / (1.0 + float(want))
            worst = max(worst, err)
            assert err <= LAMBDA_BAR, (ncols, it, lam, float(want))
            assert trace[it] == lam and np.all(trace[it:] == lam) and trace[0] == lam0              # the trace is what bias_lambda reports
            # the step behind the draw read the new word
            r = ref.step(A, X, Y, np.zeros(nrows), it, ref.TAG_MOVIES, ALPHA, lam, 0.0)
            assert np.all(np.abs(eng.bias_get(me).astype(LD) - r["b"]).astype(np.float64) <= ref.bar(r, K, ALPHA, lam))
        assert (steps, draws) == (4, 3)
        print("N %d: worst |lambda - ref| / (1 + ref) %.3g" % (ncols, worst))
        for args, msg in (((0.0, 1.0), "finite A0 > 0"), ((1.0, -1.0), "finite B0 >= 0"), ((float("nan"), 1.0), "finite A0 > 0")):
            with pytest.raises(bpmf_amd.BpmfHipError, match=msg):
                eng.bias_prior(me, *args)
        if ncols == 1:
            with pytest.raises(bpmf_amd.BpmfHipError, match="below 1"):
                eng.bias_prior(me, 0.25, 1.0)
        plain = eng.side_create(ncols, nrows, *A, 0.0)
        with pytest.raises(bpmf_amd.BpmfHipError, match="not a side with bias terms"):
            eng.bias_prior(plain, 1.0, 1.0)
    finally:
        eng.close()


def test_sampled_lambda_chain_against_cpu():
    import bpmf_amd
    from oracle.oracle import Oracle
    K, prior = 32, (2.0, 1.0)
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want = ref.restate_chain(Oracle(), K, M, Mt, T, LAM, CHAIN["nsims"], CHAIN["burnin"], CHAIN["alpha"], prior=prior)
    assert want["margin"] >= MARGIN
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, bias=LAM, bias_prior=prior, **CHAIN)
    finally:
        eng.close()
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(res["U"] - want["U"]).max() / scale, np.abs(res["V"] - want["V"]).max() / scale
    et = max(np.abs(np.array(res["rmse"]) - want["rmse"]).max(), np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max())
    el = max(np.abs(res["bias"]["lambda_rows"] / np.array(want["lam_u"]) - 1).max(), np.abs(res["bias"]["lambda_cols"] / np.array(want["lam_m"]) - 1).max())
    print("sampled lambda, K %d: U %.3g V %.3g traces %.3g lambda %.3g; lambda_rows %.3g -> %.3g" % (K, eu, ev, et, el, want["lam_u"][0], want["lam_u"][-1]))
    assert eu < 1e-6 and ev < 1e-6 and et < 1e-6 and el < 1e-6
    assert want["lam_u"][0] == LAM and len(set(want["lam_u"])) == CHAIN["nsims"]


# ---- 4c. the ring trick -------------------------------------------------------------------------------------------------------------------

def _ring_pair(eng, K, nq, nc, S, seed, roles=(1, 0), bias=(True, True)):
    """two sides without ratings, S kept samples of factors and biases -> (query side, candidate side, [S, nq, K], [S, nc, K], [S, nq], [S, nc])"""
    rng = np.random.default_rng(seed)
    q, c = _empty_side(eng, nq, nc, 0.0), _empty_side(eng, nc, nq, 0.0)
    if bias[0]:
        eng.set_bias(q, 1.0, 14, roles[0])
    if bias[1]:
        eng.set_bias(c, 1.0, 13, roles[1])
    eng.samples_reserve(q, S); eng.samples_reserve(c, S)
    Uq, Vc = 0.4 * rng.standard_normal((S, nq, K)), 0.4 * rng.standard_normal((S, nc, K))
    bq, bc = rng.standard_normal((S, nq)), rng.standard_normal((S, nc))
    for s in range(S):
        eng.set_items(q, Uq[s]); eng.set_items(c, Vc[s])
        if bias[0]:
            eng.bias_set(q, bq[s])
        if bias[1]:
            eng.bias_set(c, bc[s])
        eng.samples_add(q); eng.samples_add(c)
    return q, c, Uq, Vc, bq, bc


@pytest.mark.parametrize("K", [8, 10, 30, 32, 64])
def test_ring_rows_serve_block_topn_and_cells(K):
    """kp = roundup4(Kt + 2): 12, 12, 32, 36, 68 -- also the sizes at which the two rows fill the padding exactly (30) and open a new
    group of four (32).  predict_block, topn and predict_cells against numpy over the samples of mean + b_s + c_s + u_s . v_s, to the
    bars of tests/test_gpu_topn.py (rtol 1e-12 on the means, rtol 1e-12 / atol 1e-12 on the deviations)."""
    import bpmf_amd
    nq, nc, S, mean = 70, 130, 5, 3.25
    eng = bpmf_amd.HipEngine(K)
    try:
        q, c, Uq, Vc, bq, bc = _ring_pair(eng, K, nq, nc, S, 600 + K)
        P = mean + np.einsum("sqk,sck->sqc", Uq.astype(LD), Vc.astype(LD)) + bq.astype(LD)[:, :, None] + bc.astype(LD)[:, None, :]
        full = P.mean(0)
        sd = np.sqrt(((P - full) ** 2).sum(0) / (S - 1))
        m, s = eng.predict_block(q, c, mean)
        np.testing.assert_allclose(m, full.astype(np.float64), rtol=1e-12, atol=0)
        np.testing.assert_allclose(s, sd.astype(np.float64), rtol=1e-12, atol=1e-12)
        idx, tm, ts = eng.topn(q, c, mean, 10, exclude_rated=False)
        rows = np.arange(nq)[:, None]
        np.testing.assert_allclose(tm, full.astype(np.float64)[rows, idx], rtol=1e-12, atol=0)
        np.testing.assert_allclose(ts, sd.astype(np.float64)[rows, idx], rtol=1e-12, atol=1e-12)
        srt = -np.sort(-full.astype(np.float64), axis=1)
        for u in range(nq):
            if abs(srt[u, 9] - srt[u, 10]) > 1e-12 * abs(srt[u, 9]):
                assert set(idx[u]) == set(np.argsort(-full[u].astype(np.float64))[:10])
        cq, cc = np.random.default_rng(1).integers(0, nq, 300).astype(np.int32), np.random.default_rng(2).integers(0, nc, 300).astype(np.int32)
        out = eng.predict_cells(q, c, mean, cq, cc)
        np.testing.assert_allclose(out[0], full.astype(np.float64)[cq, cc], rtol=1e-12, atol=0)
        np.testing.assert_allclose(out[1], sd.astype(np.float64)[cq, cc], rtol=1e-12, atol=1e-12)
    finally:
        eng.close()


def test_ring_pairs_that_are_refused():
    import bpmf_amd
    from bpmf_amd import BpmfHipError
    eng = bpmf_amd.HipEngine(32)
    try:
        calls = (lambda q, c: eng.topn(q, c, 0.0, 3, exclude_rated=False), lambda q, c: eng.predict_block(q, c, 0.0),
                 lambda q, c: eng.predict_cells(q, c, 0.0, np.zeros(1, np.int32), np.zeros(1, np.int32)),
                 lambda q, c: eng.topn_scored(q, c, 0.0, 3, "ucb", 1.0, exclude_rated=False),
                 lambda q, c: eng.rank_eval(q, c, np.zeros(21, np.int64), np.zeros(0, np.int32), exclude_rated=False))
        q, c = _ring_pair(eng, 32, 20, 30, 2, 1, roles=(0, 0))[:2]
        for f in calls:
            with pytest.raises(BpmfHipError, match="the same bias role 0") as e:
                f(q, c)
            assert e.value.code == EINVAL
        q, c = _ring_pair(eng, 32, 20, 30, 2, 2, bias=(True, False))[:2]          # 36 rows per sample against 32
        for f in calls:
            with pytest.raises(BpmfHipError, match="36 and 32 rows per sample") as e:
                f(q, c)
            assert e.value.code == EINVAL
        with pytest.raises(BpmfHipError, match="not on a side with bias terms"):
            eng.similar(q, 3)
        with pytest.raises(BpmfHipError, match="not on a side with bias terms"):
            eng.samples_get(q)
    finally:
        eng.close()
    eng = bpmf_amd.HipEngine(30)                                                  # 32 rows on both sides, biases on one
    try:
        q, c = _ring_pair(eng, 30, 20, 30, 2, 3, bias=(True, False))[:2]
        with pytest.raises(BpmfHipError, match="both sides of a pair carry bias terms or neither"):
            eng.predict_block(q, c, 0.0)
    finally:
        eng.close()
    eng = bpmf_amd.HipEngine(127)
    try:
        s = _empty_side(eng, 5, 5, 0.0)
        eng.set_bias(s, 1.0, 13, 0)
        with pytest.raises(BpmfHipError, match="num_latent 127 > 126") as e:
            eng.samples_reserve(s, 2)
        assert e.value.code == EINVAL
    finally:
        eng.close()


# ---- 5. k_predict_bias ------------------------------------------------------------------------------------------------------------------

def _predict_reference(vals, col, row, factors, mean, bcol, brow):
    """tests/test_gpu_posterior_outputs.predict_reference with pred = u . v + mean + b[col] + c[row]"""
    v = vals.astype(LD)
    avg = v.copy(); m2 = v.copy()
    out = []
    for (V, U), n in zip(factors, NS):
        pred = (V[col].astype(LD) * U[row].astype(LD)).sum(1) + LD(mean) + bcol[col].astype(LD) + brow[row].astype(LD)
        if n == 0:
            avg = pred.copy(); m2 = np.zeros_like(pred)
        else:
            delta = pred - avg
            avg = avg + delta / LD(n)
            m2 = m2 + delta * (pred - avg)
        out.append((((v - pred) ** 2).sum(), ((v - avg) ** 2).sum(), avg.copy(), m2.copy()))
    return out


def _run_predict(eng, T, factors, twin, biases):
    """The five calls of the posterior-outputs tests on fresh sides; biases = (b of the movies, c of the users) or None: plain sides"""
    movies, users = _empty_side(eng, PN, PN, MEAN_M), _empty_side(eng, PN, PN, MEAN_U)
    if biases is not None:
        eng.set_bias(movies, 1.0, 13, 0); eng.set_bias(users, 1.0, 14, 1)
        eng.bias_set(movies, biases[0]); eng.bias_set(users, biases[1])
    t = eng.test_create(movies, *T)
    tw = None
    if twin is not None:
        tw = eng.test_create(users, *twin)
        eng.test_set_twin(t, tw)
    out, out_tw = [], []
    for (V, U), n in zip(factors, NS):
        eng.set_items(movies, V); eng.set_items(users, U)
        out.append(eng.predict(t, movies, users, n) + eng.test_get(t))
        if tw is not None:
            out_tw.append(eng.predict_finish(tw) + eng.test_get(tw))
    if tw is not None:
        eng.test_destroy(tw)
    eng.test_destroy(t)
    eng.side_destroy(movies); eng.side_destroy(users)
    return out, out_tw


@pytest.mark.parametrize("with_twin", [False, True])
@pytest.mark.parametrize("nnz", [0, 1, 255, 256, 257])
def test_predict_bias_against_longdouble(hip_engine_factory, monkeypatch, nnz, with_twin):
    monkeypatch.delenv("BPMF_HIP_PREDICT_WG", raising=False)
    K = 32
    eng = hip_engine_factory(K)
    T, col = predict_matrix(nnz)
    twin, order = transpose_matrix(T, col) if with_twin and nnz else (None, None)
    F = predict_factors(K)
    rng = np.random.default_rng(90 + nnz)
    bm, bu = 0.8 * rng.standard_normal(PN), 0.8 * rng.standard_normal(PN)
    a, atw = _run_predict(eng, T, F, twin, (bm, bu))
    _check_predict("k_predict_bias<32,256> nnz=%d twin=%s" % (nnz, with_twin), a, _predict_reference(T[2], col, T[1], F, MEAN_M, bm, bu) if nnz else None, nnz)
    if twin is not None:
        _check_predict("k_predict_bias<32,256> the twin nnz=%d" % nnz, atw,
                       _predict_reference(T[2][order], col[order], T[1][order], F, MEAN_U, bm, bu), nnz)
    # b = c = 0: the bytes of k_predict
    zero, zero_tw = _run_predict(eng, T, F, twin, (np.zeros(PN), np.zeros(PN)))
    plain, plain_tw = _run_predict(eng, T, F, twin, None)
    for x, y in list(zip(zero, plain)) + list(zip(zero_tw, plain_tw)):
        assert x[:3] == y[:3] and _same_bytes(x[3], y[3]) and _same_bytes(x[4], y[4])


def test_predict_bias_single_wave_workgroups(hip_engine_factory, monkeypatch):
    monkeypatch.setenv("BPMF_HIP_PREDICT_WG", "64")
    K, nnz = 32, 257
    eng = hip_engine_factory(K)
    T, col = predict_matrix(nnz)
    F = predict_factors(K)
    rng = np.random.default_rng(91)
    bm, bu = 0.8 * rng.standard_normal(PN), 0.8 * rng.standard_normal(PN)
    a, _ = _run_predict(eng, T, F, None, (bm, bu))
    _check_predict("k_predict_bias<32,64> nnz=%d" % nnz, a, _predict_reference(T[2], col, T[1], F, MEAN_M, bm, bu), nnz)


# ---- 6. one half-iteration per sampler family ---------------------------------------------------------------------------------------

def _half_iteration(oracle, eng, K, A, nrows, X, Y, it, tol, stat_tol, expect_kernel):
    ncols, mean = len(A[0]) - 1, util.mean_rating(A)
    c = np.random.default_rng(K + it).standard_normal(nrows)
    me, ot = _pair(eng, A, nrows, X, Y, c)
    assert re.search(expect_kernel, eng.kernel_name(me)), eng.kernel_name(me)
    info = eng.schedule_info(me)
    z = ref.values(A, ref.step(A, X, Y, c, it, ref.TAG_MOVIES, ALPHA, LAM, mean, np.float64)["b"], c)
    mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, it)
    want = X.copy()
    s_ref, p_ref, n_ref = oracle.sample_side(K, (A[0], A[1], z), mean, ALPHA, Y, want, it, mu, LF, nthreads=NT)
    s, p, n = eng.sample_side(me, ot, it, ALPHA, mu, LF)
    items = eng.get_items(me)
    zg = eng.bias_latent(me)
    eng.side_destroy(me); eng.side_destroy(ot)
    assert np.all(np.isfinite(items))
    err = rel_err(items, want)
    print("K %d: factors %.3g, z %.3g" % (K, err, np.abs(zg - z).max()))
    assert err < tol, err
    assert rel_err(s, s_ref) < stat_tol and rel_err(p, p_ref) < stat_tol and abs(n - n_ref) <= stat_tol * abs(n_ref)
    return info


@pytest.mark.parametrize("mode", [1, 3])
def test_half_iteration_k8(oracle, mode):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    with _env(BPMF_HIP_MODE=mode):
        eng = bpmf_amd.HipEngine(8)
        try:
            rng = np.random.default_rng(80 + mode)
            _half_iteration(oracle, eng, 8, M, nu, 0.7 * rng.standard_normal((nm, 8)), 0.7 * rng.standard_normal((nu, 8)), 3, RTOL, 1e-8,
                            {1: r"k_sample1i", 3: r"k_sample4"}[mode])
        finally:
            eng.close()


@pytest.mark.parametrize("K", [10, 32, 64, 100, 128])
def test_half_iteration_families(oracle, K):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    rng = np.random.default_rng(800 + K)
    sigma = (2.0 / K) ** 0.25
    with _env(**({"BPMF_HIP_CHUNK": 16} if K == 64 else {})):
        eng = bpmf_amd.HipEngine(K)
        try:
            if K == 64:                                              # product-form columns + a chunked heavy column in the slab launch
                A, nrows = _product_form_side(rng)
                ncols = len(A[0]) - 1
                info = _half_iteration(oracle, eng, K, A, nrows, sigma * rng.standard_normal((ncols, K)), sigma * rng.standard_normal((nrows, K)),
                                       4, RTOL, 1e-8, r"k_sample_pf")
                assert info["pf_le3"] > 0 and info["pf_4to6"] > 0 and info["pf_7to16"] > 0 and info["other_items"] > 0, info
            else:
                V, U = sigma * rng.standard_normal((nm, K)), sigma * rng.standard_normal((nu, K))
                _half_iteration(oracle, eng, K, M, nu, V, U, 4, RTOL, 1e-8, r"k_sample_wg2" if K > 64 else r"k_sample")
        finally:
            eng.close()


# ---- 7. chains against the CPU restatement ------------------------------------------------------------------------------------------

CHAIN = dict(nsims=20, burnin=8, alpha=1.5)


@pytest.mark.parametrize("K", [32, 64])
def test_bias_chain_against_cpu(K):
    import bpmf_amd
    from oracle.oracle import Oracle
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want = ref.restate_chain(Oracle(), K, M, Mt, T, LAM, CHAIN["nsims"], CHAIN["burnin"], CHAIN["alpha"])
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, bias=LAM, **CHAIN)
    finally:
        eng.close()
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(res["U"] - want["U"]).max() / scale, np.abs(res["V"] - want["V"]).max() / scale
    et = max(np.abs(np.array(res["rmse"]) - want["rmse"]).max(), np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max())
    ef = abs(res["final_rmse_avg"] - want["final_rmse_avg"])
    eb = max(np.abs(res["bias"]["cols_mean"] - want["bm_mean"]).max(), np.abs(res["bias"]["rows_mean"] - want["bu_mean"]).max())
    print("K %d: U %.3g V %.3g traces %.3g final %.3g bias means %.3g" % (K, eu, ev, et, ef, eb))
    assert eu < 1e-6 and ev < 1e-6 and et < 1e-6 and ef < 1e-6 and eb < 1e-6, (K, eu, ev, et, ef, eb)
    assert res["bias"]["kept"] == CHAIN["nsims"] - CHAIN["burnin"]
    assert res["bias"]["lambda_rows"].shape == (CHAIN["nsims"],) and np.all(res["bias"]["lambda_rows"] == LAM) and np.all(res["bias"]["lambda_cols"] == LAM)
    assert res["bias"]["rows_mean"].shape == (nu,) and res["bias"]["cols_mean"].shape == (nm,)


# ---- 8. the plain paths are untouched ---------------------------------------------------------------------------------------------------

def test_plain_runs_are_what_they_were():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = bpmf_amd.HipEngine(32)
    try:
        side = eng.side_create(nm, nu, *M, util.mean_rating(M))
        name = eng.kernel_name(side)
        a = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=4, burnin=1, Tt=Tt, alpha=1.7)
        bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=1, Tt=Tt, alpha=1.7, bias=True)
        b = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=4, burnin=1, Tt=Tt, alpha=1.7)
        biased = eng.side_create(nm, nu, *M, util.mean_rating(M))
        eng.set_bias(biased, 1.0, 13, 0)
        assert eng.kernel_name(side) == name and not re.search(r"k_sample1i", name) and re.search(r"k_sample1i", eng.kernel_name(biased))
    finally:
        eng.close()
    assert "bias" not in a and a["U"].tobytes() == b["U"].tobytes() and a["V"].tobytes() == b["V"].tobytes()
    assert a["rmse"] == b["rmse"] and a["rmse_avg"] == b["rmse_avg"] and a["norm_u"] == b["norm_u"]


# ---- 9. refusals and the failure word -------------------------------------------------------------------------------------------------

def test_refusals_and_the_failure_word():
    import ctypes as C
    import bpmf_amd
    from bpmf_amd import BpmfHipError
    K = 32
    M, Mt, T, Tt, nu, nm = util.ml100k()
    rng = np.random.default_rng(4)
    V, U = 0.4 * rng.standard_normal((nm, K)), 0.4 * rng.standard_normal((nu, K))
    mean, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    mu, LU, LF = _hyper(K, nm, 2, 5)
    eng = bpmf_amd.HipEngine(K)
    try:
        me, ot = _pair(eng, M, nu, V, U, np.zeros(nu))
        eng.sample_side(me, ot, 2, ALPHA, mu, LF)
        good = eng.bias_get(me)
        # a NaN factor row: the residuals of its ratings are not finite -> BPMF_HIP_ENUM naming one of them; the next healthy launch succeeds
        col = int(np.argmax(np.diff(M[0])))
        bad = V.copy(); bad[col] = np.nan
        eng.set_items(me, bad)
        with pytest.raises(BpmfHipError, match=r"bias: the residual of rating (\d+) is not finite") as e:
            eng.sample_side(me, ot, 3, ALPHA, mu, LF)
        assert e.value.code == ENUM
        p = int(re.search(r"rating (\d+)", str(e.value)).group(1))
        assert M[0][col] <= p < M[0][col + 1]
        eng.set_items(me, V)
        eng.sample_side(me, ot, 2, ALPHA, mu, LF)
        assert eng.bias_get(me).tobytes() == good.tobytes()

        lib = eng.lib

        def raw(side, lam, tag, role):
            bpmf_amd._lib.check(lib.bpmf_hip_side_set_bias(side.handle if side is not None else None, lam, tag, role))
        plain = eng.side_create(nm, nu, *M, mean)
        for args, msg in (((None, 1.0, 13, 0), "NULL"), ((plain, 0.0, 13, 0), "not finite and > 0"), ((plain, float("nan"), 13, 0), "not finite and > 0"),
                          ((plain, float("inf"), 13, 0), "not finite and > 0"), ((plain, 1.0, 0, 0), "tag must be >= 1"), ((plain, 1.0, 13, 2), "role must be 0 or 1"),
                          ((me, 1.0, 13, 0), "bias terms already")):
            with pytest.raises(BpmfHipError, match=msg) as e:
                raw(*args)
            assert e.value.code == EINVAL
        # a side that is something else already
        def fresh(m=mean):
            return eng.side_create(nm, nu, *M, m)
        s = fresh(0.0); eng.set_probit(s, 3.0, 1)
        with pytest.raises(BpmfHipError, match="side_set_bias: not on a probit side"):
            eng.set_bias(s)
        s = fresh(0.0); eng.set_ordinal(s, np.arange(1.0, 6.0))
        with pytest.raises(BpmfHipError, match="side_set_bias: not on an ordinal side"):
            eng.set_bias(s)
        s = fresh(); eng.set_censored(s, np.zeros(len(M[2]), np.int8), 5)
        with pytest.raises(BpmfHipError, match="side_set_bias: not on a censored side"):
            eng.set_bias(s)
        s = fresh(); eng.set_weights(s, np.full(len(M[2]), 2.0))
        with pytest.raises(BpmfHipError, match="side_set_bias: not on a side with per-rating weights"):
            eng.set_bias(s)
        s = fresh(); eng.set_robust(s, 4.0, 9)
        with pytest.raises(BpmfHipError, match="side_set_bias: not on a side with Student-t noise"):
            eng.set_bias(s)
        s = fresh(0.0); eng.set_implicit(s, 0.1, np.full(len(M[2]), 2.0))
        with pytest.raises(BpmfHipError, match="side_set_bias: not on an implicit side"):
            eng.set_bias(s)
        tns = eng.tensor_create(np.array([[0, 1, 2], [1, 0, 1], [2, 2, 0]]), np.array([1.0, 2.0, 3.0]), (3, 3, 3), 2.0)
        with pytest.raises(BpmfHipError, match="side_set_bias: not on a mode of a tensor") as e:
            eng.set_bias(tns.sides[1])
        assert e.value.code == EINVAL
        s = fresh(); eng.set_features(s, rng.standard_normal((nm, 3)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="side_set_bias: not together with features"):
            eng.set_bias(s)
        s = fresh(); eng.set_prop_posterior(s, np.tile(np.eye(K).ravel(), (nm, 1)))
        with pytest.raises(BpmfHipError, match="side_set_bias: not together with propagated priors"):
            eng.set_bias(s)
        s = fresh(); eng.samples_reserve(s, 2)
        with pytest.raises(BpmfHipError, match="side_set_bias: not on a side with a sample ring"):
            eng.set_bias(s)
        s = fresh(); eng.hyper_reserve(s, 2)
        with pytest.raises(BpmfHipError, match="side_set_bias: not together with fold-in"):
            eng.set_bias(s)
        part = eng.side_create(nm, nu, M[0][:11] - M[0][0], M[1][:M[0][10]], M[2][:M[0][10]], mean, 0, 10)
        with pytest.raises(BpmfHipError, match="whole"):
            eng.set_bias(part)
        ru, rm = eng.side_create(nu, nm, *Mt, mean_u), fresh()
        eng.sys_set_reduce(rm, ru)
        with pytest.raises(BpmfHipError, match="BPMF_REDUCE"):
            eng.set_bias(rm)
        # ... and the other add-ons refuse a side with biases
        side_msg = "not on a side with bias terms"
        for call in (lambda: eng.set_probit(me, 3.0, 1), lambda: eng.set_ordinal(me, np.arange(1.0, 6.0)),
                     lambda: eng.set_censored(me, np.zeros(len(M[2]), np.int8), 5), lambda: eng.set_weights(me, np.full(len(M[2]), 2.0)),
                     lambda: eng.set_robust(me, 4.0, 9), lambda: eng.set_implicit(me, 0.1, np.full(len(M[2]), 2.0)),
                     lambda: eng.set_features(me, rng.standard_normal((nm, 3)), 5.0, 3),
                     lambda: eng.set_prop_posterior(me, np.tile(np.eye(K).ravel(), (nm, 1))),
                     lambda: eng.hyper_reserve(me, 2)):
            with pytest.raises(BpmfHipError, match=side_msg) as e:
                call()
            assert e.value.code == EINVAL
        cu = eng.side_create(nu, nm, *Mt, mean_u)
        with pytest.raises(BpmfHipError, match="train_sse: not with a side with bias terms"):
            eng.train_sse(me, cu)
        with pytest.raises(BpmfHipError, match="sys_set_reduce: not together with bias terms"):
            eng.sys_set_reduce(me, cu)
        # both sides of a pair or neither: the half-iteration either way round, and the evaluation
        eng.set_items(cu, U)
        with pytest.raises(BpmfHipError, match="both sides of a pair carry bias terms or neither") as e:
            eng.sample_side(me, cu, 3, ALPHA, mu, LF)
        assert e.value.code == EINVAL
        mu_u, _, LF_u = _hyper(K, nu, 2, 6)
        with pytest.raises(BpmfHipError, match="both sides of a pair carry bias terms or neither"):
            eng.sample_side(cu, me, 3, ALPHA, mu_u, LF_u)
        t = eng.test_create(me, *T)
        with pytest.raises(BpmfHipError, match="both sides of a pair carry bias terms or neither"):
            eng.predict(t, me, cu, 0)
        with pytest.raises(BpmfHipError, match="alpha > 0"):
            eng.sample_side(me, ot, 3, 0.0, mu, LF)
        for f in (eng.bias_get, eng.bias_latent, eng.bias_add, eng.bias_mean, eng.bias_lambda, lambda s: eng.bias_set(s, np.zeros(nm))):
            with pytest.raises(BpmfHipError, match="not a side with bias terms"):
                f(plain)
        with pytest.raises(BpmfHipError, match="nothing added"):
            eng.bias_mean(me)
        with pytest.raises(BpmfHipError, match="is not finite"):
            eng.bias_set(me, np.full(nm, np.nan))
        with pytest.raises(ValueError, match="values for a side of"):
            eng.bias_set(me, np.zeros(nm - 1))
    finally:
        eng.close()
    eng = bpmf_amd.HipEngine(128, dtype="f32")
    try:
        with pytest.raises(BpmfHipError, match="not on an fp32 context"):
            eng.set_bias(eng.side_create(nm, nu, *M, mean))
    finally:
        eng.close()


GIBBS_REFUSALS = [(dict(pipelined=True), "pipelined=True"), (dict(probit=True), "probit=True"), (dict(ordinal=True), "ordinal"),
                  (dict(censored=(np.zeros(1, np.int64),) * 3), "censored"), (dict(robust=4.0), "robust"), (dict(weights=()), "weights"),
                  (dict(implicit=0.1), "implicit"), (dict(row_features=np.zeros((1, 1))), "row_features / col_features"),
                  (dict(col_features=np.zeros((1, 1))), "row_features / col_features"), (dict(noise="adaptive"), "noise='adaptive'"),
                  (dict(foldin=True), "foldin=True"), (dict(save_model="x"), "save_model"), (dict(similar=3), "similar"),
                  (dict(new_row_features=np.zeros((1, 1))), "new_row_features / new_col_features")]


def test_gibbs_refusals():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = bpmf_amd.HipEngine(8)
    try:
        for kw, what in GIBBS_REFUSALS:
            with pytest.raises(ValueError, match="bias does not go together with %s" % re.escape(what)):
                bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=3, burnin=1, bias=True, **kw)
        for v in (0.0, -1.0, float("nan"), "x"):
            with pytest.raises(ValueError, match="a finite lambda > 0"):
                bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=3, burnin=1, bias=v)
        with pytest.raises(ValueError, match="bias_prior needs bias"):
            bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=3, burnin=1, bias_prior=(1.0, 1.0))
        for bad in ((0.0, 1.0), (1.0, -1.0), (1.0,), "x", (float("inf"), 1.0)):
            with pytest.raises(ValueError, match="bias_prior"):
                bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=3, burnin=1, bias=True, bias_prior=bad)
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=3, burnin=1, bias=np.float32(1.0), topn=2)
        assert res["bias"]["kept"] == 2 and np.all(res["bias"]["lambda_rows"] == 1.0) and np.all(np.isfinite(res["bias"]["rows_mean"]))
        assert res["topn"][0].shape == (nu, 2)
    finally:
        eng.close()
    eng = bpmf_amd.HipEngine(128, dtype="f32")
    try:
        with pytest.raises(ValueError, match="bias does not go together with an fp32 engine"):
            bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=3, burnin=1, bias=True)
    finally:
        eng.close()


def _cli(tmp_path, args, env=None):
    import os
    import subprocess
    from tests.conftest import ROOT
    return subprocess.run([os.path.join(ROOT, "bpmf_amd", "bpmf")] + [str(a) for a in args], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, **(env or {})))


def _cli_lines(out, want, nsims):
    assert out.returncode == 0, out.stderr
    lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", out.stdout)
    got = np.array([[float(a), float(b)] for a, b in lines])
    assert got.shape == (nsims, 2)
    # (four printed decimals, six significant digits in the final line: the 1e-6 of the chain tests on top of half a unit of the print)
    assert np.abs(got[:, 0] - want["rmse"]).max() <= 1e-6 + 5e-5 and np.abs(got[:, 1] - want["rmse_avg"]).max() <= 1e-6 + 5e-5
    final = re.search(r"^Final Avg RMSE: (\S+)$", out.stdout, re.M)
    assert final and abs(float(final.group(1)) - want["final_rmse_avg"]) <= 1e-6 + 5e-6


def test_cli_bias_end_to_end(tmp_path, oracle):
    import os
    from bpmf_amd import io as bio
    M, Mt, T, Tt, nu, nm = util.tiny()
    K, nsims, burnin = 8, 6, 2
    want = ref.restate_chain(oracle, K, M, Mt, T, 2.5, nsims, burnin, 3.0)
    files = ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx"), "-a", 3, "-i", nsims, "-b", burnin, "-d", K]
    (tmp_path / "o").mkdir(); (tmp_path / "p").mkdir()
    plain = _cli(tmp_path, files + ["-o", "p/"])
    runs = [_cli(tmp_path, files + ["--bias", "--bias-lambda", 2.5, "-o", "o/"]), _cli(tmp_path, files + ["--bias", "--bias-lambda", 2.5])]
    for out in runs:
        _cli_lines(out, want, nsims)
        assert re.search(r"^bias: row and column offsets, lambda 2\.5 fixed$", out.stdout, re.M), out.stdout
    assert re.search(r"^bias: row and column offsets, lambda 1 fixed$", _cli(tmp_path, files + ["--bias"]).stdout, re.M)
    rows, cols = bio.read_dense(tmp_path / "o" / "row-bias.ddm"), bio.read_dense(tmp_path / "o" / "col-bias.ddm")
    assert rows.shape == (1, nu) and cols.shape == (1, nm)
    assert np.abs(rows[0] - want["bu_mean"]).max() < 1e-6 and np.abs(cols[0] - want["bm_mean"]).max() < 1e-6
    csv = (tmp_path / "o" / "bias_lambda.csv").read_text().splitlines()
    assert csv[0] == "iteration,lambda_rows,lambda_cols" and csv[1:] == ["%d,2.5,2.5" % i for i in range(nsims)]
    for name in ("U-mu.ddm", "V-mu.ddm", "Pavg.sdm", "Pm2.sdm"):
        assert (tmp_path / "o" / name).exists()
    # without the flag: no header line, none of the three files, and not the lines of the bias chain
    assert plain.returncode == 0 and "bias" not in plain.stdout
    assert not [p.name for p in (tmp_path / "p").iterdir() if "bias" in p.name]
    assert re.findall(r"RMSE: \S+\tavg RMSE: \S+", plain.stdout) != re.findall(r"RMSE: \S+\tavg RMSE: \S+", runs[0].stdout)


def test_cli_bias_topn_is_engine_topn_over_the_widened_rings(tmp_path):
    """bpmf --bias --bias-prior --topn --rank-eval against gibbs(bias=, bias_prior=, topn=, rank_eval=): the same chain, the same lists"""
    import os
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    K, nsims, burnin, n = 16, 6, 2, 5
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, nsims=nsims, burnin=burnin, alpha=2.0, bias=1.5, bias_prior=(2.0, 1.0), topn=n, rank_eval=n)
    finally:
        eng.close()
    (tmp_path / "o").mkdir()
    out = _cli(tmp_path, ["-i", nsims, "-b", burnin, "-d", K, "-a", 2, "-o", "o/", "-n", os.path.join(util.GOLDEN, "ml100k-train.mtx.gz"),
                          "-p", os.path.join(util.GOLDEN, "ml100k-test.mtx.gz"), "--bias", "--bias-lambda", 1.5, "--bias-prior", "2,1", "--topn", n,
                          "--rank-eval", n])
    assert out.returncode == 0, out.stderr
    assert re.search(r"^bias: row and column offsets, lambda 1\.5 sampled \(2, 1\)$", out.stdout, re.M), out.stdout
    lines = (tmp_path / "o" / "topn.csv").read_text().splitlines()
    assert lines[0] == "query,rank,candidate,mean,std"
    rec = np.array([l.split(",") for l in lines[1:]], dtype=float)
    idx, mean, std = res["topn"]
    assert rec.shape == (nu * n, 5) and np.array_equal(rec[:, 2].astype(int).reshape(nu, n) - 1, idx)
    np.testing.assert_allclose(rec[:, 3].reshape(nu, n), mean, rtol=1e-12, atol=0)
    np.testing.assert_allclose(rec[:, 4].reshape(nu, n), std, rtol=1e-9, atol=1e-12)
    # the lists are ranked with the biases: the ring means are the samples' mean + b + c + u . v, not mean + u . v
    assert np.abs(res["bias"]["cols_mean"]).max() > 0.1
    csv = np.array([l.split(",") for l in (tmp_path / "o" / "bias_lambda.csv").read_text().splitlines()[1:]], dtype=float)
    assert csv.shape == (nsims, 3)
    np.testing.assert_allclose(csv[:, 1], res["bias"]["lambda_rows"], rtol=1e-12)
    np.testing.assert_allclose(csv[:, 2], res["bias"]["lambda_cols"], rtol=1e-12)
    assert csv[0, 1] == 1.5 and len(set(csv[:, 1])) == nsims
    final = re.search(r"^Final Avg RMSE: (\S+)$", out.stdout, re.M)
    assert final and abs(float(final.group(1)) - res["final_rmse_avg"]) <= 5e-6


def test_cli_bias_files_follow_the_renumbering(tmp_path, oracle):
    """BPMF_TEST_ASSIGN_PARTS=3 renumbers rows and columns as for three ranks: the chain is the restated chain on the renumbered
    ratings, and row-bias.ddm / col-bias.ddm come back in the numbering of the input."""
    import os
    import scipy.sparse as sp
    from bpmf_amd import io as bio
    from tests.test_assign import greedy
    K, parts, nsims, burnin = 8, 3, 6, 2
    M, Mt, T, Tt, nu, nm = util.ml100k()
    pm, pu = np.arange(nm), np.arange(nu)
    for _ in range(2):
        for side in (0, 1):
            perm, csc = (pm, M) if side == 0 else (pu, Mt)
            order, _ = greedy(np.concatenate([[0], np.cumsum(np.diff(csc[0])[perm])]), parts)
            if side == 0:
                pm = perm[order]
            else:
                pu = perm[order]
    renum = lambda X: util.csc_arrays(sp.csc_matrix((X[2], X[1], X[0]), shape=(nu, nm))[pu][:, pm].tocsc())
    Mp, Tp = renum(M), renum(T)
    Mpt = util.csc_arrays(sp.csc_matrix((Mp[2], Mp[1], Mp[0]), shape=(nu, nm)).T)
    want = ref.restate_chain(oracle, K, Mp, Mpt, Tp, 1.0, nsims, burnin, 2.0)
    (tmp_path / "o").mkdir()
    out = _cli(tmp_path, ["-i", nsims, "-b", burnin, "-d", K, "-a", 2, "-o", "o/", "-n", os.path.join(util.GOLDEN, "ml100k-train.mtx.gz"),
                          "-p", os.path.join(util.GOLDEN, "ml100k-test.mtx.gz"), "--bias"], {"BPMF_TEST_ASSIGN_PARTS": str(parts)})
    _cli_lines(out, want, nsims)
    assert "assignment: greedy" in out.stdout
    rows, cols = bio.read_dense(tmp_path / "o" / "row-bias.ddm")[0], bio.read_dense(tmp_path / "o" / "col-bias.ddm")[0]
    eu, em = np.abs(rows[pu] - want["bu_mean"]).max(), np.abs(cols[pm] - want["bm_mean"]).max()
    print("renumbered: row biases %.3g, column biases %.3g; spread of the row biases %.3g" % (eu, em, want["bu_mean"].std()))
    assert eu < 1e-6 and em < 1e-6 and want["bu_mean"].std() > 0.1 and not np.array_equal(pu, np.arange(nu))


# ---- 10. the planted experiment -----------------------------------------------------------------------------------------------------------

def test_planted_biases_match_the_recorded_chains():
    import bpmf_amd
    P, rec = ref.PLANTED, ref.planted_recorded()
    assert rec["spread"] == P["spread"]
    M, Mt, T, Tt = ref.planted_data(**P)
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        got = [bpmf_amd.gibbs(eng, M, Mt, T, P["nusers"], P["nmovies"], Tt=Tt, nsims=P["nsims"], burnin=P["burnin"], alpha=P["alpha"], **kw)["final_rmse_avg"]
               for kw in (dict(bias=P["lam"]), dict())]
    finally:
        eng.close()
    print("planted: with biases %.9g (recorded %.9g), plain %.9g (recorded %.9g)" % (got[0], rec["rmse_bias"], got[1], rec["rmse_plain"]))
    assert abs(got[0] - rec["rmse_bias"]) < 1e-6 and abs(got[1] - rec["rmse_plain"]) < 1e-6
    assert got[0] < got[1]
