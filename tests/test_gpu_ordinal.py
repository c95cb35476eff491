"""Ordinal probit likelihood with sampled cutpoints (`gibbs(..., ordinal=True)`, `bpmf --ordinal`) on the GPU.

  * k_ordinal_latent against the CPU restatement of tests/ordinal_ref.py, every rating: nnz = 0, 1, 255, 256, 257, 4 097; K = 8, 10
    (padded), 32, 64, 128 fp64 and 128 fp32; C = 2, 5, 16; a level absent from training; columns without ratings; bit-identical
    between two launches
  * k_ordinal_loglik: both sums against the restatement's long-double sums, bit-identical between calls, equal words for g' = g
  * k_ordinal_prob: rows sum to 1, against the restatement at 0, 1 and 257 test entries
  * one half-iteration through each sampler family with the latent scores in place of the ratings, against oracle.sample_side
  * the chain with sampled cutpoints (plain and pipelined loop) against the restated chain: factors, traces, probabilities, the
    accept sequence and the cutpoint trace; fixed cutpoints enqueue no log-likelihood pass
  * factors scaled until |m| passes 37: the far-tail forms of the draw and of the mass; a NaN factor row raises BPMF_HIP_ENUM
  * the library's count of host waits for the main stream: fixed cutpoints wait as often as probit, sampled ones once more per iteration
  * refusals (a tensor mode and a context with a communicator included), device memory, `bpmf --ordinal` end to end, and a guard
    that an ordinal run leaves nothing behind in the fixed path

tests/test_ordinal_host.py asserts on the CPU that no decision of the cutpoint step is marginal for the inputs used here.
"""
import csv
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ordinal_ref as ref
from tests import util
from tests.conftest import ROOT
from tests.test_gpu_parity import RTOL, rel_err

pytestmark = pytest.mark.gpu

NT = ref.NT


def _hyper(K, ncols, it, seed):
    import bpmf_amd
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, 3 * K))
    return bpmf_amd.engine.hyper_sample(K, ncols, A @ A.T / (3 * K), it)


def _pair(eng, A, nrows, X, Y, levels, cut, tag):
    """An ordinal side over the ratings A holding the factors X, and a partner without ratings holding Y."""
    ncols = len(A[0]) - 1
    me = eng.side_create(ncols, nrows, *A, 0.0)
    ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_ordinal(me, levels, cut, tag)
    eng.set_items(me, X)
    eng.set_items(ot, Y)
    return me, ot


def _scale(m, lev, cut):
    """1 + |m| + the finite ends of the rating's interval: what the latent bar is relative to"""
    g = ref.table(cut)
    lo, hi = g[lev], g[lev + 1]
    ends = np.maximum(np.where(np.isfinite(lo), np.abs(lo), 0.0), np.where(np.isfinite(hi), np.abs(hi), 0.0))
    return 1.0 + np.abs(m) + ends


@pytest.mark.parametrize("K,dtype", ref.KERNEL_CASES)
def test_latent_and_loglik_against_restatement(K, dtype):
    import bpmf_amd
    it = ref.KERNEL_ITER
    worst_z = worst_l = 0.0
    eng = bpmf_amd.HipEngine(K, dtype=dtype)
    try:
        for C_, nnz, absent in [(C_, nnz, None) for C_ in (2, 5, 16) for nnz in ref.KERNEL_NNZ] + [(5, 257, 2), (16, 4097, 0)]:
            levels, cut = (np.asarray(v, np.float64) for v in ref.LEVEL_SETS[C_])
            M, Mt, nu, nm = ref.kernel_matrix(nnz, C_, absent=absent)
            U, V = ref.kernel_factors(K, dtype, nu, nm)
            rng = np.random.default_rng(nnz + C_)
            prop = np.sort(cut + 0.05 * rng.standard_normal(len(cut)))
            for A, nrows, X, Y, tag in ((M, nu, V, U, ref.TAG_MOVIES), (Mt, nm, U, V, ref.TAG_USERS)):
                ncols = len(A[0]) - 1
                assert len(A[2]) == nnz and (nnz < 256 or (np.diff(A[0]) == 0).any())
                me, ot = _pair(eng, A, nrows, X, Y, levels, cut, tag)
                assert np.array_equal(eng.get_items(me), X) and np.array_equal(eng.get_items(ot), Y)     # fp32: representable values
                assert np.array_equal(eng.ordinal_cut_get(me), cut) and np.array_equal(eng.ordinal_info(me)[0], levels)
                m, lev = ref.dots(A, X, Y), ref.level_index(A[2], levels)
                # the log-likelihood at the factors the side holds now
                l = [eng.ordinal_loglik(me, ot, prop) for _ in range(2)]
                want = (ref.loglik_from(m, lev, cut), ref.loglik_from(m, lev, prop))
                assert l[0] == l[1]                                       # the same bits
                for got, w in zip(l[0], want):
                    assert math.isfinite(got)
                    err = abs(got - w) / abs(w) if nnz else abs(got)
                    worst_l = max(worst_l, err)
                    assert err <= 1e-12, (K, dtype, C_, nnz, tag, got, w)
                same = eng.ordinal_loglik(me, ot, cut)
                assert same[0] == same[1] == l[0][0]
                assert eng.ordinal_info(me)[1] == 3
                # the latent step ahead of a sampler launch
                mu, LU, LF = _hyper(K, ncols, it, 70 + K)
                got = []
                for _ in range(2):
                    eng.set_items(me, X)
                    eng.sample_side(me, ot, it, 1.0, mu, LF)
                    got.append(eng.ordinal_latent(me, nnz))
                z, z_ref = got[0], ref.latent_from(m, lev, it, tag, cut)
                assert got[1].tobytes() == z.tobytes()
                g = ref.table(cut)
                assert np.all(np.isfinite(z)) and np.all(z >= g[lev]) and np.all(z <= g[lev + 1])
                if nnz:
                    err = np.abs(z - z_ref) / _scale(m, lev, cut)
                    worst_z = max(worst_z, float(err.max()))
                    assert err.max() <= 1e-12, (K, dtype, C_, nnz, tag, int(err.argmax()), float(err.max()))
                eng.side_destroy(me); eng.side_destroy(ot)
        print("K %d %s: worst latent error %.3g (of the bar's scale), worst log-likelihood error %.3g (relative)" % (K, dtype, worst_z, worst_l))
    finally:
        eng.close()


def test_far_tail_and_non_finite_scores():
    """Factors scaled until |m| passes 37 + |g| on both sides (tests/test_ordinal_host.py asserts that they do): the exponential form
    of the draw and the asymptotic series of the mass on the device, against the restatement at the bars of the other cases.  Then
    one factor row that is NaN: BPMF_HIP_ENUM from the launch that meets it, and the next healthy launch gives the bits of the first."""
    import bpmf_amd
    K, it = 8, ref.KERNEL_ITER
    levels, cut = (np.asarray(v, np.float64) for v in ref.LEVEL_SETS[5])
    M, Mt, nu, nm = ref.kernel_matrix(257, 5)
    U, V = ref.kernel_factors(K, "f64", nu, nm)
    U, V = ref.FAR_SCALE * U, ref.FAR_SCALE * V
    prop = cut + np.array([0.02, -0.01, 0.03, 0.01])
    eng = bpmf_amd.HipEngine(K)
    try:
        for A, nrows, X, Y, tag in ((M, nu, V, U, ref.TAG_MOVIES), (Mt, nm, U, V, ref.TAG_USERS)):
            ncols = len(A[0]) - 1
            me, ot = _pair(eng, A, nrows, X, Y, levels, cut, tag)
            m, lev = ref.dots(A, X, Y), ref.level_index(A[2], levels)
            assert np.abs(m).max() > 45
            got = eng.ordinal_loglik(me, ot, prop)
            for v, w in zip(got, (ref.loglik_from(m, lev, cut), ref.loglik_from(m, lev, prop))):
                assert math.isfinite(v) and abs(v - w) <= 1e-12 * abs(w), (tag, v, w)
            mu, LU, LF = _hyper(K, ncols, it, 70 + K)
            eng.sample_side(me, ot, it, 1.0, mu, LF)
            z = eng.ordinal_latent(me, len(m))
            g = ref.table(cut)
            assert np.all(np.isfinite(z)) and np.all(z >= g[lev]) and np.all(z <= g[lev + 1])
            err = np.abs(z - ref.latent_from(m, lev, it, tag, cut)) / _scale(m, lev, cut)
            print("tag %d: |m| <= %.1f, worst latent error %.3g (of the bar's scale)" % (tag, np.abs(m).max(), err.max()))
            assert err.max() <= 1e-12, (tag, int(err.argmax()), float(err.max()))
            # the level probabilities of the same entries, as a test matrix of this side
            test = eng.test_create(me, *A)
            eng.set_items(me, X)
            eng.ordinal_add(test, me, ot)
            prob, n = eng.ordinal_get(test)
            assert n == 1 and np.abs(prob.sum(axis=1) - 1.0).max() <= 1e-14
            assert np.abs(prob - ref.probs_from(m, cut)).max() <= 1e-12
            eng.test_destroy(test)
            # a NaN factor row of a column that has ratings
            col = int(np.argmax(np.diff(A[0])))
            bad = X.copy(); bad[col] = np.nan
            eng.set_items(me, bad)
            with pytest.raises(bpmf_amd.BpmfHipError, match="is not finite") as e:
                eng.sample_side(me, ot, it, 1.0, mu, LF)
            assert e.value.code == -5
            eng.set_items(me, X)
            eng.sample_side(me, ot, it, 1.0, mu, LF)
            assert eng.ordinal_latent(me, len(m)).tobytes() == z.tobytes()
            eng.side_destroy(me); eng.side_destroy(ot)
    finally:
        eng.close()


@pytest.mark.parametrize("K,dtype", [(10, "f64"), (32, "f64"), (128, "f32")])
def test_ordinal_add_against_restatement(K, dtype):
    import bpmf_amd
    S = 3
    eng = bpmf_amd.HipEngine(K, dtype=dtype)
    try:
        for C_ in (2, 5, 16):
            levels, cut = (np.asarray(v, np.float64) for v in ref.LEVEL_SETS[C_])
            M, Mt, nu, nm = ref.kernel_matrix(4097, C_)
            for ntest in (0, 1, 257):
                T = ref.kernel_matrix(ntest, C_, seed=99)[0]
                rng = np.random.default_rng(K + ntest)
                movies = eng.side_create(nm, nu, *M, 0.0)
                users = eng.side_create(nu, nm, *Mt, 0.0)
                eng.set_ordinal(movies, levels, cut, ref.TAG_MOVIES)
                test = eng.test_create(movies, *T)
                with pytest.raises(bpmf_amd.BpmfHipError, match="nothing added"):
                    eng.ordinal_get(test)
                acc = np.zeros((ntest, C_))
                sigma = (3.0 / K) ** 0.25
                for s in range(S):
                    eng.set_items(movies, sigma * rng.standard_normal((nm, K)))
                    eng.set_items(users, sigma * rng.standard_normal((nu, K)))
                    eng.ordinal_add(test, movies, users)
                    acc += ref.probs_from(ref.dots(T, eng.get_items(movies), eng.get_items(users)), cut)
                prob, n = eng.ordinal_get(test)
                assert n == S and prob.shape == (ntest, C_)
                if ntest:
                    assert prob.min() >= 0.0 and prob.max() <= 1.0
                    assert np.abs(prob.sum(axis=1) - 1.0).max() <= 1e-14
                    assert np.abs(prob - acc / S).max() <= 1e-12
                eng.test_destroy(test); eng.side_destroy(movies); eng.side_destroy(users)
    finally:
        eng.close()


def _half_iteration(oracle, eng, K, A, nrows, X, Y, it, tag, tol, stat_tol, expect_kernel):
    levels = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    cut = np.asarray(ref.LEVEL_SETS[5][1])
    ncols = len(A[0]) - 1
    me, ot = _pair(eng, A, nrows, X, Y, levels, cut, tag)
    assert re.search(expect_kernel, eng.kernel_name(me)), eng.kernel_name(me)
    info = eng.schedule_info(me)
    X, Y = eng.get_items(me), eng.get_items(ot)                      # (fp32: the stored values, widened)
    z = ref.latent(A, X, Y, it, tag, levels, cut)
    mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, it)
    want = X.copy()
    s_ref, p_ref, n_ref = oracle.sample_side(K, (A[0], A[1], z), 0.0, 1.0, Y, want, it, mu, LF, nthreads=NT)
    s, p, n = eng.sample_side(me, ot, it, 1.0, mu, LF)
    items = eng.get_items(me)
    eng.side_destroy(me); eng.side_destroy(ot)
    assert np.all(np.isfinite(items))
    err = rel_err(items, want)
    print("K %d %s: %.3g" % (K, eng.dtype, err))
    assert err < tol, err
    assert rel_err(s, s_ref) < stat_tol and rel_err(p, p_ref) < stat_tol and abs(n - n_ref) <= stat_tol * abs(n_ref)
    return info


@pytest.mark.parametrize("mode", [1, 3])
def test_half_iteration_k8(oracle, mode):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    old = os.environ.get("BPMF_HIP_MODE")
    os.environ["BPMF_HIP_MODE"] = str(mode)
    eng = bpmf_amd.HipEngine(8)
    try:
        rng = np.random.default_rng(80 + mode)
        for A, nrows, tag in ((M, nu, ref.TAG_MOVIES), (Mt, nm, ref.TAG_USERS)):
            ncols = len(A[0]) - 1
            _half_iteration(oracle, eng, 8, A, nrows, 0.7 * rng.standard_normal((ncols, 8)), 0.7 * rng.standard_normal((nrows, 8)), 3, tag,
                            RTOL, 1e-8, {1: r"k_sample1", 3: r"k_sample4"}[mode])
    finally:
        eng.close()
        if old is None:
            os.environ.pop("BPMF_HIP_MODE", None)
        else:
            os.environ["BPMF_HIP_MODE"] = old


@pytest.mark.parametrize("K", [64, 128])
def test_half_iteration_families(oracle, K):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = bpmf_amd.HipEngine(K)
    try:
        rng = np.random.default_rng(800 + K)
        sigma = (2.0 / K) ** 0.25
        for A, nrows, tag in ((M, nu, ref.TAG_MOVIES), (Mt, nm, ref.TAG_USERS)):
            ncols = len(A[0]) - 1
            _half_iteration(oracle, eng, K, A, nrows, sigma * rng.standard_normal((ncols, K)), sigma * rng.standard_normal((nrows, K)), 4, tag,
                            RTOL, 1e-8, {64: r"k_sample", 128: r"k_sample_wg2"}[K])
    finally:
        eng.close()


def _compare_chain(res, want, T):
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(res["U"] - want["U"]).max() / scale, np.abs(res["V"] - want["V"]).max() / scale
    ep = np.abs(res["cat_prob"] - want["cat_prob"]).max()
    o = res["ordinal"]
    print("U %.3g V %.3g cat_prob %.3g logp %.6f / %.6f; accepted %s; closest accept decision of the restatement %.3g"
          % (eu, ev, ep, res["logp"], want["logp"], o["accepted"], want["accept_margin"]))
    assert list(o["accepted"]) == list(want["accepted"])
    assert o["cutpoints"].shape == want["cutpoints"].shape and np.abs(o["cutpoints"] - want["cutpoints"]).max() < 1e-6
    assert np.abs(np.array(o["step"]) - want["step"]).max() <= 1e-12 * max(want["step"])
    assert eu < 1e-6 and ev < 1e-6
    assert np.abs(np.array(res["rmse"]) - want["rmse"]).max() < 1e-6
    assert np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max() < 1e-6
    assert ep < 1e-6 and abs(res["logp"] - want["logp"]) < 1e-6 and np.abs(res["expected"] - want["expected"]).max() < 1e-6
    assert res["cat_prob"].shape == (len(T[2]), len(o["levels"]))


@pytest.fixture(scope="module")
def chain_want(oracle):
    c = ref.CHAIN
    M, Mt, T, Tt, nu, nm = ref.planted(**c)
    levels = [1.0, 2.0, 3.0, 4.0, 5.0]
    return (M, Mt, T, Tt, nu, nm), ref.restate_chain(oracle, c["K"], M, Mt, T, c["nsims"], c["burnin"], levels)


@pytest.mark.parametrize("pipelined", [False, True])
def test_ordinal_chain_against_cpu(chain_want, pipelined):
    import bpmf_amd
    (M, Mt, T, Tt, nu, nm), want = chain_want
    c = ref.CHAIN
    assert any(want["accepted"]) and not all(want["accepted"][1:])
    eng = bpmf_amd.HipEngine(c["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=c["nsims"], burnin=c["burnin"], Tt=Tt, pipelined=pipelined, ordinal=True)
        assert eng.ordinal_info(res["movies"].side)[1] == c["nsims"] - 1          # one pass per iteration but the first
        assert np.array_equal(eng.ordinal_cut_get(res["users"].side), eng.ordinal_cut_get(res["movies"].side))
    finally:
        eng.close()
    _compare_chain(res, want, T)


@pytest.mark.parametrize("pipelined", [False, True])
def test_fixed_cutpoints_enqueue_no_loglik_pass(oracle, pipelined):
    import bpmf_amd
    c = ref.CHAIN
    M, Mt, T, Tt, nu, nm = ref.planted(**c)
    levels, cut = [1.0, 2.0, 3.0, 4.0, 5.0], [-1.4, -0.9, 0.6, 2.4]
    want = ref.restate_chain(oracle, c["K"], M, Mt, T, 5, 2, levels, cutpoints=cut)
    eng = bpmf_amd.HipEngine(c["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=5, burnin=2, Tt=Tt, pipelined=pipelined, ordinal=levels, cutpoints=cut)
        assert eng.ordinal_info(res["movies"].side)[1] == 0 and eng.ordinal_info(res["users"].side)[1] == 0
    finally:
        eng.close()
    assert not any(res["ordinal"]["accepted"]) and np.all(res["ordinal"]["cutpoints"] == np.asarray(cut))
    _compare_chain(res, want, T)


@pytest.mark.parametrize("pipelined", [False, True])
def test_fixed_cutpoints_never_drain(pipelined):
    """The host waits for the context's main stream, counted by the library: a run with fixed cutpoints waits exactly as often as
    the probit run of the same length (whose loop does not drain), a run with sampled cutpoints once more per iteration but the first."""
    import bpmf_amd
    c = ref.CHAIN
    M, Mt, T, Tt, nu, nm = ref.planted(**c)
    drains = bpmf_amd.load_library().bpmf_hip_stream_drains
    n = 6
    kw = dict(nsims=n, burnin=2, Tt=Tt, pipelined=pipelined)
    eng = bpmf_amd.HipEngine(c["K"])
    try:
        d0 = drains()
        bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, probit=True, threshold=3.0, **kw)
        d1 = drains()
        bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, ordinal=True, cutpoints=[-1.4, -0.9, 0.6, 2.4], **kw)
        d2 = drains()
        bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, ordinal=True, **kw)
        d3 = drains()
    finally:
        eng.close()
    print("host waits: probit %d, fixed cutpoints %d, sampled cutpoints %d" % (d1 - d0, d2 - d1, d3 - d2))
    assert d2 - d1 == d1 - d0
    assert d3 - d2 == (d1 - d0) + n - 1


def test_given_step_disables_the_adaptation(oracle):
    import bpmf_amd
    c = ref.CHAIN
    M, Mt, T, Tt, nu, nm = ref.planted(**c)
    g = ref.GIVEN_STEP                                                   # (its margins: tests/test_ordinal_host.py)
    want = ref.restate_chain(oracle, c["K"], M, Mt, T, g["nsims"], g["burnin"], [1.0, 2.0, 3.0, 4.0, 5.0], step=g["step"])
    eng = bpmf_amd.HipEngine(c["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=g["nsims"], burnin=g["burnin"], Tt=Tt, ordinal=True, ordinal_step=g["step"])
    finally:
        eng.close()
    assert res["ordinal"]["step"] == [g["step"]] * g["nsims"]
    _compare_chain(res, want, T)


def _live():
    import bpmf_amd
    return int(bpmf_amd.load_library().bpmf_hip_live_device_bytes())


def test_refusals_and_device_memory():
    import bpmf_amd
    from bpmf_amd import BpmfHipError
    K = 8
    M, Mt, T, Tt, nu, nm = ref.planted(**ref.CHAIN)
    levels, cut = [1.0, 2.0, 3.0, 4.0, 5.0], [-1.5, -1.0, 0.5, 2.5]
    start = _live()
    eng = bpmf_amd.HipEngine(K)
    try:
        new = lambda mean=0.0: eng.side_create(nm, nu, *M, mean)
        s = new()
        for lv, cp, tag, msg in (([1.0, 2.0, 3.0, 4.0], None, 11, "is not one of the levels"),
                                 ([1.0], None, 11, "2 .. 16"), (list(range(17)), None, 11, "2 .. 16"),
                                 (levels, [-1.0, -1.0, 0.5, 2.5], 11, "strictly increasing"), (levels, [-1.0, 0.0, 0.5, float("inf")], 11, "not finite"),
                                 (levels, [-1.0, 0.0, float("nan"), 2.0], 11, "not finite"), ([1.0, 2.0, 2.0, 4.0, 5.0], None, 11, "levels are not strictly"),
                                 (levels, cut, 0, "tag")):
            with pytest.raises(BpmfHipError, match=msg):
                eng.set_ordinal(s, lv, cp, tag)
        with pytest.raises(BpmfHipError, match="mean_rating = 0"):
            eng.set_ordinal(new(3.0), levels, cut, 11)
        with pytest.raises(BpmfHipError, match="not an ordinal side"):
            eng.ordinal_latent(s, len(M[2]))
        part = eng.side_create(nm, nu, M[0][:11] - M[0][0], M[1][:M[0][10]], M[2][:M[0][10]], 0.0, 0, 10)
        with pytest.raises(BpmfHipError, match="whole"):
            eng.set_ordinal(part, levels, cut, 11)
        # a side that is something else already
        other = new(); eng.set_probit(other, 3.0, 1)
        with pytest.raises(BpmfHipError, match="probit side"):
            eng.set_ordinal(other, levels, cut, 11)
        other = new(); eng.set_censored(other, np.zeros(len(M[2]), np.int8), 5)
        with pytest.raises(BpmfHipError, match="censored side"):
            eng.set_ordinal(other, levels, cut, 11)
        other = new(); eng.set_weights(other, np.ones(len(M[2])))
        with pytest.raises(BpmfHipError, match="weights"):
            eng.set_ordinal(other, levels, cut, 11)
        other = new(); eng.set_robust(other, 4.0, 9)
        with pytest.raises(BpmfHipError, match="Student-t"):
            eng.set_ordinal(other, levels, cut, 11)
        other = new(); eng.set_features(other, np.ones((nm, 2)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="features"):
            eng.set_ordinal(other, levels, cut, 11)
        other = new(); eng.set_prop_posterior(other, np.tile(np.eye(K).reshape(-1), (nm, 1)))
        with pytest.raises(BpmfHipError, match="propagated priors"):
            eng.set_ordinal(other, levels, cut, 11)
        # the ordinal side in turn
        eng.set_ordinal(s, levels, None, 11)
        with pytest.raises(BpmfHipError, match="ordinal"):
            eng.set_prop_posterior(s, np.tile(np.eye(K).reshape(-1), (nm, 1)))
        assert np.abs(eng.ordinal_cut_get(s) - ref.default_cutpoints(M[2], levels)).max() <= 1e-14
        A = ref.kernel_matrix(257, 5, absent=2)[0]                       # a level without a rating: half a rating more for every level
        ab = eng.side_create(len(A[0]) - 1, 211, *A, 0.0)
        eng.set_ordinal(ab, levels, None, 11)
        assert np.abs(eng.ordinal_cut_get(ab) - ref.default_cutpoints(A[2], levels)).max() <= 1e-14
        with pytest.raises(BpmfHipError, match="already"):
            eng.set_ordinal(s, levels, cut, 11)
        with pytest.raises(BpmfHipError, match="ordinal"):
            eng.set_probit(s, 3.0, 1)
        with pytest.raises(BpmfHipError, match="ordinal"):
            eng.set_censored(s, np.zeros(len(M[2]), np.int8), 5)
        with pytest.raises(BpmfHipError, match="ordinal"):
            eng.set_weights(s, np.ones(len(M[2])))
        with pytest.raises(BpmfHipError, match="ordinal"):
            eng.set_robust(s, 4.0, 9)
        with pytest.raises(BpmfHipError, match="ordinal"):
            eng.set_features(s, np.ones((nm, 2)), 5.0, 3)
        u = eng.side_create(nu, nm, *Mt, 0.0)
        with pytest.raises(BpmfHipError, match="ordinal"):
            eng.sys_set_reduce(s, u)
        with pytest.raises(BpmfHipError, match="ordinal"):
            eng.train_sse(s, u)
        eng.set_ordinal(u, levels, cut, 12)
        with pytest.raises(BpmfHipError, match="same cutpoints"):
            eng.ordinal_cut_step(s, u, 1, 0.1)
        eng.ordinal_cut_set(u, eng.ordinal_cut_get(s))
        with pytest.raises(BpmfHipError, match="step size"):
            eng.ordinal_cut_step(s, u, 1, 0.0)
        with pytest.raises(BpmfHipError, match="strictly increasing"):
            eng.ordinal_cut_set(s, [0.0, 0.0, 1.0, 2.0])
        with pytest.raises(BpmfHipError, match="strictly increasing"):
            eng.ordinal_loglik(s, u, [0.0, 0.0, 1.0, 2.0])
        mu, LU, LF = _hyper(K, nm, 1, 3)
        with pytest.raises(BpmfHipError, match="alpha = 1"):
            eng.sample_side(s, u, 1, 2.0, mu, LF)
        red_m, red_u = new(), eng.side_create(nu, nm, *Mt, 0.0)
        eng.sys_set_reduce(red_m, red_u)
        with pytest.raises(BpmfHipError, match="BPMF_REDUCE"):
            eng.set_ordinal(red_m, levels, cut, 11)
        assert _live() > start
    finally:
        eng.close()
    assert _live() == start


def test_a_tensor_mode_refuses_an_ordinal_side():
    """A mode's side is an ordinary side, so bpmf_hip_side_set_ordinal takes it; the tensor's own sampling call refuses it, in a
    line, as it refuses every other add-on of a mode."""
    import bpmf_amd
    from tests import tensor_ref
    idx, vals, dims = tensor_ref.edge_tensor()                           # values 1 .. 5
    eng = bpmf_amd.HipEngine(8)
    try:
        T = eng.tensor_create(idx, vals, dims, 0.0)
        eng.set_ordinal(T.sides[1], [1.0, 2.0, 3.0, 4.0, 5.0], [-1.5, -1.0, 0.5, 2.5], 11)
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            eng.tensor_sample(T, 0, 0, 1.0, np.zeros(8), np.eye(8))
        assert e.value.code == -1 and "not together with an ordinal likelihood on a mode of a tensor" in str(e.value)
        eng.tensor_destroy(T)
    finally:
        eng.close()


_COMM_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bpmf_amd
eng = bpmf_amd.HipEngine(8)
eng.comm_init(1, 0, eng.comm_unique_id())
side = eng.side_create(2, 4, np.array([0, 4, 6], np.int64), np.array([0, 1, 2, 3, 0, 2], np.int32), np.array([2., 3., 1., 3., 2., 1.]), 0.0)
try:
    eng.set_ordinal(side, [1.0, 2.0, 3.0], [-0.5, 0.5], 11)
    print("ACCEPTED")
except bpmf_amd.BpmfHipError as e:
    print("REFUSED %d %s" % (e.code, e))
eng.close()
"""


def test_set_ordinal_refuses_a_context_with_a_communicator():
    """The other branch of the single-GPU check: a whole side on a context that has a communicator (one rank, as `bpmf -g 1`
    makes one).  In a process of its own: a communicator is process-wide state of the communication library."""
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("BPMF_HIP_RCCL_LIBRARY", None)
    r = subprocess.run([sys.executable, "-c", _COMM_CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert re.search(r"^REFUSED -1 .*side_set_ordinal: .*communicator", r.stdout, re.M), r.stdout


def _write_mtx(path, nrows, ncols, A):
    colptr, rowidx, vals = A
    cols = np.repeat(np.arange(ncols), np.diff(colptr))
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (nrows, ncols, len(vals)))
        for i in range(len(vals)):
            f.write("%d %d %g\n" % (rowidx[i] + 1, cols[i] + 1, vals[i]))


def test_cli_ordinal_end_to_end(tmp_path):
    import bpmf_amd
    c = ref.CHAIN
    M, Mt, T, Tt, nu, nm = ref.planted(**c)
    _write_mtx(tmp_path / "train.mtx", nu, nm, M)
    _write_mtx(tmp_path / "test.mtx", nu, nm, T)
    eng = bpmf_amd.HipEngine(c["K"])
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=c["nsims"], burnin=c["burnin"], Tt=Tt, ordinal=True)
    finally:
        eng.close()
    o = res["ordinal"]
    true = np.asarray(T[2])
    rmse = math.sqrt(np.mean((res["expected"] - true) ** 2))
    accuracy = float(np.mean(o["levels"][np.argmax(res["cat_prob"], axis=1)] == true))
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    args = [exe, "-n", str(tmp_path / "train.mtx"), "-p", str(tmp_path / "test.mtx"), "-i", str(c["nsims"]), "-b", str(c["burnin"]),
            "-d", str(c["K"]), "--ordinal"]
    (tmp_path / "o").mkdir()
    runs = [subprocess.run(args + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
            for extra in (["-o", str(tmp_path / "o")], [])]               # -o: the plain loop; without: the pipelined one
    for run in runs:
        assert run.returncode == 0, run.stderr
        head = re.search(r"^likelihood: ordinal probit, 5 levels 1,2,3,4,5; cutpoints (\S+) \(sampled\); the RMSE columns compare the latent "
                         r"score with the raw value and are not an error measure$", run.stdout, re.M)
        assert head, run.stdout
        assert np.abs(np.array([float(x) for x in head.group(1).split(",")]) - o["cutpoints"][0]).max() < 1e-5
        assert re.search(r"^mean rating: 0$", run.stdout, re.M) and re.search(r"^alpha: 1$", run.stdout, re.M)
        assert len(re.findall(r"iteration \d+:\t RMSE: \S+\tavg RMSE: \S+\tFU\(", run.stdout)) == c["nsims"]
        fin = re.search(r"^Final Avg RMSE: \S+\nFinal ordinal RMSE: (\S+)\nFinal accuracy: (\S+)\nFinal log-prob: (\S+)$", run.stdout, re.M)
        assert fin, run.stdout
        got = [float(x) for x in fin.groups()]
        assert abs(got[0] - rmse) < 1e-5 and abs(got[1] - accuracy) < 1e-5 and abs(got[2] - res["logp"]) < 1e-5, (got, rmse, accuracy, res["logp"])
    with open(tmp_path / "o" / "ordinal.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["row", "col", "value", "expected", "p1", "p2", "p3", "p4", "p5"] and len(rows) == 1 + len(T[2])
    tcols = np.repeat(np.arange(nm), np.diff(T[0]))
    assert [int(x[0]) - 1 for x in rows[1:]] == list(T[1]) and [int(x[1]) - 1 for x in rows[1:]] == list(tcols)      # test-set order
    assert np.array_equal(np.array([float(x[2]) for x in rows[1:]]), true)
    assert np.abs(np.array([float(x[3]) for x in rows[1:]]) - res["expected"]).max() <= 1e-6
    assert np.abs(np.array([[float(v) for v in x[4:]] for x in rows[1:]]) - res["cat_prob"]).max() <= 1e-6
    with open(tmp_path / "o" / "cutpoints.csv") as f:
        cp = list(csv.reader(f))
    assert cp[0] == ["iteration", "accepted", "step", "g1", "g2", "g3", "g4"] and len(cp) == 1 + c["nsims"]
    assert [int(x[0]) for x in cp[1:]] == list(range(c["nsims"]))
    assert [int(x[1]) for x in cp[1:]] == [int(a) for a in o["accepted"]]
    assert np.abs(np.array([float(x[2]) for x in cp[1:]]) - o["step"]).max() <= 1e-6 * max(o["step"])
    assert np.abs(np.array([[float(v) for v in x[3:]] for x in cp[1:]]) - o["cutpoints"]).max() <= 1e-6
    assert not (tmp_path / "ordinal.csv").exists()
    # fixed cutpoints and given levels
    run = subprocess.run(args + ["--ordinal-levels", "1,2,3,4,5,6", "--ordinal-cutpoints", "-1.4,-0.9,0.6,2.4,5"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    assert re.search(r"^likelihood: ordinal probit, 6 levels 1,2,3,4,5,6; cutpoints -1\.4,-0\.9,0\.6,2\.4,5 \(fixed\);", run.stdout, re.M), run.stdout


def test_fixed_path_is_untouched_by_an_ordinal_run():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = bpmf_amd.HipEngine(16)
    try:
        before = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
        od = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True, ordinal=True)
        after = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
    finally:
        eng.close()
    assert before["U"].tobytes() == after["U"].tobytes() and before["V"].tobytes() == after["V"].tobytes()
    assert before["rmse"] == after["rmse"] and before["rmse_avg"] == after["rmse_avg"]
    assert "cat_prob" not in before and "ordinal" not in after and od["cat_prob"].shape[0] == len(T[2])
    assert not np.array_equal(od["U"], before["U"])
