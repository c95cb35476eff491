"""Model comparison on the device: bpmf_hip_score_cells, bpmf_amd.score_cells / score_summary / score_compare and
gibbs(score=True) against tests/score_ref.py.  Rings are filled through samples_set from seeded numpy factors: no chain is needed
for the kernel tests.

  1. against the longdouble reference, every kind: K in {4, 8, 36, 128} (lane groups of 2, 4, 16 and 64; a K that is no power of two;
     the full width), S in {1, 2, pc_chunk(Kp), pc_chunk(Kp) + 1}; one query with segment, segment + 1 and 1 cells, 40 queries x 3 cells,
     the empty list; gaussian (scalar alpha; weights with S alphas; flags 0 / +-1 with weights), student (nu = 4 with S alphas, nu = 1
     scalar), probit.  lpd and pwaic within 8 x the error of the fp64 restatement against the same reference (the largest over the
     cells of the four lists of a case, which share rings, kind and S), not less than S 2^-52.
  2. mean and std are the bytes of engine.predict_cells on the same list (every case of 1)
  3. shift invariance: residuals of 40 / sqrt(alpha) (l near -800: a plain mean of exponentials is -inf) and probit / censored cells at
     p_s = +-40: finite, within the bar of 1
  4. independence: the list permuted, every cell twice, batches of 1 and 7 cells and automatic, two calls: equal bytes
  5. the refusals of the C entry point, one line each
  6. through gibbs on ml-100k (K = 8, nsims = 10, burnin = 4): plain, robust = 4, noise = "adaptive", probit against score_ref.logdens
     on engine.samples_get of the run; the adaptive run uses the alpha of every iteration; bias = True against hand-filled rings
     (samples_get does not read a side with bias terms) and through the chain against engine.score_cells; weights= and censored= runs
     on the 60 x 40 matrix of tests/model_ref.py: the training cells with the run's weights / flags, the test cells without
  7. a saved model: load_model + score_cells gives the bytes of the training process; bpmf --score -o DIR prints the two Final lines and
     writes score.csv and waic-elpd.sdm, all equal to the Python result, and --model DIR --predict FILE --score serves the same file
  8. the planted experiment: the Student-t chain leads the Gaussian one by more than 2 paired standard errors, held-out and by WAIC

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import bpmf_amd
from bpmf_amd import io as bio
from tests import model_ref as mr
from tests import score_ref as sr
from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")

NQ = 41


def chunk(Kp):
    return 2048 // Kp


def group(Kp):
    g = 2
    while 2 * g <= Kp // 2 and g < 64:
        g *= 2
    return g


def segment(Kp):
    return 4 * 256 // group(Kp)


def rings(rng, nq, nc, S, K):
    """(U [nq, S, K], V [nc, S, K]): u . v has standard deviation 1; a sample moves a little around a level of the entity"""
    sigma = (1.0 / K) ** 0.25
    U = sigma * (rng.standard_normal((nq, 1, K)) + 0.3 * rng.standard_normal((nq, S, K)))
    V = sigma * (rng.standard_normal((nc, 1, K)) + 0.3 * rng.standard_normal((nc, S, K)))
    return U, V


def load(eng, sq, sc, U, V):
    S = U.shape[1]
    eng.samples_reserve(sq, S); eng.samples_reserve(sc, S)
    eng.samples_set(sq, U); eng.samples_set(sc, V)


def lists(rng, Kp, nc):
    seg = segment(Kp)
    one = lambda n, q: (np.full(n, q), rng.permutation(nc)[:n])
    many = (np.repeat(np.arange(40), 3), rng.integers(0, nc, 120))
    return dict(empty=(np.zeros(0, int), np.zeros(0, int)), segment=one(seg, 3), segment1=one(seg + 1, 40), single=one(1, 7), many=many)


def cases(rng, n, S, p):
    """name -> the arguments of one call for n cells whose posterior-mean prediction is p"""
    al_s = 1.0 + rng.random(S)
    y = p + rng.standard_normal(n) / np.sqrt(2.0)
    flag = rng.integers(-1, 2, n).astype(np.int8)
    return dict(gaussian=dict(kind="gaussian", y=y, alpha=2.0),
                weighted=dict(kind="gaussian", y=y, alpha=al_s, w=0.25 + 4.0 * rng.random(n)),
                censored=dict(kind="gaussian", y=y, alpha=al_s, w=0.5 + rng.random(n), flag=flag),
                student4=dict(kind="student", y=y + 6.0 * (rng.random(n) < 0.1), alpha=al_s, nu=4.0),
                student1=dict(kind="student", y=y, alpha=0.7, nu=1.0),
                probit=dict(kind="probit", y=np.where(rng.random(n) < 0.5, 1.0, -1.0), alpha=1.0))


def reference(U, V, mean, q, c, kw):
    """(want, bars): the longdouble reference (lpd, pwaic) of the cells and what the device is held to on them: 8 x the largest error of
    the fp64 restatement over these cells, not less than S 2^-52 (score_ref.bar)"""
    args = (U, V, mean, q, c, kw["y"], kw.get("w"), kw.get("flag"), kw["kind"], kw.get("nu"), kw["alpha"])
    want, f64 = sr.logdens(*args), sr.logdens_f64(*args)
    return want, tuple(sr.bar(f64[k], want[k], U.shape[1]) for k in (0, 1))


def sub(kw, idx):
    return {k: (v[idx] if k in ("y", "w", "flag") else v) for k, v in kw.items()}


def check(eng, sq, sc, U, V, mean, q, c, kw, tag, want=None, bars=None):
    """one call held to the reference (given, or of these cells): (err / bar of lpd, of pwaic)"""
    S = U.shape[1]
    got = eng.score_cells(sq, sc, mean, q, c, kw["y"], kw["alpha"], kw["kind"], kw.get("nu", 0.0), kw.get("w"), kw.get("flag"))
    assert sorted(got) == ["lpd", "mean", "pwaic", "std"] and all(v.shape == (len(q),) for v in got.values())
    pm, ps = eng.predict_cells(sq, sc, mean, q, c)
    assert got["mean"].tobytes() == pm.tobytes() and got["std"].tobytes() == ps.tobytes(), tag
    if len(q) == 0:
        return 0.0, 0.0
    if want is None:
        want, bars = reference(U, V, mean, q, c, kw)
    out = []
    for k, name in ((0, "lpd"), (1, "pwaic")):
        assert np.isfinite(got[name]).all(), (tag, name)
        err = sr.relative_error(got[name], want[k])
        assert err <= bars[k], (tag, name, err, bars[k])
        out.append(err / bars[k])
    if S == 1:
        assert not got["pwaic"].any()
    return tuple(out)


# ---- 1. and 2. against the reference -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [4, 8, 36, 128])
def test_score_cells_against_longdouble(hip_engine_factory, K):
    """The cells of the four lists form one pool per (S, case): the reference and the bar (8 x the largest error of the fp64 restatement
    over the pool, as tests/test_gpu_diag.py pools a kind's traces) are computed once, and every list is scored by a call of its own."""
    eng = hip_engine_factory(K)
    nc = segment(K) + 8
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    mean = 3.25
    try:
        for S in (1, 2, chunk(K), chunk(K) + 1):
            rng = np.random.default_rng(1000 * K + S)
            U, V = rings(rng, NQ, nc, S, K)
            load(eng, sq, sc, U, V)
            L = lists(rng, K, nc)
            names = [k for k in L if k != "empty"]
            q, c = (np.concatenate([L[k][i] for k in names]) for i in (0, 1))
            at = np.cumsum([0] + [len(L[k][0]) for k in names])
            p = mean + np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1)
            for cname, kw in cases(rng, len(q), S, p).items():
                mean_c = 0.0 if cname == "probit" else mean
                want, bars = reference(U, V, mean_c, q, c, kw)
                worst = [0.0, 0.0]
                for j, lname in enumerate(names):
                    idx = np.arange(at[j], at[j + 1])
                    w = check(eng, sq, sc, U, V, mean_c, q[idx], c[idx], sub(kw, idx), "K %d S %d %s %s" % (K, S, lname, cname),
                              tuple(x[idx] for x in want), bars)
                    worst = [max(a, b) for a, b in zip(worst, w)]
                check(eng, sq, sc, U, V, mean_c, *L["empty"], sub(kw, np.zeros(0, int)), "empty")
                print("K %d S %d %s: err / bar lpd %.3g pwaic %.3g (bars %.2e %.2e: 8 x the fp64 restatement's error)" %
                      (K, S, cname, worst[0], worst[1], bars[0], bars[1]))
        assert eng.score_last_ms(sq) >= 0.0
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 3. shift invariance -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [8, 128])
def test_shift_invariance(hip_engine_factory, K):
    eng = hip_engine_factory(K)
    nc, S = 60, 17
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    try:
        rng = np.random.default_rng(K)
        U, V = rings(rng, NQ, nc, S, K)
        load(eng, sq, sc, U, V)
        q, c = rng.integers(0, NQ, 200), rng.integers(0, nc, 200)
        p = np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1)
        alpha = 2.0
        far = np.where(rng.random(200) < 0.5, 40.0, -40.0) / np.sqrt(alpha)
        # residuals of 40 / sqrt(alpha): exp(l) underflows in every sample
        kw = dict(kind="gaussian", y=1.0 + p + far, alpha=alpha)
        with np.errstate(divide="ignore"):
            plain = np.log(np.mean(np.exp(sr._per_sample(U, V, 1.0, q, c, kw["y"], None, None, "gaussian", None, alpha, np.float64, None, None)), axis=1))
        assert np.isneginf(plain).any()                          # (exp(-745) is the last positive double)
        check(eng, sq, sc, U, V, 1.0, q, c, kw, "K %d far gaussian" % K)
        got = eng.score_cells(sq, sc, 1.0, q, c, kw["y"], alpha)
        assert (got["lpd"] < -700).all() and (got["lpd"] > -900).all()
        check(eng, sq, sc, U, V, 1.0, q, c, dict(kind="student", y=1.0 + p + 1e6 * far, alpha=alpha, nu=4.0), "K %d far student" % K)
        # censored cells whose bound is 40 standard deviations away, on both sides, with both flags
        flag = np.where(rng.random(200) < 0.5, 1, -1).astype(np.int8)
        kwc = dict(kind="gaussian", y=1.0 + p + far, alpha=alpha, flag=flag)
        check(eng, sq, sc, U, V, 1.0, q, c, kwc, "K %d far censored" % K)
        got = eng.score_cells(sq, sc, 1.0, q, c, kwc["y"], alpha, flag=flag)
        deep = flag * far > 0                                    # Phi(flag sqrt(alpha) (p - y)) with p - y = -far
        assert deep.any() and (~deep).any() and (got["lpd"][deep] < -700).all() and (np.abs(got["lpd"][~deep]) < 1e-300).all()
        # probit at p_s = +-40 (the mean rating carries the shift), both labels
        for shift in (40.0, -40.0):
            y = np.where(rng.random(200) < 0.5, 1.0, -1.0)
            check(eng, sq, sc, U, V, shift, q, c, dict(kind="probit", y=y, alpha=1.0), "K %d probit at %g" % (K, shift))
            got = eng.score_cells(sq, sc, shift, q, c, y, 1.0, "probit")
            assert np.isfinite(got["lpd"]).all() and (got["lpd"][y * shift < 0] < -600).all() and (got["lpd"][y * shift > 0] > -1e-200).all()
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 4. independence -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [4, 20, 128])
def test_bits_depend_on_the_cell_alone(hip_engine_factory, K):
    eng = hip_engine_factory(K)
    Kp = (K + 3) // 4 * 4
    nc, S = segment(Kp) + 8, 5
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    keys = ("lpd", "pwaic", "mean", "std")
    try:
        rng = np.random.default_rng(K)
        U, V = rings(rng, NQ, nc, S, K)
        load(eng, sq, sc, U, V)
        L = lists(rng, Kp, nc)
        q, c = (np.concatenate([L[k][i] for k in ("segment1", "many", "single")]) for i in (0, 1))
        p = np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1)
        for cname, kw in cases(rng, len(q), S, p).items():
            call = lambda idx: eng.score_cells(sq, sc, 0.5, q[idx], c[idx], kw["y"][idx], kw["alpha"], kw["kind"], kw.get("nu", 0.0),
                                               None if kw.get("w") is None else kw["w"][idx], None if kw.get("flag") is None else kw["flag"][idx])
            every = np.arange(len(q))
            base = call(every)
            again = call(every)
            assert all(base[k].tobytes() == again[k].tobytes() for k in keys), (K, cname)
            perm = rng.permutation(len(q))
            got = call(perm)
            assert all(base[k][perm].tobytes() == got[k].tobytes() for k in keys), (K, cname)
            twice = np.repeat(every, 2)
            got = call(twice)
            assert all(base[k][twice].tobytes() == got[k].tobytes() for k in keys), (K, cname)
            for cells in (1, 7, 0):
                eng.score_batch_cells(cells)
                got = call(every)
                assert all(base[k].tobytes() == got[k].tobytes() for k in keys), (K, cname, cells)
    finally:
        eng.score_batch_cells(0)
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_score_cells_refusals(hip_engine_factory):
    K, S, nc = 8, 5, 30
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    try:
        with pytest.raises(bpmf_amd.BpmfHipError, match="score_cells: no sample ring"):
            eng.score_cells(sq, sc, 0.0, [0], [0], [1.0], 2.0)
        rng = np.random.default_rng(5)
        load(eng, sq, sc, *rings(rng, NQ, nc, S, K))
        with pytest.raises(bpmf_amd.BpmfHipError, match="no scoring"):
            eng.score_last_ms(sq)
        q, c, y = [0, 1, 2], [3, 4, 5], [1.0, 2.0, 3.0]

        def refused(match, *args, **kw):
            with pytest.raises(bpmf_amd.BpmfHipError, match=match) as e:
                eng.score_cells(sq, sc, 0.0, *args, **kw)
            assert e.value.code == -1 and "\n" not in str(e.value).strip()
        refused("3 values of alpha for 5 samples", q, c, y, [1.0, 2.0, 3.0])
        refused("alpha of sample 1 is not finite and > 0", q, c, y, [1.0, 0.0, 1.0, 1.0, 1.0])
        refused("alpha of sample 0 is not finite and > 0", q, c, y, np.inf)
        refused(r"the weight of cell 1 \(1, 4\) is not finite and > 0", q, c, y, 2.0, w=[1.0, 0.0, 1.0])
        refused(r"the weight of cell 2 \(2, 5\) is not finite and > 0", q, c, y, 2.0, w=[1.0, 1.0, np.nan])
        refused(r"the value of cell 2 \(2, 5\) is not finite", q, c, [1.0, 2.0, np.nan], 2.0)
        refused("nu must be finite and >= 1", q, c, y, 2.0, "student", 0.5)
        refused("nu must be finite and >= 1", q, c, y, 2.0, "student", np.nan)
        refused("flags go with the gaussian kind alone", q, c, y, 1.0, "probit", flag=[0, 1, 0])
        refused("flags go with the gaussian kind alone", q, c, y, 1.0, "student", 4.0, flag=[0, 1, 0])
        refused("weights go with the gaussian kind alone", q, c, y, 1.0, "student", 4.0, w=[1.0, 1.0, 1.0])
        refused(r"the flag 2 of cell 1 \(1, 4\) is not -1, 0 or \+1", q, c, y, 2.0, flag=[0, 2, 0])
        refused(r"cell 1 \(41, 4\) is out of range", [0, NQ, 2], c, y, 2.0)
        with pytest.raises(ValueError, match="kind must be one of"):
            eng.score_cells(sq, sc, 0.0, q, c, y, 2.0, "poisson")
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        one = np.zeros(1, np.int32); out = np.zeros(1); al = np.ones(1)
        f = eng.lib.bpmf_hip_score_cells
        assert f(None, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, None, 0, 0.0, 1, ptr(al), ptr(out), ptr(out), ptr(out), ptr(out)) == -1
        assert f(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), None, None, None, 0, 0.0, 1, ptr(al), ptr(out), ptr(out), ptr(out), ptr(out)) == -1
        assert f(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, None, 0, 0.0, 1, None, ptr(out), ptr(out), ptr(out), ptr(out)) == -1
        assert f(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, None, 0, 0.0, 1, ptr(al), ptr(out), None, ptr(out), ptr(out)) == -1
        assert f(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, None, 7, 0.0, 1, ptr(al), ptr(out), ptr(out), ptr(out), ptr(out)) == -1
        assert f(sq.handle, sc.handle, 0.0, 0, None, None, None, None, None, 0, 0.0, 1, ptr(al), None, None, None, None) == 0
        assert eng.lib.bpmf_hip_score_batch_cells(-1) == -1
        assert eng.lib.bpmf_hip_abi_version() == 1
        got = eng.score_cells(sq, sc, 0.0, q, c, y, 2.0)         # the context goes on working
        assert all(np.isfinite(v).all() for v in got.values()) and eng.score_last_ms(sq) >= 0.0
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 6. through gibbs ----------------------------------------------------------------------------------------------------------------------

CHAIN = dict(nsims=10, burnin=4)


@pytest.fixture(scope="module")
def ml100k():
    return util.ml100k()


def held_to_reference(res, A, key, kind, nu, alpha, weights=None, flags=None, sub=None):
    """res["score"][key] against score_ref.logdens on samples_get of the run, for the cells of the CSC triple A (sub: every sub-th)"""
    eng = res["users"].engine
    U, V = eng.samples_get(res["users"].side), eng.samples_get(res["movies"].side)
    rows, cols = sr.cells_of(A)
    y = np.asarray(A[2], np.float64)
    if kind == "probit":
        y = np.where(y > res["model_info"]["probit_threshold"], 1.0, -1.0)
    sel = slice(None, None, sub)
    args = (U, V, res["movies"].mean_rating, rows[sel], cols[sel], y[sel], weights, flags, kind, nu, alpha)
    want, f64 = sr.logdens(*args), sr.logdens_f64(*args)
    d = res["score"][key]
    S = U.shape[1]
    assert d["samples"] == S == 6 and len(d["lpd"]) == len(rows) and d["kind"] == kind
    assert np.array_equal(d["rows"], rows) and np.array_equal(d["cols"], cols)
    assert d["elpd"].tobytes() == (d["lpd"] - d["pwaic"]).tobytes() and d["summary"] == bpmf_amd.score_summary(d)
    for k, name in ((0, "lpd"), (1, "pwaic")):
        err, bar = sr.relative_error(d[name][sel], want[k]), sr.bar(f64[k], want[k], S)
        print("%s %s %s: err %.3g bar %.3g" % (kind, key, name, err, bar))
        assert err <= bar, (kind, key, name, err, bar)
    return want


@pytest.mark.parametrize("variant", ["plain", "robust", "adaptive", "probit"])
def test_gibbs_score(hip_engine_factory, ml100k, variant):
    M, Mt, T, Tt, nu, nm = ml100k
    eng = hip_engine_factory(8)
    kw = dict(plain={}, robust=dict(robust=4.0), adaptive=dict(noise="adaptive"), probit=dict(probit=True, threshold=3.5))[variant]
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, score=True, **CHAIN, **kw)
    info = res["model_info"]
    kind = dict(plain="gaussian", robust="student", adaptive="gaussian", probit="probit")[variant]
    if variant == "adaptive":
        alpha = np.array(res["alpha"][4:10])
        assert info["alpha_samples"] == list(alpha) and len(set(alpha)) == 6
    else:
        alpha = info["alpha"]
        assert info["alpha_samples"] is None
    assert info["nu"] == (4.0 if variant == "robust" else None)
    assert sorted(res["score"]) == ["test", "train"]
    want_t = held_to_reference(res, T, "test", kind, info["nu"], alpha)
    held_to_reference(res, M, "train", kind, info["nu"], alpha, sub=7 if variant == "probit" else None)
    s = res["score"]["train"]["summary"]
    assert s["n"] == len(M[2]) and s["waic"] == -2.0 * s["elpd"] and s["p_waic"] > 0 and 0.0 <= s["pwaic_above"] <= 1.0
    if variant == "adaptive":                                    # a single alpha is another figure
        U, V = eng.samples_get(res["users"].side), eng.samples_get(res["movies"].side)
        rows, cols = sr.cells_of(T)
        first = sr.logdens(U, V, res["movies"].mean_rating, rows, cols, T[2], kind="gaussian", alpha=res["alpha"][0])
        S = 6
        assert sr.relative_error(res["score"]["test"]["lpd"], first[0]) > 100 * sr.bar(want_t[0], want_t[0], S)
    # the chain is untouched
    plain = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, **CHAIN, **kw)
    assert "score" not in plain and np.array(plain["rmse"]).tobytes() == np.array(res["rmse"]).tobytes() and plain["U"].tobytes() == res["U"].tobytes()


@pytest.mark.parametrize("variant", ["weights", "censored"])
def test_gibbs_score_with_the_weights_and_flags_of_the_run(hip_engine_factory, variant):
    """the training cells are scored with the run's per-rating weights / censoring flags, the test cells without"""
    import scipy.sparse as sp
    from bpmf_amd.censor import censor_flags
    from bpmf_amd.weights import rating_weights
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    rows, cols = sr.cells_of(M)
    rng = np.random.default_rng(12)
    pick = rng.random(len(rows)) < 0.3
    vals = 0.25 + 2.0 * rng.random(pick.sum()) if variant == "weights" else np.where(rng.random(pick.sum()) < 0.5, 1.0, -1.0)
    X = util.csc_arrays(sp.coo_matrix((vals, (rows[pick], cols[pick])), shape=(nu, nm)).tocsc())
    eng = hip_engine_factory(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, score=True, alpha=2.0, **CHAIN, **{variant: X})
    w = rating_weights(M, X) if variant == "weights" else None
    flag = censor_flags(M, X) if variant == "censored" else None
    assert (w is None or (w != 1.0).sum() == pick.sum()) and (flag is None or (flag != 0).sum() == pick.sum())
    held_to_reference(res, T, "test", "gaussian", None, 2.0)
    held_to_reference(res, M, "train", "gaussian", None, 2.0, weights=w, flags=flag)
    unweighted = sr.logdens(eng.samples_get(res["users"].side), eng.samples_get(res["movies"].side), res["movies"].mean_rating, rows, cols, M[2], alpha=2.0)
    assert sr.relative_error(res["score"]["train"]["lpd"], unweighted[0]) > 1e-3


def test_score_with_biases(hip_engine_factory, ml100k):
    """samples_get does not read a side with bias terms, so the bias rows of the rings are held to the reference on hand-filled rings
    (p_s = mean + u . v + b + c), and the chain to engine.score_cells on its own rings."""
    K, S, nq, nc = 8, 16, 11, 23
    eng = hip_engine_factory(K)
    A = (np.zeros(nq + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    B = (np.zeros(nc + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    sq, sc = eng.side_create(nq, nc, *A, 0.0), eng.side_create(nc, nq, *B, 0.0)
    try:
        eng.set_bias(sq, 1.0, 14, 1); eng.set_bias(sc, 1.0, 13, 0)
        eng.samples_reserve(sq, S); eng.samples_reserve(sc, S)
        rng = np.random.default_rng(4)
        U, V = rings(rng, nq, nc, S, K)
        bq, bc = 0.5 * rng.standard_normal((S, nq)), 0.5 * rng.standard_normal((S, nc))
        for s in range(S):
            eng.set_items(sq, U[:, s]); eng.set_items(sc, V[:, s])
            eng.bias_set(sq, bq[s]); eng.bias_set(sc, bc[s])
            eng.samples_add(sq); eng.samples_add(sc)
        q, c = np.divmod(np.arange(nq * nc), nc)
        extra = (bq[:, q] + bc[:, c]).T
        y = 1.25 + np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1) + extra.mean(axis=1) + rng.standard_normal(len(q)) / np.sqrt(2.0)
        got = eng.score_cells(sq, sc, 1.25, q, c, y, 2.0)
        pm, ps = eng.predict_cells(sq, sc, 1.25, q, c)
        assert got["mean"].tobytes() == pm.tobytes() and got["std"].tobytes() == ps.tobytes()
        want = sr.logdens(U, V, 1.25, q, c, y, alpha=2.0, extra=extra)
        f64 = sr.logdens_f64(U, V, 1.25, q, c, y, alpha=2.0, extra=extra)
        for k, name in ((0, "lpd"), (1, "pwaic")):
            assert sr.relative_error(got[name], want[k]) <= sr.bar(f64[k], want[k], S), name
        without = sr.logdens(U, V, 1.25, q, c, y, alpha=2.0)
        assert sr.relative_error(got["lpd"], without[0]) > 1e-3                       # the bias rows of the rings are read
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)
    M, Mt, T, Tt, nu, nm = ml100k
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, score=True, bias=True, **CHAIN)
    rows, cols = sr.cells_of(T)
    direct = eng.score_cells(res["users"].side, res["movies"].side, res["movies"].mean_rating, rows, cols, T[2], res["model_info"]["alpha"])
    d = res["score"]["test"]
    assert all(d[k].tobytes() == direct[k].tobytes() for k in ("lpd", "pwaic", "mean", "std")) and np.isfinite(d["lpd"]).all()
    pm, ps = eng.predict_cells(res["users"].side, res["movies"].side, res["movies"].mean_rating, rows, cols)
    assert d["mean"].tobytes() == pm.tobytes()
    assert (d["lpd"] < 0.5 * np.log(2.0 / (2 * np.pi))).all()     # (no Gaussian of precision alpha = 2 has a larger density)
    assert len(res["score"]["train"]["lpd"]) == len(M[2])


# ---- 7. a saved model ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["plain", "adaptive", "probit"])
def test_saved_model_serves_the_same_bytes(tmp_path, hip_engine_factory, variant):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    eng = hip_engine_factory(8)
    kw = dict(plain={}, adaptive=dict(noise="adaptive"), probit=dict(probit=True, threshold=3.5))[variant]
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, score=True, save_model=str(tmp_path / "model"), **CHAIN, **kw)
    rows, cols = sr.cells_of(T)
    mrows, mcols = sr.cells_of(M)
    serve = bpmf_amd.HipEngine(8)
    try:
        loaded = bpmf_amd.load_model(serve, str(tmp_path / "model"))
        assert loaded["model_info"]["nu"] is None
        if variant == "adaptive":
            assert loaded["model_info"]["alpha_samples"] == res["model_info"]["alpha_samples"]
        for key, (r, c, v) in dict(test=(rows, cols, T[2]), train=(mrows, mcols, M[2])).items():
            again = bpmf_amd.score_cells(loaded, r, c, v)
            assert all(again[k].tobytes() == res["score"][key][k].tobytes() for k in ("lpd", "pwaic", "elpd", "mean", "std")), (variant, key)
            assert again["summary"] == res["score"][key]["summary"]
    finally:
        serve.close()


def run(args, cwd):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def final_lines(score):
    """the Final lines bpmf prints for res["score"]"""
    out = []
    if "test" in score:
        s = score["test"]["summary"]
        out.append("Final test log-density: mean %.6f se %.6f (%d cells, %d samples)" % (s["lpd_mean"], s["se_lpd"] / s["n"], s["n"], s["samples"]))
    s = score["train"]["summary"]
    out.append("Final WAIC: %.4f elpd %.4f p_waic %.4f se %.4f (%d cells, %.2f%% with var > 0.4)" %
               (s["waic"], s["elpd"], s["p_waic"], s["se"], s["n"], 100.0 * s["pwaic_above"]))
    return out


def read_score(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "row,col,value,lpd,mean,std"
    return np.array([ln.split(",") for ln in lines[1:]], dtype=float).reshape(-1, 6)


@pytest.mark.parametrize("variant", ["plain", "robust"])
def test_cli_score(tmp_path, hip_engine_factory, variant):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    bio.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    bio.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    for name in ("A", "B", "P"):
        os.mkdir(tmp_path / name)
    flags, kw = (["--robust", 4], dict(robust=4.0)) if variant == "robust" else ([], {})
    chain = ["-n", "train.sdm", "-p", "test.sdm", "-d", 8, "-i", 10, "-b", 4] + flags
    plain = run(chain + ["-o", "P"], tmp_path)
    a = run(chain + ["--score", "-o", "A"] + (["--save-model", "model"] if variant == "plain" else []), tmp_path)
    assert "score: WAIC of the training cells and log density of the test cells\n" in a.stdout
    strip = lambda text: [ln for ln in text.splitlines() if not ln.startswith(("score: ", "save-model: ", "Final test log-density", "Final WAIC", "Total time"))
                          and "items/sec" not in ln and "ratings/sec" not in ln]
    assert [ln for ln in a.stdout.splitlines() if ln.startswith("Final Avg RMSE")] == [ln for ln in plain.stdout.splitlines() if ln.startswith("Final Avg RMSE")]
    assert len(strip(a.stdout)) == len(strip(plain.stdout))
    assert sorted(set(os.listdir(tmp_path / "A")) - set(os.listdir(tmp_path / "P"))) == ["score.csv", "waic-elpd.sdm"]
    lines = a.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("Final Avg RMSE: ")][0]
    # the Python run of the same chain gives the same figures
    eng = hip_engine_factory(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, score=True, alpha=2.0, **CHAIN, **kw)
    assert lines[at + 1:at + 3] == final_lines(res["score"])
    rec = read_score(tmp_path / "A" / "score.csv")
    rows, cols = sr.cells_of(T)
    d = res["score"]["test"]
    assert np.array_equal(rec[:, 0], rows + 1) and np.array_equal(rec[:, 1], cols + 1) and rec[:, 2].tobytes() == np.asarray(T[2]).tobytes()
    for j, k in ((3, "lpd"), (4, "mean"), (5, "std")):
        assert rec[:, j].tobytes() == d[k].tobytes(), k
    nr, ncol, E = bio.read_sparse(tmp_path / "A" / "waic-elpd.sdm")
    assert (nr, ncol) == (nu, nm) and np.array_equal(E[0], M[0]) and np.array_equal(E[1], M[1])
    assert np.asarray(E[2]).tobytes() == res["score"]["train"]["elpd"].tobytes()
    if variant != "plain":
        return
    # a saved model serves the same file for the same cells, and the WAIC of the training cells with -n
    b = run(["--model", "model", "--predict", "test.sdm", "--score", "-n", "train.sdm", "-o", "B"], tmp_path)
    assert (tmp_path / "B" / "score.csv").read_bytes() == (tmp_path / "A" / "score.csv").read_bytes()
    assert (tmp_path / "B" / "waic-elpd.sdm").read_bytes() == (tmp_path / "A" / "waic-elpd.sdm").read_bytes()
    assert b.stdout.splitlines()[1:] == final_lines(res["score"]) and b.stdout.startswith("model: model, ")
    os.mkdir(tmp_path / "C")
    c = run(["--model", "model", "--predict", "test.sdm", "--score", "-o", "C"], tmp_path)
    assert c.stdout.splitlines()[1:] == final_lines(res["score"])[:1] and sorted(os.listdir(tmp_path / "C")) == ["predict.csv", "score.csv"]


# ---- 8. the planted experiment -------------------------------------------------------------------------------------------------------------

def test_planted_outliers_rank_the_models(hip_engine_factory):
    """robust_ref.PLANTED: 5 % of the training cells shifted by +-10, clean test cells.  The restated CPU chains
    (score_ref.PLANTED_MEASURED) put the Student-t model (nu = 4) ahead of the Gaussian one at the same alpha by 8.9 paired standard
    errors of the held-out lpd and by 23.9 of the training elpd (WAIC).  Asserted of the GPU chains: more than 2 on both."""
    from tests import robust_ref
    P = robust_ref.PLANTED
    d = robust_ref.planted_data(**P)
    eng = hip_engine_factory(P["K"])
    run = lambda **kw: bpmf_amd.gibbs(eng, d["M"], d["Mt"], d["T"], P["nusers"], P["nmovies"], nsims=P["nsims"], burnin=P["burnin"], Tt=d["Tt"],
                                      alpha=P["alpha"], score=True, **kw)["score"]
    student, gauss = run(robust=P["nu"]), run()
    for key, what in (("test", "lpd"), ("train", "elpd")):
        cmp = bpmf_amd.score_compare(student[key], gauss[key])
        diff, se = cmp[what + "_diff"], cmp[what + "_se"]
        print("%s %s: student %.2f gaussian %.2f difference %.2f paired se %.2f (%.1f se); restated CPU chains %.2f / %.2f" %
              (key, what, student[key]["summary"]["lpd_sum" if what == "lpd" else "elpd"], gauss[key]["summary"]["lpd_sum" if what == "lpd" else "elpd"],
               diff, se, diff / se, *sr.PLANTED_MEASURED[key]))
        assert diff > sr.PLANTED_MARGIN_SE * se, (key, diff, se)
