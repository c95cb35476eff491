"""PSIS-LOO on the device: bpmf_hip_loo_traces / _cells, bpmf_amd.loo_cells / loo_summary, gibbs(loo=True) and
`bpmf --loo` against tests/loo_ref.py.

  1. k_trace_psis on crafted traces against the longdouble form of the rule: S in {1, 2, 24, 25, 26, 63, 64, 65, 224, 225, 226, 1000, 2048,
     2049, 4096} (the M < 5 edge, the wave edges, where the two terms of M cross, the padding to a power of two), two dozen traces per
     family: Gaussian log densities with a sample spread of 0.3, 1.5 and 4 sigma (khat from below 0 to above 10), each of them on a
     2^-40 grid shifted by +-700, all values equal, a constant tail over a varying body, ties across the cutoff, one sample that dominates.  No tolerance is
     stated in advance: per (S, family) the bar of elpd_loo, lpd and khat is 16 x the largest error of the fp64 form of the rule
     against its longdouble form over the group, computed here; an infinite khat must match exactly.
  2. a NaN or an infinity in one trace gives NaN in that trace only
  3. loo_cells through the rings, K in {4, 36, 128}, S in {1, 30, 200}, 240 cells, every kind: the reference is the longdouble rule on the
     longdouble log densities of samples_set's factors, the bar 16 x the error of the fp64 restatement (its own dot products and log
     densities included: the trace's rounding term); mean and std are predict_cells's bytes; lpd differs from score_cells's by at
     most the sum of this bar and the bar tests/test_gpu_score.py holds score_cells to
  4. equal bytes across permutations, doubled lists, batch sizes, repeated calls, with or without the optional outputs, and for an
     uncensored cell whether or not another cell of its list is censored
  5. the refusals of both entry points; a fp32 context
  6. gibbs(loo=True) on ml-100k, plain and robust = 4, against the reference on the run's rings; a saved model serves the same bytes;
     bpmf --loo: the line, both .sdm files, --model

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import bpmf_amd
from bpmf_amd import io as bio
from tests import loo_ref as lr
from tests import model_ref as mr
from tests import score_ref as sr
from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
LD = np.longdouble
NQ = 41
KEYS = ("elpd_loo", "khat", "lpd")


def gaussian_traces(rng, n, S, spread):
    th = rng.standard_normal((n, S)) * spread
    y = rng.standard_normal((n, 1))
    return -0.5 * math.log(2 * math.pi) - 0.5 * (y - th) ** 2


def families(rng, S, n=24):
    M = max(lr.tail_length(S), 1)
    out = {"spread %.1f" % sp: gaussian_traces(rng, n, S, sp) for sp in (0.3, 1.5, 4.0)}
    body = gaussian_traces(rng, n, S, 1.0)
    out["all equal"] = np.repeat(rng.standard_normal((n, 1)) * 5.0, S, axis=1)
    const = np.sort(body, axis=1)
    const[:, :min(M, S)] = const[:, :1] - 1.0
    out["constant tail"] = rng.permuted(const, axis=1)
    tie = np.sort(body, axis=1)
    lo, hi = max(M - 2, 0), min(M + 3, S)
    tie[:, lo:hi] = tie[:, lo:lo + 1]
    out["ties across the cutoff"] = rng.permuted(tie, axis=1)
    dom = body.copy()
    dom[np.arange(n), rng.integers(0, S, n)] -= 30.0
    out["one dominates"] = dom
    return out


# ---- 1. crafted traces ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 2, 24, 25, 26, 63, 64, 65, 224, 225, 226, 1000, 2048, 2049, 4096])
def test_traces_against_longdouble(hip_engine_factory, S):
    eng = hip_engine_factory(8)
    rng = np.random.default_rng(7000 + S)
    for name, L in families(rng, S).items():
        got = eng.loo_traces(L)
        used, g, err = lr.held_to_reference(got, L, tag="S %d %s" % (S, name))
        print("S %d %s: share of the bar elpd %.3f khat %.3f lpd %.3f (fp64 rule's errors %.2e %.2e %.2e)" %
              (S, name, used["elpd_loo"], used["khat"], used["lpd"], err["elpd_loo"], err["khat"], err["lpd"]))
        if S < 25 or name in ("all equal", "constant tail"):
            assert np.isposinf(got["khat"]).all()
        if name.startswith("spread"):                            # shift invariance: elpd moves by the shift, khat keeps its value
            Lq = np.round(L * 2.0 ** 40) / 2.0 ** 40              # multiples of 2^-40 below 2^9: Lq +- 700 is exact, the shifted traces are the same traces
            base = eng.loo_traces(Lq)
            ub, gb, eb = lr.held_to_reference(base, Lq, tag="S %d on the 2^-40 grid" % S)
            for shift in (700.0, -700.0):
                assert np.array_equal((Lq + shift) - shift, Lq)
                sh = eng.loo_traces(Lq + shift)
                us, gs, es = lr.held_to_reference(sh, Lq + shift, tag="S %d shifted by %g" % (S, shift))
                fin = np.isfinite(gb["khat"])
                assert np.array_equal(np.isposinf(sh["khat"]), np.isposinf(base["khat"]))
                assert np.all(np.abs(sh["khat"][fin] - base["khat"][fin]) <= lr.BAR_FACTOR * (eb["khat"] + es["khat"]))
                assert np.all(np.abs((sh["elpd_loo"] - shift) - base["elpd_loo"]) <= lr.BAR_FACTOR * (eb["elpd_loo"] + es["elpd_loo"]))
    one = eng.loo_traces(L[0], want_lpd=False)                  # a single trace as a vector, without lpd
    assert one["lpd"] is None and one["elpd_loo"].tobytes() == got["elpd_loo"][:1].tobytes() and one["khat"].tobytes() == got["khat"][:1].tobytes()


# ---- 2. values that are not finite -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [3, 64, 1000])
def test_a_trace_that_is_not_finite_gives_nan_for_itself_alone(hip_engine_factory, S):
    eng = hip_engine_factory(8)
    rng = np.random.default_rng(S)
    L = gaussian_traces(rng, 9, S, 1.0)
    base = eng.loo_traces(L)
    bad = L.copy()
    bad[1, 0] = np.nan; bad[3, S - 1] = np.inf; bad[4, S // 2] = -np.inf; bad[8, :] = np.nan
    got = eng.loo_traces(bad)
    hit = [1, 3, 4, 8]
    rest = [0, 2, 5, 6, 7]
    for k in KEYS:
        assert np.isnan(got[k][hit]).all() and got[k][rest].tobytes() == base[k][rest].tobytes(), k


# ---- 3. through the rings --------------------------------------------------------------------------------------------------------------------

def rings(rng, nq, nc, S, K):
    sigma = (1.0 / K) ** 0.25
    U = sigma * (rng.standard_normal((nq, 1, K)) + 0.3 * rng.standard_normal((nq, S, K)))
    V = sigma * (rng.standard_normal((nc, 1, K)) + 0.3 * rng.standard_normal((nc, S, K)))
    return U, V


def load(eng, sq, sc, U, V):
    S = U.shape[1]
    eng.samples_reserve(sq, S); eng.samples_reserve(sc, S)
    eng.samples_set(sq, U); eng.samples_set(sc, V)


def cases(rng, n, S, p):
    al_s = 1.0 + rng.random(S)
    y = p + rng.standard_normal(n) / np.sqrt(2.0)
    flag = rng.integers(-1, 2, n).astype(np.int8)
    return dict(weighted=dict(kind="gaussian", y=y, alpha=al_s, w=0.25 + 4.0 * rng.random(n), mean=3.25),
                censored=dict(kind="gaussian", y=y, alpha=2.0, flag=flag, mean=3.25),
                student4=dict(kind="student", y=y + 6.0 * (rng.random(n) < 0.1), alpha=al_s, nu=4.0, mean=3.25),
                probit40=dict(kind="probit", y=np.where(rng.random(n) < 0.5, 1.0, -1.0), alpha=1.0, mean=40.0),
                probitm40=dict(kind="probit", y=np.where(rng.random(n) < 0.5, 1.0, -1.0), alpha=1.0, mean=-40.0))


def log_densities(U, V, q, c, kw, mean=None):
    """(fp64, longdouble) log densities [n, S] of the cells under every sample (tests/score_ref.py)"""
    args = (U, V, kw["mean"] if mean is None else mean, q, c, kw["y"], kw.get("w"), kw.get("flag"), kw["kind"], kw.get("nu"), kw["alpha"])
    return (sr._per_sample(*args, np.float64, sr.log_phi_f64, lambda x: np.float64(math.lgamma(float(x)))),
            sr._per_sample(*args, LD, sr.log_phi_ld, sr._lgamma_ld))


def call(eng, sq, sc, q, c, kw, idx=slice(None), **more):
    pick = lambda a: None if a is None else a[idx]
    return eng.loo_cells(sq, sc, kw["mean"], q[idx], c[idx], kw["y"][idx], kw["alpha"], kw["kind"], kw.get("nu", 0.0), pick(kw.get("w")),
                         pick(kw.get("flag")), **more)


@pytest.mark.parametrize("K", [4, 36, 128])
def test_loo_cells_against_longdouble(hip_engine_factory, K):
    eng = hip_engine_factory(K)
    nc, n = 60, 240
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    try:
        for S in (1, 30, 200):
            rng = np.random.default_rng(100 * K + S)
            U, V = rings(rng, NQ, nc, S, K)
            load(eng, sq, sc, U, V)
            q, c = rng.integers(0, NQ, n), rng.integers(0, nc, n)
            p = np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1)
            for cname, kw in cases(rng, n, S, 3.25 + p).items():
                if kw["kind"] == "probit":
                    kw["y"] = np.where(rng.random(n) < 0.9, np.sign(kw["mean"]), -np.sign(kw["mean"]))
                tag = "K %d S %d %s" % (K, S, cname)
                got = call(eng, sq, sc, q, c, kw)
                assert sorted(got) == ["elpd_loo", "khat", "lpd", "mean", "std"] and all(v.shape == (n,) for v in got.values())
                pm, ps = eng.predict_cells(sq, sc, kw["mean"], q, c)
                assert got["mean"].tobytes() == pm.tobytes() and got["std"].tobytes() == ps.tobytes(), tag
                l64, lld = log_densities(U, V, q, c, kw)
                used, g, err = lr.held_to_reference(got, l64, lld, tag)
                sc_ = eng.score_cells(sq, sc, kw["mean"], q, c, kw["y"], kw["alpha"], kw["kind"], kw.get("nu", 0.0), kw.get("w"), kw.get("flag"))
                # lpd against score_cells: each is held to the same longdouble lpd, loo's to the bar above and score's to the bar of
                # tests/test_gpu_score.py (score_ref.bar, relative to max(1, |lpd|)), so the two differ by at most the sum of the two bars
                args = (U, V, kw["mean"], q, c, kw["y"], kw.get("w"), kw.get("flag"), kw["kind"], kw.get("nu"), kw["alpha"])
                want_lpd, f64_lpd = sr.logdens(*args)[0], sr.logdens_f64(*args)[0]
                assert float(np.abs(want_lpd - g["lpd"]).max()) <= (S + 64) * 2.0 ** -64 * max(1.0, float(np.abs(want_lpd).max())), tag   # one truth: the two references differ by longdouble rounding
                both = lr.BAR_FACTOR * err["lpd"] + sr.bar(f64_lpd, want_lpd, S) * np.maximum(1.0, np.abs(want_lpd.astype(np.float64)))
                diff = np.abs(sc_["lpd"] - got["lpd"])
                assert np.all(diff <= both), (tag, float((diff / both).max()))
                print("%s: share of the bar elpd %.3f khat %.3f lpd %.3f, lpd against score_cells %.3f of the two bars; khat %.2f .. %.2f" %
                      (tag, used["elpd_loo"], used["khat"], used["lpd"], float((diff / both).max()), np.nanmin(got["khat"]), np.max(got["khat"])))
        assert eng.loo_last_ms(sq) >= 0.0
        empty = eng.loo_cells(sq, sc, 0.0, np.zeros(0, int), np.zeros(0, int), np.zeros(0), 2.0)
        assert all(v.shape == (0,) for v in empty.values())
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,S", [(4, 30), (20, 200), (128, 65)])
def test_bits_depend_on_the_cell_alone(hip_engine_factory, K, S):
    eng = hip_engine_factory(K)
    nc, n = 50, 150
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    keys = KEYS + ("mean", "std")
    try:
        rng = np.random.default_rng(K)
        U, V = rings(rng, NQ, nc, S, K)
        load(eng, sq, sc, U, V)
        q, c = rng.integers(0, NQ, n), rng.integers(0, nc, n)
        p = np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1)
        for cname, kw in cases(rng, n, S, 3.25 + p).items():
            every = np.arange(n)
            base = call(eng, sq, sc, q, c, kw)
            again = call(eng, sq, sc, q, c, kw)
            assert all(base[k].tobytes() == again[k].tobytes() for k in keys), (K, cname)
            perm = rng.permutation(n)
            got = call(eng, sq, sc, q, c, kw, perm)
            assert all(base[k][perm].tobytes() == got[k].tobytes() for k in keys), (K, cname)
            twice = np.repeat(every, 2)
            got = call(eng, sq, sc, q, c, kw, twice)
            assert all(base[k][twice].tobytes() == got[k].tobytes() for k in keys), (K, cname)
            for cells in (1, 7, 0):
                eng.loo_batch_cells(cells)
                got = call(eng, sq, sc, q, c, kw)
                assert all(base[k].tobytes() == got[k].tobytes() for k in keys), (K, cname, cells)
            if kw["kind"] == "gaussian":
                # an uncensored cell does not know whether another cell of its list is censored (the list picks the kernel's instance)
                flag = kw["flag"] if kw.get("flag") is not None else rng.integers(-1, 2, n).astype(np.int8)
                mixed = call(eng, sq, sc, q, c, dict(kw, flag=flag))
                free = np.flatnonzero(flag == 0)
                assert 0 < len(free) < n
                for fl in (None, np.zeros(n, np.int8)):
                    alone = call(eng, sq, sc, q, c, dict(kw, flag=fl), free)
                    assert all(mixed[k][free].tobytes() == alone[k].tobytes() for k in keys), (K, cname, fl is None)
            bare = call(eng, sq, sc, q, c, kw, want=())
            assert bare["lpd"] is None and bare["mean"] is None and bare["std"] is None
            assert all(base[k].tobytes() == bare[k].tobytes() for k in ("elpd_loo", "khat")), (K, cname)
        # the traces entry point: permuted, doubled and in batches
        L = gaussian_traces(rng, 40, S, 1.5)
        base = eng.loo_traces(L)
        perm = rng.permutation(40)
        for cells in (1, 7, 0):
            eng.loo_batch_cells(cells)
            got = eng.loo_traces(np.concatenate([L[perm], L]))
            assert all(got[k].tobytes() == np.concatenate([base[k][perm], base[k]]).tobytes() for k in KEYS), cells
    finally:
        eng.loo_batch_cells(0)
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 5. refusals; a fp32 context ---------------------------------------------------------------------------------------------------------------

def test_loo_refusals(hip_engine_factory):
    K, S, nc = 8, 5, 30
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    try:
        with pytest.raises(bpmf_amd.BpmfHipError, match="loo_cells: no sample ring"):
            eng.loo_cells(sq, sc, 0.0, [0], [0], [1.0], 2.0)
        rng = np.random.default_rng(5)
        load(eng, sq, sc, *rings(rng, NQ, nc, S, K))
        with pytest.raises(bpmf_amd.BpmfHipError, match="no PSIS-LOO"):
            eng.loo_last_ms(sq)
        q, c, y = [0, 1, 2], [3, 4, 5], [1.0, 2.0, 3.0]

        def refused(match, *args, **kw):
            with pytest.raises(bpmf_amd.BpmfHipError, match=match) as e:
                eng.loo_cells(sq, sc, 0.0, *args, **kw)
            assert e.value.code == -1 and "\n" not in str(e.value).strip() and "loo_cells: " in str(e.value)
        refused("3 values of alpha for 5 samples", q, c, y, [1.0, 2.0, 3.0])
        refused("alpha of sample 1 is not finite and > 0", q, c, y, [1.0, 0.0, 1.0, 1.0, 1.0])
        refused("alpha of sample 0 is not finite and > 0", q, c, y, np.inf)
        refused(r"the weight of cell 1 \(1, 4\) is not finite and > 0", q, c, y, 2.0, w=[1.0, 0.0, 1.0])
        refused(r"the value of cell 2 \(2, 5\) is not finite", q, c, [1.0, 2.0, np.nan], 2.0)
        refused("nu must be finite and >= 1", q, c, y, 2.0, "student", 0.5)
        refused("flags go with the gaussian kind alone", q, c, y, 1.0, "probit", flag=[0, 1, 0])
        refused("flags go with the gaussian kind alone", q, c, y, 1.0, "student", 4.0, flag=[0, 1, 0])
        refused("weights go with the gaussian kind alone", q, c, y, 1.0, "student", 4.0, w=[1.0, 1.0, 1.0])
        refused(r"the flag 2 of cell 1 \(1, 4\) is not -1, 0 or \+1", q, c, y, 2.0, flag=[0, 2, 0])
        refused(r"cell 1 \(41, 4\) is out of range", [0, NQ, 2], c, y, 2.0)
        with pytest.raises(ValueError, match="kind must be one of"):
            eng.loo_cells(sq, sc, 0.0, q, c, y, 2.0, "poisson")
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        one = np.zeros(1, np.int32); out = np.zeros(1); al = np.ones(1)
        f = eng.lib.bpmf_hip_loo_cells
        ok = lambda *a: f(*a)
        assert ok(None, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, None, 0, 0.0, 1, ptr(al), ptr(out), ptr(out), None, None, None) == -1
        assert ok(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), None, None, None, 0, 0.0, 1, ptr(al), ptr(out), ptr(out), None, None, None) == -1
        assert ok(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, None, 0, 0.0, 1, None, ptr(out), ptr(out), None, None, None) == -1
        assert ok(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, None, 0, 0.0, 1, ptr(al), ptr(out), None, None, None, None) == -1
        assert ok(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, None, 7, 0.0, 1, ptr(al), ptr(out), ptr(out), None, None, None) == -1
        assert ok(sq.handle, sc.handle, 0.0, 0, None, None, None, None, None, 0, 0.0, 1, ptr(al), None, None, None, None, None) == 0
        assert ok(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, None, 0, 0.0, 1, ptr(al), ptr(out), ptr(out), None, None, None) == 0
        assert eng.lib.bpmf_hip_loo_batch_cells(-1) == -1
        # the traces
        g = eng.lib.bpmf_hip_loo_traces
        L = np.zeros((2, 3))
        assert g(None, 2, 3, ptr(L), ptr(L), ptr(L), None) == -1
        assert g(eng.ctx, -1, 3, ptr(L), ptr(L), ptr(L), None) == -1
        assert g(eng.ctx, 2, 0, ptr(L), ptr(L), ptr(L), None) == -1
        assert g(eng.ctx, 2, 4097, ptr(L), ptr(L), ptr(L), None) == -1 and b"4097 samples" in eng.lib.bpmf_hip_last_error()
        assert g(eng.ctx, 2, 3, None, ptr(L), ptr(L), None) == -1
        assert g(eng.ctx, 2, 3, ptr(L), None, ptr(L), None) == -1
        assert g(eng.ctx, 0, 3, None, None, None, None) == 0
        with pytest.raises(bpmf_amd.BpmfHipError, match="loo_traces: 4097 samples"):
            eng.loo_traces(np.zeros((1, 4097)))
        with pytest.raises(ValueError, match=r"L must be \[n, S\]"):
            eng.loo_traces(np.zeros((1, 2, 3)))
        assert eng.lib.bpmf_hip_abi_version() == 1
        got = eng.loo_cells(sq, sc, 0.0, q, c, y, 2.0)           # the context goes on working
        assert all(np.isfinite(got[k]).all() for k in ("elpd_loo", "lpd", "mean", "std")) and np.isposinf(got["khat"]).all() and eng.loo_last_ms(sq) >= 0.0
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)
    # more samples than the kernel sorts
    K, S = 4, 4097
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, 3, 2)
    try:
        load(eng, sq, sc, np.zeros((3, S, K)), np.zeros((2, S, K)))
        with pytest.raises(bpmf_amd.BpmfHipError, match="loo_cells: 4097 samples"):
            eng.loo_cells(sq, sc, 0.0, [0], [0], [1.0], 2.0)
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_fp32_context(hip_engine_factory):
    """the rings are fp64 on a fp32 context too"""
    K, S, nc, n = 128, 40, 20, 60
    eng = hip_engine_factory(K, "f32")
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    try:
        rng = np.random.default_rng(9)
        U, V = rings(rng, NQ, nc, S, K)
        load(eng, sq, sc, U, V)
        q, c = rng.integers(0, NQ, n), rng.integers(0, nc, n)
        y = 1.0 + np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1) + rng.standard_normal(n)
        kw = dict(kind="gaussian", y=y, alpha=2.0, mean=1.0)
        lr.held_to_reference(call(eng, sq, sc, q, c, kw), *log_densities(U, V, q, c, kw), "fp32 context")
        L = gaussian_traces(rng, 10, 100, 1.5)
        lr.held_to_reference(eng.loo_traces(L), L, tag="fp32 context, traces")
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 6. chains, models and the executable ------------------------------------------------------------------------------------------------------

CHAIN = dict(nsims=36, burnin=6)                                # 30 kept samples: M = 6, the tails are smoothed


@pytest.fixture(scope="module")
def ml100k():
    return util.ml100k()


@pytest.mark.parametrize("variant", ["plain", "robust"])
def test_gibbs_loo(hip_engine_factory, ml100k, variant):
    M, Mt, T, Tt, nu, nm = ml100k
    eng = hip_engine_factory(8)
    kw = dict(plain={}, robust=dict(robust=4.0))[variant]
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, loo=True, **CHAIN, **kw)
    info = res["model_info"]
    d = res["loo"]
    rows, cols = sr.cells_of(M)
    assert d["samples"] == 30 and d["kind"] == ("student" if variant == "robust" else "gaussian") and len(d["elpd_loo"]) == len(M[2])
    assert np.array_equal(d["rows"], rows) and np.array_equal(d["cols"], cols)
    assert d["p_loo"].tobytes() == (d["lpd"] - d["elpd_loo"]).tobytes() and d["summary"] == bpmf_amd.loo_summary(d)
    U, V = eng.samples_get(res["users"].side), eng.samples_get(res["movies"].side)
    sel = slice(None, None, 5)
    args = dict(kind=d["kind"], y=np.asarray(M[2], np.float64)[sel], alpha=info["alpha"], nu=info["nu"], mean=res["movies"].mean_rating)
    l64, lld = log_densities(U, V, rows[sel], cols[sel], args)
    used, g, err = lr.held_to_reference({k: d[k][sel] for k in KEYS}, l64, lld, variant)
    s = d["summary"]
    print("%s: share of the bar %r; %r" % (variant, used, s))
    assert s["n"] == len(M[2]) and s["looic"] == -2.0 * s["elpd_loo"] and s["p_loo"] > 0 and sum(s["khat_counts"].values()) == s["n"]
    # the chain is untouched
    plain = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, **CHAIN, **kw)
    assert "loo" not in plain and np.array(plain["rmse"]).tobytes() == np.array(res["rmse"]).tobytes() and plain["U"].tobytes() == res["U"].tobytes()


def run(args, cwd):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def final_line(d):
    s = d["summary"]
    return ("Final PSIS-LOO: looic %.4f elpd %.4f p_loo %.4f se %.4f (%d cells, %d samples, %.2f%% with k > 0.7)" %
            (s["looic"], s["elpd_loo"], s["p_loo"], s["se"], s["n"], s["samples"], 100.0 * s["khat_above_07"]))


def test_saved_model_and_cli(tmp_path, hip_engine_factory):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    bio.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    bio.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    for name in ("A", "B", "P"):
        os.mkdir(tmp_path / name)
    chain = ["-n", "train.sdm", "-p", "test.sdm", "-d", 8, "-i", CHAIN["nsims"], "-b", CHAIN["burnin"]]
    plain = run(chain + ["-o", "P"], tmp_path)
    a = run(chain + ["--loo", "-o", "A", "--save-model", "model"], tmp_path)
    assert "loo: PSIS-LOO cross-validation of the training cells\n" in a.stdout
    strip = lambda text: [ln for ln in text.splitlines() if not ln.startswith(("loo: ", "save-model: ", "Final PSIS-LOO", "Total time"))
                          and "items/sec" not in ln and "ratings/sec" not in ln]
    assert len(strip(a.stdout)) == len(strip(plain.stdout))
    assert sorted(set(os.listdir(tmp_path / "A")) - set(os.listdir(tmp_path / "P"))) == ["loo-elpd.sdm", "loo-khat.sdm"]
    lines = a.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("Final Avg RMSE: ")][0]
    # the Python run of the same chain gives the same figures, and its saved model the same bytes
    eng = hip_engine_factory(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, loo=True, alpha=2.0, save_model=str(tmp_path / "pymodel"), **CHAIN)
    d = res["loo"]
    assert lines[at + 1] == final_line(d)
    for name, key in (("loo-elpd.sdm", "elpd_loo"), ("loo-khat.sdm", "khat")):
        nr, ncol, E = bio.read_sparse(tmp_path / "A" / name)
        assert (nr, ncol) == (nu, nm) and np.array_equal(E[0], M[0]) and np.array_equal(E[1], M[1])
        assert np.asarray(E[2]).tobytes() == d[key].tobytes(), name
    rows, cols = sr.cells_of(M)
    serve = bpmf_amd.HipEngine(8)
    try:
        loaded = bpmf_amd.load_model(serve, str(tmp_path / "pymodel"))
        again = bpmf_amd.loo_cells(loaded, rows, cols, M[2])
        assert all(again[k].tobytes() == d[k].tobytes() for k in KEYS + ("p_loo", "mean", "std")) and again["summary"] == d["summary"]
    finally:
        serve.close()
    b = run(["--model", "model", "--loo", "-n", "train.sdm", "-o", "B"], tmp_path)
    for name in ("loo-elpd.sdm", "loo-khat.sdm"):
        assert (tmp_path / "B" / name).read_bytes() == (tmp_path / "A" / name).read_bytes()
    assert b.stdout.splitlines()[1:] == [final_line(d)] and b.stdout.startswith("model: model, ")
    assert sorted(os.listdir(tmp_path / "B")) == ["loo-elpd.sdm", "loo-khat.sdm"]
