"""Predictive intervals on the device: bpmf_hip_interval_traces / _cells, bpmf_amd.predict_intervals /
calibration_summary, gibbs(intervals=) and `bpmf --intervals` against tests/interval_ref.py.  Rings are filled through samples_set from
seeded numpy factors: no chain is needed for the kernel tests.

  1. the root finder on crafted traces (interval_traces): S in {1, 2, 7, 63, 64, 65, 129, 2048, 2049, 4096} (the lane-stride edges, the
     switch of waves per workgroup, the cap), n in {1, 3, 4, 5, 9} (the last workgroup partly live), the seven taus 0.001 .. 0.999 in
     one call, the six families of interval_ref.families.  The criterion is the residual in longdouble,
         |F_ld(q) - tau| <= (S / 64 + 32) 2^-53 + 4 f_ld(q) ulp(q)
     and for the pit the same with ulp(y) + ulp(max |p|).  Quantiles never decrease in tau; a trace with a NaN or an infinity gives NaN
     for that trace alone and the neighbours keep their bytes.
  2. cells through the rings: K in {4, 36, 128}, S in {1, 9, 200}, the lists of tests/test_gpu_score.py; mean and std are the bytes of
     predict_cells; pit and quantiles against longdouble predictions from U, V by the bound of 1 plus the trace's own rounding
     f_ld (K + 2) 2^-53 max_s sum_k |u_k v_k|
  3. the bits depend on the cell alone: a permuted list, repeated cells, batches of 1, 3 and automatic, two calls, with or without y
  4. every refusal of the C entry points names its offender
  5. gibbs(intervals=(0.5, 0.9)) on ml-100k: plain, noise="adaptive" (alpha per sample) against the reference from samples_get;
     bias=True (samples_get does not read such a side) against engine.interval_cells on the run's rings
  6. / 7. `bpmf --intervals`: both Final lines equal calibration_summary of the pit column of intervals.csv, the file equals the Python
     run; without the flag stdout and the other files are what they were; a saved model serves byte-identical intervals.csv
  8. the rings of a chain on planted continuous data scored with the run's alpha and with 4 alpha: the over-confident model covers
     less at 90 % and has a larger KS distance (the honest coverage is printed, not asserted); and values drawn from the predictive
     of hand-filled rings itself, calibrated by construction, are covered at 50 / 80 / 90 / 95 % within 5 binomial standard errors

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import bpmf_amd
from bpmf_amd import io as bio
from tests import interval_ref as ir
from tests import model_ref as mr
from tests import score_ref as sr
from tests import util
from tests.conftest import ROOT
from tests.test_gpu_score import NQ, lists, load, rings, segment

pytestmark = pytest.mark.gpu

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
LD = np.longdouble

# n per S: every n at the small sizes; at the large ones a full and a partly live last workgroup (4 waves up to 2048, then 2)
N_OF = {1: (1, 3, 4, 5, 9), 2: (1, 3, 4, 5, 9), 7: (1, 3, 4, 5, 9), 63: (1, 3, 4, 5, 9), 64: (1, 3, 4, 5, 9), 65: (1, 3, 4, 5, 9),
        129: (1, 3, 4, 5, 9), 2048: (4, 5), 2049: (3,), 4096: (1, 4)}


# ---- 1. the root finder --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", sorted(N_OF))
def test_root_finder_on_crafted_traces(hip_engine_factory, S):
    eng = hip_engine_factory(8)
    worst_q = worst_p = 0.0
    for n in N_OF[S]:
        rng = np.random.default_rng(100 * S + n)
        for name, fam in ir.families(rng, n, S).items():
            D, alpha, w = fam["D"], fam["alpha"], fam["w"]
            sd = 1.0 / np.sqrt(np.min(alpha) * (1.0 if w is None else w))
            y = D[:, 0] + sd * rng.standard_normal(n)
            pit, quant = eng.interval_traces(D, alpha, ir.TAUS, y=y, w=w)
            tag = "S %d n %d %s" % (S, n, name)
            assert pit.shape == (n,) and quant.shape == (n, len(ir.TAUS)), tag
            assert np.isfinite(pit).all() and np.isfinite(quant).all() and (np.diff(quant, axis=1) >= 0).all(), tag
            for j, tau in enumerate(ir.TAUS):
                res, bound = ir.quantile_residual(D, alpha, tau, quant[:, j], w=w)
                print("%s tau %g: residual %.3g bound %.3g" % (tag, tau, res.max(), bound[np.argmax(res / bound)]))
                assert (res <= bound).all(), (tag, tau, res, bound)
                worst_q = max(worst_q, float((res / bound).max()))
            res, bound = ir.pit_residual(D, alpha, y, pit, w=w)
            assert (res <= bound).all(), (tag, "pit", res, bound)
            worst_p = max(worst_p, float((res / bound).max()))
            # without y, and the quantiles alone in two calls: the same bytes
            none, again = eng.interval_traces(D, alpha, ir.TAUS, w=w)
            assert none is None and again.tobytes() == quant.tobytes(), tag
            only, empty = eng.interval_traces(D, alpha, (), y=y, w=w)
            assert only.tobytes() == pit.tobytes() and empty.shape == (n, 0), tag
    print("S %d: residual / bound at most %.3f (quantiles) %.3f (pit)" % (S, worst_q, worst_p))


@pytest.mark.parametrize("S", [1, 65, 2049])
def test_a_trace_that_is_not_finite_gives_nan_for_itself_alone(hip_engine_factory, S):
    eng = hip_engine_factory(8)
    rng = np.random.default_rng(S)
    n = 9
    D = rng.standard_normal((n, S))
    y = rng.standard_normal(n)
    taus = (0.05, 0.5, 0.95)
    pit, quant = eng.interval_traces(D, 2.0, taus, y=y)
    bad = D.copy()
    bad[1, S - 1] = np.nan; bad[4, 0] = np.inf; bad[5, S // 2] = -np.inf; bad[8, :] = np.nan
    pit_b, quant_b = eng.interval_traces(bad, 2.0, taus, y=y)
    hit = np.zeros(n, bool); hit[[1, 4, 5, 8]] = True
    assert np.isnan(pit_b[hit]).all() and np.isnan(quant_b[hit]).all()
    assert pit_b[~hit].tobytes() == pit[~hit].tobytes() and quant_b[~hit].tobytes() == quant[~hit].tobytes()
    assert np.isfinite(eng.interval_traces(D, 2.0, taus, y=y)[0]).all()           # the context goes on working


# ---- 2. cells through the rings ------------------------------------------------------------------------------------------------------------

def traces_ld(U, V, q, c):
    """(D [n, S] longdouble, amax [n] = max_s sum_k |u_k v_k|), in chunks of cells"""
    D = np.empty((len(q), U.shape[1]), LD); amax = np.empty(len(q))
    for i0 in range(0, len(q), 64):
        P = U[q[i0:i0 + 64]].astype(LD) * V[c[i0:i0 + 64]].astype(LD)
        D[i0:i0 + 64] = P.sum(axis=2)
        amax[i0:i0 + 64] = np.abs(P).sum(axis=2).max(axis=1).astype(np.float64)
    return D, amax


def held_to_reference(got, D, amax, K, mean, alpha, taus, y, w, tag):
    """pit and quant of one call against the longdouble mixture around the longdouble traces D: (worst residual / bound)"""
    S = D.shape[1]
    r = ir.rates(alpha, w, S)
    worst = 0.0
    own = (K + 2) * ir.EPS * amax                                    # the trace's own rounding, times f
    for j, tau in enumerate(taus):
        qd = got["quant"][:, j]
        F, f = ir.mixture(qd.astype(LD) - LD(mean), D, r)
        res = np.abs(F - LD(tau)).astype(np.float64)
        bound = ir.residual_bound(S, f, ir.ulp(qd)) + f.astype(np.float64) * own
        assert (res <= bound).all(), (tag, tau, res.max(), bound[np.argmax(res / bound)])
        worst = max(worst, float((res / bound).max()))
    F, f = ir.mixture(np.asarray(y, LD) - LD(mean), D, r)
    res = np.abs(F - got["pit"].astype(LD)).astype(np.float64)
    pmax = np.abs(D.astype(np.float64) + mean).max(axis=1)
    bound = ir.residual_bound(S, f, ir.ulp(y) + ir.ulp(pmax)) + f.astype(np.float64) * own
    assert (res <= bound).all(), (tag, "pit", res.max(), bound[np.argmax(res / bound)])
    return max(worst, float((res / bound).max()))


LEVELS = (0.5, 0.9)
LEVEL_TAUS = tuple((1.0 + sg * l) / 2.0 for sg, l in ((-1, 0.9), (-1, 0.5), (1, 0.5), (1, 0.9)))   # the ends of the central 50 % and 90 % intervals, as predict_intervals forms them


@pytest.mark.parametrize("K", [4, 36, 128])
def test_interval_cells_against_longdouble(hip_engine_factory, K):
    """mean 16.5: |q| >= |q - mean| for every quantile, so that ulp(q) of the bound covers the rounding of the root too"""
    eng = hip_engine_factory(K)
    nc = segment(K) + 8
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    mean = 0.0 if K == 36 else 16.5
    try:
        for S in (1, 9, 200):
            rng = np.random.default_rng(1000 * K + S)
            U, V = rings(rng, NQ, nc, S, K)
            load(eng, sq, sc, U, V)
            L = lists(rng, K, nc)
            for lname, (q, c) in L.items():
                n = len(q)
                alpha = 2.0 if lname in ("segment", "empty") else 1.0 + rng.random(S)
                w = None if lname in ("segment", "single") else 0.25 + 4.0 * rng.random(n)
                p = mean + np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1)
                y = p + rng.standard_normal(n) / np.sqrt(2.0)
                got = eng.interval_cells(sq, sc, mean, q, c, alpha, LEVEL_TAUS, y=y, w=w)
                tag = "K %d S %d %s" % (K, S, lname)
                assert sorted(got) == ["mean", "pit", "quant", "std"] and got["quant"].shape == (n, 4) and got["pit"].shape == (n,), tag
                pm, ps = eng.predict_cells(sq, sc, mean, q, c)
                assert got["mean"].tobytes() == pm.tobytes() and got["std"].tobytes() == ps.tobytes(), tag
                if n == 0:
                    continue
                assert (np.diff(got["quant"], axis=1) >= 0).all() and ((got["pit"] > 0) & (got["pit"] < 1)).all(), tag
                D, amax = traces_ld(U, V, q, c)
                worst = held_to_reference(got, D, amax, K, mean, alpha, LEVEL_TAUS, y, w, tag)
                print("%s: %d cells, residual / bound at most %.3f" % (tag, n, worst))
        assert eng.interval_last_ms(sq) >= 0.0
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 3. independence -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [4, 20, 128])
def test_bits_depend_on_the_cell_alone(hip_engine_factory, K):
    eng = hip_engine_factory(K)
    Kp = (K + 3) // 4 * 4
    nc, S = segment(Kp) + 8, 11
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    keys = ("pit", "quant", "mean", "std")
    try:
        rng = np.random.default_rng(K)
        U, V = rings(rng, NQ, nc, S, K)
        load(eng, sq, sc, U, V)
        L = lists(rng, Kp, nc)
        q, c = (np.concatenate([L[k][i] for k in ("segment1", "many", "single")]) for i in (0, 1))
        n = len(q)
        y = 0.5 + np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1) + rng.standard_normal(n)
        w = 0.25 + 4.0 * rng.random(n)
        alpha = 1.0 + rng.random(S)
        call = lambda idx: eng.interval_cells(sq, sc, 0.5, q[idx], c[idx], alpha, LEVEL_TAUS, y=y[idx], w=w[idx])
        every = np.arange(n)
        base = call(every)
        again = call(every)
        assert all(base[k].tobytes() == again[k].tobytes() for k in keys), K
        perm = rng.permutation(n)
        got = call(perm)
        assert all(base[k][perm].tobytes() == got[k].tobytes() for k in keys), K
        twice = np.repeat(every, 2)
        got = call(twice)
        assert all(base[k][twice].tobytes() == got[k].tobytes() for k in keys), K
        for cells in (1, 3, 0):
            eng.interval_batch_cells(cells)
            sel = every[:40] if cells == 1 else every                # (a launch per cell: a part of the list)
            got = call(sel)
            assert all(base[k][sel].tobytes() == got[k].tobytes() for k in keys), (K, cells)
        eng.interval_batch_cells(3)                                  # without y: the same quantiles, no pit
        got = eng.interval_cells(sq, sc, 0.5, q, c, alpha, LEVEL_TAUS, w=w)
        assert got["pit"] is None and got["quant"].tobytes() == base["quant"].tobytes()
        got = eng.interval_cells(sq, sc, 0.5, q, c, alpha, (), y=y, w=w)
        assert got["pit"].tobytes() == base["pit"].tobytes() and got["quant"].shape == (n, 0)
    finally:
        eng.interval_batch_cells(0)
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_interval_refusals(hip_engine_factory):
    K, S, nc = 8, 5, 30
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    try:
        with pytest.raises(bpmf_amd.BpmfHipError, match="interval_cells: no sample ring"):
            eng.interval_cells(sq, sc, 0.0, [0], [0], 2.0, (0.5,))
        rng = np.random.default_rng(5)
        load(eng, sq, sc, *rings(rng, NQ, nc, S, K))
        with pytest.raises(bpmf_amd.BpmfHipError, match="no intervals"):
            eng.interval_last_ms(sq)
        q, c, y = [0, 1, 2], [3, 4, 5], [1.0, 2.0, 3.0]
        D = rng.standard_normal((3, S))

        def refused(match, *args, **kw):
            """by both entry points: the cells' line names the cell, the traces' line the trace"""
            for who, f in (("interval_cells", lambda: eng.interval_cells(sq, sc, 0.0, q, c, *args, **kw)), ("interval_traces", lambda: eng.interval_traces(D, *args, **kw))):
                with pytest.raises(bpmf_amd.BpmfHipError, match=who + ": " + match.replace("ITEM", r"cell 1 \(1, 4\)" if who == "interval_cells" else "trace 1")) as e:
                    f()
                assert e.value.code == -1 and "\n" not in str(e.value).strip()
        refused(r"nq = 9 quantiles \(0 .. 8\)", 2.0, np.linspace(0.1, 0.9, 9))
        refused(r"nothing to do \(y is NULL and nq = 0\)", 2.0, ())
        refused(r"tau 0 is outside \[0.001, 0.999\]", 2.0, (0.0005, 0.5))
        refused(r"tau 1 is outside \[0.001, 0.999\]", 2.0, (0.5, 0.9995))
        refused(r"tau 1 is outside \[0.001, 0.999\]", 2.0, (0.5, np.nan))
        refused(r"tau 2 is not above tau 1 \(strictly increasing\)", 2.0, (0.1, 0.5, 0.5))
        refused(r"tau 1 is not above tau 0 \(strictly increasing\)", 2.0, (0.5, 0.1))
        refused("3 values of alpha for 5 samples", [1.0, 2.0, 3.0], (0.5,))
        refused("alpha of sample 1 is not finite and > 0", [1.0, 0.0, 1.0, 1.0, 1.0], (0.5,))
        refused("alpha of sample 0 is not finite and > 0", np.inf, (0.5,))
        refused("the weight of ITEM is not finite and > 0", 2.0, (0.5,), w=[1.0, 0.0, 1.0])
        refused("the weight of ITEM is not finite and > 0", 2.0, (0.5,), w=[1.0, np.nan, 1.0])
        refused("the value of ITEM is not finite", 2.0, (0.5,), y=[1.0, np.inf, 3.0])
        with pytest.raises(bpmf_amd.BpmfHipError, match=r"interval_cells: cell 1 \(41, 4\) is out of range"):
            eng.interval_cells(sq, sc, 0.0, [0, NQ, 2], c, 2.0, (0.5,))
        with pytest.raises(bpmf_amd.BpmfHipError, match=r"interval_traces: 4097 samples: the root finder takes 1 .. 4096"):
            eng.interval_traces(np.zeros((1, 4097)), 2.0, (0.5,))
        with pytest.raises(ValueError, match="one value per item"):
            eng.interval_cells(sq, sc, 0.0, q, c, 2.0, (0.5,), y=[1.0])
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        one = np.zeros(1, np.int32); out = np.zeros(8); al = np.ones(1); tau = np.array([0.5])
        f = eng.lib.bpmf_hip_interval_cells
        ok = lambda: (sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), None, 1, ptr(al), 1, ptr(tau), ptr(out), ptr(out), ptr(out), ptr(out))
        swap = lambda at, v: tuple(v if i == at else a for i, a in enumerate(ok()))
        assert f(*ok()) == 0
        for at, v, line in ((0, None, "NULL"), (9, None, "interval_cells: NULL alpha"), (11, None, "interval_cells: NULL tau"),
                            (12, None, "interval_cells: NULL pit output with y given"), (13, None, "interval_cells: NULL quantile output with nq > 0"),
                            (8, 0, "interval_cells: nalpha must be 1 or the number of samples"), (10, -1, "interval_cells: nq = -1 quantiles")):
            assert f(*swap(at, v)) == -1 and line in eng.lib.bpmf_hip_last_error().decode(), (at, eng.lib.bpmf_hip_last_error())
        assert f(*swap(14, None)) == 0 and f(*swap(15, None)) == 0                     # mean and std may be left out
        assert f(sq.handle, sc.handle, 0.0, 0, None, None, None, None, 1, ptr(al), 1, ptr(tau), None, None, None, None) == 0
        g = eng.lib.bpmf_hip_interval_traces
        assert g(None, 1, 5, ptr(out), 0.0, ptr(out), None, 1, ptr(al), 1, ptr(tau), ptr(out), ptr(out)) == -1
        assert g(eng.ctx, 1, 5, None, 0.0, ptr(out), None, 1, ptr(al), 1, ptr(tau), ptr(out), ptr(out)) == -1
        assert b"interval_traces: NULL traces" in eng.lib.bpmf_hip_last_error()
        assert g(eng.ctx, 1, 0, ptr(out), 0.0, ptr(out), None, 1, ptr(al), 1, ptr(tau), ptr(out), ptr(out)) == -1
        assert g(eng.ctx, 0, 5, None, 0.0, None, None, 1, ptr(al), 1, ptr(tau), None, None) == 0
        assert eng.lib.bpmf_hip_interval_batch_cells(-1) == -1
        assert eng.lib.bpmf_hip_abi_version() == 1
        got = eng.interval_cells(sq, sc, 0.0, q, c, 2.0, (0.5,), y=y)                 # the context goes on working
        assert np.isfinite(got["pit"]).all() and np.isfinite(got["quant"]).all() and eng.interval_last_ms(sq) >= 0.0
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_fp32_context(hip_engine_factory):
    """the rings are fp64 on a fp32 context too"""
    K, S, nc = 128, 7, 20
    eng = hip_engine_factory(K, "f32")
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    try:
        rng = np.random.default_rng(9)
        U, V = rings(rng, NQ, nc, S, K)
        load(eng, sq, sc, U, V)
        q, c = rng.integers(0, NQ, 50), rng.integers(0, nc, 50)
        y = 1.0 + np.einsum("nsk,nsk->ns", U[q], V[c]).mean(axis=1)
        got = eng.interval_cells(sq, sc, 1.0, q, c, 2.0, LEVEL_TAUS, y=y)
        D, amax = traces_ld(U, V, q, c)
        held_to_reference(got, D, amax, K, 1.0, 2.0, LEVEL_TAUS, y, None, "fp32 context")
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 5. through gibbs ----------------------------------------------------------------------------------------------------------------------

CHAIN = dict(nsims=10, burnin=4)


@pytest.fixture(scope="module")
def ml100k():
    return util.ml100k()


def check_result(d, rows, cols, S):
    assert d["samples"] == S and d["levels"] == list(LEVELS) and np.array_equal(d["rows"], rows) and np.array_equal(d["cols"], cols)
    n = len(rows)
    assert d["lo"].shape == d["hi"].shape == (n, 2) and d["pit"].shape == (n,)
    assert (d["lo"][:, 1] <= d["lo"][:, 0]).all() and (d["lo"][:, 0] <= d["hi"][:, 0]).all() and (d["hi"][:, 0] <= d["hi"][:, 1]).all()
    s = d["summary"]
    want = bpmf_amd.calibration_summary(d["pit"], LEVELS, d["lo"], d["hi"])
    assert s["hist"].tolist() == want["hist"].tolist() and {k: v for k, v in s.items() if k != "hist"} == {k: v for k, v in want.items() if k != "hist"}
    return s


@pytest.mark.parametrize("variant", ["plain", "adaptive"])
def test_gibbs_intervals(hip_engine_factory, ml100k, variant):
    M, Mt, T, Tt, nu, nm = ml100k
    eng = hip_engine_factory(8)
    kw = dict(plain={}, adaptive=dict(noise="adaptive"))[variant]
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, intervals=LEVELS, **CHAIN, **kw)
    info = res["model_info"]
    if variant == "adaptive":
        alpha = np.array(res["alpha"][4:10])
        assert info["alpha_samples"] == list(alpha) and len(set(alpha)) == 6
    else:
        alpha = info["alpha"]
    assert sorted(res["intervals"]) == ["test"]
    d = res["intervals"]["test"]
    rows, cols = sr.cells_of(T)
    s = check_result(d, rows, cols, 6)
    y = np.asarray(T[2], np.float64)
    # the pit says where the value lies: inside the central interval exactly when |pit - 1/2| <= l / 2 (up to the roots' own rounding)
    for k, l in enumerate(LEVELS):
        inside = (d["lo"][:, k] <= y) & (y <= d["hi"][:, k])
        by_pit = np.abs(d["pit"] - 0.5) <= 0.5 * l
        assert (inside != by_pit).mean() < 1e-3 and abs(inside.mean() - s["coverage"][k]) < 1e-3
    print("%s: coverage %s (se %s) width %s KS %.3f over %d cells" % (variant, s["coverage"], s["se"], s["width"], s["ks"], s["n"]))
    U, V = eng.samples_get(res["users"].side), eng.samples_get(res["movies"].side)
    sel = slice(None, None, 5)
    D, amax = traces_ld(U, V, rows[sel], cols[sel])
    got = dict(pit=d["pit"][sel], quant=np.stack([d["lo"][sel, 1], d["lo"][sel, 0], d["hi"][sel, 0], d["hi"][sel, 1]], axis=1))
    worst = held_to_reference(got, D, amax, 8, res["movies"].mean_rating, alpha, LEVEL_TAUS, y[sel], None, variant)
    print("%s: residual / bound at most %.3f" % (variant, worst))
    pm, ps = eng.predict_cells(res["users"].side, res["movies"].side, res["movies"].mean_rating, rows, cols)
    assert d["mean"].tobytes() == pm.tobytes() and d["std"].tobytes() == ps.tobytes()
    if variant == "adaptive":                                        # a single alpha is another figure
        first = eng.interval_cells(res["users"].side, res["movies"].side, res["movies"].mean_rating, rows, cols, res["alpha"][0], LEVEL_TAUS, y=y)
        assert np.abs(first["pit"] - d["pit"]).max() > 1e-6
    # the chain is untouched, and intervals=True is the 90 % level
    plain = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, **CHAIN, **kw)
    assert "intervals" not in plain and np.array(plain["rmse"]).tobytes() == np.array(res["rmse"]).tobytes() and plain["U"].tobytes() == res["U"].tobytes()
    if variant == "plain":
        one = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, intervals=True, **CHAIN)["intervals"]["test"]
        assert one["levels"] == [0.9] and one["pit"].tobytes() == d["pit"].tobytes()
        assert np.abs(one["lo"][:, 0] - d["lo"][:, 1]).max() < 1e-12 and np.abs(one["hi"][:, 0] - d["hi"][:, 1]).max() < 1e-12


def test_gibbs_intervals_with_biases(hip_engine_factory, ml100k):
    """the widened rings: samples_get does not read a side with bias terms, so the bias rows are held to the reference on hand-filled
    rings (p_s = mean + u . v + b + c) and the chain to engine.interval_cells on its own rings"""
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
        D, amax = traces_ld(U, V, q, c)
        y = 16.5 + D.astype(np.float64).mean(axis=1) + extra.mean(axis=1) + rng.standard_normal(len(q)) / np.sqrt(2.0)
        got = eng.interval_cells(sq, sc, 16.5, q, c, 2.0, LEVEL_TAUS, y=y)
        held_to_reference(got, D + extra.astype(LD), amax + np.abs(extra).max(axis=1), K + 2, 16.5, 2.0, LEVEL_TAUS, y, None, "bias rows")
        without = ir.pit(D, 2.0, y, mean=16.5).astype(np.float64)
        assert np.abs(got["pit"] - without).max() > 1e-3                              # the bias rows of the rings are read
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)
    M, Mt, T, Tt, nu, nm = ml100k
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, intervals=LEVELS, bias=True, **CHAIN)
    rows, cols = sr.cells_of(T)
    d = res["intervals"]["test"]
    check_result(d, rows, cols, 6)
    direct = eng.interval_cells(res["users"].side, res["movies"].side, res["movies"].mean_rating, rows, cols, res["model_info"]["alpha"], LEVEL_TAUS, y=T[2])
    assert d["pit"].tobytes() == direct["pit"].tobytes() and d["lo"].tobytes() == direct["quant"][:, [1, 0]].tobytes()
    assert d["hi"].tobytes() == direct["quant"][:, [2, 3]].tobytes() and np.isfinite(d["lo"]).all() and np.isfinite(d["hi"]).all()
    pm, _ = eng.predict_cells(res["users"].side, res["movies"].side, res["movies"].mean_rating, rows, cols)
    assert d["mean"].tobytes() == pm.tobytes()


# ---- 6. and 7. the executable and a saved model --------------------------------------------------------------------------------------------

def run(args, cwd):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def final_lines(d):
    """the Final lines bpmf prints for res["intervals"]["test"]"""
    s = d["summary"]
    parts = ["%.10g%%: %.3f (se %.3f, width %.2f)" % (100.0 * l, c, e, w) for l, c, e, w in zip(s["levels"], s["coverage"], s["se"], s["width"])]
    return ["Final coverage: " + " ".join(parts) + " (%d cells, %d samples)" % (s["n"], d["samples"]), "Final PIT: KS %.3f" % s["ks"]]


def read_intervals(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "row,col,value,mean,std,pit,lo50,hi50,lo90,hi90"
    return np.array([ln.split(",") for ln in lines[1:]], dtype=float).reshape(-1, 10)


@pytest.mark.parametrize("variant", ["plain", "adaptive"])
def test_cli_intervals(tmp_path, hip_engine_factory, variant):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    bio.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    bio.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    for name in ("A", "B", "P"):
        os.mkdir(tmp_path / name)
    flags, kw = (["--noise", "adaptive"], dict(noise="adaptive")) if variant == "adaptive" else ([], {})
    chain = ["-n", "train.sdm", "-p", "test.sdm", "-d", 8, "-i", 10, "-b", 4] + flags
    plain = run(chain + ["-o", "P"], tmp_path)
    a = run(chain + ["--intervals", "0.5,0.9", "-o", "A", "--save-model", "model"], tmp_path)
    assert "intervals: central predictive intervals of the test cells at 50% 90%, and the calibration of their held-out values\n" in a.stdout
    # without the flag: stdout and the files are what they were
    new = ("intervals: ", "save-model: ", "Final coverage", "Final PIT", "Total time")
    strip = lambda text: [ln for ln in text.splitlines() if not ln.startswith(new) and "items/sec" not in ln and "ratings/sec" not in ln]
    assert len(strip(a.stdout)) == len(strip(plain.stdout)) and not any(ln.startswith(new[:1] + new[2:4]) for ln in plain.stdout.splitlines())
    assert [ln for ln in a.stdout.splitlines() if ln.startswith("Final Avg RMSE")] == [ln for ln in plain.stdout.splitlines() if ln.startswith("Final Avg RMSE")]
    assert sorted(set(os.listdir(tmp_path / "A")) - set(os.listdir(tmp_path / "P"))) == ["intervals.csv"]
    for name in os.listdir(tmp_path / "P"):
        assert (tmp_path / "A" / name).read_bytes() == (tmp_path / "P" / name).read_bytes(), name
    lines = a.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("Final Avg RMSE: ")][0]
    rec = read_intervals(tmp_path / "A" / "intervals.csv")
    rows, cols = sr.cells_of(T)
    assert np.array_equal(rec[:, 0], rows + 1) and np.array_equal(rec[:, 1], cols + 1) and rec[:, 2].tobytes() == np.asarray(T[2]).tobytes()
    # both lines parse and equal calibration_summary of the file
    s = bpmf_amd.calibration_summary(rec[:, 5], LEVELS, rec[:, [6, 8]], rec[:, [7, 9]])
    assert lines[at + 1:at + 3] == final_lines(dict(summary=s, samples=6))
    import re
    m = re.fullmatch(r"Final coverage: 50%: ([01]\.\d{3}) \(se (0\.\d{3}), width (\d+\.\d{2})\) 90%: ([01]\.\d{3}) \(se (0\.\d{3}), width (\d+\.\d{2})\) \((\d+) cells, 6 samples\)", lines[at + 1])
    assert m and int(m.group(7)) == len(rows) and re.fullmatch(r"Final PIT: KS 0\.\d{3}", lines[at + 2]), lines[at + 1:at + 3]
    # the Python run of the same chain gives the same file
    eng = hip_engine_factory(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, intervals=LEVELS, alpha=2.0, **CHAIN, **kw)
    d = res["intervals"]["test"]
    for j, v in ((3, d["mean"]), (4, d["std"]), (5, d["pit"]), (6, d["lo"][:, 0]), (7, d["hi"][:, 0]), (8, d["lo"][:, 1]), (9, d["hi"][:, 1])):
        assert rec[:, j].tobytes() == np.ascontiguousarray(v).tobytes(), j
    assert lines[at + 1:at + 3] == final_lines(d)
    # a saved model serves the same file for the same cells
    b = run(["--model", "model", "--predict", "test.sdm", "--intervals", "0.5,0.9", "-o", "B"], tmp_path)
    assert (tmp_path / "B" / "intervals.csv").read_bytes() == (tmp_path / "A" / "intervals.csv").read_bytes()
    assert b.stdout.splitlines()[1:] == final_lines(d) and sorted(os.listdir(tmp_path / "B")) == ["intervals.csv", "predict.csv"]
    os.mkdir(tmp_path / "C")
    run(["--model", "model", "--predict", "test.sdm", "-o", "C"], tmp_path)
    assert (tmp_path / "C" / "predict.csv").read_bytes() == (tmp_path / "B" / "predict.csv").read_bytes()
    # and the loaded model in Python
    serve = bpmf_amd.HipEngine(8)
    try:
        loaded = bpmf_amd.load_model(serve, str(tmp_path / "model"))
        again = bpmf_amd.predict_intervals(loaded, rows, cols, LEVELS, values=T[2])
        assert all(again[k].tobytes() == d[k].tobytes() for k in ("pit", "lo", "hi", "mean", "std"))
    finally:
        serve.close()


# ---- 8. an over-confident model ------------------------------------------------------------------------------------------------------------

def planted(nusers=120, nmovies=80, rank=2, density=0.3, alpha=2.0, seed=21):
    """a planted low-rank matrix with continuous values (noise of precision alpha), a fifth of the cells held out: (M, Mt, T, Tt)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    A, B = rng.standard_normal((nusers, rank)), rng.standard_normal((nmovies, rank))
    r, c = np.nonzero(rng.random((nusers, nmovies)) < density)
    v = 3.0 + (A[r] * B[c]).sum(axis=1) / np.sqrt(rank) + rng.standard_normal(len(r)) / np.sqrt(alpha)
    test = rng.random(len(r)) < 0.2
    mat = lambda sel, rows, cols, shape: util.csc_arrays(sp.coo_matrix((v[sel], (rows[sel], cols[sel])), shape=shape).tocsc())
    return (mat(~test, r, c, (nusers, nmovies)), mat(~test, c, r, (nmovies, nusers)), mat(test, r, c, (nusers, nmovies)), mat(test, c, r, (nmovies, nusers)))


def test_an_overconfident_model_covers_less(hip_engine_factory):
    """The rings of one chain on planted continuous data, scored with the run's alpha and with 4 alpha (half the noise standard
    deviation).  The honest coverage is reported, not asserted: a chain of test length is not a calibrated posterior."""
    M, Mt, T, Tt = planted()
    eng = hip_engine_factory(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, 120, 80, Tt=Tt, alpha=2.0, intervals=(0.9,), nsims=24, burnin=8)
    honest = res["intervals"]["test"]
    res["model_info"] = dict(res["model_info"], alpha=4.0 * res["model_info"]["alpha"])
    rows, cols = sr.cells_of(T)
    over = bpmf_amd.predict_intervals(res, rows, cols, (0.9,), values=T[2])
    h, o = honest["summary"], over["summary"]
    print("90%%: honest coverage %.3f (se %.3f) width %.2f KS %.3f; 4 alpha: coverage %.3f width %.2f KS %.3f (%d cells, %d samples)" %
          (h["coverage"][0], h["se"][0], h["width"][0], h["ks"], o["coverage"][0], o["width"][0], o["ks"], h["n"], honest["samples"]))
    assert o["coverage"][0] < h["coverage"][0] - 5 * h["se"][0] and o["ks"] > h["ks"] and o["width"][0] < h["width"][0]
    assert over["mean"].tobytes() == honest["mean"].tobytes()


def test_values_drawn_from_the_predictive_are_covered_at_the_level(hip_engine_factory):
    """Calibrated by construction: y is drawn from the mixture the rings and alpha define (a sample picked at random, then the noise),
    so every pit is uniform: the coverage of every level within 5 binomial standard errors, the Kolmogorov distance below the 1e-6
    quantile of its null distribution, sqrt(-log(5e-7) / 2n)."""
    K, S, nc, n = 8, 40, 50, 20000
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, nc)
    try:
        rng = np.random.default_rng(77)
        U, V = rings(rng, NQ, nc, S, K)
        load(eng, sq, sc, U, V)
        q, c = rng.integers(0, NQ, n), rng.integers(0, nc, n)
        alpha = 1.0 + rng.random(S)
        pick = rng.integers(0, S, n)
        y = 2.5 + np.einsum("nk,nk->n", U[q, pick], V[c, pick]) + rng.standard_normal(n) / np.sqrt(alpha[pick])
        levels = (0.5, 0.8, 0.9, 0.95)
        taus = sorted([(1 - l) / 2 for l in levels] + [(1 + l) / 2 for l in levels])
        got = eng.interval_cells(sq, sc, 2.5, q, c, alpha, taus, y=y)
        s = bpmf_amd.calibration_summary(got["pit"], levels, got["quant"][:, [3, 2, 1, 0]], got["quant"][:, [4, 5, 6, 7]])
        print("calibrated by construction: coverage %s (se %s) width %s KS %.4f" % (s["coverage"], s["se"], s["width"], s["ks"]))
        assert all(abs(cv - l) <= 5 * e for cv, l, e in zip(s["coverage"], levels, s["se"])) and s["ks"] < np.sqrt(-np.log(5e-7) / (2 * n))
        inside = (got["quant"][:, 1] <= y) & (y <= got["quant"][:, 6])               # the 90 % interval itself agrees with the pits
        assert abs(inside.mean() - s["coverage"][2]) < 1e-3
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)
