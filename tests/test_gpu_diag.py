"""Convergence diagnostics on the device: bpmf_hip_diag_traces, bpmf_hip_diag_cells, gibbs(diagnose=),
bpmf_amd.diagnose and bpmf --diagnose against tests/diag_ref.py.

  1. diag_traces against the longdouble reference: S in {8, 9, 15, 16, 63, 64, 65, 127, 128, 129, 257, 1000, 4096}, lists of 1, 3, 64 and
     257 traces; iid normal, AR(1) with rho in {0.5, 0.9, 0.99, -0.5}, shifted halves (the loop runs to the lag limit), 1e8 + N(0, 1),
     values scaled by 4^20 and 4^-20, constant (NaN on both), one NaN inside (NaN out, the call returns).  Tolerance per kind, for rhat
     and for ess: 8 x the largest relative error of the fp64 restatement against longdouble over that kind's traces, not less than
     1e-12 (the convention of tests/test_gpu_posterior_outputs.py).  Refusals: S = 7, S = 4097, NULL.
  2. bits: a trace gives equal bytes at another place in the list, in a list of 1 and of 257 and on a second call; diag_cells with
     batches of 1 cell, 7 cells and automatic gives equal bytes
  3. diag_cells on planted rings (samples_set; 70 queries x 130 candidates as tests/test_gpu_model.py; an AR(1) recursion over s per
     factor entry): K in {1, 8, 20, 32, 64, 128}, S in {8, 65}; an empty list, one cell, every cell of one query five times over, the last
     row and column, a random list; mean and std byte-equal to predict_cells, rhat and ess within the tolerance of 1 of diag_ref on
     the longdouble traces of samples_get; an fp32 context; a pair of sides with biases against u . v + b + c; every refusal
     predict_cells has, and S < 8
  4. gibbs(diagnose=True) on the 60 x 40 matrix of tests/model_ref.py, K = 8, nsims = 40, burnin = 8: res["diag"] is engine.diag_cells
     on the final rings byte for byte, summary is diag_summary, scalars are diag_traces of the recorded traces, and the chain is
     untouched; bpmf --diagnose -o DIR prints the four Final lines and writes diagnostics.csv, both equal to the Python result; a
     saved model serves the same rhat and ess

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import bpmf_amd
from bpmf_amd import io as bio
from tests import diag_ref as dr
from tests import model_ref as mr
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
ld = np.longdouble
FLOOR = 1e-12


# ---- 1. diag_traces against longdouble ----------------------------------------------------------------------------------------------------

SIZES = [8, 9, 15, 16, 63, 64, 65, 127, 128, 129, 257, 1000, 4096]
NAN_KINDS = ("constant", "nan")


def traces_of_kinds(S, seed):
    """kind -> [m, S]: the traces of the module docstring (fewer of them at the two long sizes: the reference is a Python loop)"""
    rng = np.random.default_rng(seed)
    m = 4 if S <= 257 else 2
    n = S // 2
    out = dict(iid=rng.standard_normal((m, S)))
    for rho in (0.5, 0.9, 0.99, -0.5):
        out["ar%g" % rho] = dr.ar1(rng, m, S, rho)
    shifted = rng.standard_normal((m, S)); shifted[:, S - n:] += 3.0
    out["shifted"] = shifted
    out["offset1e8"] = 1e8 + rng.standard_normal((m, S))
    out["scaled_up"] = rng.standard_normal((m, S)) * 4.0 ** 20
    out["scaled_down"] = rng.standard_normal((m, S)) * 4.0 ** -20
    out["constant"] = np.repeat(np.array([0.0, 3.0, 0.1, -1e300])[:m, None], S, axis=1)
    bad = rng.standard_normal((m, S))
    for i, at in enumerate((0, S - 1, n - 1, S - n)[:m]):
        bad[i, at] = np.nan
    out["nan"] = bad
    return out


def tolerances(X, X64=None):
    """(want_rhat, want_ess, tol): the longdouble reference of the traces X and 8 x the worst relative error of the fp64 restatement
    (on X64 where the fp64 traces differ from the longdouble ones) for (rhat, ess), not less than FLOOR"""
    want = dr.diag_many(X)
    f64 = dr.diag_many(X if X64 is None else X64, dr.diag_f64)
    tol = tuple(max(8.0 * dr.relative_error(f64[k], want[k]), FLOOR) for k in (0, 1))
    return want[0], want[1], tol


def check(got, want, tol, tag):
    for k, name in ((0, "rhat"), (1, "ess")):
        err = dr.relative_error(got[k], want[k])
        assert err <= tol[k], (tag, name, err, tol[k])
    return dr.relative_error(got[0], want[0]) / tol[0], dr.relative_error(got[1], want[1]) / tol[1]


@pytest.mark.parametrize("S", SIZES)
def test_diag_traces_against_longdouble(hip_engine_factory, S):
    eng = hip_engine_factory(8)
    kinds = traces_of_kinds(S, 1000 + S)
    names = list(kinds)
    base = np.concatenate([kinds[k] for k in names])
    kind_of = np.repeat(np.arange(len(names)), [len(kinds[k]) for k in names])
    ref = {k: tolerances(kinds[k]) for k in names}
    want_r = np.concatenate([ref[k][0] for k in names]); want_e = np.concatenate([ref[k][1] for k in names])
    for k in NAN_KINDS:
        assert np.isnan(ref[k][0]).all() and np.isnan(ref[k][1]).all()
    worst = [0.0, 0.0]
    for n in (1, 3, 64, 257):
        # lists of n traces: every base trace alone; a window of 3 at every offset; the base traces cycled to 64 and 257
        lists = [np.array([i]) for i in range(len(base))] if n == 1 else \
                [np.arange(i, i + 3) % len(base) for i in range(0, len(base), 3)] if n == 3 else [(np.arange(n) * 7 + n) % len(base)]
        for idx in lists:
            rhat, ess = eng.diag_traces(base[idx])
            assert rhat.shape == (n,) and ess.shape == (n,)
            for kk, name in enumerate(names):
                sel = kind_of[idx] == kk
                if sel.any():
                    w = check((rhat[sel], ess[sel]), (want_r[idx][sel], want_e[idx][sel]), ref[name][2], (S, n, name))
                    worst = [max(a, b) for a, b in zip(worst, w)]
    print("S %d: worst err / tolerance rhat %.3g ess %.3g; tolerances rhat %s" % (S, worst[0], worst[1],
          " ".join("%s %.1e/%.1e" % (k, ref[k][2][0], ref[k][2][1]) for k in names if k not in NAN_KINDS)))
    # the shifted halves ran to the lag limit and are flagged
    sel = kind_of == names.index("shifted")
    rhat, ess = eng.diag_traces(base[sel])
    if S >= 63:
        assert (rhat > 1.5).all() and (ess < 0.2 * S).all()


def test_diag_traces_shapes_and_refusals(hip_engine_factory):
    eng = hip_engine_factory(8)
    rhat, ess = eng.diag_traces(np.zeros((0, 16)))
    assert rhat.shape == (0,) and ess.shape == (0,)
    one = eng.diag_traces(np.arange(16.0))
    assert one[0].shape == (1,) and np.isfinite(one[0]).all()
    for S in (7, 4097):
        with pytest.raises(bpmf_amd.BpmfHipError, match="%d samples" % S) as e:
            eng.diag_traces(np.zeros((2, S)))
        assert e.value.code == -1
    out = np.zeros(2)
    x = np.zeros((2, 16))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert eng.lib.bpmf_hip_diag_traces(None, 2, 16, ptr(x), ptr(out), ptr(out)) == -1
    for args in ((None, ptr(out), ptr(out)), (ptr(x), None, ptr(out)), (ptr(x), ptr(out), None)):
        assert eng.lib.bpmf_hip_diag_traces(eng.ctx, 2, 16, *args) == -1
    assert eng.lib.bpmf_hip_diag_traces(eng.ctx, 0, 16, None, None, None) == 0
    assert eng.lib.bpmf_hip_diag_batch_cells(-1) == -1
    assert np.isfinite(eng.diag_traces(np.random.default_rng(0).standard_normal((3, 16)))[1]).all()    # the context goes on working


# ---- 2. bits -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [9, 64, 129, 1000, 2049])
def test_trace_bits_depend_on_the_trace_alone(hip_engine_factory, S):
    eng = hip_engine_factory(8)
    rng = np.random.default_rng(S)
    X = np.concatenate([dr.ar1(rng, 129, S, 0.8), rng.standard_normal((128, S))])
    X[200, S // 2:] += 2.0
    base = eng.diag_traces(X)
    again = eng.diag_traces(X)
    assert len(X) == 257 and all(a.tobytes() == b.tobytes() for a, b in zip(base, again))
    perm = rng.permutation(len(X))
    got = eng.diag_traces(X[perm])
    assert all(a[perm].tobytes() == b.tobytes() for a, b in zip(base, got))
    for i in (0, 3, 200, 256):
        alone = eng.diag_traces(X[i])
        assert all(a[i:i + 1].tobytes() == b.tobytes() for a, b in zip(base, alone)), i


NQ, NC = 70, 130


def ar1_rings(rng, S, K, rho=0.7):
    """(Es [S, NQ, K], Vs [S, NC, K]): every factor entry an AR(1) recursion over s around a level of its own"""
    def side(n):
        x = dr.ar1(rng, n * K, S, rho).T.reshape(S, n, K)
        return 0.5 * rng.standard_normal((n, K)) + 0.3 * x
    return side(NQ), side(NC)


def load_rings(eng, sq, sc, Es, Vs):
    S = Es.shape[0]
    eng.samples_reserve(sq, S); eng.samples_reserve(sc, S)
    eng.samples_set(sq, np.transpose(Es, (1, 0, 2))); eng.samples_set(sc, np.transpose(Vs, (1, 0, 2)))


def cell_lists(rng):
    q1 = 37
    every = (np.full(5 * NC, q1), np.tile(np.arange(NC), 5))
    rand = (rng.integers(0, NQ, 300), rng.integers(0, NC, 300))
    return dict(empty=(np.zeros(0, int), np.zeros(0, int)), one=(np.array([5]), np.array([77])), every=every,
                last=(np.array([NQ - 1, 0, NQ - 1]), np.array([NC - 1, NC - 1, 0])), random=rand)


@pytest.mark.parametrize("K", [4, 20, 128])
def test_cell_bits_do_not_depend_on_the_batch(hip_engine_factory, K):
    S = 9
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    try:
        rng = np.random.default_rng(K)
        load_rings(eng, sq, sc, *ar1_rings(rng, S, K))
        lists = cell_lists(rng)
        q, c = (np.concatenate([lists[k][i] for k in ("every", "last", "random")]) for i in (0, 1))
        base = eng.diag_cells(sq, sc, 2.5, q, c)
        for cells in (1, 7, 0):
            eng.diag_batch_cells(cells)
            got = eng.diag_cells(sq, sc, 2.5, q, c)
            assert all(base[k].tobytes() == got[k].tobytes() for k in ("mean", "std", "rhat", "ess")), (K, cells)
        perm = rng.permutation(len(q))
        got = eng.diag_cells(sq, sc, 2.5, q[perm], c[perm])
        assert all(base[k][perm].tobytes() == got[k].tobytes() for k in base)
        assert eng.diag_last_ms(sq) >= 0.0
    finally:
        eng.diag_batch_cells(0)
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 3. diag_cells on planted rings --------------------------------------------------------------------------------------------------------

def cell_reference(Es, Vs, q, c, extra=None):
    """the longdouble reference of the unique cells of the list and its tolerance (the fp64 restatement on the fp64 dot products):
    (want_rhat, want_ess, tol) in list order.  extra [S, n]: added to the dot products of the list's cells"""
    cells, inv = np.unique(np.stack([q, c]), axis=1, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    Tl = np.einsum("sik,sik->is", Es[:, cells[0]].astype(ld), Vs[:, cells[1]].astype(ld))
    T64 = np.einsum("sik,sik->is", Es[:, cells[0]], Vs[:, cells[1]])
    if extra is not None:
        first = np.array([np.flatnonzero(inv == u)[0] for u in range(cells.shape[1])])
        Tl = Tl + extra.T[first].astype(ld); T64 = T64 + extra.T[first]
    sub = np.arange(0, len(Tl), max(1, len(Tl) // 24))                 # the fp64 restatement is a Python loop: a sample of the cells
    want_r, want_e = dr.diag_many(Tl)
    f64 = dr.diag_many(T64[sub], dr.diag_f64)
    tol = tuple(max(8.0 * dr.relative_error(f64[k], w[sub]), FLOOR) for k, w in ((0, want_r), (1, want_e)))
    return want_r[inv], want_e[inv], tol


@pytest.mark.parametrize("K,dtype", [(1, "f64"), (8, "f64"), (20, "f64"), (32, "f64"), (64, "f64"), (128, "f64"), (72, "f32")])
def test_diag_cells_against_longdouble(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    mean_rating = 3.5
    try:
        for S in (8, 65):
            rng = np.random.default_rng(100 * K + S)
            Es, Vs = ar1_rings(rng, S, K)
            load_rings(eng, sq, sc, Es, Vs)
            Eg, Vg = np.transpose(eng.samples_get(sq), (1, 0, 2)), np.transpose(eng.samples_get(sc), (1, 0, 2))
            assert Eg.tobytes() == Es.tobytes() and Vg.tobytes() == Vs.tobytes()
            for name, (q, c) in cell_lists(rng).items():
                got = eng.diag_cells(sq, sc, mean_rating, q, c)
                assert sorted(got) == ["ess", "mean", "rhat", "std"] and all(v.shape == (len(q),) for v in got.values())
                mean, std = eng.predict_cells(sq, sc, mean_rating, q, c)
                assert got["mean"].tobytes() == mean.tobytes() and got["std"].tobytes() == std.tobytes(), (K, S, name)
                if len(q) == 0:
                    continue
                want_r, want_e, tol = cell_reference(Eg, Vg, q, c)
                w = check((got["rhat"], got["ess"]), (want_r, want_e), tol, (K, dtype, S, name))
                if name == "random":
                    print("K %d %s S %d: err / tolerance rhat %.3g ess %.3g (tolerance %.1e %.1e); median ess %.1f" %
                          (K, dtype, S, w[0], w[1], tol[0], tol[1], np.median(got["ess"])))
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_diag_cells_with_biases(hip_engine_factory):
    K, S, nq, nc = 8, 16, 11, 23
    eng = hip_engine_factory(K)
    A = (np.zeros(nq + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    B = (np.zeros(nc + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    sq, sc = eng.side_create(nq, nc, *A, 0.0), eng.side_create(nc, nq, *B, 0.0)
    try:
        eng.set_bias(sq, 1.0, 14, 1); eng.set_bias(sc, 1.0, 13, 0)
        eng.samples_reserve(sq, S); eng.samples_reserve(sc, S)
        rng = np.random.default_rng(4)
        Es = 0.4 * dr.ar1(rng, nq * K, S, 0.6).T.reshape(S, nq, K); Vs = 0.4 * dr.ar1(rng, nc * K, S, 0.6).T.reshape(S, nc, K)
        bq, bc = dr.ar1(rng, nq, S, 0.8).T.copy(), dr.ar1(rng, nc, S, 0.8).T.copy()
        for s in range(S):
            eng.set_items(sq, Es[s]); eng.set_items(sc, Vs[s])
            eng.bias_set(sq, bq[s]); eng.bias_set(sc, bc[s])
            eng.samples_add(sq); eng.samples_add(sc)
        q, c = np.divmod(np.arange(nq * nc), nc)
        got = eng.diag_cells(sq, sc, 1.25, q, c)
        mean, std = eng.predict_cells(sq, sc, 1.25, q, c)
        assert got["mean"].tobytes() == mean.tobytes() and got["std"].tobytes() == std.tobytes()
        want_r, want_e, tol = cell_reference(Es, Vs, q, c, extra=bq[:, q] + bc[:, c])
        w = check((got["rhat"], got["ess"]), (want_r, want_e), tol, "bias")
        print("bias: err / tolerance rhat %.3g ess %.3g" % w)
        # without the biases the figures are others: the bias rows of the rings are read
        plain = dr.diag_many(np.einsum("sik,sik->is", Es[:, q], Vs[:, c]))
        assert dr.relative_error(got["ess"], plain[1]) > 1e-3
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_diag_cells_refusals(hip_engine_factory):
    K = 8
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    try:
        with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells: no sample ring"):
            eng.diag_cells(sq, sc, 0.0, [0], [0])
        rng = np.random.default_rng(1)
        load_rings(eng, sq, sc, rng.standard_normal((7, NQ, K)), rng.standard_normal((7, NC, K)))
        with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells: 7 samples") as e:
            eng.diag_cells(sq, sc, 0.0, [0], [0])
        assert e.value.code == -1
        with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells: 7 samples"):
            eng.diag_cells(sq, sc, 0.0, [], [])
        with pytest.raises(bpmf_amd.BpmfHipError, match="no diagnostics"):
            eng.diag_last_ms(sq)
        eng.samples_reserve(sq, 9); eng.samples_reserve(sc, 9)
        eng.samples_set(sq, rng.standard_normal((NQ, 9, K))); eng.samples_set(sc, rng.standard_normal((NC, 8, K)))
        with pytest.raises(bpmf_amd.BpmfHipError, match="same number"):
            eng.diag_cells(sq, sc, 0.0, [0], [0])
        eng.samples_set(sq, rng.standard_normal((NQ, 8, K)))
        for q, c, cell in (([0, NQ], [0, 0], "cell 1"), ([0, 1, 2], [0, 1, NC], "cell 2"), ([-1], [0], "cell 0")):
            with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells: " + cell + " .*out of range") as e:
                eng.diag_cells(sq, sc, 0.0, q, c)
            assert e.value.code == -1
        with pytest.raises(bpmf_amd.BpmfHipError, match="mean_rating is not finite"):
            eng.diag_cells(sq, sc, np.nan, [0], [0])
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        one = np.zeros(1, np.int32); out = np.zeros(1)
        assert eng.lib.bpmf_hip_diag_cells(None, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), ptr(out), ptr(out), ptr(out)) == -1
        assert eng.lib.bpmf_hip_diag_cells(sq.handle, sc.handle, 0.0, 1, ptr(one), None, ptr(out), ptr(out), ptr(out), ptr(out)) == -1
        assert eng.lib.bpmf_hip_diag_cells(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), ptr(out), ptr(out), None, ptr(out)) == -1
        other = bpmf_amd.HipEngine(K)
        try:
            oq, oc = mr.pair_of_sides(other, NQ, NC)
            with pytest.raises(bpmf_amd.BpmfHipError, match="different contexts"):
                eng.diag_cells(sq, oc, 0.0, [0], [0])
        finally:
            other.close()
        got = eng.diag_cells(sq, sc, 0.0, [0], [0])
        assert all(np.isfinite(v).all() for v in got.values()) and eng.diag_last_ms(sq) >= 0.0
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------------

CHAIN = dict(nsims=40, burnin=8, alpha=2.0)


def test_gibbs_diagnose(hip_engine_factory):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    eng = hip_engine_factory(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, diagnose=True, **CHAIN)
    d = res["diag"]
    tcol = np.repeat(np.arange(nm), np.diff(T[0]))
    assert np.array_equal(d["rows"], T[1]) and np.array_equal(d["cols"], tcol) and d["samples"] == 32
    direct = eng.diag_cells(res["users"].side, res["movies"].side, res["movies"].mean_rating, T[1], tcol)
    assert all(d[k].tobytes() == direct[k].tobytes() for k in ("mean", "std", "rhat", "ess"))
    assert d["mcse"].tobytes() == (d["std"] / np.sqrt(d["ess"])).tobytes()
    assert d["summary"] == bpmf_amd.diag_summary(d) and d["summary"]["n"] == len(T[1]) and d["summary"]["samples"] == 32
    assert d["summary"]["n_nan"] == 0 and 1.0 <= d["summary"]["ess_min"] <= d["summary"]["ess_median"] <= 32 * np.log10(32)
    assert sorted(d["scalars"]) == ["norm_m", "norm_u", "rmse"]
    rhat, ess = eng.diag_traces(np.array([res[k][8:] for k in ("rmse", "norm_u", "norm_m")]))
    for i, k in enumerate(("rmse", "norm_u", "norm_m")):
        assert d["scalars"][k] == (rhat[i], ess[i]) and np.isfinite(ess[i])
    want = dr.diag_many(np.array([res[k][8:] for k in ("rmse", "norm_u", "norm_m")]))
    assert dr.relative_error(rhat, want[0]) < 1e-9 and dr.relative_error(ess, want[1]) < 1e-9
    # the chain is untouched, and the cells may be given
    plain = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, **CHAIN)
    assert "diag" not in plain and np.array(plain["rmse"]).tobytes() == np.array(res["rmse"]).tobytes()
    assert plain["U"].tobytes() == res["U"].tobytes()
    some = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, diagnose=(T[1][::3], tcol[::3]), noise="adaptive", **CHAIN)
    assert len(some["diag"]["rhat"]) == len(T[1][::3]) and sorted(some["diag"]["scalars"]) == ["alpha", "norm_m", "norm_u", "rmse"]
    again = bpmf_amd.diagnose(some, T[1][::3], tcol[::3])
    assert all(again[k].tobytes() == some["diag"][k].tobytes() for k in ("mean", "std", "rhat", "ess", "mcse"))


def run(args, cwd):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def final_lines(s, samples, with_traces=None):
    """the Final lines bpmf prints for the summary `s`"""
    out = ["Final ESS: min %.1f median %.1f of %d samples (%d cells)" % (s["ess_min"], s["ess_median"], samples, s["n"]),
           "Final split-Rhat: median %.4f max %.4f above 1.01: %.2f%%" % (s["rhat_median"], s["rhat_max"], 100.0 * s["rhat_above"]),
           "Final MCSE/std: median %.4f" % s["mcse_over_std_median"]]
    if with_traces is not None:
        out.append("Final trace ESS: RMSE %.1f FU %.1f FM %.1f" % tuple(with_traces[k][1] for k in ("rmse", "norm_u", "norm_m")))
    return out


def read_diagnostics(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "row,col,mean,std,rhat,ess,mcse"
    return np.array([ln.split(",") for ln in lines[1:]], dtype=float).reshape(-1, 7)


def test_cli_diagnose(tmp_path, hip_engine_factory):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    bio.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    bio.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    for name in ("A", "B", "P"):
        os.mkdir(tmp_path / name)
    chain = ["-n", "train.sdm", "-p", "test.sdm", "-d", 8, "-i", 40, "-b", 8]
    plain = run(chain + ["-o", "P"], tmp_path)
    a = run(chain + ["--diagnose", "--save-model", "model", "-o", "A"], tmp_path)
    assert "diagnose: split-Rhat and ESS of the test predictions\n" in a.stdout
    final = lambda text: [ln for ln in text.splitlines() if ln.startswith("Final Avg RMSE: ")]
    assert final(a.stdout) == final(plain.stdout) and len(final(a.stdout)) == 1
    assert sorted(set(os.listdir(tmp_path / "A")) - set(os.listdir(tmp_path / "P"))) == ["diagnostics.csv"]
    lines = a.stdout.splitlines()
    at = lines.index(final(a.stdout)[0])
    got = lines[at + 1:at + 5]
    pat = (r"Final ESS: min (\S+) median (\S+) of 32 samples \((\d+) cells\)", r"Final split-Rhat: median (\S+) max (\S+) above 1.01: (\S+)%",
           r"Final MCSE/std: median (\S+)", r"Final trace ESS: RMSE (\S+) FU (\S+) FM (\S+)")
    for ln, p in zip(got, pat):
        m = re.fullmatch(p, ln)
        assert m and all(np.isfinite(float(g)) for g in m.groups()), ln
    # the file: one row per test cell in the order of T, mcse = std / sqrt(ess)
    rec = read_diagnostics(tmp_path / "A" / "diagnostics.csv")
    tcol = np.repeat(np.arange(nm), np.diff(T[0]))
    assert np.array_equal(rec[:, 0], T[1] + 1) and np.array_equal(rec[:, 1], tcol + 1)
    assert rec[:, 6].tobytes() == (rec[:, 3] / np.sqrt(rec[:, 5])).tobytes()
    # the Python run of the same chain gives the same figures
    eng = hip_engine_factory(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, diagnose=True, **CHAIN)
    d = res["diag"]
    for j, k in enumerate(("mean", "std", "rhat", "ess", "mcse")):
        assert rec[:, 2 + j].tobytes() == d[k].tobytes(), k
    assert got == final_lines(d["summary"], 32, d["scalars"])
    # a saved model serves the same figures for the same cells, without the trace line
    b = run(["--model", "model", "--predict", "test.sdm", "--diagnose", "-o", "B"], tmp_path)
    assert (tmp_path / "B" / "diagnostics.csv").read_bytes() == (tmp_path / "A" / "diagnostics.csv").read_bytes()
    assert b.stdout.splitlines()[1:] == final_lines(d["summary"], 32) and b.stdout.startswith("model: model, ")
    serve = bpmf_amd.HipEngine(8)
    try:
        loaded = bpmf_amd.load_model(serve, str(tmp_path / "model"))
        again = bpmf_amd.diagnose(loaded, T[1], tcol)
        assert all(again[k].tobytes() == d[k].tobytes() for k in ("mean", "std", "rhat", "ess"))
    finally:
        serve.close()
