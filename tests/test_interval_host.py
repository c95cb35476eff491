"""Predictive intervals without a GPU: the restatements of tests/interval_ref.py against what is known of them,
calibration_summary, and every refusal of `bpmf --intervals` and gibbs(intervals=) before a GPU is touched.

  1. the library has the entry points, the ABI version is still 1, the usage text names the flag
  2. interval_ref: Phi_ld against scipy; the quantile against the closed form p + z / sqrt(alpha w) at S = 1 and against
     scipy.optimize.brentq on the fp64 mixture; the pit against scipy.stats.norm
  3. the device's rule restated in fp64 (interval_ref.rule_f64) on every trace family and every tau of the GPU test: the residual bound
     the device is held to, roots that never decrease, and never the cap of 128 evaluations
  4. calibration_summary on exactly uniform pits (coverage = level, KS <= 1 / n), on pits squeezed towards 1/2 (coverage above the
     level), the widths and the histogram by hand
  5. the refusals of predict_intervals, gibbs(intervals=) and `bpmf --intervals`: one line, status 1

These fail on the commit before the feature (no entry points, no bpmf_amd.calibration_summary, an unknown option prints the usage).
"""
import math
import os
import subprocess

import numpy as np
import pytest
import bpmf_amd
from tests import interval_ref as ir
from tests import model_ref as mr
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
LD = np.longdouble


# ---- 1. entry points -----------------------------------------------------------------------------------------------------------------------

def test_library_has_the_entry_points():
    from bpmf_amd import _lib
    lib = _lib.load_library()
    names = ("bpmf_hip_interval_cells", "bpmf_hip_interval_traces", "bpmf_hip_interval_batch_cells", "bpmf_hip_interval_last_ms")
    for name in names:
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None
    assert len(_lib._SIGNATURES["bpmf_hip_interval_cells"][1]) == 16 and len(_lib._SIGNATURES["bpmf_hip_interval_traces"][1]) == 13
    for name in ("interval_cells", "interval_traces", "interval_batch_cells", "interval_last_ms"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
    assert callable(bpmf_amd.predict_intervals) and callable(bpmf_amd.calibration_summary)
    assert lib.bpmf_hip_abi_version() == 1
    with open(os.path.join(ROOT, "include", "bpmf_hip.h")) as f:
        text = f.read()
    assert "#define BPMF_HIP_INTERVAL_MAX_SAMPLES %d\n" % bpmf_amd.HipEngine.INTERVAL_MAX_SAMPLES in text
    assert "#define BPMF_HIP_INTERVAL_MAX_QUANTILES %d\n" % bpmf_amd.HipEngine.INTERVAL_MAX_QUANTILES in text
    for name in names:
        assert "BPMF_API int %s(" % name in text


def test_usage_names_the_flag(tmp_path):
    p = subprocess.run([BPMF, "-h"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert "[--intervals L1[,L2..]]" in p.stdout + p.stderr and "intervals.csv" in p.stdout + p.stderr


# ---- 2. the reference ----------------------------------------------------------------------------------------------------------------------

def test_reference_against_closed_forms():
    special = pytest.importorskip("scipy.special")
    stats = pytest.importorskip("scipy.stats")
    optimize = pytest.importorskip("scipy.optimize")
    t = np.concatenate([np.linspace(-9, 9, 181), [-2.9999999, 3.0, -3.0, 2.9999999, 40.0, -40.0]])
    got = ir.Phi_ld(t)
    assert float(np.max(np.abs(got - special.ndtr(t)))) < 3e-16 and float(np.max(np.abs(got + ir.Phi_ld(-t) - 1))) < 3e-19
    assert got[-2] == 1 and 0 < got[-1] < 1e-300
    # S = 1: q = p + z / sqrt(alpha w), to longdouble resolution of the longdouble z
    rng = np.random.default_rng(1)
    n = 6
    D = rng.standard_normal((n, 1)) * 3
    w = 10.0 ** rng.uniform(-2, 2, n)
    for tau in ir.TAUS:
        z = ir.quantile(np.zeros((1, 1)), 1.0, tau)[0]
        assert abs(float(z) - stats.norm.ppf(tau)) < 1e-14
        q = ir.quantile(D, 2.5, tau, w=w, mean=1.5)
        want = LD(1.5) + D[:, 0].astype(LD) + z / np.sqrt(LD(2.5) * w.astype(LD))
        assert float(np.max(np.abs(q - want))) < 1e-17 * 30
        assert abs(float(ir.normal_quantile(tau) - z)) < 1e-15
    # several samples: brentq on the fp64 mixture, and the pit against scipy
    S = 9
    D = rng.standard_normal((n, S)) * 2
    al = 0.5 + rng.random(S)
    y = rng.standard_normal(n) * 2
    for i in range(n):
        F = lambda x: stats.norm.cdf((x - D[i]) * np.sqrt(al * w[i])).mean()
        assert abs(float(ir.pit(D[i:i + 1], al, y[i:i + 1] + 0.25, w=w[i:i + 1], mean=0.25)[0]) - F(y[i])) < 1e-15
        for tau in (0.025, 0.5, 0.975):
            root = optimize.brentq(lambda x: F(x) - tau, -60.0, 60.0, xtol=1e-15, rtol=8.9e-16)
            q = float(ir.quantile(D[i:i + 1], al, tau, w=w[i:i + 1])[0])
            assert abs(q - root) < 1e-12 * max(1.0, abs(root)), (i, tau, q, root)
            res, bound = ir.quantile_residual(D[i:i + 1], al, tau, np.array([q]), w=w[i:i + 1])
            assert res[0] <= bound[0]                            # (the rounding of q to fp64 alone)


# ---- 3. the rule ---------------------------------------------------------------------------------------------------------------------------

def test_rule_in_fp64_meets_the_residual_bound():
    """The rule of k_trace_quantiles with numpy's sums in place of the lanes': what the device is asked for is within reach of fp64."""
    worst, most = 0.0, 0
    for S in (1, 2, 7, 64, 65, 129, 700):
        rng = np.random.default_rng(S)
        n = 3
        for name, fam in ir.families(rng, n, S).items():
            r = ir.rates(fam["alpha"], fam["w"], S).astype(np.float64)
            r = np.broadcast_to(r, (n, S))
            for i in range(n):
                roots, evals = ir.rule_f64(fam["D"][i], r[i], ir.TAUS)
                assert np.isfinite(roots).all() and (np.diff(roots) >= 0).all(), (S, name, roots)
                most = max(most, max(evals))
                w = None if fam["w"] is None else fam["w"][i:i + 1]
                for tau, q in zip(ir.TAUS, roots):
                    res, bound = ir.quantile_residual(fam["D"][i:i + 1], fam["alpha"], tau, np.array([q]), w=w)
                    assert res[0] <= bound[0], (S, name, i, tau, res[0], bound[0])
                    worst = max(worst, res[0] / bound[0])
    print("rule_f64: residual / bound at most %.3f, at most %d evaluations" % (worst, most))
    assert most < 128


# ---- 4. the summary ------------------------------------------------------------------------------------------------------------------------

def test_calibration_summary():
    n = 1000
    levels = (0.5, 0.8, 0.9)
    pit = (np.arange(n) + 0.5) / n
    rng = np.random.default_rng(3)
    s = bpmf_amd.calibration_summary(rng.permutation(pit), levels)
    assert s["n"] == n and s["n_nan"] == 0 and s["levels"] == list(levels)
    assert s["coverage"] == list(levels) and s["ks"] <= 1.0 / n and s["ks"] == pytest.approx(0.5 / n, rel=1e-9)
    assert s["se"] == [math.sqrt(l * (1 - l) / n) for l in levels]
    assert s["hist"].tolist() == [100] * 10 and all(math.isnan(w) for w in s["width"])
    # squeezed towards 1/2 (intervals too wide): every coverage above its level, a hump in the histogram, a visible KS distance
    sq = bpmf_amd.calibration_summary(0.5 + 0.6 * (pit - 0.5), levels)
    assert all(c > l + 3 * e for c, l, e in zip(sq["coverage"], levels, sq["se"])) and sq["ks"] == pytest.approx(0.2, abs=2e-3)
    assert sq["hist"][0] == sq["hist"][9] == 0 and sq["hist"][4] > 100
    # stretched (intervals too narrow): below
    st = bpmf_amd.calibration_summary(np.clip(0.5 + 1.5 * (pit - 0.5), 0.0, 1.0), levels)
    assert all(c < l - 3 * e for c, l, e in zip(st["coverage"], levels, st["se"]))
    # by hand: five cells, one NaN; |pit - 1/2| = 0.45, 0.1, 0.25, 0.5 against 0.25 and 0.45
    lo = np.array([[0.0, -1.0], [1.0, 0.0], [2.0, 1.0], [0.0, 0.0], [5.0, 4.0]])
    hi = lo + np.array([[1.0, 3.0], [2.0, 4.0], [3.0, 5.0], [9.0, 9.0], [4.0, 6.0]])
    h = bpmf_amd.calibration_summary([0.05, 0.6, 0.75, np.nan, 1.0], (0.5, 0.9), lo, hi)
    assert h["n"] == 4 and h["n_nan"] == 1 and h["coverage"] == [0.5, 0.75] and h["width"] == [2.5, 4.5]
    assert h["hist"].tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0, 1] and h["ks"] == pytest.approx(0.35)
    e = bpmf_amd.calibration_summary([], (0.9,))
    assert e["n"] == 0 and math.isnan(e["coverage"][0]) and math.isnan(e["ks"]) and e["hist"].sum() == 0


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_python_refusals(monkeypatch):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    none = object()                                                  # (refused before the engine is used)
    run = lambda intervals=True, **kw: bpmf_amd.gibbs(none, M, Mt, T, nu, nm, intervals=intervals, **{**dict(nsims=10, burnin=4), **kw})
    for bad, why in (((0.9, 0.9), "levels must differ"), ((0.999,), "outside"), ((0.005,), "outside"), ((0.1, 0.2, 0.3, 0.4, 0.5), "1 .. 4 levels"), ((), "1 .. 4 levels")):
        with pytest.raises(ValueError, match=why):
            run(intervals=bad)
    with pytest.raises(ValueError, match="intervals needs 1 .. 4096 post-burn-in samples"):
        run(nsims=5, burnin=5)
    with pytest.raises(ValueError, match="intervals needs 1 .. 4096 post-burn-in samples"):
        run(nsims=5000, burnin=4)
    for kw, what in ((dict(ordinal=True), "ordinal"), (dict(implicit=0.1), "implicit"), (dict(probit=True), "probit"), (dict(robust=4.0), "robust")):
        with pytest.raises(ValueError, match="intervals does not go together with %s" % what):
            run(**kw)
    with pytest.raises(ValueError, match="out of scope"):
        run(robust=4.0)
    with pytest.raises(ValueError, match="intervals needs a test matrix"):
        bpmf_amd.gibbs(none, M, Mt, None, nu, nm, intervals=True, nsims=10, burnin=4)

    class Ranks:
        def comm_nranks(self):
            return 2
    with pytest.raises(ValueError, match="intervals does not go together with a communicator"):
        bpmf_amd.gibbs(Ranks(), M, Mt, T, nu, nm, intervals=True, nsims=10, burnin=4)
    monkeypatch.setenv("BPMF_REDUCE", "1")
    with pytest.raises(ValueError, match="intervals does not go together with BPMF_REDUCE"):
        run()
    res = dict(users=None, movies=None)
    with pytest.raises(ValueError, match="no model_info"):
        bpmf_amd.predict_intervals(res, [0], [0])
    with pytest.raises(ValueError, match="no Gaussian predictive"):
        bpmf_amd.predict_intervals(dict(res, model_info=dict(probit=True)), [0], [0])
    with pytest.raises(ValueError, match="no Gaussian predictive"):
        bpmf_amd.predict_intervals(dict(res, model_info=dict(scored=False)), [0], [0])
    with pytest.raises(ValueError, match="not after robust="):
        bpmf_amd.predict_intervals(dict(res, model_info=dict(nu=4.0)), [0], [0])
    with pytest.raises(ValueError, match="outside"):
        bpmf_amd.predict_intervals(dict(res, model_info=dict(alpha=2.0)), [0], [0], levels=(1.0,))


def refused(args, reason, cwd, env=None):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 1 and p.stdout == "", (args, p.stdout, p.stderr)
    lines = p.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("bpmf: ") and reason in lines[0], (args, p.stderr)


def test_cli_refusals(tmp_path):
    base = ["-n", "train.sdm", "-p", "test.sdm", "--intervals", "0.9"]       # (nothing is read before the refusal)
    ok = ["-i", 20, "-b", 5]
    for bad in ("", "0.9,", "0.9,0.9", "0.999", "0.005", "ninety", "0.1,0.2,0.3,0.4,0.5", "0.9x"):
        refused(["-n", "train.sdm", "-p", "test.sdm", "--intervals", bad] + ok, "--intervals expects 1 .. 4 distinct levels in [0.01, 0.998]", tmp_path)
    refused(base + ["-i", 5, "-b", 5], "needs 1 .. 4096 post-burn-in samples (-i - -b = 0)", tmp_path)
    refused(base + ["-i", 5000, "-b", 5], "needs 1 .. 4096 post-burn-in samples (-i - -b = 4995)", tmp_path)
    refused(["-n", "train.sdm", "--intervals", "0.9"] + ok, "--intervals needs a test matrix", tmp_path)
    refused(base + ok + ["-g", 2], "one GPU without -g", tmp_path)
    refused(base + ok, "BPMF_REDUCE=1", tmp_path, env={"BPMF_REDUCE": "1"})
    refused(base + ok + ["-m", "mu.ddm", "-l", "lambda.ddm"], "propagated posterior", tmp_path)
    refused(base + ok + ["--ordinal"], "--intervals does not go together with --ordinal", tmp_path)
    refused(base + ok + ["--probit"], "--intervals does not go together with --probit", tmp_path)
    refused(base + ok + ["--implicit", 0.1], "--intervals does not go together with --implicit", tmp_path)
    refused(base + ok + ["--robust", 4], "--intervals does not go together with --robust", tmp_path)
    refused(base + ok + ["--robust", 4], "incomplete beta function on the device: deliberately out of scope", tmp_path)
    refused(["--tensor", "x.tns", "--intervals", "0.9"] + ok, "--tensor", tmp_path)
    refused(["--model", "model", "--intervals", "0.9", "--topn", 3, "-o", "out"], "needs --predict FILE", tmp_path)
    # a probit model: read, then refused before a context is created
    bpmf_amd.write_model(tmp_path / "model", mr.random_model(4, 6, 5, 3, seed=1, hyper=False, probit=True))
    os.mkdir(tmp_path / "out")
    refused(["--model", "model", "--intervals", "0.9", "--predict", "cells.sdm", "-o", "out"], "is a probit model", tmp_path)
