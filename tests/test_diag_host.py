"""Convergence diagnostics without a GPU: the estimator as tests/diag_ref.py restates it against what is known
of it, the summary, and every refusal of `bpmf --diagnose` and gibbs(diagnose=) before a GPU is touched.

  1. AR(1) traces (fixed seed, S = 1000, 400 traces per rho in {0, 0.5, 0.9}): the median of ess / S within 15 % of
     (1 - rho) / (1 + rho), the 99th percentile of rhat < 1.03 at rho <= 0.5 -- for the longdouble reference and for the fp64
     restatement, which must agree with it
  2. two halves N(0, 1) and N(3, 1) at S = 200: rhat > 2, ess < 5; a constant trace: NaN, NaN; rho = -0.5: 0 < ess <= 2n log10(2n);
     S = 8 and 9 run; a value that is not finite: NaN, NaN
  3. diag_summary against figures worked out by hand, NaNs left out and counted
  4. the library has the entry points, the ABI version is still 1, and the refusals come in one line with a non-zero status

These fail on the commit before the feature (no tests/diag_ref.py figures to hold, an unknown option prints the usage, no entry points).
"""
import os
import subprocess

import numpy as np
import pytest
import bpmf_amd
from tests import diag_ref as dr
from tests import model_ref as mr
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")


# ---- 1. AR(1) ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ar1_results():
    """rho -> (rhat, ess) of 400 traces of S = 1000 in longdouble, computed once"""
    rng = np.random.default_rng(20211)
    return {rho: dr.diag_many(dr.ar1(rng, 400, 1000, rho)) for rho in (0.0, 0.5, 0.9)}


@pytest.mark.parametrize("rho", [0.0, 0.5, 0.9])
def test_ar1_ess_and_rhat(ar1_results, rho):
    rhat, ess = ar1_results[rho]
    assert np.isfinite(rhat).all() and np.isfinite(ess).all()
    want = (1.0 - rho) / (1.0 + rho)
    got = float(np.median(ess / 1000.0))
    q99 = float(np.quantile(rhat, 0.99))
    print("rho %.1f: median ess / S %.4f against %.4f, q99 rhat %.4f" % (rho, got, want, q99))
    assert abs(got - want) <= 0.15 * want, (rho, got, want)
    if rho <= 0.5:
        assert q99 < 1.03, (rho, q99)
    assert (rhat > 0.99).all()


def test_fp64_restatement_agrees_with_longdouble():
    rng = np.random.default_rng(5)
    X = np.concatenate([dr.ar1(rng, 20, 257, rho) for rho in (0.0, 0.9, -0.5)])
    a, b = dr.diag_many(X), dr.diag_many(X, dr.diag_f64)
    assert dr.relative_error(b[0], a[0]) < 1e-12 and dr.relative_error(b[1], a[1]) < 1e-12


# ---- 2. other traces ---------------------------------------------------------------------------------------------------------------------

def test_shifted_halves_are_flagged():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.standard_normal(100), 3.0 + rng.standard_normal(100)])
    for fn in (dr.diag, dr.diag_f64):
        rhat, ess = fn(x)
        assert rhat > 2.0 and 0.0 < ess < 5.0, (rhat, ess)


@pytest.mark.parametrize("value", [0.0, 3.0, 0.1, -1e300, 1e-300])
def test_constant_trace_is_nan(value):
    for S in (8, 9, 200):
        for fn in (dr.diag, dr.diag_f64):
            rhat, ess = fn(np.full(S, value))
            assert np.isnan(rhat) and np.isnan(ess), (value, S)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_value_that_is_not_finite_gives_nan(bad):
    rng = np.random.default_rng(9)
    for S, at in ((8, 0), (65, 64), (200, 100), (200, 199)):
        x = rng.standard_normal(S); x[at] = bad
        for fn in (dr.diag, dr.diag_f64):
            rhat, ess = fn(x)
            assert np.isnan(rhat) and np.isnan(ess), (bad, S, at)


def test_antithetic_trace_is_capped():
    rng = np.random.default_rng(11)
    for S in (200, 1000):
        n = S // 2
        for x in dr.ar1(rng, 20, S, -0.5):
            rhat, ess = dr.diag(x)
            assert 0.0 < ess <= 2 * n * np.log10(2 * n) * (1 + 1e-15) and ess > 2 * n, (S, ess)
            assert 0.99 < rhat < 1.05


@pytest.mark.parametrize("S", [8, 9])
def test_the_shortest_traces_run(S):
    rng = np.random.default_rng(S)
    for x in rng.standard_normal((50, S)):
        a, b = dr.diag(x), dr.diag_f64(x)
        assert np.isfinite(a).all() and a[0] > 0 and 0 < a[1] <= 2 * (S // 2) * np.log10(2 * (S // 2)) * (1 + 1e-15)
        assert abs(a[0] - b[0]) <= 1e-12 * a[0] and abs(a[1] - b[1]) <= 1e-12 * a[1]


def test_an_odd_length_drops_the_middle_sample():
    x = np.random.default_rng(3).standard_normal(9); y = x.copy(); y[4] = 1e6
    assert dr.diag(x) == dr.diag(y) and dr.diag_f64(x) == dr.diag_f64(y)


# ---- 3. the summary ------------------------------------------------------------------------------------------------------------------------

def test_diag_summary():
    d = dict(std=np.array([1.0, 2.0, 3.0, 4.0, 5.0]), rhat=np.array([1.0, 1.02, np.nan, 1.005, 1.5]), ess=np.array([4.0, 16.0, 9.0, np.nan, 100.0]),
             samples=32)
    s = bpmf_amd.diag_summary(d)
    assert s["n"] == 5 and s["n_nan"] == 2 and s["samples"] == 32
    assert s["ess_min"] == 4.0 and s["ess_median"] == 16.0
    assert s["rhat_median"] == 1.02 and s["rhat_max"] == 1.5 and s["rhat_above"] == 2.0 / 3.0
    assert s["mcse_over_std_median"] == 0.25
    empty = bpmf_amd.diag_summary(dict(rhat=np.array([np.nan]), ess=np.array([np.nan]), std=np.zeros(1)))
    assert empty["n"] == 1 and empty["n_nan"] == 1 and empty["samples"] is None and all(np.isnan(empty[k]) for k in ("ess_min", "rhat_max", "mcse_over_std_median"))


# ---- 4. entry points and refusals ----------------------------------------------------------------------------------------------------------

def test_library_has_the_entry_points():
    from bpmf_amd import _lib
    lib = _lib.load_library()
    for name in ("bpmf_hip_diag_traces", "bpmf_hip_diag_cells", "bpmf_hip_diag_batch_cells", "bpmf_hip_diag_last_ms"):
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None
    for name in ("diag_traces", "diag_cells", "diag_batch_cells", "diag_last_ms"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
    assert callable(bpmf_amd.diagnose) and callable(bpmf_amd.diag_summary)
    assert lib.bpmf_hip_abi_version() == 1
    assert (bpmf_amd.HipEngine.DIAG_MIN_SAMPLES, bpmf_amd.HipEngine.DIAG_MAX_SAMPLES) == (dr.MIN_SAMPLES, dr.MAX_SAMPLES)
    with open(os.path.join(ROOT, "include", "bpmf_hip.h")) as f:
        assert "#define BPMF_HIP_DIAG_MAX_SAMPLES %d\n" % dr.MAX_SAMPLES in f.read()


def refused(args, reason, cwd, env=None):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 1 and p.stdout == "", (args, p.stdout, p.stderr)
    lines = p.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("bpmf: ") and reason in lines[0], (args, p.stderr)


def test_cli_refusals(tmp_path):
    base = ["-n", "train.sdm", "-p", "test.sdm", "--diagnose"]      # (nothing is read before the refusal)
    refused(base + ["-i", 20, "-b", 13], "8 .. 4096 post-burn-in samples", tmp_path)
    refused(base + ["-i", 5000, "-b", 5], "8 .. 4096 post-burn-in samples", tmp_path)
    refused(base + ["-i", 20, "-b", 5, "-g", 2], "one GPU without -g", tmp_path)
    refused(base + ["-i", 20, "-b", 5], "BPMF_REDUCE=1", tmp_path, env={"BPMF_REDUCE": "1"})
    refused(base + ["-i", 20, "-b", 5, "-m", "mu.ddm", "-l", "lambda.ddm"], "propagated posterior", tmp_path)
    refused(["--tensor", "x.tns", "--diagnose", "-i", 20, "-b", 5], "--tensor", tmp_path)
    refused(["--model", "model", "--diagnose", "--topn", 3, "-n", "train.sdm", "-o", "out"], "needs --predict FILE", tmp_path)
    # a model with too few samples: read, then refused before a context is created
    bpmf_amd.write_model(tmp_path / "model", mr.random_model(4, 6, 5, 7, seed=1))
    os.mkdir(tmp_path / "out")
    refused(["--model", "model", "--diagnose", "--predict", "cells.sdm", "-o", "out"], "the model model holds 7", tmp_path)


def test_gibbs_refusals():
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    none = object()                                                  # (refused before the engine is used)
    with pytest.raises(ValueError, match="8 .. 4096 post-burn-in samples"):
        bpmf_amd.gibbs(none, M, Mt, T, nu, nm, nsims=12, burnin=5, diagnose=True)
    with pytest.raises(ValueError, match="8 .. 4096 post-burn-in samples"):
        bpmf_amd.gibbs(none, M, Mt, T, nu, nm, nsims=5000, burnin=5, diagnose=True)
    with pytest.raises(ValueError, match="needs a test matrix"):
        bpmf_amd.gibbs(none, M, Mt, None, nu, nm, nsims=20, burnin=5, diagnose=True)
    with pytest.raises(ValueError, match="same length"):
        bpmf_amd.gibbs(none, M, Mt, T, nu, nm, nsims=20, burnin=5, diagnose=([0, 1], [0]))
