"""Model comparison without a GPU: the restatements of tests/score_ref.py against what is known of them, the
summaries, and every refusal of `bpmf --score` and gibbs(score=True) before a GPU is touched.

  1. the library has the entry points, the ABI version is still 1
  2. score_summary and score_compare against sums worked out by hand on five cells
  3. score_ref.logdens against scipy.stats (norm, t, norm.logcdf) on one sample, and its log-sum-exp and variance on several; the
     longdouble log Phi against its own 3000-term continued fraction and lgamma against known values; the fp64 log Phi (the kernel's
     form) finite and close on -1e4 .. 40
  4. the refusals of gibbs(score=True) and of `bpmf --score`: one line, status 1
  5. the planted experiment: the restated CPU chains reproduce score_ref.PLANTED_MEASURED, and the Student-t model leads by more than
     2 paired standard errors on both sets of cells

These fail on the commit before the feature (no entry points, no tests/score_ref.py figures to hold, an unknown option prints the usage).
"""
import math
import os
import subprocess

import numpy as np
import pytest
import bpmf_amd
from tests import model_ref as mr
from tests import score_ref as sr
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
LD = np.longdouble


# ---- 1. entry points -----------------------------------------------------------------------------------------------------------------------

def test_library_has_the_entry_points():
    from bpmf_amd import _lib
    lib = _lib.load_library()
    for name in ("bpmf_hip_score_cells", "bpmf_hip_score_batch_cells", "bpmf_hip_score_last_ms"):
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None
    assert len(_lib._SIGNATURES["bpmf_hip_score_cells"][1]) == 17
    for name in ("score_cells", "score_batch_cells", "score_last_ms"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
    assert callable(bpmf_amd.score_cells) and callable(bpmf_amd.score_summary) and callable(bpmf_amd.score_compare)
    assert lib.bpmf_hip_abi_version() == 1
    assert bpmf_amd.HipEngine.LOGDENS_KINDS == dict(gaussian=0, student=1, probit=2)
    with open(os.path.join(ROOT, "include", "bpmf_hip.h")) as f:
        text = f.read()
    for name, v in bpmf_amd.HipEngine.LOGDENS_KINDS.items():
        assert "#define BPMF_HIP_LOGDENS_%s %d\n" % (name.upper(), v) in text


# ---- 2. the summaries ----------------------------------------------------------------------------------------------------------------------

def test_summary_and_compare_by_hand():
    lpd = np.array([-1.0, -2.0, -0.5, -3.0, -1.5])
    pw = np.array([0.25, 0.5, 0.0, 0.75, 0.125])
    s = bpmf_amd.score_summary(dict(lpd=lpd, pwaic=pw, samples=7))
    # elpd_i = -1.25, -2.5, -0.5, -3.75, -1.625: sum -9.625, mean -1.925, sum of squared deviations 6.2375
    assert s["n"] == 5 and s["samples"] == 7 and s["lpd_sum"] == -8.0 and s["lpd_mean"] == -1.6 and s["p_waic"] == 1.625
    assert s["elpd"] == -9.625 and s["waic"] == 19.25
    assert s["se"] == pytest.approx(math.sqrt(5 * 6.2375 / 4), rel=1e-15)
    assert s["se_lpd"] == pytest.approx(math.sqrt(5 * 3.7 / 4), rel=1e-15)          # lpd: deviations 0.6, -0.4, 1.1, -1.4, 0.1
    assert s["pwaic_above"] == 0.4
    assert sr.summary(lpd, pw)["elpd"] == s["elpd"] and sr.summary(lpd, pw)["se"] == pytest.approx(s["se"], rel=1e-15)
    other = dict(lpd=lpd - np.array([0.5, 0.0, 1.0, -0.5, 0.25]), pwaic=pw + 0.125)
    c = bpmf_amd.score_compare(dict(lpd=lpd, pwaic=pw), other)
    # lpd differences 0.5, 0, 1, -0.5, 0.25: sum 1.25, mean 0.25, squared deviations 0.0625 + 0.0625 + 0.5625 + 0.5625 + 0 = 1.25
    assert c["n"] == 5 and c["lpd_diff"] == 1.25 and c["lpd_se"] == pytest.approx(math.sqrt(5 * 1.25 / 4), rel=1e-15)
    assert c["elpd_diff"] == 1.875 and c["elpd_se"] == pytest.approx(c["lpd_se"], rel=1e-15)   # every difference moved by 0.125
    assert sr.compare(lpd, other["lpd"]) == pytest.approx((c["lpd_diff"], c["lpd_se"]), rel=1e-15)
    empty = bpmf_amd.score_summary(dict(lpd=[], pwaic=[]))
    assert empty["n"] == 0 and empty["elpd"] == 0.0 and empty["se"] == 0.0 and math.isnan(empty["lpd_mean"]) and math.isnan(empty["pwaic_above"])
    one = bpmf_amd.score_summary(dict(lpd=[-2.0], pwaic=[0.5]))
    assert one["elpd"] == -2.5 and one["se"] == 0.0 and one["pwaic_above"] == 1.0
    with pytest.raises(ValueError, match="same cells"):
        bpmf_amd.score_compare(dict(lpd=lpd, pwaic=pw), dict(lpd=lpd[:3], pwaic=pw[:3]))


# ---- 3. the restatements -------------------------------------------------------------------------------------------------------------------

def small_rings(S, K=3, n=6, m=5, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, S, K)), rng.standard_normal((m, S, K)), rng


def test_logdens_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    U, V, rng = small_rings(1)
    rows, cols = rng.integers(0, 6, 40), rng.integers(0, 5, 40)
    y = rng.standard_normal(40) * 3
    p = 0.75 + np.einsum("nk,nk->n", U[rows, 0], V[cols, 0])
    w = 0.25 + rng.random(40)
    flag = rng.integers(-1, 2, 40)
    alpha, nu = 1.7, 4.0
    for f in (sr.logdens, sr.logdens_f64):
        close = lambda got, want: np.allclose(np.asarray(got, np.float64), want, rtol=1e-13, atol=1e-13)
        lpd, pw = f(U, V, 0.75, rows, cols, y, alpha=alpha)
        assert close(lpd, stats.norm.logpdf(y, p, 1 / math.sqrt(alpha))) and not np.asarray(pw, np.float64).any()
        lpd, _ = f(U, V, 0.75, rows, cols, y, w=w, alpha=alpha)
        assert close(lpd, stats.norm.logpdf(y, p, 1 / np.sqrt(alpha * w)))
        lpd, _ = f(U, V, 0.75, rows, cols, y, w=w, flag=flag, alpha=alpha)
        want = np.where(flag == 0, stats.norm.logpdf(y, p, 1 / np.sqrt(alpha * w)), stats.norm.logcdf(flag * math.sqrt(alpha) * (p - y)))
        assert close(lpd, want)
        lpd, _ = f(U, V, 0.75, rows, cols, y, kind="student", nu=nu, alpha=alpha)
        assert close(lpd, stats.t.logpdf(y, nu, p, 1 / math.sqrt(alpha)))
        lpd, _ = f(U, V, 0.75, rows, cols, y, kind="student", nu=1.0, alpha=alpha)
        assert close(lpd, stats.cauchy.logpdf(y, p, 1 / math.sqrt(alpha)))
        lpd, _ = f(U, V, 0.75, rows, cols, y, kind="probit")
        assert close(lpd, stats.norm.logcdf(np.where(y > 0, p, -p)))


def test_logdens_over_samples():
    """lpd is the log of the mean density and pw the variance of the log density, with the alpha of every sample"""
    S = 7
    U, V, rng = small_rings(S)
    rows, cols = rng.integers(0, 6, 30), rng.integers(0, 5, 30)
    y = rng.standard_normal(30)
    alpha = 1.0 + rng.random(S)
    per = np.stack([np.asarray(sr.logdens_f64(U[:, s:s + 1], V[:, s:s + 1], 0.5, rows, cols, y, alpha=alpha[s])[0]) for s in range(S)], axis=1)
    for f in (sr.logdens, sr.logdens_f64):
        lpd, pw = (np.asarray(a, np.float64) for a in f(U, V, 0.5, rows, cols, y, alpha=alpha))
        assert np.allclose(lpd, np.log(np.mean(np.exp(per), axis=1)), rtol=1e-13) and np.allclose(pw, per.var(axis=1, ddof=1), rtol=1e-12)
    extra = rng.standard_normal((30, S))
    a = sr.logdens_f64(U, V, 0.5, rows, cols, y, alpha=alpha, extra=extra)[0]
    b = np.stack([sr.logdens_f64(U[:, s:s + 1], V[:, s:s + 1], 0.5 + extra[i, s], rows[i:i + 1], cols[i:i + 1], y[i:i + 1], alpha=alpha[s])[0][0]
                  for i in range(30) for s in range(S)]).reshape(30, S)
    assert np.allclose(a, np.log(np.mean(np.exp(b), axis=1)), rtol=1e-13)
    # far residuals: finite where the plain mean of exponentials is -inf
    lpd, pw = sr.logdens_f64(U, V, 0.5, rows, cols, y + 60.0, alpha=2.0)
    assert np.isfinite(lpd).all() and (lpd < -1000).all() and np.isfinite(pw).all()


def test_log_phi_and_lgamma():
    x = np.concatenate([-np.logspace(0, 4, 60), np.linspace(-1, 1, 41), np.logspace(0, 1.6, 40)])
    ld = sr.log_phi_ld(x)
    assert np.isfinite(ld).all() and (np.diff(ld[np.argsort(x)]) >= 0).all()
    a = np.abs(x[np.abs(x) >= 1]).astype(LD)
    assert float(np.max(np.abs(sr._log_upper_tail_ld(a) - sr._upper_tail_terms(a, 3000)))) < 2e-18
    f64 = sr.log_phi_f64(x)
    assert np.isfinite(f64).all() and sr.relative_error(f64, ld) < 1e-15
    special = pytest.importorskip("scipy.special")
    assert sr.relative_error(special.log_ndtr(x), ld) < 1e-14
    # the join of the centre series and the tail at +-1, and the symmetry Phi(x) + Phi(-x) = 1
    for v in (1.0, 0.999999, 0.5):
        s = np.exp(sr.log_phi_ld(np.array([v]))) + np.exp(sr.log_phi_ld(np.array([-v])))
        assert abs(float(s[0] - 1)) < 1e-18
    assert abs(float(sr._lgamma_ld(1.0))) < 1e-17 and abs(float(sr._lgamma_ld(2.0))) < 1e-17
    assert abs(float(sr._lgamma_ld(0.5) - np.log(sr.PI_LD) / 2)) < 1e-17
    assert abs(float(sr._lgamma_ld(5.0) - np.log(LD(24)))) < 1e-17
    assert abs(float(sr._lgamma_ld(2.5) - np.log(LD(0.75) * np.sqrt(sr.PI_LD)))) < 1e-17
    assert abs(float(sr._lgamma_ld(50.5)) - math.lgamma(50.5)) < 1e-13


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_gibbs_refusals(monkeypatch):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    none = object()                                                  # (refused before the engine is used)
    run = lambda **kw: bpmf_amd.gibbs(none, M, Mt, T, nu, nm, score=True, **kw)
    with pytest.raises(ValueError, match="score needs at least 2 post-burn-in samples"):
        run(nsims=6, burnin=5)
    with pytest.raises(ValueError, match="score does not go together with ordinal"):
        run(nsims=10, burnin=4, ordinal=True)
    with pytest.raises(ValueError, match="score does not go together with implicit"):
        run(nsims=10, burnin=4, implicit=0.1)

    class Ranks:
        def comm_nranks(self):
            return 2
    with pytest.raises(ValueError, match="score does not go together with a communicator"):
        bpmf_amd.gibbs(Ranks(), M, Mt, T, nu, nm, score=True, nsims=10, burnin=4)
    monkeypatch.setenv("BPMF_REDUCE", "1")
    with pytest.raises(ValueError, match="score does not go together with BPMF_REDUCE"):
        run(nsims=10, burnin=4)


def test_score_cells_needs_a_scorable_result():
    with pytest.raises(ValueError, match="no model_info"):
        bpmf_amd.score_cells(dict(users=None, movies=None), [0], [0], [1.0])
    with pytest.raises(ValueError, match="ordinal and implicit runs are not scored"):
        bpmf_amd.score_cells(dict(users=None, movies=None, model_info=dict(scored=False)), [0], [0], [1.0])


def refused(args, reason, cwd, env=None):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 1 and p.stdout == "", (args, p.stdout, p.stderr)
    lines = p.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("bpmf: ") and reason in lines[0], (args, p.stderr)


def test_cli_refusals(tmp_path):
    base = ["-n", "train.sdm", "-p", "test.sdm", "--score"]         # (nothing is read before the refusal)
    refused(base + ["-i", 6, "-b", 5], "at least 2 post-burn-in samples", tmp_path)
    refused(base + ["-i", 20, "-b", 5, "-g", 2], "one GPU without -g", tmp_path)
    refused(base + ["-i", 20, "-b", 5], "BPMF_REDUCE=1", tmp_path, env={"BPMF_REDUCE": "1"})
    refused(base + ["-i", 20, "-b", 5, "-m", "mu.ddm", "-l", "lambda.ddm"], "propagated posterior", tmp_path)
    refused(base + ["-i", 20, "-b", 5, "--ordinal"], "--score does not go together with --ordinal", tmp_path)
    refused(base + ["-i", 20, "-b", 5, "--implicit", 0.1], "--score does not go together with --implicit", tmp_path)
    refused(["--tensor", "x.tns", "--score", "-i", 20, "-b", 5], "--tensor", tmp_path)
    refused(["--model", "model", "--score", "--topn", 3, "-o", "out"], "needs --predict FILE", tmp_path)
    # a model with one sample: read, then refused before a context is created
    bpmf_amd.write_model(tmp_path / "model", mr.random_model(4, 6, 5, 1, seed=1))
    os.mkdir(tmp_path / "out")
    refused(["--model", "model", "--score", "--predict", "cells.sdm", "-o", "out"], "the model model holds 1", tmp_path)


# ---- 5. the planted experiment -------------------------------------------------------------------------------------------------------------

def test_planted_figures_are_reproduced(oracle):
    got = sr.planted_measure(oracle)
    want = sr.PLANTED_MEASURED
    for key in ("test", "train"):
        assert got[key] == pytest.approx(want[key], rel=1e-6), key
        diff, se = got[key]
        print("%s: difference %.2f, paired se %.2f: %.1f se" % (key, diff, se, diff / se))
        assert diff > 2 * sr.PLANTED_MARGIN_SE * se                # a visible gap over the margin the GPU test asks for
    for name in ("student", "gaussian"):
        for k, v in want[name].items():
            assert got[name][k] == pytest.approx(v, rel=1e-6), (name, k)
