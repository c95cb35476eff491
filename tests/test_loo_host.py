"""PSIS-LOO without a GPU: the restatement of tests/loo_ref.py against what is known independently of it, the
summary, and every refusal of `bpmf --loo` and gibbs(loo=True) before a GPU is touched.

  1. the library has the four entry points, the ABI version is still 1
  2. the fp64 form of the rule agrees with its longdouble form to the rounding level, over S in 25 .. 4096 and khat up to above 10;
     nothing is smoothed below S = 25, on a constant tail and across a tie at x*; a trace that is not finite gives NaN for itself alone
  3. the generalised Pareto fit recovers the shape of seeded scipy.stats.genpareto draws within 4 asymptotic standard errors
  4. a closed-form toy model: y_i ~ N(theta, 1) with a flat prior, where the exact leave-one-out density is N(y_i; mean of the others,
     1 + 1 / (n - 1)): the mean of elpd_loo over 20 replications lies within 4 of its standard errors of the exact one
  5. loo_summary on five cells worked out by hand; score_compare on elpd_loo arrays
  6. the refusals of gibbs(loo=True) and of `bpmf --loo`: one line, status 1

1, 5 and 6 fail on the commit before the feature (no entry points, no loo_summary, no loo= argument, an unknown option prints the
usage); 2, 3 and 4 hold tests/loo_ref.py, which the GPU tests take as the truth, to what is known independently of it.
"""
import math
import os
import subprocess

import numpy as np
import pytest
import bpmf_amd
from tests import loo_ref as lr
from tests import model_ref as mr
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")


# ---- 1. entry points -----------------------------------------------------------------------------------------------------------------------

def test_library_has_the_entry_points():
    from bpmf_amd import _lib
    lib = _lib.load_library()
    for name in ("bpmf_hip_loo_cells", "bpmf_hip_loo_traces", "bpmf_hip_loo_batch_cells", "bpmf_hip_loo_last_ms"):
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None
    assert len(_lib._SIGNATURES["bpmf_hip_loo_cells"][1]) == 18 and len(_lib._SIGNATURES["bpmf_hip_loo_traces"][1]) == 7
    for name in ("loo_cells", "loo_traces", "loo_batch_cells", "loo_last_ms"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
    assert callable(bpmf_amd.loo_cells) and callable(bpmf_amd.loo_summary)
    assert lib.bpmf_hip_abi_version() == 1
    with open(os.path.join(ROOT, "include", "bpmf_hip.h")) as f:
        assert "#define BPMF_HIP_LOO_MAX_SAMPLES %d\n" % bpmf_amd.HipEngine.LOO_MAX_SAMPLES in f.read()
    assert lr.MAX_SAMPLES == bpmf_amd.HipEngine.LOO_MAX_SAMPLES == 4096


# ---- 2. the rule ---------------------------------------------------------------------------------------------------------------------------

def gaussian_traces(rng, n, S, spread):
    """log densities of y ~ N(0, 1) under S draws of a mean with the given spread: khat grows with the spread"""
    th = rng.standard_normal((n, S)) * spread
    y = rng.standard_normal((n, 1))
    return -0.5 * math.log(2 * math.pi) - 0.5 * (y - th) ** 2


def test_tail_length_and_edges():
    assert [lr.tail_length(S) for S in (1, 4, 5, 24, 25, 26, 224, 225, 226, 1000, 4096)] == [0, 0, 1, 4, 5, 5, 44, 45, 45, 95, 192]
    for S in range(1, 4097):                                             # the integer form is the formula, and M <= 192
        assert lr.tail_length(S) == min(int(math.floor(0.2 * S + 1e-9)), int(math.ceil(3 * math.sqrt(S) - 1e-9))) <= 192
    rng = np.random.default_rng(5)
    for S in (1, 2, 24):                                                 # M < 5: plain importance sampling, khat = +inf
        L = gaussian_traces(rng, 6, S, 1.0)
        r = lr.psis(L)
        assert np.isposinf(r["khat"]).all()
        want = -np.log(np.mean(np.exp(-(L - L.max(axis=1, keepdims=True))), axis=1)) + L.max(axis=1)   # the harmonic mean of the densities
        assert np.allclose(r["elpd_loo"], want, rtol=1e-13, atol=1e-13)
        assert np.allclose(r["lpd"], np.log(np.mean(np.exp(L), axis=1)), rtol=1e-13, atol=1e-13)
    S = 100                                                              # M = 20
    body = gaussian_traces(rng, 4, S, 1.0)
    const = body.copy()
    const[:, :20] = body.min(axis=1, keepdims=True) - 1.0                # a constant tail over a varying body
    tie = np.sort(body, axis=1)
    tie[:, 10:21] = tie[:, 10:11]                                        # a tie from x* (index 5: position 15) across the cutoff: x* = 0
    for L in (const, tie, np.zeros((3, S))):
        assert np.isposinf(lr.psis(L)["khat"]).all() and np.isposinf(lr.psis(L, np.longdouble)["khat"]).all()
    ok = gaussian_traces(rng, 5, S, 1.0)
    bad = ok.copy()
    bad[1, 7] = np.nan; bad[3, 0] = -np.inf; bad[4, 99] = np.inf
    a, b = lr.psis(ok), lr.psis(bad)
    for key in ("elpd_loo", "khat", "lpd"):
        assert np.isnan(b[key][[1, 3, 4]]).all() and np.array_equal(b[key][[0, 2]], a[key][[0, 2]])


@pytest.mark.parametrize("S", [25, 64, 225, 1000, 4096])
def test_fp64_rule_against_longdouble(S):
    """The two forms of the rule agree to the rounding level.  The bars are reasoned, not measured: a term of the final sums rounds a few
    times at the magnitude A = max(1, max |l_s|) (rho = a_0 - a_i, lw + a_i, the subtraction of the maximum, the difference of the two
    log-sum-exps), so lpd is held to 32 ulp(A); khat is a smooth function of the tail through L_j = M (..) with |L_j| up to about 1e4
    carrying a few ulp each, which the softmax turns into relative errors of the weights of about 1e-11: held to 1e-10 max(1, |khat|);
    a smoothed log weight moves with khat by at most t_j <= log(2 M), so elpd_loo is held to 32 ulp(A) plus log(2 M) times the bar of
    khat.  Seen on the CPU: lpd at most 0.03 of its bar, khat at most 2e-12 (S = 25, where five points are fitted), elpd_loo at most 2e-13."""
    rng = np.random.default_rng(S)
    M = lr.tail_length(S)
    seen = 0.0
    for spread in (0.3, 1.5, 4.0):
        L = gaussian_traces(rng, 24, S, spread)
        f, g, err = lr.rule_error(L)
        A = max(1.0, float(np.abs(L).max()))
        bar = 32 * 2.0 ** -52 * A
        kbar = 1e-10 * np.maximum(1.0, np.abs(f["khat"]))
        print("S = %d spread %.1f: errors %r, bar %.3g, khat %.2f .. %.2f" % (S, spread, err, bar, f["khat"].min(), f["khat"].max()))
        assert err["lpd"] <= bar
        assert np.all(np.abs(f["khat"] - g["khat"].astype(np.float64)) <= kbar)
        assert np.all(np.abs(f["elpd_loo"] - g["elpd_loo"].astype(np.float64)) <= bar + math.log(2 * M) * kbar)
        seen = max(seen, float(f["khat"].max()))
    assert seen > 10.0 or S < 225                                        # the family reaches khat above 10


# ---- 3. the generalised Pareto fit -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [192, 10 ** 4])
def test_gpd_fit_recovers_the_shape(M):
    from scipy import stats
    worst = 0.0
    for k in (-0.3, 0.0, 0.3, 0.7, 1.2):
        for seed in range(10):
            x = np.sort(stats.genpareto.rvs(k, size=M, random_state=seed))[None, :]
            kfit, sigma, khat, ok = lr.gpd_fit(x)
            assert ok[0] and khat[0] == pytest.approx((kfit[0] * M + 5) / (M + 10), rel=1e-14)
            worst = max(worst, abs(kfit[0] - k) / ((1 + k) / math.sqrt(M)))
    print("M = %d: worst |k - k0| = %.2f asymptotic standard errors" % (M, worst))
    assert worst <= 4.0


# ---- 4. the closed-form toy model ------------------------------------------------------------------------------------------------------------

def test_toy_model_against_exact_loo():
    n, S, reps = 20, 4000, 20
    rng = np.random.default_rng(2024)
    y = rng.standard_normal(n)
    y[0] = 3.5                                                           # one planted outlier
    ybar = y.mean()
    others = (n * ybar - y) / (n - 1)
    v = 1.0 + 1.0 / (n - 1)
    exact = -0.5 * np.log(2 * np.pi * v) - 0.5 * (y - others) ** 2 / v   # log N(y_i; mean of the others, 1 + 1 / (n - 1))
    est, khat = [], []
    for rep in range(reps):
        theta = ybar + np.random.default_rng(1000 + rep).standard_normal(S) / math.sqrt(n)     # exact posterior draws
        r = lr.psis(-0.5 * math.log(2 * math.pi) - 0.5 * (y[:, None] - theta[None, :]) ** 2)
        est.append(r["elpd_loo"]); khat.append(r["khat"])
    est = np.array(est)
    for what, got, want in (("the outlier", est[:, 0], exact[0]), ("the sum", est.sum(axis=1), exact.sum())):
        se = got.std(ddof=1) / math.sqrt(reps)
        print("%s: mean %.5f exact %.5f: %.2f standard errors; khat of the outlier %.2f" % (what, got.mean(), want, abs(got.mean() - want) / se, np.mean(khat, axis=0)[0]))
        assert abs(got.mean() - want) <= 4.0 * se
    assert np.max(khat) < 0.7


# ---- 5. the summary --------------------------------------------------------------------------------------------------------------------------

def test_summary_by_hand():
    elpd = np.array([-1.25, -2.5, -0.5, -3.75, -1.625])
    lpd = np.array([-1.0, -2.0, -0.5, -3.0, -1.5])
    khat = np.array([0.25, 0.6, 0.75, 1.5, np.inf])
    s = bpmf_amd.loo_summary(dict(elpd_loo=elpd, khat=khat, lpd=lpd, samples=100))
    # sum -9.625, mean -1.925, squared deviations 6.2375; p_loo = 0.25 + 0.5 + 0 + 0.75 + 0.125
    assert s["n"] == 5 and s["samples"] == 100 and s["elpd_loo"] == -9.625 and s["looic"] == 19.25 and s["p_loo"] == 1.625
    assert s["se"] == pytest.approx(math.sqrt(5 * 6.2375 / 4), rel=1e-15)
    assert s["khat_counts"] == dict(good=1, ok=1, bad=1, very_bad=1, inf=1) and s["n_nan"] == 0
    assert s["khat_threshold"] == 0.5 and s["khat_above"] == 0.8 and s["khat_above_07"] == 0.6        # 1 - 1 / log10(100)
    assert bpmf_amd.loo_summary(dict(elpd_loo=elpd, khat=khat, lpd=lpd, samples=4000))["khat_threshold"] == 0.7
    ref = lr.loo_summary_ref(elpd, khat, lpd, 100)
    assert (ref["elpd_loo"], ref["p_loo"], ref["looic"], ref["threshold"]) == (s["elpd_loo"], s["p_loo"], s["looic"], s["khat_threshold"])
    assert ref["se"] == pytest.approx(s["se"], rel=1e-15)
    withnan = bpmf_amd.loo_summary(dict(elpd_loo=elpd, khat=np.array([0.25, np.nan, 0.75, 1.5, np.inf]), lpd=lpd, samples=100))
    assert withnan["n_nan"] == 1 and withnan["khat_counts"] == dict(good=1, ok=0, bad=1, very_bad=1, inf=1)
    empty = bpmf_amd.loo_summary(dict(elpd_loo=[], khat=[], lpd=[], samples=50))
    assert empty["n"] == 0 and empty["elpd_loo"] == 0.0 and empty["se"] == 0.0 and math.isnan(empty["khat_above"])
    # two runs compared by their per-cell elpd_loo: differences 0.5, 0, 1, -0.5, 0.25
    other = elpd - np.array([0.5, 0.0, 1.0, -0.5, 0.25])
    c = bpmf_amd.score_compare(elpd, other)
    assert c == dict(n=5, elpd_diff=1.25, elpd_se=pytest.approx(math.sqrt(5 * 1.25 / 4), rel=1e-15))
    d = bpmf_amd.score_compare(dict(elpd_loo=elpd, lpd=lpd), dict(elpd_loo=other, lpd=lpd - 0.5))
    assert d["elpd_diff"] == 1.25 and d["lpd_diff"] == 2.5 and d["lpd_se"] == 0.0
    with pytest.raises(ValueError, match="same cells"):
        bpmf_amd.score_compare(elpd, other[:3])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------

def test_gibbs_refusals(monkeypatch):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    none = object()                                                  # (refused before the engine is used)
    run = lambda **kw: bpmf_amd.gibbs(none, M, Mt, T, nu, nm, loo=True, **kw)
    with pytest.raises(ValueError, match="loo needs 2 .. 4096 post-burn-in samples"):
        run(nsims=6, burnin=5)
    with pytest.raises(ValueError, match="loo needs 2 .. 4096 post-burn-in samples"):
        run(nsims=4102, burnin=5)
    with pytest.raises(ValueError, match="loo does not go together with ordinal"):
        run(nsims=10, burnin=4, ordinal=True)
    with pytest.raises(ValueError, match="loo does not go together with implicit"):
        run(nsims=10, burnin=4, implicit=0.1)

    class Ranks:
        def comm_nranks(self):
            return 2
    with pytest.raises(ValueError, match="loo does not go together with a communicator"):
        bpmf_amd.gibbs(Ranks(), M, Mt, T, nu, nm, loo=True, nsims=10, burnin=4)
    monkeypatch.setenv("BPMF_REDUCE", "1")
    with pytest.raises(ValueError, match="loo does not go together with BPMF_REDUCE"):
        run(nsims=10, burnin=4)


def test_loo_cells_needs_a_scorable_result():
    with pytest.raises(ValueError, match="loo_cells: the result carries no model_info"):
        bpmf_amd.loo_cells(dict(users=None, movies=None), [0], [0], [1.0])
    with pytest.raises(ValueError, match="loo_cells: ordinal and implicit runs are not scored"):
        bpmf_amd.loo_cells(dict(users=None, movies=None, model_info=dict(scored=False)), [0], [0], [1.0])


def refused(args, reason, cwd, env=None):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 1 and p.stdout == "", (args, p.stdout, p.stderr)
    lines = p.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("bpmf: ") and reason in lines[0], (args, p.stderr)


def test_cli_refusals(tmp_path):
    base = ["-n", "train.sdm", "-p", "test.sdm", "--loo"]           # (nothing is read before the refusal)
    refused(base + ["-i", 6, "-b", 5], "--loo needs 2 .. 4096 post-burn-in samples", tmp_path)
    refused(base + ["-i", 4102, "-b", 5], "--loo needs 2 .. 4096 post-burn-in samples", tmp_path)
    refused(base + ["-i", 20, "-b", 5, "-g", 2], "--loo runs on one GPU without -g", tmp_path)
    refused(base + ["-i", 20, "-b", 5], "--loo does not go together with BPMF_REDUCE=1", tmp_path, env={"BPMF_REDUCE": "1"})
    refused(base + ["-i", 20, "-b", 5, "-m", "mu.ddm", "-l", "lambda.ddm"], "--loo does not go together with a propagated posterior", tmp_path)
    refused(base + ["-i", 20, "-b", 5, "--ordinal"], "--loo does not go together with --ordinal", tmp_path)
    refused(base + ["-i", 20, "-b", 5, "--implicit", 0.1], "--loo does not go together with --implicit", tmp_path)
    refused(["--tensor", "x.tns", "--loo", "-i", 20, "-b", 5], "--loo does not go together with --tensor", tmp_path)
    refused(["--model", "model", "--loo", "-o", "out"], "--loo with --model needs -n TRAIN", tmp_path)
    refused(["--model", "model", "--loo", "--predict", "cells.sdm", "-o", "out"], "--loo with --model needs -n TRAIN", tmp_path)
    # a model with one sample: read, then refused before a context is created
    bpmf_amd.write_model(tmp_path / "model", mr.random_model(4, 6, 5, 1, seed=1))
    os.mkdir(tmp_path / "out")
    refused(["--model", "model", "--loo", "-n", "train.sdm", "-o", "out"], "--loo needs 2 .. 4096 samples, the model model holds 1", tmp_path)
