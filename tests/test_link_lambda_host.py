"""A sampled link precision lambda_beta, CPU part:

  * bpmf_hip_link_lambda_sample is the Gamma draw of the oracle on the stream BPMF_LINK_LAMBDA_COUNTER(iter, tag), bit for bit,
    shapes below 1 included; its counter range is apart from the hyper-parameter and noise streams
  * the conditional Gamma(A0 + D K / 2, B0 + t / 2), checked statistically on the restatement for a fixed beta and Lambda
  * argument refusals of every new entry point; BPMF_HIP_ENODEV, not a crash, where a device is needed and there is none
  * gibbs argument checks and the `bpmf --lambda-beta-prior` refusals
  * the planted experiment through the restated chain with the real stream: a sampled lambda_beta started at 500 recovers what a
    fixed 500 loses on cold rows
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bpmf_amd
from bpmf_amd import _lib, engine
from tests import link_lambda_ref as lref
from tests import link_ref as ref
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
EINVAL, ENODEV = -1, -2

NEW = ("bpmf_hip_link_lambda_sample", "bpmf_hip_side_link_lambda_prior", "bpmf_hip_side_link_lambda_set", "bpmf_hip_side_link_lambda_get",
       "bpmf_hip_link_chol_solve")


def run(args, cwd):
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_lambda_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    lib = _lib.load_library()
    sigs = _lib.exported_signatures()
    for name in NEW:
        assert hasattr(raw, name) and name in sigs, name
        assert getattr(lib, name).argtypes == sigs[name][1]
    assert lib.bpmf_hip_abi_version() == 1


# (a0, b0, trace, D, K, it, tag): D = K = 1 with a small a0 puts the shape below 1 (libstdc++ then boosts it and corrects by a power)
DRAWS = [(5e-4, 5e-4, 3.25, 16, 8, 1, 3), (5e-4, 5e-4, 1234.5, 1024, 64, 7, 4), (5e-4, 5e-4, 0.75, 1, 1, 2, 1), (0.25, 0.0, 1e-3, 1, 1, 5, 15),
          (2.0, 10.0, 0.0, 5, 10, 0, 4), (5e-4, 5e-4, 4.0e5, 2048, 100, 2 ** 27 - 1, 3)]


@pytest.mark.parametrize("a0,b0,t,D,K,it,tag", DRAWS)
def test_lambda_sample_is_the_oracle_draw(oracle, a0, b0, t, D, K, it, tag):
    g, _ = oracle.gamma_stream(lref.counter(it, tag), [a0 + D * K / 2])
    want = g[0] / (b0 + t / 2)
    got = bpmf_amd.link_lambda_sample(a0, b0, t, D * K, it, tag)
    assert np.float64(got).tobytes() == np.float64(want).tobytes(), (got, want)
    assert lref.draw_lambda(oracle, a0, b0, t, D, K, it, tag) == got      # the restatement's draw is the same number
    assert engine.link_lambda_counter(it, tag) == lref.counter(it, tag)


def test_lambda_counters_are_apart_from_the_other_streams():
    """Hyper-parameter streams count up from 0 (counter = iteration), noise streams count down from 2^32 - 1.  For it < 2^27 and
    1 <= tag <= 15 the lambda_beta counters lie in [2^31 + 1, 2^32 - 1] without wrapping: above every hyper counter of such an
    iteration, and two (it, tag) pairs never share one.  Against the noise counters 2^32 - 1 - it' the claim "apart for it < 2^27"
    holds with one qualification, which this test pins: counter(it, tag) = noise(it') needs 16 it + tag + it' = 2^31 - 1, so the two
    ranges are disjoint for all it' < 2^27 only while it < 2^27 - 2^23, and within ONE chain (it' <= it) while it < (2^31 - 16) / 17
    = 126 322 567 iterations.  (A side with features refuses the adaptive noise, so no chain draws from both today.)"""
    top = 2 ** 27 - 1
    lo, hi = lref.counter(0, 1), lref.counter(top, 15)
    assert lo == 0x80000001 and hi == 0xFFFFFFFF                         # no wrap up to it = 2^27 - 1
    assert 0x80000000 + 16 * top + 15 == hi
    assert lo > top                                                      # hyper streams: 0 .. 2^27 - 1
    safe = 2 ** 27 - 2 ** 23 - 1                                         # the last it whose counters stay below every noise counter
    assert lref.counter(safe, 15) < 0xFFFFFFFF - top <= lref.counter(safe + 1, 15)
    one_chain = (2 ** 31 - 16) // 17
    assert lref.counter(one_chain - 1, 15) < 0xFFFFFFFF - (one_chain - 1)
    its = np.concatenate([np.arange(0, 4096), np.arange(top - 4096, top + 1)])
    seen = set()
    for tag in range(1, 16):
        c = {lref.counter(int(i), tag) for i in its}
        assert len(c) == len(its) and not (c & seen)
        seen |= c
    assert all(lo <= c <= hi for c in seen)


def test_conditional_of_lambda_on_the_restatement(oracle):
    """For a fixed beta (D x K) and Lambda: 3 000 draws of the restated step (iterations 1 .. 3 000 of one tag) have the mean and
    variance of Gamma(shape A0 + D K / 2, rate B0 + t / 2) within 5 standard errors.  With shape a and rate b the mean is a / b, the
    variance a / b^2; the standard error of the sample variance of a Gamma is var sqrt((2 + 6 / a) / n)."""
    rng = np.random.default_rng(15)
    D, K, n = 6, 4, 3000
    a0, b0 = 0.5, 0.25
    beta = rng.standard_normal((D, K))
    R = np.triu(rng.standard_normal((K, K))) + 3.0 * np.eye(K)
    t = lref.trace(beta, R)
    assert abs(t - np.trace(R.T @ R @ beta.T @ beta)) <= 1e-12 * t         # t = tr(Lambda beta^T beta)
    draws = np.array([lref.draw_lambda(oracle, a0, b0, t, D, K, it, 3) for it in range(1, n + 1)])
    a, b = a0 + D * K / 2, b0 + t / 2
    mean, var = a / b, a / b ** 2
    se_mean, se_var = math.sqrt(var / n), var * math.sqrt((2.0 + 6.0 / a) / n)
    print("mean %.6g (want %.6g, %.2f se), var %.6g (want %.6g, %.2f se)" % (draws.mean(), mean, (draws.mean() - mean) / se_mean,
                                                                            draws.var(ddof=1), var, (draws.var(ddof=1) - var) / se_var))
    assert abs(draws.mean() - mean) <= 5 * se_mean
    assert abs(draws.var(ddof=1) - var) <= 5 * se_var


def test_lambda_sample_refusals():
    ok = dict(a0=1.0, b0=1.0, trace=2.0, count=8, it=1, tag=3)
    assert bpmf_amd.link_lambda_sample(**ok) > 0
    bad = [dict(a0=0.0), dict(a0=-1.0), dict(a0=math.nan), dict(a0=math.inf), dict(b0=-1.0), dict(b0=math.nan), dict(b0=math.inf),
           dict(trace=-1.0), dict(trace=math.nan), dict(trace=math.inf), dict(count=0), dict(count=-3), dict(tag=0), dict(tag=16),
           dict(it=-1), dict(it=2 ** 27), dict(b0=0.0, trace=0.0)]
    for change in bad:
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            bpmf_amd.link_lambda_sample(**dict(ok, **change))
        assert e.value.code == EINVAL, change
    with pytest.raises(bpmf_amd.BpmfHipError, match="without a rate"):
        bpmf_amd.link_lambda_sample(1.0, 0.0, 0.0, 8, 1, 3)
    lib = _lib.load_library()
    assert lib.bpmf_hip_link_lambda_sample(1.0, 1.0, 2.0, 8, 1, 3, None) == EINVAL


def test_null_and_range_arguments_are_refused():
    lib = _lib.load_library()
    out = C.c_double()
    assert lib.bpmf_hip_side_link_lambda_prior(None, 1.0, 1.0) == EINVAL
    assert lib.bpmf_hip_side_link_lambda_set(None, 5.0) == EINVAL
    assert lib.bpmf_hip_side_link_lambda_get(None, C.byref(out), None, None) == EINVAL
    A, P, X = np.eye(2), np.ones((2, 1)), np.zeros((2, 1))
    ptr = engine._ptr
    assert lib.bpmf_hip_link_chol_solve(0, None, 2, ptr(P), None, 1, ptr(X), None) == EINVAL
    assert lib.bpmf_hip_link_chol_solve(0, ptr(A), 2, None, None, 1, ptr(X), None) == EINVAL
    assert lib.bpmf_hip_link_chol_solve(0, ptr(A), 2, ptr(P), None, 1, None, None) == EINVAL
    for D, n in ((0, 1), (1025, 1), (2, 0), (2, 129)):
        assert lib.bpmf_hip_link_chol_solve(0, ptr(A), D, ptr(P), None, n, ptr(X), None) == EINVAL, (D, n)
        assert lib.bpmf_hip_last_error()
    with pytest.raises(ValueError):
        engine.link_chol_solve(np.eye(3), np.ones((2, 1)))
    with pytest.raises(ValueError):
        engine.link_chol_solve(np.eye(2), np.ones((2, 1)), np.ones((2, 2)))


def test_chol_solve_needs_a_device():
    """Without a HIP device the factorisation reports BPMF_HIP_ENODEV: no crash, no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        engine.link_chol_solve(np.eye(4), np.ones((4, 2)))
    assert e.value.code == ENODEV


def test_gibbs_refuses_bad_lambda_beta_priors():
    F = np.zeros((1, 1))
    with pytest.raises(ValueError, match="lambda_beta_prior needs row_features or col_features"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, lambda_beta_prior=(1.0, 1.0))
    for prior in ((0.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (math.nan, 1.0), (1.0, math.inf), (1.0,), (1.0, 2.0, 3.0), 5.0, ("a", "b")):
        with pytest.raises(ValueError, match="lambda_beta_prior"):
            bpmf_amd.gibbs(None, None, None, None, 1, 1, row_features=F, lambda_beta_prior=prior)
    with pytest.raises(ValueError, match="pipelined=True"):              # the refusals of the features loop stay in front
        bpmf_amd.gibbs(None, None, None, None, 1, 1, row_features=F, lambda_beta_prior=(1.0, 1.0), pipelined=True)


def test_cli_lambda_beta_prior_refusals(tmp_path):
    from bpmf_amd import io
    nu = util.tiny()[4]
    io.write_dense(tmp_path / "rows.ddm", ref.features(nu, 3, 1))
    rows = ["--row-features", "rows.ddm"]
    r = run(data_args() + ["--lambda-beta-prior", "1,1", "-o", str(tmp_path)], tmp_path)
    assert r.returncode != 0 and "--lambda-beta-prior needs --row-features or --col-features" in r.stderr
    for prior in ("1", "1,", ",1", "a,b", "1,2,3", "1;1"):
        r = run(data_args() + rows + ["--lambda-beta-prior", prior, "-o", str(tmp_path)], tmp_path)
        assert r.returncode != 0 and "--lambda-beta-prior expects A0,B0" in r.stderr, prior
        assert "num_latent" not in r.stdout                              # stopped before Sys::init printed anything
    for prior in ("0,1", "-1,1", "1,-1", "nan,1", "1,inf"):
        r = run(data_args() + rows + ["--lambda-beta-prior", prior, "-o", str(tmp_path)], tmp_path)
        assert r.returncode != 0 and "--lambda-beta-prior expects a shape A0 > 0 and a rate B0 >= 0" in r.stderr, prior
    assert not (tmp_path / "lambda_beta.csv").exists()
    r = run(data_args() + rows + ["--lambda-beta-prior", "1,1", "--probit"], tmp_path)     # the refusals of the features stay
    assert r.returncode != 0 and "do not go together with --probit" in r.stderr


def test_cli_usage_names_the_flag(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "--lambda-beta-prior A0,B0" in text and "lambda_beta.csv" in text and "burn-in" in text


def test_planted_sampled_lambda_recovers_cold_rows(oracle):
    """tests/link_ref.py::PLANTED with 120 iterations, 60 of them burn-in, through the restated chain with the real stream; user
    features, K = 8, the default prior Gamma(5e-4, 5e-4).  Measured on the CPU before this test was written (warm / cold-row RMSE):

        fixed lambda_beta = 500          0.9663 / 1.4626
        fixed lambda_beta = 5            0.7291 / 0.7794
        sampled from a start of 500      0.7266 / 0.7750     (lambda_beta: 1006 at iteration 1, 1712 at 5, 12.3 at 38, 1.59 at 58,
                                                              1.02 .. 2.11 over iterations 60 .. 119)

    The margin of sampled over fixed 500 on cold rows, 0.6876, is asserted at half its size; sampled may be no worse than fixed 5 by
    more than 0.05 (it is better by 0.0044)."""
    runs = lref.planted_runs(oracle)
    M, Mt, T, Tt, F, cold = runs["data"]
    assert len(T[2]) == 2992 and int(cold.sum()) == 1200
    score = {k: ref.split_rmse(runs[k]["pred"], T, cold) for k in ("fixed500", "fixed5", "sampled")}
    lam = runs["sampled"]["lambda_rows"]
    print("warm / cold: " + ", ".join("%s %.4f / %.4f" % (k, v[0], v[1]) for k, v in score.items()))
    print("lambda_beta: %s ... at 40 %.3g, at 60 %.3g, 60 .. 119 in [%.3g, %.3g]" % (["%.4g" % v for v in lam[:6]], lam[40], lam[60],
                                                                                    min(lam[60:]), max(lam[60:])))
    assert len(lam) == 120 and lam[0] == 500.0 and runs["fixed5"]["lambda_rows"] == [5.0] * 120
    assert score["fixed500"][1] - score["sampled"][1] >= 0.5 * 0.6876
    assert score["sampled"][1] <= score["fixed5"][1] + 0.05
