"""Probit likelihood, CPU part: bpmf_hip_auc against a pair count; the restatement of the latent draw (tests/probit_ref.py) is a
truncated normal, and no accept / reject decision of it lies within 1e-9 of its threshold for the inputs the GPU parity test
(tests/test_gpu_probit.py) uses; the `bpmf` flags --probit / --probit-threshold and gibbs(probit=True) refuse what they cannot do
before anything touches a GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bpmf_amd
from bpmf_amd import _lib
from tests import probit_ref as ref
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
EINVAL = -1
MARGIN = 1e-9          # no comparison of the restatement may be closer to its threshold than this (the GPU differs by ~1e-15)


def run(args, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=e)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_probit_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    lib = _lib.load_library()
    sigs = _lib.exported_signatures()
    for name in ("bpmf_hip_side_set_probit", "bpmf_hip_side_probit_latent", "bpmf_hip_test_probit_add", "bpmf_hip_test_probit_get",
                 "bpmf_hip_auc"):
        assert hasattr(raw, name) and name in sigs
    assert lib.bpmf_hip_abi_version() == 1
    for name in ("set_probit", "probit_latent", "probit_add", "probit_get"):
        assert callable(getattr(bpmf_amd.HipEngine, name))


def test_auc_against_pair_count():
    rng = np.random.default_rng(5)
    for n, frac in ((1, 0.5), (2, 0.5), (50, 0.5), (1500, 0.3), (1500, 0.9)):
        for _ in range(3):
            score = np.round(rng.random(n), 1)                          # eleven distinct values: many ties
            label = (rng.random(n) < frac).astype(np.float64)
            num, den = ref.auc_pairs(score, label)
            got = bpmf_amd.auc(score, label)
            if den == 0:
                assert math.isnan(got)
            else:
                assert abs(got - num / den) <= 1e-15, (n, got, num / den)
    # labels through a threshold; scores may be anything finite
    score = rng.standard_normal(400) * 1e3
    value = rng.integers(1, 6, 400).astype(np.float64)
    num, den = ref.auc_pairs(score, value > 3.0)
    assert abs(bpmf_amd.auc(score, value, threshold=3.0) - num / den) <= 1e-15


def test_auc_special_cases():
    label = np.array([0, 0, 1, 1, 1, 0], np.float64)
    assert bpmf_amd.auc(label * 2.0 - 7.0, label) == 1.0                 # perfect
    assert bpmf_amd.auc(-label, label) == 0.0                            # inverted
    assert bpmf_amd.auc(np.full(6, 0.25), label) == 0.5                  # constant
    assert math.isnan(bpmf_amd.auc(np.arange(4.0), np.ones(4)))          # one class
    assert math.isnan(bpmf_amd.auc(np.arange(4.0), np.zeros(4)))
    assert math.isnan(bpmf_amd.auc(np.zeros(0), np.zeros(0)))
    lib = _lib.load_library()
    out = C.c_double()
    a = np.zeros(3)
    p = a.ctypes.data_as(C.c_void_p)
    assert lib.bpmf_hip_auc(None, p, 3, 0.5, C.byref(out)) == EINVAL
    assert lib.bpmf_hip_auc(p, None, 3, 0.5, C.byref(out)) == EINVAL
    assert lib.bpmf_hip_auc(p, p, 3, 0.5, None) == EINVAL
    assert lib.bpmf_hip_auc(p, p, -1, 0.5, C.byref(out)) == EINVAL
    bad = np.array([0.0, np.nan, 1.0])
    assert lib.bpmf_hip_auc(bad.ctypes.data_as(C.c_void_p), p, 3, 0.5, C.byref(out)) == EINVAL
    with pytest.raises(ValueError):
        bpmf_amd.auc(np.zeros(3), np.zeros(4))


def test_restated_philox_is_the_oracles(oracle):
    rng = np.random.default_rng(9)
    ctr = rng.integers(0, 2 ** 32, (64, 4), dtype=np.uint64)
    ctr[0] = 0; ctr[1] = 2 ** 32 - 1
    for tag in (1, 2, 0):
        w = np.stack(ref.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], 42, tag), axis=1)
        for i in range(len(ctr)):
            assert list(oracle.philox(ctr[i].astype(np.uint32), [42, tag])) == list(w[i].astype(np.uint32)), (i, tag)
    # rating positions beyond 2^32 use the second counter word
    a = ref.philox4x32_10(np.array([5]), np.array([1]), 3, 0, 42, 1)
    assert [int(x[0]) for x in a] == [int(x) for x in oracle.philox([5, 1, 3, 0], [42, 1])]


def test_restated_draw_is_a_truncated_normal():
    from scipy.stats import norm
    rng = np.random.default_rng(2026)
    n = 10 ** 6
    m = rng.standard_normal(n) * 1.5
    s = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    z, attempts, margin, _ = ref.truncated_draw(np.arange(n), 3, ref.TAG_MOVIES, m, s)
    print("attempts: mean %.4f, max %d; closest comparison %.3g" % (attempts.mean(), attempts.max(), margin))
    assert np.all(np.isfinite(z)) and np.all(z * s > 0)                  # every score has the sign of its label
    assert attempts.max() < ref.MAX_ATTEMPTS and attempts.mean() < 1.2
    assert margin >= MARGIN
    # E[s z | mu] = mu + phi(mu) / Phi(mu), Var = 1 - d (d + mu), d = phi / Phi: the mean of every bucket of mu within 4 standard errors
    mu = s * m
    edges = np.arange(-6.0, 6.5, 0.5)
    checked = 0
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (mu >= lo) & (mu < hi)
        if sel.sum() < 30:
            continue
        d = np.exp(norm.logpdf(mu[sel]) - norm.logcdf(mu[sel]))
        want = mu[sel] + d
        var = 1.0 - d * (d + mu[sel])
        err = (s[sel] * z[sel] - want).sum()
        assert abs(err) <= 4.0 * math.sqrt(var.sum()), (lo, hi, err, math.sqrt(var.sum()))
        checked += 1
    assert checked >= 16
    # the two sides' streams differ, and so do two iterations
    z2 = ref.truncated_draw(np.arange(1000), 3, ref.TAG_USERS, m[:1000], s[:1000])[0]
    z3 = ref.truncated_draw(np.arange(1000), 4, ref.TAG_MOVIES, m[:1000], s[:1000])[0]
    assert np.mean(z2 == z[:1000]) < 0.01 and np.mean(z3 == z[:1000]) < 0.01


def test_no_decision_of_the_gpu_parity_inputs_is_marginal():
    """What tests/test_gpu_probit.py::test_latent_against_restatement relies on: for its inputs, every accept / reject comparison
    and every choice of proposal is at least 1e-9 from its threshold, while the device's m differs from numpy's by ~1e-15."""
    M, Mt, nu, nm = ref.skewed()
    assert np.diff(M[0]).max() >= 50000 and (np.diff(M[0]) == 0).sum() == 19 and np.diff(Mt[0]).max() <= 3
    worst = math.inf
    for K, dtype in ref.LATENT_CASES:
        U, V = ref.latent_factors(K, dtype, nu, nm)
        for A, X, Y, tag in ((M, V, U, ref.TAG_MOVIES), (Mt, U, V, ref.TAG_USERS)):
            z, m, att, margin, bmargin = ref.latent(A, X, Y, ref.LATENT_ITER, tag, ref.LATENT_THRESHOLD, full=True)
            assert np.abs(m).max() > 5.0                                 # the dot products do span the tails
            assert margin >= MARGIN and bmargin >= MARGIN, (K, dtype, tag, margin, bmargin)
            worst = min(worst, margin, bmargin)
    print("closest decision over the GPU parity inputs: %.3g" % worst)


def test_gibbs_refuses_bad_probit_arguments():
    with pytest.raises(ValueError, match="noise='adaptive'"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, probit=True, noise="adaptive")
    with pytest.raises(ValueError, match="alpha = 1"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, probit=True, alpha=2.0)
    with pytest.raises(ValueError, match="threshold"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, probit=True, threshold=float("nan"))


def test_cli_probit_refusals(tmp_path):
    cases = [
        (["--probit", "-g", "2"], None, "--probit runs on one GPU without -g"),
        (["--probit", "-g", "1"], None, "--probit runs on one GPU without -g"),
        (["--probit", "--noise", "adaptive"], None, "--probit does not go together with --noise adaptive"),
        (["--probit"], {"BPMF_REDUCE": "1"}, "--probit does not go together with BPMF_REDUCE=1"),
        (["--probit", "-a", "2"], None, "--probit runs with alpha = 1"),
        (["--probit", "-a", "0.5"], None, "--probit runs with alpha = 1"),
        (["--probit-threshold", "0.5"], None, "--probit-threshold needs --probit"),
        (["--probit", "--probit-threshold", "x"], None, "--probit-threshold expects a number"),
        (["--probit", "--probit-threshold", "1x"], None, "--probit-threshold expects a number"),
        (["--probit", "--probit-threshold", "nan"], None, "--probit-threshold expects a number"),
        (["--probit", "--probit-threshold", ""], None, "--probit-threshold expects a number"),
    ]
    for extra, env, msg in cases:
        r = run(data_args() + extra + ["-o", str(tmp_path)], tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert "num_latent" not in r.stdout                              # stopped before Sys::init printed anything
        assert not (tmp_path / "probit.csv").exists()


def test_cli_usage_names_probit(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "--probit" in text and "--probit-threshold F" in text
    assert "--noise fixed|adaptive" in text
