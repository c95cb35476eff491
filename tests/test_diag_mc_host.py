"""Multi-chain rank-normalised convergence diagnostics without a GPU: the estimator as tests/diag_mc_ref.py
restates it against what is known of it, pool_models, diag_summary and every refusal of gibbs(chain=) before a GPU is touched.

  1. AR(1) chains (fixed seed, C = 4, S = 250, 200 traces per rho in {0, 0.5, 0.9}): the median of ess_bulk / N within 15 % of
     (1 - rho) / (1 + rho) (the slack tests/test_diag_host.py gives its own figures; measured 0.99 / 0.35 / 0.056 against 1 / 0.333 /
     0.053), the 99th percentile of rhat below 1.02 / 1.05 / 1.3 (measured 1.009 / 1.030 / 1.18)
  2. what the estimator of section 29 misses, C = 4, S = 100, rho = 0.3, 200 traces each: one chain of four shifted by one standard
     deviation (measured median rhat 1.11, minimum 1.048); one chain scaled by 3 (measured median 1.147, minimum 1.058, where the
     estimator of section 29 on the same values has median 1.004); a Cauchy trace gives finite sane values
  3. C = 1: est of the raw trace is tests/diag_ref.py's estimator; ties get average ranks and the scores are antisymmetric; an odd S
     drops the middle draw; constant and per-chain-constant traces are NaN, a value that is not finite is NaN; the tail indicator is
     x <= np.quantile(x, p); the fp64 restatement agrees with longdouble
  4. pool_models and its refusals; diag_summary on both kinds of dict; every ValueError of gibbs(chain=); the entry points exist and the
     ABI version is still 1

These fail on the commit before the feature (no tests/diag_mc_ref.py, no pool_models, no chain= argument, no entry points).
"""
import os
import subprocess

import numpy as np
import pytest
import bpmf_amd
from tests import diag_ref as dr
from tests import diag_mc_ref as mc
from tests import model_ref as mr
from tests.conftest import ROOT


# ---- 1. AR(1) ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rho,q99_max", [(0.0, 1.02), (0.5, 1.05), (0.9, 1.3)])
def test_ar1_bulk_ess_and_rhat(rho, q99_max):
    C, S, N = 4, 250, 1000
    X = mc.chains_ar1(np.random.default_rng(20211 + int(10 * rho)), 200, C, S, rho)
    rhat, bulk, tail = mc.diag_mc_many(X, C, S)
    assert np.isfinite(rhat).all() and np.isfinite(bulk).all() and np.isfinite(tail).all()
    want = (1.0 - rho) / (1.0 + rho)
    got = float(np.median(bulk / N))
    q99 = float(np.quantile(rhat, 0.99))
    print("rho %.1f: median ess_bulk / N %.4f against %.4f, q99 rhat %.4f, median ess_tail / N %.4f" % (rho, got, want, q99, np.median(tail / N)))
    assert abs(got - want) <= 0.15 * want, (rho, got, want)
    assert q99 < q99_max and (rhat > 0.99).all()
    assert (bulk <= N * np.log10(N) * (1 + 1e-15)).all() and (tail > 0).all()


# ---- 2. what one chain's split-Rhat misses -----------------------------------------------------------------------------------------------

def test_a_shifted_chain_is_flagged():
    X = mc.chains_ar1(np.random.default_rng(31), 200, 4, 100, 0.3)
    X[:, 300:] += 1.0
    rhat = mc.diag_mc_many(X, 4, 100)[0]
    print("shifted: median rhat %.4f min %.4f" % (np.median(rhat), rhat.min()))
    assert np.median(rhat) > 1.07 and rhat.min() > 1.02


def test_a_scaled_chain_is_flagged_by_the_folded_rhat_alone():
    X = mc.chains_ar1(np.random.default_rng(32), 200, 4, 100, 0.3)
    X[:, 300:] *= 3.0
    rhat = mc.diag_mc_many(X, 4, 100)[0]
    parts = [mc.parts(x, 4, 100) for x in X[:50]]
    plain = dr.diag_many(X)[0]
    print("scaled: median rank-rhat %.4f min %.4f; section 29 median %.4f" % (np.median(rhat), rhat.min(), np.median(plain)))
    assert np.median(rhat) > 1.09 and rhat.min() > 1.03 and np.median(plain) < 1.02
    assert all(p["folded"][0] > p["bulk"][0] for p in parts)                      # it is the folded pass that sees it


def test_cauchy_traces_give_sane_values():
    X = np.random.default_rng(33).standard_cauchy((100, 400))
    rhat, bulk, tail = mc.diag_mc_many(X, 4, 100)
    assert np.isfinite(rhat).all() and np.isfinite(bulk).all() and np.isfinite(tail).all()
    assert np.quantile(rhat, 0.99) < 1.05 and 0.7 < np.median(bulk / 400) < 1.3 and (tail > 20).all()


# ---- 3. the parts ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [8, 9, 64, 257])
def test_one_chain_is_the_estimator_of_section_29(S):
    X = np.concatenate([dr.ar1(np.random.default_rng(S), 6, S, rho) for rho in (0.0, 0.9, -0.5)])
    for x in X:
        a, b = mc.est(mc.half_chains(x, 1, S)), dr.diag(x)
        assert abs(a[0] - b[0]) <= 1e-14 * b[0] and abs(a[1] - b[1]) <= 1e-12 * b[1], (S, a, b)


def test_ties_get_average_ranks_and_scores_are_antisymmetric():
    assert mc.ranks2(np.array([1.0, 2.0, 2.0, 3.0])).tolist() == [2, 5, 5, 8]
    assert mc.ranks2(np.array([[5.0, 5.0], [5.0, 5.0]])).tolist() == [[5, 5], [5, 5]]
    x = np.round(np.random.default_rng(2).standard_normal(40), 1)
    for f64 in (False, True):
        z, zm = mc.zscores(x, f64), mc.zscores(-x, f64)
        assert np.array_equal(z, -zm)
        assert np.array_equal(mc.zscores(np.full(8, 3.0), f64), np.zeros(8))        # every rank (N + 1) / 2
    z = mc.zscores(np.arange(1000.0))
    from scipy.special import ndtri
    assert np.abs(z.astype(np.float64) - ndtri((np.arange(1, 1001) - 0.375) / 1000.25)).max() < 1e-13


def test_an_odd_length_drops_the_middle_draw_of_every_chain():
    x = np.random.default_rng(3).standard_normal(27); y = x.copy(); y[[4, 13, 22]] = 1e6
    assert mc.diag_mc(x, 3, 9) == mc.diag_mc(y, 3, 9) and mc.diag_mc_f64(x, 3, 9) == mc.diag_mc_f64(y, 3, 9)
    assert mc.diag_mc(x, 3, 9) == mc.diag_mc(np.delete(x, [4, 13, 22]), 3, 8)


def test_nan_rules():
    rng = np.random.default_rng(4)
    for f64 in (False, True):
        for C, S in ((1, 8), (3, 9), (4, 50)):
            assert all(np.isnan(v) for v in mc.diag_mc(np.full(C * S, 0.1), C, S, f64))
            per_chain = np.repeat(np.arange(C, dtype=np.float64), S)
            assert all(np.isnan(v) for v in mc.diag_mc(per_chain, C, S, f64))
            for bad in (np.nan, np.inf, -np.inf):
                x = rng.standard_normal(C * S); x[S // 2] = bad                     # (the draw an odd S drops: it counts)
                assert all(np.isnan(v) for v in mc.diag_mc(x, C, S, f64))
        # a tail indicator that is constant in every half-chain: ess_tail alone is NaN
        x = rng.standard_normal(80); x[:4] -= 100.0                                 # N = 80, n = 4: the 4 values <= x_(4) fill half-chain 0
        r = mc.diag_mc(x, 10, 8, f64)
        assert np.isfinite(r[0]) and np.isfinite(r[1]) and np.isnan(r[2])


def test_the_tail_indicator_is_the_type_7_quantile():
    rng = np.random.default_rng(5)
    for N in (8, 21, 64, 100, 101, 1000, 4096):
        for x in (rng.standard_normal(N), np.round(rng.standard_normal(N), 1), rng.standard_cauchy(N)):
            lo, hi = mc.tail_cuts(x)
            assert np.array_equal(x <= lo, x <= np.quantile(x, 0.05)) and np.array_equal(x <= hi, x <= np.quantile(x, 0.95)), N


def test_fp64_restatement_agrees_with_longdouble():
    rng = np.random.default_rng(6)
    for C, S in ((1, 64), (4, 17), (8, 32)):
        X = np.concatenate([mc.chains_ar1(rng, 5, C, S, rho) for rho in (0.0, 0.9)] + [np.round(rng.standard_normal((5, C * S)), 1)])
        a, b = mc.diag_mc_many(X, C, S), mc.diag_mc_many(X, C, S, True)
        assert all(dr.relative_error(b[k], a[k]) < 1e-12 for k in range(3))


# ---- 4. pooling, the summary, refusals -----------------------------------------------------------------------------------------------------

def chains_of(n, **kw):
    return [mr.random_model(4, 6, 5, 8, seed=10 + c, **kw) for c in range(n)]


def test_pool_models():
    ms = chains_of(3)
    p = bpmf_amd.pool_models(ms)
    assert p["chains"] == 3 and p["samples"] == 24 and p["U"].shape == (6, 24, 4) and p["V"].shape == (5, 24, 4)
    for c, m in enumerate(ms):
        assert p["U"][:, 8 * c:8 * c + 8].tobytes() == m["U"].tobytes() and p["V"][:, 8 * c:8 * c + 8].tobytes() == m["V"].tobytes()
        for key in ("U_hyper", "V_hyper"):
            assert all(p[key][j][8 * c:8 * c + 8].tobytes() == m[key][j].tobytes() for j in range(3))
    assert all(p[k] == ms[0][k] for k in ("num_latent", "rows", "cols", "mean_rating", "alpha", "probit", "dtype"))
    assert ms[0]["samples"] == 8 and "chains" not in ms[0]                          # the chains are left as they were
    one = bpmf_amd.pool_models(ms[:1])
    assert one["chains"] == 1 and one["U"].tobytes() == ms[0]["U"].tobytes()
    nohyp = bpmf_amd.pool_models(chains_of(2, hyper=False))
    assert nohyp["U_hyper"] is None and nohyp["V_hyper"] is None and nohyp["samples"] == 16


def test_pool_models_refusals():
    a, b = chains_of(2)
    with pytest.raises(ValueError, match="no chain given"):
        bpmf_amd.pool_models([])
    for change, what in ((dict(rows=7, U=np.zeros((7, 8, 4))), "shape"), (dict(cols=4, V=np.zeros((4, 8, 4))), "shape"),
                         (dict(num_latent=5), "num_latent"), (dict(probit=True), "likelihood"), (dict(probit_threshold=0.25), "likelihood"),
                         (dict(mean_rating=3.0), "mean rating"), (dict(dtype="f32"), "dtype"), (dict(samples=7), "samples")):
        with pytest.raises(ValueError, match="pool_models: chain 1 differs from chain 0 in " + what):
            bpmf_amd.pool_models([a, dict(b, **change)])
    with pytest.raises(ValueError, match="presence of the hyper-parameters"):
        bpmf_amd.pool_models([a, dict(b, U_hyper=None, V_hyper=None)])
    with pytest.raises(ValueError, match="chain 1 has the first kept sample of chain 0, byte for byte"):
        bpmf_amd.pool_models([a, dict(a)])
    same_head = dict(b, U=b["U"].copy()); same_head["U"][:, 0] = a["U"][:, 0]
    with pytest.raises(ValueError, match="chain 2 has the first kept sample of chain 0"):
        bpmf_amd.pool_models([a, b, same_head])
    with pytest.raises(ValueError, match="needs the result of gibbs"):
        bpmf_amd.pool_models([a, 3])


def test_diag_summary_of_both_kinds():
    old = dict(std=np.array([1.0, 2.0, 3.0]), rhat=np.array([1.0, 1.02, 1.5]), ess=np.array([4.0, 16.0, 100.0]), samples=32)
    s = bpmf_amd.diag_summary(old)
    assert sorted(s) == sorted(["n", "n_nan", "samples", "ess_min", "ess_median", "rhat_median", "rhat_max", "rhat_above", "mcse_over_std_median"])
    d = dict(std=np.ones(5), rhat=np.array([1.0, 1.02, np.nan, 1.005, 1.5]), ess_bulk=np.array([4.0, 16.0, 9.0, 25.0, 100.0]),
             ess_tail=np.array([8.0, 2.0, 9.0, np.nan, 50.0]), samples=64, chains=4)
    s = bpmf_amd.diag_summary(d)
    assert s["n"] == 5 and s["n_nan"] == 2 and s["samples"] == 64 and s["chains"] == 4
    assert s["ess_bulk_min"] == 4.0 and s["ess_bulk_median"] == 16.0 and s["ess_tail_min"] == 2.0 and s["ess_tail_median"] == 8.0
    assert s["ess_min"] == 4.0 and s["ess_median"] == 16.0                          # the old keys: of the bulk ESS
    assert s["rhat_median"] == 1.02 and s["rhat_max"] == 1.5 and s["rhat_above"] == 2.0 / 3.0 and s["mcse_over_std_median"] == 0.25
    empty = bpmf_amd.diag_summary(dict(rhat=np.array([np.nan]), ess_bulk=np.array([np.nan]), ess_tail=np.array([1.0]), std=np.zeros(1)))
    assert empty["n_nan"] == 1 and all(np.isnan(empty[k]) for k in ("ess_bulk_min", "ess_tail_median", "rhat_max"))


def test_gibbs_chain_refusals(monkeypatch):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    none = object()                                                  # (refused before the engine is used)
    F = np.ones((nu, 2))
    for bad in (-1, 64, 1.5, "1", True, None):
        with pytest.raises(ValueError, match="chain must be an integer 0 .. 63"):
            bpmf_amd.gibbs(none, M, Mt, T, nu, nm, chain=bad)
    for kw, what in ((dict(row_features=F), "features"), (dict(col_features=np.ones((nm, 2))), "features"), (dict(new_row_features=F), "features"),
                     (dict(ordinal=True), "ordinal"), (dict(bias=True), "bias"), (dict(bias_prior=(1.0, 1.0)), "bias"), (dict(implicit=0.1), "implicit")):
        with pytest.raises(ValueError, match="chain=2 does not go together with " + what):
            bpmf_amd.gibbs(none, M, Mt, T, nu, nm, chain=2, **kw)
    with pytest.raises(ValueError, match=r"chain=1 needs nsims <= 1048576"):
        bpmf_amd.gibbs(none, M, Mt, T, nu, nm, chain=1, nsims=(1 << 20) + 1, burnin=5)
    monkeypatch.setenv("BPMF_REDUCE", "1")
    with pytest.raises(ValueError, match="chain=1 does not go together with BPMF_REDUCE"):
        bpmf_amd.gibbs(none, M, Mt, T, nu, nm, chain=1)
    monkeypatch.delenv("BPMF_REDUCE")

    class Ranks:
        def comm_nranks(self):
            return 2
    with pytest.raises(ValueError, match="chain=1 does not go together with a communicator"):
        bpmf_amd.gibbs(Ranks(), M, Mt, T, nu, nm, chain=1)
    with pytest.raises(ValueError, match="run_chains: chains must be 1 .. 64"):
        bpmf_amd.run_chains(none, M, Mt, T, nu, nm, chains=65)
    with pytest.raises(ValueError, match="run_chains sets chain itself"):
        bpmf_amd.run_chains(none, M, Mt, T, nu, nm, chains=2, chain=1)


def test_library_has_the_entry_points():
    from bpmf_amd import _lib
    lib = _lib.load_library()
    for name in ("bpmf_hip_diag_traces_mc", "bpmf_hip_diag_cells_mc", "bpmf_hip_side_set_chain", "bpmf_hip_side_chain"):
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None
    for name in ("diag_traces_mc", "diag_cells_mc", "side_set_chain", "side_chain"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
    assert callable(bpmf_amd.pool_models) and callable(bpmf_amd.run_chains)
    assert lib.bpmf_hip_abi_version() == 1
    assert (bpmf_amd.HipEngine.CHAIN_STRIDE, bpmf_amd.HipEngine.CHAIN_MAX, bpmf_amd.HipEngine.DIAG_MAX_CHAINS) == (1 << 20, 63, mc.MAX_CHAINS)
    with open(os.path.join(ROOT, "include", "bpmf_hip.h")) as f:
        text = f.read()
    assert "#define BPMF_HIP_CHAIN_STRIDE (1 << 20)\n" in text and "#define BPMF_HIP_CHAIN_MAX 63\n" in text
    assert "#define BPMF_HIP_DIAG_MAX_CHAINS %d\n" % mc.MAX_CHAINS in text


BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")


def refused(args, reason, cwd, env=None):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=60, env=dict(os.environ, **(env or {})))
    assert p.returncode == 1 and p.stdout == "", (args, p.stdout, p.stderr)
    lines = p.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("bpmf: ") and reason in lines[0], (args, p.stderr)


def test_cli_chain_refusals(tmp_path):
    base = ["-n", "train.sdm", "-p", "test.sdm", "-i", 20, "-b", 5]   # (nothing is read before the refusal)
    for bad in (-1, 64, "x", "1.5"):
        refused(base + ["--chain", bad], "--chain expects 0 <= c <= 63", tmp_path)
    refused(base + ["--chain", 1, "--row-features", "f.ddm"], "--chain does not go together with features", tmp_path)
    refused(base + ["--chain", 1, "--col-features", "f.ddm"], "--chain does not go together with features", tmp_path)
    refused(base + ["--chain", 1, "--ordinal"], "--chain does not go together with --ordinal", tmp_path)
    refused(base + ["--chain", 1, "--bias"], "--chain does not go together with --bias", tmp_path)
    refused(base + ["--chain", 1, "--implicit", 0.1], "--chain does not go together with --implicit", tmp_path)
    refused(["--tensor", "x.tns", "--chain", 1, "-i", 20, "-b", 5], "--chain does not go together with --tensor", tmp_path)
    refused(base + ["--chain", 1, "-g", 2], "one GPU without -g", tmp_path)
    refused(base + ["--chain", 1, "-m", "mu.ddm", "-l", "lambda.ddm"], "propagated posterior", tmp_path)
    refused(base + ["--chain", 1], "BPMF_REDUCE=1", tmp_path, env={"BPMF_REDUCE": "1"})
    refused(["-n", "train.sdm", "-p", "test.sdm", "--chain", 0, "-i", 1048577, "-b", 5], "--chain needs -i <= 1048576", tmp_path)
    refused(["--model", "model", "--chain", 1, "--predict", "cells.sdm", "-o", "out"], "--chain", tmp_path)
    refused(base[:4] + ["--diagnose-rank", "-i", 20, "-b", 13], "8 .. 4096 post-burn-in samples", tmp_path)
    refused(["--model", "model", "--diagnose-rank", "-o", "out"], "needs --predict FILE", tmp_path)
    # pooled models: read, then refused before a context is created
    for c in range(2):
        bpmf_amd.write_model(tmp_path / ("m%d" % c), mr.random_model(4, 6, 5, 7, seed=1 + c))
    bpmf_amd.write_model(tmp_path / "other", mr.random_model(4, 6, 5, 9, seed=5))
    os.mkdir(tmp_path / "out")
    refused(["--model", "m0,m1", "--diagnose", "--predict", "cells.sdm", "-o", "out"], "8 or more samples per chain", tmp_path)
    refused(["--model", "m0,m0", "--predict", "cells.sdm", "-o", "out"], "the same chain twice", tmp_path)
    refused(["--model", "m0,other", "--predict", "cells.sdm", "-o", "out"], "differs from m0 in samples", tmp_path)
    p = subprocess.run([BPMF], capture_output=True, text=True, timeout=60)
    assert "--chain c" in p.stdout + p.stderr and "--diagnose-rank" in p.stdout + p.stderr and "a comma is not supported" in p.stdout + p.stderr
