"""Ordinal probit likelihood, CPU part: the restatement (tests/ordinal_ref.py) draws truncated normals and forms interval masses
that agree with scipy's; for the inputs of the GPU parity tests (tests/test_gpu_ordinal.py) no decision of the cutpoint step is
marginal; a planted experiment through the oracle chain beats the marginal-frequency predictor and the Gaussian chain; gibbs and the
`bpmf` flags refuse what they cannot do before anything touches a GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bpmf_amd
from bpmf_amd import _lib
from tests import ordinal_ref as ref
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
ACCEPT_MARGIN = 1e-6    # no accept decision of the GPU parity inputs may be closer to its threshold (the device's sums differ by ~1e-12 relative)
BOUND_MARGIN = 1e-9     # no proposal attempt closer to a bound (host arithmetic on both sides: ~1e-16)


def run(args, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=e)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_ordinal_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    lib = _lib.load_library()
    sigs = _lib.exported_signatures()
    for name in ("bpmf_hip_side_set_ordinal", "bpmf_hip_side_ordinal_info", "bpmf_hip_side_ordinal_latent", "bpmf_hip_side_ordinal_cut_get",
                 "bpmf_hip_side_ordinal_cut_set", "bpmf_hip_ordinal_loglik", "bpmf_hip_ordinal_cut_step", "bpmf_hip_test_ordinal_add",
                 "bpmf_hip_test_ordinal_get"):
        assert hasattr(raw, name) and name in sigs
    assert lib.bpmf_hip_abi_version() == 1
    for name in ("set_ordinal", "ordinal_latent", "ordinal_loglik", "ordinal_cut_step", "ordinal_cut_get", "ordinal_cut_set", "ordinal_add",
                 "ordinal_get"):
        assert callable(getattr(bpmf_amd.HipEngine, name))


def truncated_cdf(t, a, b):
    """the CDF of N(0, 1) | a < t <= b at t, from log_ndtr on the side where both tails are small"""
    from scipy.special import log_ndtr
    if a + b < 0:
        return 1.0 - truncated_cdf(-t, -b, -a)
    la, lb, lt = log_ndtr(-a), (log_ndtr(-b) if math.isfinite(b) else -math.inf), log_ndtr(-np.asarray(t))
    # (Phic(a) - Phic(t)) / (Phic(a) - Phic(b))
    return -np.expm1(lt - la) / -np.expm1(lb - la)


INTERVALS = [("central", -0.7, 1.1), ("central, left-heavy", -2.5, 0.4), ("one tail", 1.3, math.inf), ("one tail, left", -math.inf, -0.2),
             ("wide", -6.5, 7.0), ("narrow", 0.8, 0.801), ("narrow, far", 9.0, 9.001), ("far tail", 40.0, math.inf), ("far tail, closed", 40.0, 40.05),
             ("far tail, left", -math.inf, -45.0), ("at the switch", 36.9, math.inf)]


@pytest.mark.parametrize("name,a,b", INTERVALS, ids=[i[0] for i in INTERVALS])
def test_draws_lie_inside_and_follow_the_truncated_normal(name, a, b):
    n = 10 ** 5
    t, u, form = ref.truncated(np.arange(n), 2, ref.TAG_MOVIES, np.full(n, a), np.full(n, b), full=True)
    assert np.all(np.isfinite(t)) and np.all(t >= a) and np.all(t <= b)
    if name.startswith("far tail"):
        assert np.all(form == 2)
    if name == "wide":
        assert np.any(form == 1) and np.any(form == 0)                  # both erfcinv forms are taken
    ts = np.sort(t)
    F = truncated_cdf(ts, a, b)
    ks = max(np.max(np.abs(F - np.arange(1, n + 1) / n)), np.max(np.abs(F - np.arange(n) / n)))
    # Kolmogorov's bound at a one-sided level of 1e-6 for n draws, sqrt(ln(2e6) / 2 n), plus what the exponential form leaves out
    # of the density beyond 37, 1 / (2 a^2)
    lim = math.sqrt(math.log(2e6) / (2 * n)) + (1.0 / (2 * min(abs(a), abs(b)) ** 2) if np.any(form == 2) else 0.0)
    print("%s: KS distance %.3g (limit %.3g), forms %s" % (name, ks, lim, np.bincount(form, minlength=3).tolist()))
    assert ks <= lim
    # the draw is monotone in u: an inversion
    o = np.argsort(u)
    d = np.diff(t[o])
    assert np.all(d >= 0) or np.all(d <= 0)


def test_streams_differ():
    n = 1000
    a, b = np.full(n, -0.5), np.full(n, 1.5)
    t = ref.truncated(np.arange(n), 3, ref.TAG_MOVIES, a, b)
    assert np.mean(ref.truncated(np.arange(n), 3, ref.TAG_USERS, a, b) == t) < 0.01
    assert np.mean(ref.truncated(np.arange(n), 4, ref.TAG_MOVIES, a, b) == t) < 0.01
    assert np.mean(ref.truncated(np.arange(n) + 2 ** 32, 3, ref.TAG_MOVIES, a, b) == t) < 0.01


def test_log_mass_against_log_ndtr():
    """log[Phi(a + w) - Phi(a)] on a grid of (a, w).  Bound: erfc and log_ndtr are good to a few ulp each; their difference loses a
    factor E_a / (E_a - E_b) <= ~2 / (1 - exp(-(|a| + w / 2) w)) + 1 <= 4e3 at the narrowest width 1e-3, so 1e-11 absolute leaves
    a factor ten; beyond 37 the series of the tail drops a term < 2e-13."""
    from scipy.special import log_ndtr
    worst = 0.0
    for a in (-50.0, -38.0, -12.0, -3.0, -1.0, -1e-3, 0.0, 0.4, 2.0, 8.0, 20.0, 36.0, 36.99, 37.01, 38.0, 45.0, 80.0):
        for w in (1e-3, 1e-2, 0.3, 1.0, 5.0, 30.0, math.inf):
            b = a + w
            lo, hi = (a, b) if a + b >= 0 else (-b, -a)
            la, lb = log_ndtr(-lo), (log_ndtr(-hi) if math.isfinite(hi) else -math.inf)
            want = la + math.log(-math.expm1(lb - la))
            got = float(ref.logmass(a, b))
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-11 * max(1.0, abs(want)), (a, w, got, want)
            assert abs(float(ref.mass(a, b)) - math.exp(want)) <= 1e-11 * math.exp(want) + 1e-300
        got = float(ref.logmass(-math.inf, a))
        assert abs(got - log_ndtr(a)) <= 1e-11 * max(1.0, abs(log_ndtr(a))), (a, got)
    print("largest |log mass - reference|: %.3g" % worst)


def test_level_probabilities_sum_to_one():
    rng = np.random.default_rng(3)
    m = np.concatenate((rng.standard_normal(2000) * 3.0, [0.0, 50.0, -50.0, 1e3]))
    for C_, (levels, cut) in ref.LEVEL_SETS.items():
        pr = ref.probs_from(m, cut)
        assert pr.shape == (len(m), C_) and np.all(pr >= 0)
        assert np.max(np.abs(pr.sum(axis=1) - 1.0)) <= 1e-14


def test_default_cutpoints_reproduce_the_frequencies():
    M, _, _, _ = ref.kernel_matrix(4097, 5)
    levels = np.asarray(ref.LEVEL_SETS[5][0])
    cut = ref.default_cutpoints(M[2], levels)
    pr = ref.probs_from(np.zeros(1), cut)[0]
    freq = np.bincount(ref.level_index(M[2], levels), minlength=5) / len(M[2])
    assert np.max(np.abs(pr - freq)) <= 1e-14
    # a level without a rating: every level counts half a rating more, the cutpoints stay apart
    M, _, _, _ = ref.kernel_matrix(257, 5, absent=2)
    cut = ref.default_cutpoints(M[2], levels)
    assert np.all(np.diff(cut) > 0) and np.all(np.isfinite(cut))


def test_proposals_respect_their_bounds_and_the_cap():
    cut = np.array([-1.5, -1.0, 0.5, 2.5])
    for it in range(1, 40):
        prop, attempts, _ = ref.propose(cut, 0.8, it)
        g, gp = ref.table(cut), ref.table(prop)
        for k in range(1, 5):
            assert gp[k - 1] < gp[k] < g[k + 1]
        assert max(attempts) <= ref.MAX_ATTEMPTS
    # the correction vanishes for a proposal that changes nothing
    acc, _ = ref.accept(cut, cut, 0.3, 5, -10.0, -10.0)
    assert acc                                                           # ln u < 0 = the ratio


def test_no_decision_of_the_gpu_parity_inputs_is_marginal(oracle):
    """What the chain tests of tests/test_gpu_ordinal.py rely on: over their inputs no accept decision of the cutpoint step lies
    within 1e-6 of its threshold and no proposal attempt within 1e-9 of a bound, so a device mismatch is never a flipped branch."""
    M, Mt, T, Tt, nu, nm = ref.planted(**ref.CHAIN)
    c = ref.CHAIN
    out = ref.restate_chain(oracle, c["K"], M, Mt, T, c["nsims"], c["burnin"], [1.0, 2.0, 3.0, 4.0, 5.0])
    print("accepted %s; closest accept decision %.3g, closest bound %.3g" % (out["accepted"], out["accept_margin"], out["bound_margin"]))
    assert out["accept_margin"] >= ACCEPT_MARGIN and out["bound_margin"] >= BOUND_MARGIN
    assert any(out["accepted"]) and not all(out["accepted"][1:])         # both outcomes occur
    g = ref.GIVEN_STEP
    out = ref.restate_chain(oracle, c["K"], M, Mt, T, g["nsims"], g["burnin"], [1.0, 2.0, 3.0, 4.0, 5.0], step=g["step"])
    print("given step: accepted %s; closest accept decision %.3g, closest bound %.3g" % (out["accepted"], out["accept_margin"], out["bound_margin"]))
    assert out["accept_margin"] >= ACCEPT_MARGIN and out["bound_margin"] >= BOUND_MARGIN
    # the stand-alone cutpoint step of the kernel inputs
    for C_ in (2, 5, 16):
        levels, cut = ref.LEVEL_SETS[C_]
        A, At, nu, nm = ref.kernel_matrix(4097, C_)
        U, V = ref.kernel_factors(8, "f64", nu, nm)
        m, lev = ref.dots(A, V, U), ref.level_index(A[2], levels)
        for it in (1, 2, 3):
            _, _, am, bm, _ = ref.cut_step(cut, 0.02, it, m, lev)
            assert am >= ACCEPT_MARGIN and bm >= BOUND_MARGIN, (C_, it, am, bm)


def test_far_tail_inputs_of_the_gpu_test_reach_every_form():
    """The scaled factors of tests/test_gpu_ordinal.py::test_far_tail_and_non_finite_scores put ratings beyond 37 on both sides."""
    levels, cut = (np.asarray(v, np.float64) for v in ref.LEVEL_SETS[5])
    A, At, nu, nm = ref.kernel_matrix(257, 5)
    U, V = ref.kernel_factors(8, "f64", nu, nm)
    m, lev = ref.dots(A, ref.FAR_SCALE * V, ref.FAR_SCALE * U), ref.level_index(A[2], levels)
    g = ref.table(cut)
    _, _, form = ref.truncated(np.arange(len(m)), 3, ref.TAG_MOVIES, g[lev] - m, g[lev + 1] - m, full=True)
    assert np.bincount(form, minlength=3)[2] >= 20 and (form != 2).sum() >= 20
    assert (m > 45).sum() >= 5 and (m < -45).sum() >= 5
    z = ref.latent_from(m, lev, 3, ref.TAG_MOVIES, cut)
    assert np.all(np.isfinite(z)) and np.all(z >= g[lev]) and np.all(z <= g[lev + 1])
    assert math.isfinite(ref.loglik_from(m, lev, cut)) and ref.loglik_from(m, lev, cut) < -1e4
    pr = ref.probs_from(m, cut)
    assert np.max(np.abs(pr.sum(axis=1) - 1.0)) <= 1e-14


PLANTED = dict(nusers=300, nmovies=150, nobs=13500, ntest=1500, rank=3, seed=4, K=8, nsims=150, burnin=50)


def test_planted_experiment_through_the_oracle_chain(oracle):
    """Assert orderings only: the ordinal chain's mean log-probability of the true level lies above the marginal-frequency
    predictor's, and its most probable level is right more often than the Gaussian chain's rounded prediction."""
    M, Mt, T, Tt, nu, nm = ref.planted(**PLANTED)
    c = PLANTED
    levels = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    out = ref.restate_chain(oracle, c["K"], M, Mt, T, c["nsims"], c["burnin"], levels)
    true = ref.level_index(T[2], levels)
    freq = np.bincount(ref.level_index(M[2], levels), minlength=5) / len(M[2])
    logp_marginal = float(np.mean(np.log(freq[true])))
    acc_ordinal = float(np.mean(np.argmax(out["cat_prob"], axis=1) == true))
    rate = np.mean(out["accepted"][1:])
    print("log-prob %.4f against %.4f (marginal); accuracy %.4f; acceptance %.2f; final step x sqrt(nnz) %.2f; cutpoints %s" % (
        out["logp"], logp_marginal, acc_ordinal, rate, out["step"][-1] * math.sqrt(len(M[2])), out["cutpoints"][-1]))
    assert out["logp"] > logp_marginal + 0.1
    pred = np.clip(np.rint(gaussian_chain(oracle, c["K"], M, Mt, T, c["nsims"], c["burnin"])), 1, 5)
    acc_gauss = float(np.mean(pred == T[2]))
    rmse_ord = math.sqrt(np.mean((out["expected"] - T[2]) ** 2))
    print("accuracy %.4f against %.4f (Gaussian, rounded); ordinal RMSE %.4f" % (acc_ordinal, acc_gauss, rmse_ord))
    assert acc_ordinal > acc_gauss + 0.02
    assert 0.1 <= rate <= 0.8


def gaussian_chain(oracle, K, M, Mt, T, nsims, burnin, alpha=2.0):
    """The plain chain from the oracle's pieces; returns the posterior-mean prediction of every test entry."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    mean = float(np.mean(M[2]))
    U, V = np.zeros((nu, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    psum, n = np.zeros(len(T[2])), 0
    for it in range(nsims):
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        s, prod, _ = oracle.sample_side(K, M, mean, alpha, U, V, it, mu, LF, nthreads=ref.NT)
        cov_m = oracle.cov(K, nm, s, prod)
        mu, LU, LF = oracle.hyper_sample(K, nu, cov_u, it)
        s, prod, _ = oracle.sample_side(K, Mt, mean, alpha, V, U, it, mu, LF, nthreads=ref.NT)
        cov_u = oracle.cov(K, nu, s, prod)
        if it >= burnin:
            psum += mean + ref.dots(T, V, U)
            n += 1
    return psum / n


def test_gibbs_refuses_bad_ordinal_arguments():
    M = (np.array([0, 2]), np.array([0, 1], np.int32), np.array([1.0, 2.0]))
    g = lambda **kw: bpmf_amd.gibbs(None, M, M, None, 2, 1, **kw)
    for kw, msg in ((dict(probit=True), "probit=True"), (dict(foldin=True), "foldin=True"), (dict(noise="adaptive"), "noise='adaptive'"),
                    (dict(censored=M), "censored"), (dict(weights=M), "weights"), (dict(robust=4.0), "robust"),
                    (dict(row_features=np.zeros((2, 1))), "row_features")):
        with pytest.raises(ValueError, match="ordinal does not go together with " + msg):
            g(ordinal=True, **kw)
    with pytest.raises(ValueError, match="alpha = 1"):
        g(ordinal=True, alpha=2.0)
    with pytest.raises(ValueError, match="2 .. 16"):
        g(ordinal=[1.0])
    with pytest.raises(ValueError, match="2 .. 16"):
        g(ordinal=list(range(17)))
    with pytest.raises(ValueError, match="strictly increasing"):
        g(ordinal=[1.0, 2.0, 2.0])
    with pytest.raises(ValueError, match="training value is not one of the levels"):
        g(ordinal=[1.0, 3.0])
    with pytest.raises(ValueError, match="test value is not one of the levels"):
        bpmf_amd.gibbs(None, M, M, (M[0], M[1], np.array([1.0, 2.5])), 2, 1, ordinal=True)
    with pytest.raises(ValueError, match="need 1 cutpoints"):
        g(ordinal=True, cutpoints=[0.0, 1.0])
    with pytest.raises(ValueError, match="cutpoints must be finite and strictly increasing"):
        g(ordinal=[1.0, 2.0, 3.0], cutpoints=[1.0, 0.0])
    with pytest.raises(ValueError, match="ordinal_step must be positive"):
        g(ordinal=True, ordinal_step=0.0)
    with pytest.raises(ValueError, match="need ordinal"):
        g(cutpoints=[0.0])
    with pytest.raises(ValueError, match="need ordinal"):
        g(ordinal_step=0.1)


def test_cli_ordinal_refusals(tmp_path):
    cases = [
        (["--ordinal", "-g", "2"], None, "--ordinal runs on one GPU without -g"),
        (["--ordinal", "-g", "1"], None, "--ordinal runs on one GPU without -g"),
        (["--ordinal", "--noise", "adaptive"], None, "--ordinal does not go together with --noise adaptive"),
        (["--ordinal"], {"BPMF_REDUCE": "1"}, "--ordinal does not go together with BPMF_REDUCE=1"),
        (["--ordinal", "-a", "2"], None, "--ordinal runs with alpha = 1"),
        (["--ordinal", "--probit"], None, "--ordinal does not go together with --probit"),
        (["--ordinal", "--weights", "w.mtx"], None, "--ordinal does not go together with --weights"),
        (["--ordinal", "--robust", "4"], None, "--ordinal does not go together with --robust"),
        (["--ordinal", "--censored", "c.mtx"], None, "--ordinal does not go together with --censored"),
        (["--ordinal", "--fold-in-rows", "f.mtx"], None, "--ordinal does not go together with --fold-in-rows / --fold-in-cols"),
        (["--ordinal", "--fold-in-cols", "f.mtx"], None, "--ordinal does not go together with --fold-in-rows / --fold-in-cols"),
        (["--ordinal", "--row-features", "f.ddm"], None, "--ordinal does not go together with --row-features / --col-features"),
        (["--ordinal", "-m", "a,b"], None, "--ordinal does not go together with a propagated posterior"),
        (["--ordinal-levels", "1,2"], None, "--ordinal-levels needs --ordinal"),
        (["--ordinal-cutpoints", "0"], None, "--ordinal-cutpoints needs --ordinal"),
        (["--ordinal-step", "0.1"], None, "--ordinal-step needs --ordinal"),
        (["--ordinal", "--ordinal-levels", "1,x"], None, "--ordinal-levels expects finite numbers"),
        (["--ordinal", "--ordinal-levels", "1,2,2"], None, "--ordinal-levels expects strictly increasing"),
        (["--ordinal", "--ordinal-levels", "1"], None, "--ordinal-levels expects 2 .. 16 levels"),
        (["--ordinal", "--ordinal-levels", ",".join(str(i) for i in range(17))], None, "--ordinal-levels expects 2 .. 16 levels"),
        (["--ordinal", "--ordinal-levels", "1,2,3,4,5"], None, "is not one of the levels"),          # the tiny matrix holds a 7
        (["--ordinal", "--ordinal-levels", "1,2,3", "--ordinal-cutpoints", "0"], None, "--ordinal-cutpoints expects 2 cutpoints"),
        (["--ordinal", "--ordinal-cutpoints", "0,1"], None, "--ordinal-cutpoints expects 5 cutpoints for 6 levels"),
        (["--ordinal", "--ordinal-cutpoints", "1,0"], None, "--ordinal-cutpoints expects strictly increasing"),
        (["--ordinal", "--ordinal-cutpoints", "nan"], None, "--ordinal-cutpoints expects finite numbers"),
        (["--ordinal", "--ordinal-step", "0"], None, "--ordinal-step expects a number F > 0"),
        (["--ordinal", "--ordinal-step", "0.1", "--ordinal-cutpoints", "0,1,2,3,4"], None, "--ordinal-step does not go together with --ordinal-cutpoints"),
        (["--tensor", "t.tns", "--ordinal"], None, "--tensor does not go together with --ordinal"),
    ]
    for extra, env, msg in cases:
        args = (extra if "--tensor" in extra else data_args() + extra) + ["-o", str(tmp_path)]
        r = run(args, tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert "num_latent" not in r.stdout                              # stopped before Sys::init printed anything
        assert not (tmp_path / "ordinal.csv").exists() and not (tmp_path / "cutpoints.csv").exists()


def test_cli_usage_names_ordinal(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "--ordinal" in text and "--ordinal-levels a,b,.." in text and "--ordinal-cutpoints g1,.." in text and "--ordinal-step F" in text
    assert "--probit [--probit-threshold F]" in text
