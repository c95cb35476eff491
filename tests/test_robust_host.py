"""Student-t noise, CPU part: the restated weight draw of tests/robust_ref.py has no marginal accept / reject decision on any input
the GPU parity tests (tests/test_gpu_robust.py) use, its draws have the moments of Gamma(a, rate b), a chain with nu = 1e8 is the
Gaussian chain; gibbs(robust=...) and `bpmf --robust` refuse what they cannot do before anything touches a GPU; the recorded
figures of the planted experiment."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bpmf_amd
from bpmf_amd import _lib
from tests import robust_ref as ref
from tests import util
from tests.conftest import ROOT
from tests.oracle_engine import OracleEngine

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")


def run(args, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=e)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_robust_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    _lib.load_library()
    sigs = _lib.exported_signatures()
    for name in ("bpmf_hip_side_set_robust", "bpmf_hip_side_robust_add", "bpmf_hip_side_robust_get"):
        assert hasattr(raw, name) and name in sigs
    for name in ("set_robust", "robust_add", "robust_get"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
    from bpmf_amd import sys as bsys
    assert bsys.ROBUST_TAGS == (ref.TAG_MOVIES, ref.TAG_USERS) == (9, 10)
    assert not set(bsys.ROBUST_TAGS) & ({1, 2, 3, 4, 5, 6} | set(bsys.FOLDIN_TAGS.values()))


# ---- no decision is marginal ----------------------------------------------------------------------------------------------------------
# The accept / reject decisions of the Gamma draw depend on (rating position, iteration, tag, nu) only -- never on the factors, alpha or
# K: g is drawn from Gamma(a, 1) and divided by b afterwards.  So the inputs of a GPU test are covered by the positions 0 .. nnz - 1 of
# its largest side, its iterations, its tags and its nu.

def _margin(nnz, iters, tags, nus):
    worst = math.inf
    for it in iters:
        for tag in tags:
            for nu in nus:
                worst = min(worst, ref.gamma_draw(np.arange(nnz), it, tag, 0.5 * (nu + 1.0))[2])
    return worst


def test_no_decision_is_marginal_in_the_weight_and_half_iteration_inputs():
    A, _ = ref.edge_side()
    nnz = max(len(A[2]), max(ref.SMALL_NNZ))
    assert nnz == 894
    # tests 1 - 3 and 7 of test_gpu_robust.py: iterations ITER and ITER + 1, both tags, every nu
    worst = _margin(nnz, (ref.ITER, ref.ITER + 1), (ref.TAG_MOVIES, ref.TAG_USERS), ref.NUS)
    print("closest decision: %.3g" % worst)
    assert worst >= ref.MARGIN


def test_no_decision_is_marginal_in_the_chain_inputs():
    M, Mt, T, Tt, nu, nm = util.ml100k()
    worst = _margin(len(M[2]), range(ref.CHAIN["nsims"]), (ref.TAG_MOVIES, ref.TAG_USERS), (ref.CHAIN["nu"],))
    print("ml-100k chain, closest decision: %.3g" % worst)
    assert worst >= ref.MARGIN
    P = ref.PLANTED
    worst = _margin(P["nusers"] * P["per_user"], range(P["nsims"]), (ref.TAG_MOVIES, ref.TAG_USERS), (P["nu"],))
    print("planted chain, closest decision: %.3g" % worst)
    assert worst >= ref.MARGIN
    worst = _margin(len(util.tiny()[0][2]), range(ref.CLI["nsims"]), (ref.TAG_MOVIES, ref.TAG_USERS), (ref.CLI["nu"],))
    assert worst >= ref.MARGIN


# ---- the draw ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nu", [1.0, 4.0, 30.0])
def test_moments_of_the_restated_draw(nu):
    """For a fixed residual e, w ~ Gamma(a, rate b): mean a / b and variance a / b^2 of 20 000 draws within 4 standard errors.  The
    standard error of the sample variance comes from the fourth central moment of the Gamma law, 3 a (a + 2) / b^4."""
    n, alpha, e = 20000, 2.0, 0.8
    A = (np.array([0, n], np.int64), np.arange(n, dtype=np.int32), np.full(n, 3.0 + e))
    X, Y = np.zeros((1, 4)), np.zeros((n, 4))                         # m = 0: every rating has the residual e
    sw, zw, m, attempts, margin = ref.weights(A, X, Y, 2, ref.TAG_MOVIES, alpha, nu, 3.0, full=True)
    w = sw * sw
    a, b = 0.5 * (nu + 1.0), 0.5 * (nu + alpha * e * e)
    se_mean = math.sqrt(a / (b * b) / n)
    se_var = math.sqrt((3.0 * a * (a + 2.0) - a * a) / b ** 4 / n)
    print("nu %g: mean %.5f (a / b = %.5f, se %.2g), var %.5f (a / b^2 = %.5f, se %.2g), %.4f attempts per draw"
          % (nu, w.mean(), a / b, se_mean, w.var(ddof=1), a / (b * b), se_var, attempts.mean()))
    assert abs(w.mean() - a / b) <= 4.0 * se_mean
    assert abs(w.var(ddof=1) - a / (b * b)) <= 4.0 * se_var
    assert np.allclose(zw, sw * e, rtol=1e-15, atol=0.0) and np.all(m == 0.0)
    assert attempts.mean() <= 1.0 / 0.95 and attempts.max() < ref.MAX_ATTEMPTS      # acceptance >= 0.95 for a >= 1


def test_a_large_residual_draws_a_small_weight():
    n = 4000
    A = (np.array([0, n], np.int64), np.arange(n, dtype=np.int32), np.concatenate([np.full(n // 2, 3.1), np.full(n // 2, 13.0)]))
    sw, _ = ref.weights(A, np.zeros((1, 4)), np.zeros((n, 4)), 0, ref.TAG_USERS, 16.0, 4.0, 3.0)
    w = sw * sw
    assert w[:n // 2].mean() > 1.0 and w[n // 2:].mean() < 0.01


def test_large_nu_is_the_gaussian_chain(oracle):
    M, Mt, T, Tt, nu, nm = util.tiny()
    t = ref.restate_chain(oracle, 8, M, Mt, T, 1e8, 8, 3, 2.0)
    g = ref.restate_chain(oracle, 8, M, Mt, T, None, 8, 3, 2.0)
    d = max(np.abs(np.array(t["rmse"]) - g["rmse"]).max(), np.abs(np.array(t["rmse_avg"]) - g["rmse_avg"]).max())
    print("nu = 1e8 against the Gaussian chain: RMSE traces %.3g apart, weights within %.3g of 1" % (d, np.abs(t["weight_mean"] - 1.0).max()))
    assert d < 1e-3
    assert np.abs(t["weight_mean"] - 1.0).max() < 1e-3 and t["kept"] == 5


# ---- gibbs ------------------------------------------------------------------------------------------------------------------------------

def test_gibbs_refuses_what_does_not_go_with_robust():
    Wm = (np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0))
    for bad in (0.5, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"robust.*finite and >= 1"):
            bpmf_amd.gibbs(None, None, None, None, 1, 1, robust=bad)
    with pytest.raises(ValueError, match=r"robust must be a number"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, robust="heavy")
    with pytest.raises(ValueError, match=r"robust.*weights"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, robust=4, weights=Wm)
    with pytest.raises(ValueError, match=r"robust.*probit=True"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, robust=4, probit=True)
    with pytest.raises(ValueError, match=r"robust.*censored"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, robust=4, censored=Wm)
    with pytest.raises(ValueError, match=r"robust.*noise='adaptive'"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, robust=4, noise="adaptive")
    with pytest.raises(ValueError, match=r"robust.*row_features / col_features"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, robust=4, row_features=np.zeros((1, 1)))
    with pytest.raises(ValueError, match=r"robust.*row_features / col_features"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, robust=4, col_features=np.zeros((1, 1)))
    for kind in ("prob", "ei"):
        with pytest.raises(ValueError, match=r"robust.*topn_score '%s'" % kind):
            bpmf_amd.gibbs(None, None, None, None, 1, 1, robust=4, topn=3, topn_score=(kind, 3.0))
    with pytest.raises(ValueError, match=r"robust needs a finite alpha > 0"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, robust=4, alpha=0.0)

    class Fp32:
        dtype = "f32"
    with pytest.raises(ValueError, match=r"robust.*fp64"):
        bpmf_amd.gibbs(Fp32(), None, None, None, 1, 1, robust=4)


class _RecordingEngine(OracleEngine):
    """The oracle-backed test engine with the three robust entry points recorded (the weights stay 1: what is checked is what gibbs
    asks of its engine and what it returns)."""

    def __init__(self, K):
        super().__init__(K)
        self.calls = []

    def set_robust(self, side, nu, tag):
        self.calls.append(("set", side, nu, tag))

    def robust_add(self, side):
        self.calls.append(("add", side))

    def robust_get(self, side):
        n = sum(1 for c in self.calls if c[0] == "add" and c[1] is side)
        return np.full(len(side.csc[2]), 0.5), n, 4.0


def test_gibbs_robust_result_and_what_it_asks_of_the_engine():
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = _RecordingEngine(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=5, burnin=2, robust=4, topn_score=None)
    sets = [c for c in eng.calls if c[0] == "set"]
    adds = [c for c in eng.calls if c[0] == "add"]
    movies, users = res["movies"].side, res["users"].side
    assert [(c[1], c[2], c[3]) for c in sets] == [(movies, 4.0, 9), (users, 4.0, 10)]
    assert len(adds) == 3 and all(c[1] is movies for c in adds)       # one per kept iteration, the movies' side
    r = res["robust"]
    assert set(r) == {"nu", "weight_mean", "kept"} and r["nu"] == 4.0 and r["kept"] == 3
    assert r["weight_mean"].shape == (len(M[2]),) and r["weight_mean"].dtype == np.float64
    # no kept sample: zeros, and the engine is not asked
    eng = _RecordingEngine(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=2, robust=1)
    assert res["robust"]["kept"] == 0 and res["robust"]["nu"] == 1.0 and not res["robust"]["weight_mean"].any()
    assert not [c for c in eng.calls if c[0] == "add"]
    # without robust nothing is asked and nothing returned
    eng = _RecordingEngine(8)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=1)
    assert "robust" not in res and not eng.calls


# ---- the executable ---------------------------------------------------------------------------------------------------------------------

def test_cli_robust_refusals(tmp_path):
    good = tmp_path / "w.mtx"
    good.write_text("%%MatrixMarket matrix coordinate real general\n4 2 2\n1 1 2.5\n2 1 0.25\n")
    feat = tmp_path / "f.csv"
    feat.write_text("1\n2\n3\n4\n")
    cases = [
        (["--robust", "4", "-g", "2"], None, "--robust runs on one GPU without -g"),
        (["--robust", "4", "-g", "1"], None, "--robust runs on one GPU without -g"),
        (["--robust", "4", "--weights", str(good)], None, "--robust does not go together with --weights"),
        (["--robust", "4", "--probit"], None, "--robust does not go together with --probit"),
        (["--robust", "4", "--censored", str(good)], None, "--robust does not go together with --censored"),
        (["--robust", "4", "--noise", "adaptive"], None, "--robust does not go together with --noise adaptive"),
        (["--robust", "4", "--row-features", str(feat)], None, "--robust does not go together with --row-features / --col-features"),
        (["--robust", "4", "--col-features", str(feat)], None, "--robust does not go together with --row-features / --col-features"),
        (["--robust", "4", "-m", "a,b"], None, "--robust does not go together with a propagated posterior (-m / -l)"),
        (["--robust", "4", "-l", "a,b"], None, "--robust does not go together with a propagated posterior (-m / -l)"),
        (["--robust", "4", "--fp32", "-d", "100"], None, "--robust does not go together with --fp32"),
        (["--robust", "4", "-o", "o", "--topn", "1", "--topn-score", "prob", "--topn-threshold", "3"], None,
         "--robust does not go together with --topn-score prob"),
        (["--robust", "4", "-o", "o", "--topn", "1", "--topn-score", "ei", "--topn-threshold", "3"], None,
         "--robust does not go together with --topn-score ei"),
        (["--robust", "4"], {"BPMF_REDUCE": "1"}, "--robust does not go together with BPMF_REDUCE=1"),
        (["--robust", "4", "-a", "0"], None, "--robust needs a noise precision -a F > 0"),
        (["--robust", ""], None, "--robust expects the degrees of freedom NU"),
        (["--robust", "0.5"], None, "--robust expects the degrees of freedom NU"),
        (["--robust", "nan"], None, "--robust expects the degrees of freedom NU"),
        (["--robust", "inf"], None, "--robust expects the degrees of freedom NU"),
        (["--robust", "4x"], None, "--robust expects the degrees of freedom NU"),
        (["--robust", "-3"], None, "--robust expects the degrees of freedom NU"),
    ]
    for extra, env, msg in cases:
        r = run(data_args() + extra, tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr
        assert "num_latent" not in r.stdout                              # stopped before Sys::init printed anything


def test_cli_usage_names_robust(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "[--robust NU]" in text and "Student-t noise with NU >= 1 degrees of freedom" in text


def test_planted_figures_are_the_recorded_ones(oracle):
    """The three restated CPU chains of the planted-outlier experiment (robust_ref.PLANTED) give the recorded test RMSEs -- Student-t
    noise with nu = 4, Gaussian noise at the same alpha, Gaussian noise at the best single alpha -- and the recorded AUC of a small
    posterior-mean weight against the planted cells.  The Student-t chain must beat the best single alpha."""
    got, auc = ref.planted_measure(oracle)
    print("test RMSE: Student-t %.4f, Gaussian %.4f, best single alpha %.4f; AUC of the weights %.4f" % (got + (auc,)))
    assert np.abs(np.array(got) - np.array(ref.PLANTED_MEASURED)).max() < 1e-6 and abs(auc - ref.PLANTED_AUC) < 1e-6
    a, b, c = ref.PLANTED_MEASURED
    assert a < c < b and ref.PLANTED_HALF_MARGIN == 0.5 * (c - a) > 0.4
    d = ref.planted_data(**ref.PLANTED)
    assert d["nplanted"] == 1209 and abs(d["nplanted"] / len(d["M"][2]) - 0.05) < 0.002 and len(d["planted"]) == len(d["M"][2])
