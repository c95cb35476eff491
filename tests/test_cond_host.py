"""The host side of tests/test_gpu_conditioning.py: that its reference and its inputs are what it takes them for.  No GPU.

  1. np.longdouble is the 80-bit format (eps 1.08e-19): asserted, never skipped -- on a platform without it the accuracy tests
     would compare the device with fp64 and say nothing.
  2. tests/cond_ref.sample_columns at np.float64 IS the oracle's column update: on a benign input at K = 8, 50, 128 it agrees with
     oracle.sample_side to 1e-12 of max|x| (observed: at most 8.7e-16 -- the restatement takes every element's operations in
     chol_lower's order; only the back substitution subtracts in another order).  That pins the counter convention, the stream at
     a padded num_latent and the order of the solves.
  3. The conditions on the inputs, for the edge side at every num_latent a form runs (8, 16, 32, 20, 64, 50, 128, 100, 65, 127) and
     matrix B at 64 and 50: kappa_2(Lambda*) <= 1e12 in every column of every fp64 case, the oracle factorises every column of
     every fp64 case, the float32 restatement every column of every fp32 case, the longdouble restatement both.
  4. E_ref -- the worst column's error of the project's reference against the longdouble restatement -- is finite, at least eps of
     its dtype, and grows with kappa along the P family: the inputs are hard for an honest Cholesky too.

Observed (edge side, K = 128): fp64 E_ref 7.7e-14 / 3.1e-11 / 1.8e-8 at P(1e3) / P(1e6) / P(1e9), 1.7e-10 and 1.4e-9 on the two D
cases, 5.9e-14 / 2.4e-13 at S(-20) / S(+20); fp32 3.5e-6 .. 4.8e-4 over P(1e1) .. P(1e4), 1.0e-4 and 1.2e-3 on the D cases.  The
largest kappa_2(Lambda*) of an fp64 case is 6.1e9 (P(1e9)), of an fp32 case 1.5e5 (D(1, 0.1, 8)).
"""
import numpy as np
import pytest

from tests import cond_ref, util
from tests.test_gpu_schedule_edges import EDGE_NROWS, PF_NROWS, _edge, _pf_matrix

EDGE_K = [8, 16, 32, 20, 64, 50, 128, 100, 65, 127]
SIDES = [pytest.param("edge", K, id="edge-%d" % K) for K in EDGE_K] + [pytest.param("pf", K, id="pf-%d" % K) for K in (64, 50)]


def _side(name):
    counts, M = _edge() if name == "edge" else _pf_matrix()
    return counts, M, util.mean_rating(M), EDGE_NROWS if name == "edge" else PF_NROWS


def test_longdouble_is_the_80_bit_format():
    assert np.finfo(np.longdouble).eps <= 1.1e-19


@pytest.mark.parametrize("K", [8, 50, 128])
def test_restatement_at_float64_is_the_oracle(oracle, K):
    counts, M, mean, nrows = _side("edge")
    ncols = len(counts)
    rng = np.random.default_rng(50 + K)
    U = 0.3 * rng.standard_normal((nrows, K))
    A = rng.standard_normal((K, 3 * K))
    for it, alpha in ((0, 2.0), (7, 1.5)):
        mu, LU, LF = oracle.hyper_sample(K, ncols, A @ A.T / (3 * K), it)
        ref = np.zeros((ncols, K))
        oracle.sample_side(K, M, mean, alpha, U, ref, it, mu, LF)
        x, ok = cond_ref.sample_columns(np.float64, K, M, mean, alpha, U, mu, LF, it, oracle)
        assert x.dtype == np.float64 and ok.all()
        err = np.abs(x - ref).max() / np.abs(ref).max()
        print("cond-host restatement K=%d it=%d: %.3e of max|x|" % (K, it, err))
        assert err <= 1e-12


def test_restatement_stays_in_its_dtype(oracle):
    counts, M, mean, nrows = _side("edge")
    for dtype in (np.float32, np.longdouble):
        U, it, alpha, mu, LF = cond_ref.inputs(cond_ref.FP32_CASES[0], 8, nrows, True)
        x, ok = cond_ref.sample_columns(dtype, 8, M, mean, alpha, U, mu, LF, it, oracle)
        assert x.dtype == dtype and x.shape == (len(counts), 8) and ok.all()
    bad, ok = cond_ref.sample_columns(np.float64, 8, M, mean, 2.0, U, mu, -1e6 * np.eye(8), it, oracle)
    assert not ok.any() and np.isnan(bad).all()                       # a failed column is flagged, never a number


@pytest.mark.parametrize("side,K", SIDES)
def test_conditions_on_the_inputs(oracle, side, K):
    counts, M, mean, nrows = _side(side)
    for f32 in (False, True):
        for case in cond_ref.cases(f32):
            r = cond_ref.references(side, K, M, mean, nrows, case, f32, oracle)
            U, it, alpha, mu, LF = r["inputs"]
            assert np.array_equal(LF, LF.T)
            if f32:
                assert all(np.array_equal(a, a.astype(np.float32)) for a in (U, mu, LF))
            kappa = np.linalg.cond(cond_ref.posterior_precisions(K, M, alpha, U, LF)).max()
            print("cond-host %s K=%d %s %s: kappa_2 %.2e  E_ref %.3e" % (side, K, "fp32" if f32 else "fp64", case[0], kappa, r["e_ref"].max()))
            assert r["ok_ld"].all() and r["ok_ref"].all(), case[0]   # oracle (fp64) / float32 restatement (fp32) factorise every column
            if not f32:
                assert kappa <= cond_ref.KAPPA_MAX, (case[0], kappa)


@pytest.mark.parametrize("side,K", SIDES)
def test_the_reference_itself_loses_digits(oracle, side, K):
    counts, M, mean, nrows = _side(side)
    for f32 in (False, True):
        eps = cond_ref.EPS[np.float32 if f32 else np.float64]
        E = {}
        for case in cond_ref.cases(f32):
            e = cond_ref.references(side, K, M, mean, nrows, case, f32, oracle)["e_ref"]
            E[case[0]] = e.max()
            assert np.isfinite(e).all() and e.max() >= eps, (case[0], e.max())
        along_P = [E[c[0]] for c in cond_ref.cases(f32) if c[1][0] == "P"]
        assert len(along_P) >= 3 and along_P[-1] > along_P[0], along_P
        if not f32:                                                   # three decades of kappa apiece: every step shows (in fp32 the
            assert all(b > a for a, b in zip(along_P, along_P[1:])), along_P   # first decade is still at the rounding floor at K = 8)
