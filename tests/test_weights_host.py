"""Per-rating precision weights, CPU part: the expanded-rows reference of tests/weights_ref.py against the plain oracle (weights all 1:
the same bits; a constant weight c: the plain call at alpha c), bpmf_amd.rating_weights against the cell-by-cell statement on both
orientations and every refusal of it; gibbs(weights=...) and `bpmf --weights` refuse what they cannot do before anything touches a
GPU; the recorded figures of the planted experiment."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import bpmf_amd
from bpmf_amd import _lib
from tests import util
from tests import weights_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_parity import RTOL, rel_err

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
# The oracle adds its column statistics per thread and the threads' sums in the order they finish: two calls with the same inputs differ
# in the last bits of sum / prod (measured: 188 of 200 repeats), never in the factors.  1e-13 is ~500 roundings of a sum of 15 columns.
STAT_REPEAT = 1e-13


def run(args, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=e)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_weights_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    _lib.load_library()
    sigs = _lib.exported_signatures()
    for name in ("bpmf_hip_side_set_weights", "bpmf_hip_side_weights_get", "bpmf_hip_side_weights_count"):
        assert hasattr(raw, name) and name in sigs
    for name in ("set_weights", "weights_get", "weights_count"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
    assert callable(bpmf_amd.rating_weights)


def _edge_inputs(oracle, K=8, it=3):
    A, nrows, w = ref.edge_side()
    ncols = len(A[0]) - 1
    rng = np.random.default_rng(1)
    X, Y = 0.6 * rng.standard_normal((ncols, K)), 0.6 * rng.standard_normal((nrows, K))
    mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, it)
    return A, nrows, w, X, Y, mu, LF, util.mean_rating(A)


def test_edge_side_has_the_boundary_counts():
    A, nrows, w = ref.edge_side()
    assert nrows == 300 and tuple(np.diff(A[0])) == (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
    assert len(w) == len(A[2]) and np.all(w > 0) and np.all(np.isfinite(w))
    sw = np.sqrt(w)
    assert np.count_nonzero(sw * sw != w) > len(w) // 4                # the square roots round
    assert all(np.all(np.diff(A[1][A[0][c]:A[0][c + 1]]) > 0) for c in range(len(A[0]) - 1))


def test_unit_weights_are_the_plain_oracle(oracle):
    K, it, alpha = 8, 3, 1.7
    A, nrows, w, X, Y, mu, LF, mean = _edge_inputs(oracle, K, it)
    plain = X.copy()
    s0, p0, n0 = oracle.sample_side(K, A, mean, alpha, Y, plain, it, mu, LF, nthreads=ref.NT)
    ones = X.copy()
    s1, p1, n1 = ref.sample_side_weighted(oracle, K, A, np.ones(len(A[2])), mean, alpha, Y, ones, it, mu, LF)
    assert plain.tobytes() == ones.tobytes()
    assert rel_err(s1, s0) <= STAT_REPEAT and rel_err(p1, p0) <= STAT_REPEAT and abs(n1 - n0) <= STAT_REPEAT * abs(n0)
    # ... and seeded weights are another draw
    seeded = X.copy()
    ref.sample_side_weighted(oracle, K, A, w, mean, alpha, Y, seeded, it, mu, LF)
    assert rel_err(seeded, plain) > 1e-3


def test_constant_weight_is_a_scaled_alpha(oracle):
    K, it, alpha, c = 8, 3, 1.7, 2.5
    A, nrows, w, X, Y, mu, LF, mean = _edge_inputs(oracle, K, it)
    scaled = X.copy()
    oracle.sample_side(K, A, mean, alpha * c, Y, scaled, it, mu, LF, nthreads=ref.NT)
    const = X.copy()
    ref.sample_side_weighted(oracle, K, A, np.full(len(A[2]), c), mean, alpha, Y, const, it, mu, LF)
    err = rel_err(const, scaled)
    print("constant weight %g against alpha %g: %.3g of max|x|" % (c, alpha * c, err))
    assert err < RTOL


def test_reference_is_the_weighted_conditional(oracle):
    """The mean of the expanded-rows draw over many iterations' normals is Lambda*^-1 b of the weighted conditional: one column,
    checked against numpy's solve at 5 standard errors per coordinate."""
    K, alpha, n = 4, 1.3, 40
    rng = np.random.default_rng(12)
    A = (np.array([0, n], np.int64), np.arange(n, dtype=np.int32), rng.integers(1, 6, n).astype(np.float64))
    w = rng.gamma(2.0, 0.5, n)
    Y = rng.standard_normal((n, K))
    mean = 3.0
    mu, LU, LF = oracle.hyper_sample(K, 1, np.eye(K) * 0.2, 0)
    Ls = LF + alpha * (Y * w[:, None]).T @ Y
    b = LF @ mu + alpha * Y.T @ (w * (A[2] - mean))
    want, cov = np.linalg.solve(Ls, b), np.linalg.inv(Ls)
    draws = []
    for it in range(400):
        x = np.zeros((1, K))
        ref.sample_side_weighted(oracle, K, A, w, mean, alpha, Y, x, it, mu, LF)
        draws.append(x[0].copy())
    draws = np.array(draws)
    assert np.all(np.abs(draws.mean(0) - want) <= 5.0 * np.sqrt(np.diag(cov) / len(draws))), (draws.mean(0), want)


def _small():
    """7 users x 5 movies, 17 ratings less an empty column; W weights 6 of them"""
    rng = np.random.default_rng(3)
    cells = rng.choice(7 * 5, size=17, replace=False)
    r, c = cells // 5, cells % 5
    keep = c != 2
    r, c = r[keep], c[keep]
    m = sp.coo_matrix((rng.integers(1, 6, len(r)).astype(np.float64), (r, c)), shape=(7, 5))
    pick = rng.choice(len(r), size=6, replace=False)
    wm = sp.coo_matrix((np.array([2.5, 0.25, 1.0, 0.37, 7.0, 1e-3]), (r[pick], c[pick])), shape=(7, 5))
    return m, wm


def test_rating_weights_both_orientations():
    m, wm = _small()
    M, Mt = util.csc_arrays(m), util.csc_arrays(m.T)
    Wm, Wt = util.csc_arrays(wm), util.csc_arrays(wm.T)
    a, b = bpmf_amd.rating_weights(M, Wm), bpmf_amd.rating_weights(Mt, Wt)
    assert a.dtype == np.float64 and len(a) == len(M[2]) and len(b) == len(Mt[2])
    assert np.array_equal(a, ref.weights_of(M, Wm)) and np.array_equal(b, ref.weights_of(Mt, Wt))
    assert (a != 1.0).sum() == 5 and (b != 1.0).sum() == 5 and a.min() == 1e-3 and a.max() == 7.0
    # the weight of a cell is the same whichever orientation stores it
    am = sp.csc_matrix((a, M[1], M[0]), shape=(7, 5))
    bm = sp.csc_matrix((b, Mt[1], Mt[0]), shape=(5, 7))
    assert (am != bm.T).nnz == 0
    # the transpose gibbs() forms for the users' side is the matrix's transpose
    from bpmf_amd.censor import transpose_csc
    assert all(np.array_equal(x, y) for x, y in zip(transpose_csc(Wm, 7), Wt))
    assert all(np.array_equal(x, y) for x, y in zip(ref.transpose(Wm, 7), Wt))
    # nothing listed: all one
    empty = (np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0))
    assert np.array_equal(bpmf_amd.rating_weights(M, empty), np.ones(len(M[2])))


def test_rating_weights_refusals():
    m, wm = _small()
    M, Wm = util.csc_arrays(m), util.csc_arrays(wm)
    free = [(r, c) for r in range(7) for c in range(5) if m.tocsr()[r, c] == 0]
    r0, c0 = free[0]
    outside = util.csc_arrays(sp.coo_matrix(([2.0], ([r0], [c0])), shape=(7, 5)))
    with pytest.raises(ValueError, match=r"cell \(%d, %d\).*not a stored rating" % (r0, c0)):
        bpmf_amd.rating_weights(M, outside)
    cols = np.repeat(np.arange(5), np.diff(Wm[0]))
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        vals = Wm[2].copy(); vals[2] = bad
        with pytest.raises(ValueError, match=r"cell \(%d, %d\) is not finite and > 0" % (Wm[1][2], cols[2])):
            bpmf_amd.rating_weights(M, (Wm[0], Wm[1], vals))
    with pytest.raises(ValueError, match="columns"):
        bpmf_amd.rating_weights(M, (Wm[0][:-1], Wm[1], Wm[2]))
    with pytest.raises(ValueError, match="not a CSC triple"):
        bpmf_amd.rating_weights(M, (Wm[0], Wm[1][:-1], Wm[2][:-1]))
    twice = (Wm[0].copy(), Wm[1].copy(), Wm[2].copy())
    col = int(np.argmax(np.diff(Wm[0]) >= 2))
    assert Wm[0][col + 1] - Wm[0][col] >= 2
    twice[1][Wm[0][col] + 1] = twice[1][Wm[0][col]]
    with pytest.raises(ValueError, match="listed twice"):
        bpmf_amd.rating_weights(M, twice)
    with pytest.raises(ValueError):
        bpmf_amd.rating_weights(M, util.csc_arrays(wm.T))


def test_gibbs_refuses_what_does_not_go_with_weights():
    Wm = (np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(ValueError, match=r"weights.*probit=True"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, weights=Wm, probit=True)
    with pytest.raises(ValueError, match=r"weights.*censored"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, weights=Wm, censored=Wm)
    with pytest.raises(ValueError, match=r"weights.*noise='adaptive'"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, weights=Wm, noise="adaptive")
    with pytest.raises(ValueError, match=r"weights.*row_features / col_features"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, weights=Wm, row_features=np.zeros((1, 1)))
    with pytest.raises(ValueError, match=r"weights.*row_features / col_features"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, weights=Wm, col_features=np.zeros((1, 1)))

    class Fp32:
        dtype = "f32"
    with pytest.raises(ValueError, match=r"weights.*fp64"):
        bpmf_amd.gibbs(Fp32(), None, None, None, 1, 1, weights=Wm)
    # a weight matrix that does not fit the ratings is refused before a side is created (engine = None would raise otherwise)
    M = (np.array([0, 1], np.int64), np.array([0], np.int32), np.array([3.0]))
    bad = (np.array([0, 1], np.int64), np.array([1], np.int32), np.array([2.0]))
    with pytest.raises(ValueError, match="not a stored rating"):
        bpmf_amd.gibbs(None, M, M, None, 2, 1, weights=bad)
    zero = (np.array([0, 1], np.int64), np.array([0], np.int32), np.array([0.0]))
    with pytest.raises(ValueError, match="not finite and > 0"):
        bpmf_amd.gibbs(None, M, M, None, 2, 1, weights=zero)


def _write_mtx(path, nrows, ncols, entries):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (nrows, ncols, len(entries)))
        for r, c, v in entries:
            f.write("%d %d %s\n" % (r, c, v))


def test_cli_weights_refusals(tmp_path):
    good = tmp_path / "w.mtx"
    _write_mtx(good, 4, 2, [(1, 1, 2.5), (2, 1, 0.25)])
    feat = tmp_path / "f.csv"
    feat.write_text("1\n2\n3\n4\n")
    cases = [
        (["--weights", str(good), "-g", "2"], None, "--weights runs on one GPU without -g"),
        (["--weights", str(good), "-g", "1"], None, "--weights runs on one GPU without -g"),
        (["--weights", str(good), "--probit"], None, "--weights does not go together with --probit"),
        (["--weights", str(good), "--censored", str(good)], None, "--weights does not go together with --censored"),
        (["--weights", str(good), "--noise", "adaptive"], None, "--weights does not go together with --noise adaptive"),
        (["--weights", str(good), "--row-features", str(feat)], None, "--weights does not go together with --row-features / --col-features"),
        (["--weights", str(good), "--col-features", str(feat)], None, "--weights does not go together with --row-features / --col-features"),
        (["--weights", str(good), "-m", "a,b"], None, "--weights does not go together with a propagated posterior (-m / -l)"),
        (["--weights", str(good), "-l", "a,b"], None, "--weights does not go together with a propagated posterior (-m / -l)"),
        (["--weights", str(good), "--fp32", "-d", "100"], None, "--weights does not go together with --fp32"),
        (["--weights", str(good)], {"BPMF_REDUCE": "1"}, "--weights does not go together with BPMF_REDUCE=1"),
        (["--weights", ""], None, "--weights expects a file"),
    ]
    for extra, env, msg in cases:
        r = run(data_args() + extra, tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr
        assert "num_latent" not in r.stdout                              # stopped before Sys::init printed anything


def test_cli_weights_bad_files(tmp_path):
    """tiny-train.mtx is 4 x 2 with the cells (1..4, 1) and (1, 2), (3, 2): the first offending cell is named in 1-based ids"""
    files = {
        "absent.mtx": ([(2, 2, 1.5), (4, 2, 1.5)], "cell (2, 2) of", "is not a cell of the training matrix"),
        "zero.mtx": ([(1, 1, 1), (3, 1, 0), (4, 1, 0)], "cell (3, 1) of", "is not finite and > 0"),
        "neg.mtx": ([(1, 1, 1), (4, 1, -2.0)], "cell (4, 1) of", "is not finite and > 0"),
        "nan.mtx": ([(1, 1, 1), (2, 1, "nan")], "cell (2, 1) of", "is not finite and > 0"),
        "inf.mtx": ([(1, 2, "inf")], "cell (1, 2) of", "is not finite and > 0"),
    }
    for name, (entries, cell, what) in files.items():
        _write_mtx(tmp_path / name, 4, 2, entries)
        r = run(data_args() + ["--weights", str(tmp_path / name)], tmp_path)
        assert r.returncode != 0 and cell in r.stderr and what in r.stderr and "--weights" in r.stderr, (name, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1 and "num_latent" not in r.stdout, (name, r.stderr)
    _write_mtx(tmp_path / "shape.mtx", 5, 2, [(1, 1, 1)])
    r = run(data_args() + ["--weights", str(tmp_path / "shape.mtx")], tmp_path)
    assert r.returncode != 0 and "is 5 x 2, the training matrix is 4 x 2" in r.stderr and "num_latent" not in r.stdout, r.stderr
    r = run(data_args() + ["--weights", str(tmp_path / "missing.sdm")], tmp_path)
    assert r.returncode != 0 and "missing.sdm" in r.stderr and "num_latent" not in r.stdout, r.stderr
    (tmp_path / "dense.ddm").write_bytes(b"\0" * 32)
    r = run(data_args() + ["--weights", str(tmp_path / "dense.ddm")], tmp_path)
    assert r.returncode != 0 and "num_latent" not in r.stdout, r.stderr


def test_cli_usage_names_weights(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "[--weights FILE]" in text and "precision alpha w" in text


def test_planted_figures_are_the_recorded_ones(oracle):
    """The four restated CPU chains of the planted heteroscedastic experiment (weights_ref.PLANTED) give the recorded test RMSEs: the
    weights honoured, ignored at alpha = 16, ignored at the best single alpha, the noisy cells dropped.  (The factors of a restated
    chain do not depend on the oracle's thread schedule, its statistics do in their last bits: the bar is the 1e-6 of the chain tests.)"""
    got = ref.planted_measure(oracle)
    print("test RMSE: honoured %.4f, ignored %.4f, best single alpha %.4f, dropped %.4f" % got)
    assert np.abs(np.array(got) - np.array(ref.PLANTED_MEASURED)).max() < 1e-6
    a, b, c, d = ref.PLANTED_MEASURED
    assert a < d < c < b and ref.PLANTED_HALF_MARGIN == 0.5 * (c - a) > 0.2
