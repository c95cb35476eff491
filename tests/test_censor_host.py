"""Censored ratings, CPU part: bpmf_amd.censor_flags against the cell-by-cell statement of tests/censor_ref.py on both orientations
and every refusal of it; gibbs(censored=...) and `bpmf --censored` refuse what they cannot do before anything touches a GPU; and
no accept / reject decision of the restated draw lies within 1e-9 of its threshold for the inputs the GPU parity test
(tests/test_gpu_censored.py) uses."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import bpmf_amd
from bpmf_amd import _lib
from tests import censor_ref as ref
from tests import probit_ref
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
MARGIN = 1e-9          # the bar of tests/test_probit_host.py, for the same reason (the GPU's m differs from numpy's by ~1e-15)


def run(args, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=e)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_censor_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    lib = _lib.load_library()
    sigs = _lib.exported_signatures()
    for name in ("bpmf_hip_side_set_censored", "bpmf_hip_side_censored_count", "bpmf_hip_side_censored_latent"):
        assert hasattr(raw, name) and name in sigs
    assert lib.bpmf_hip_abi_version() == 1
    for name in ("set_censored", "censored_count", "censored_latent"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
    assert callable(bpmf_amd.censor_flags)


def _small():
    """7 users x 5 movies, 17 ratings, one empty column; C marks 6 of them"""
    rng = np.random.default_rng(3)
    cells = rng.choice(7 * 5, size=17, replace=False)
    r, c = cells // 5, cells % 5
    keep = c != 2
    r, c = r[keep], c[keep]
    m = sp.coo_matrix((rng.integers(1, 6, len(r)).astype(np.float64), (r, c)), shape=(7, 5))
    pick = rng.choice(len(r), size=6, replace=False)
    cm = sp.coo_matrix((np.array([2.5, -1.0, 1.0, -0.25, 7.0, -3.0]), (r[pick], c[pick])), shape=(7, 5))
    return m, cm


def test_censor_flags_both_orientations():
    m, cm = _small()
    M, Mt = util.csc_arrays(m), util.csc_arrays(m.T)
    Cm, Ct = util.csc_arrays(cm), util.csc_arrays(cm.T)
    fm, fu = bpmf_amd.censor_flags(M, Cm), bpmf_amd.censor_flags(Mt, Ct)
    assert fm.dtype == np.int8 and fu.dtype == np.int8 and len(fm) == len(M[2]) and len(fu) == len(Mt[2])
    assert np.array_equal(fm, ref.flags_of(M, Cm)) and np.array_equal(fu, ref.flags_of(Mt, Ct))
    assert (fm > 0).sum() == 3 and (fm < 0).sum() == 3 and (fu > 0).sum() == 3 and (fu < 0).sum() == 3
    # the flag of a cell is the same whichever orientation stores it
    flag_m = sp.csc_matrix((fm.astype(np.float64) + 4.0, M[1], M[0]), shape=(7, 5))
    flag_u = sp.csc_matrix((fu.astype(np.float64) + 4.0, Mt[1], Mt[0]), shape=(5, 7))
    assert (flag_m != flag_u.T).nnz == 0
    # the transpose gibbs() forms for the users' side is the matrix's transpose
    from bpmf_amd.censor import transpose_csc
    got = transpose_csc(Cm, 7)
    assert all(np.array_equal(a, b) for a, b in zip(got, Ct))
    assert all(np.array_equal(a, b) for a, b in zip(ref.transpose(Cm, 7), Ct))
    # nothing listed: all zero
    empty = (np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0))
    assert not bpmf_amd.censor_flags(M, empty).any()


def test_censor_flags_refusals():
    m, cm = _small()
    M, Cm = util.csc_arrays(m), util.csc_arrays(cm)
    free = [(r, c) for r in range(7) for c in range(5) if m.tocsr()[r, c] == 0]
    r0, c0 = free[0]
    not_stored = util.csc_arrays(sp.coo_matrix(([1.0], ([r0], [c0])), shape=(7, 5)))
    with pytest.raises(ValueError, match=r"cell \(%d, %d\).*not a stored rating" % (r0, c0)):
        bpmf_amd.censor_flags(M, not_stored)
    for bad in (0.0, float("nan"), float("inf"), -float("inf")):
        vals = Cm[2].copy(); vals[2] = bad
        with pytest.raises(ValueError, match="zero or not finite"):
            bpmf_amd.censor_flags(M, (Cm[0], Cm[1], vals))
    with pytest.raises(ValueError, match="columns"):
        bpmf_amd.censor_flags(M, (Cm[0][:-1], Cm[1], Cm[2]))
    with pytest.raises(ValueError, match="not a CSC triple"):
        bpmf_amd.censor_flags(M, (Cm[0], Cm[1][:-1], Cm[2][:-1]))
    twice = (Cm[0].copy(), Cm[1].copy(), Cm[2].copy())
    col = int(np.argmax(np.diff(Cm[0]) >= 2))
    assert Cm[0][col + 1] - Cm[0][col] >= 2
    twice[1][Cm[0][col] + 1] = twice[1][Cm[0][col]]
    with pytest.raises(ValueError, match="listed twice"):
        bpmf_amd.censor_flags(M, twice)
    # a cell of the other orientation's shape is not a cell of this one
    with pytest.raises(ValueError):
        bpmf_amd.censor_flags(M, util.csc_arrays(cm.T))


def test_gibbs_refuses_what_does_not_go_with_censored():
    Cm = (np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(ValueError, match=r"censored.*probit=True"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, censored=Cm, probit=True)
    with pytest.raises(ValueError, match=r"censored.*noise='adaptive'"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, censored=Cm, noise="adaptive")
    with pytest.raises(ValueError, match=r"censored.*row_features / col_features"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, censored=Cm, row_features=np.zeros((1, 1)))
    with pytest.raises(ValueError, match=r"censored.*row_features / col_features"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, censored=Cm, col_features=np.zeros((1, 1)))
    with pytest.raises(ValueError, match=r"censored.*alpha"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, censored=Cm, alpha=0.0)
    # a censoring matrix that does not fit the ratings is refused before a side is created (engine = None would raise otherwise)
    M = (np.array([0, 1], np.int64), np.array([0], np.int32), np.array([3.0]))
    bad = (np.array([0, 1], np.int64), np.array([1], np.int32), np.array([1.0]))
    with pytest.raises(ValueError, match="not a stored rating"):
        bpmf_amd.gibbs(None, M, M, None, 2, 1, censored=bad)


def _write_mtx(path, nrows, ncols, entries, pattern=False):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (nrows, ncols, len(entries)))
        for r, c, v in entries:
            f.write("%d %d %s\n" % (r, c, v))


def test_cli_censored_refusals(tmp_path):
    good = tmp_path / "c.mtx"
    _write_mtx(good, 4, 2, [(1, 1, 1), (2, 1, -1)])
    feat = tmp_path / "f.csv"
    feat.write_text("1\n2\n3\n4\n")
    cases = [
        (["--censored", str(good), "-g", "2"], None, "--censored runs on one GPU without -g"),
        (["--censored", str(good), "-g", "1"], None, "--censored runs on one GPU without -g"),
        (["--censored", str(good), "--probit"], None, "--censored does not go together with --probit"),
        (["--censored", str(good), "--noise", "adaptive"], None, "--censored does not go together with --noise adaptive"),
        (["--censored", str(good), "--row-features", str(feat)], None, "--censored does not go together with --row-features / --col-features"),
        (["--censored", str(good), "--col-features", str(feat)], None, "--censored does not go together with --row-features / --col-features"),
        (["--censored", str(good), "-m", "a,b"], None, "--censored does not go together with a propagated posterior (-m / -l)"),
        (["--censored", str(good), "-l", "a,b"], None, "--censored does not go together with a propagated posterior (-m / -l)"),
        (["--censored", str(good)], {"BPMF_REDUCE": "1"}, "--censored does not go together with BPMF_REDUCE=1"),
        (["--censored", str(good), "-a", "0"], None, "--censored needs a noise precision -a F > 0"),
        (["--censored", ""], None, "--censored expects a file"),
    ]
    for extra, env, msg in cases:
        r = run(data_args() + extra, tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr
        assert "num_latent" not in r.stdout                              # stopped before Sys::init printed anything


def test_cli_censored_bad_files(tmp_path):
    """tiny-train.mtx is 4 x 2 with the cells (1..4, 1) and (1, 2), (3, 2): the first offending cell is named in 1-based ids"""
    files = {
        "absent.mtx": ([(2, 2, 1), (4, 2, 1)], "cell (2, 2) of", "is not a cell of the training matrix"),
        "zero.mtx": ([(1, 1, 1), (3, 1, 0), (4, 1, 0)], "cell (3, 1) of", "is zero or not finite"),
        "nan.mtx": ([(1, 1, 1), (2, 1, "nan")], "cell (2, 1) of", "is zero or not finite"),
    }
    for name, (entries, cell, what) in files.items():
        _write_mtx(tmp_path / name, 4, 2, entries)
        r = run(data_args() + ["--censored", str(tmp_path / name)], tmp_path)
        assert r.returncode != 0 and cell in r.stderr and what in r.stderr and "--censored" in r.stderr, (name, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1 and "num_latent" not in r.stdout, (name, r.stderr)
    _write_mtx(tmp_path / "shape.mtx", 5, 2, [(1, 1, 1)])
    r = run(data_args() + ["--censored", str(tmp_path / "shape.mtx")], tmp_path)
    assert r.returncode != 0 and "is 5 x 2, the training matrix is 4 x 2" in r.stderr and "num_latent" not in r.stdout, r.stderr
    r = run(data_args() + ["--censored", str(tmp_path / "missing.sdm")], tmp_path)
    assert r.returncode != 0 and "missing.sdm" in r.stderr and "num_latent" not in r.stdout, r.stderr
    (tmp_path / "dense.ddm").write_bytes(b"\0" * 32)
    r = run(data_args() + ["--censored", str(tmp_path / "dense.ddm")], tmp_path)
    assert r.returncode != 0 and "num_latent" not in r.stdout, r.stderr


def test_cli_usage_names_censored(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "[--censored FILE]" in text and "lower bound" in text


def test_no_decision_of_the_gpu_parity_inputs_is_marginal():
    """What tests/test_gpu_censored.py::test_latent_against_restatement relies on: for its inputs, every accept / reject
    comparison and every choice of proposal is at least 1e-9 from its threshold.  (An input that violated it would get another
    seed of its flags, never another bar.)"""
    sides, nu, nm = ref.latent_inputs()
    for A, nrows, side, tag, flags in sides:
        frac_r, frac_l = (flags > 0).mean(), (flags < 0).mean()
        assert 0.14 < frac_r < 0.16 and 0.09 < frac_l < 0.11
    worst = math.inf
    for K, dtype in probit_ref.LATENT_CASES:
        U, V = probit_ref.latent_factors(K, dtype, nu, nm)
        for A, nrows, side, tag, flags in sides:
            X, Y = (V, U) if side == 0 else (U, V)
            mean = util.mean_rating(A)
            for alpha in ref.LATENT_ALPHAS:
                z, pos, m, att, margin, bmargin = ref.latent(A, flags, X, Y, ref.LATENT_ITER, tag, alpha, mean, full=True)
                assert margin >= MARGIN and bmargin >= MARGIN, (K, dtype, tag, alpha, margin, bmargin)
                s = flags[pos].astype(np.float64)
                assert np.all(s * (z[pos] - A[2][pos]) >= 0.0) and np.array_equal(np.delete(z, pos), np.delete(A[2], pos))
                worst = min(worst, margin, bmargin)
    print("closest decision over the GPU parity inputs: %.3g" % worst)
    # ... and for the list-length edges
    A, nrows = ref.edge_side()
    rng = np.random.default_rng(5)
    X, Y = 0.6 * rng.standard_normal((len(A[0]) - 1, 8)), 0.6 * rng.standard_normal((nrows, 8))
    for count in ref.EDGE_COUNTS:
        for signs in ref.EDGE_SIGNS:
            flags = ref.edge_flags(A, count, signs)
            _, _, _, _, margin, bmargin = ref.latent(A, flags, X, Y, 2, ref.TAG_MOVIES, 3.0, util.mean_rating(A), full=True)
            assert margin >= MARGIN and bmargin >= MARGIN, (count, signs, margin, bmargin)


def test_restated_draw_is_the_truncated_normal_of_the_model():
    """z | censored ~ N(mean + m, 1 / alpha) beyond the bound: the mean of the restated draws against the closed form, per bucket"""
    from scipy.stats import norm
    n = 400000
    rng = np.random.default_rng(8)
    colptr = np.array([0, n], np.int64)
    A = (colptr, np.arange(n, dtype=np.int32), rng.integers(1, 6, n).astype(np.float64))
    flags = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)
    X = np.ones((1, 1)); Y = rng.standard_normal((n, 1)) * 1.5
    alpha, mean = 3.0, 3.1
    z = ref.latent(A, flags, X, Y, 4, ref.TAG_USERS, alpha, mean)
    s = flags.astype(np.float64)
    assert np.all(s * (z - A[2]) >= 0.0)
    sa = math.sqrt(alpha)
    a = s * sa * ((A[2] - mean) - Y[:, 0])                           # standardised distance of the bound from the centre, towards the tail
    t = s * sa * (z - mean - Y[:, 0])                                # the standardised draw: N(0, 1) | t > a
    lam = np.exp(norm.logpdf(a) - norm.logsf(a))
    var = 1.0 + a * lam - lam * lam
    checked = 0
    for lo, hi in zip(np.arange(-5.0, 5.0, 0.5), np.arange(-4.5, 5.5, 0.5)):
        sel = (a >= lo) & (a < hi)
        if sel.sum() < 30:
            continue
        assert abs((t[sel] - lam[sel]).sum()) <= 4.0 * math.sqrt(var[sel].sum()), (lo, hi)
        checked += 1
    assert checked >= 14
