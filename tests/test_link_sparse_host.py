"""Sparse side information: what can be checked without a GPU.

  * the new entry points are exported and bound, the ABI version is unchanged
  * the restated row streams (tests/link_sparse_ref.py::randn_rows): a row whose counter has one non-zero word is the keyed stream
    tests/link_ref.py::randn_tag restates (pinned against the oracle in tests/test_link_host.py), bit for bit; the streams of the
    key words tag + 0x10000 / tag + 0x20000 differ from those of the key words 0, 3, 4
  * the exact draw: mean and covariance of the restated beta over many iterations against G^-1 F^T (U - 1 mu^T) and
    G^-1 (x) Lambda^-1
  * the restated lockstep CG: a zero column stays exactly zero with no iteration charged, max_iter is reported
  * argument refusals of every new entry point; BPMF_HIP_ENODEV, not a crash, where a device is needed and there is none; gibbs
    takes a scipy.sparse matrix up to the point where it needs the device
  * the `bpmf` flags: --link-tol without a sparse file, a sparse file with the wrong row count, the usage text; the .sdm / .sbm
    round trip of a feature file

Fails on the commit before the feature: every test but test_feature_files_round_trip (it pins a piece the feature builds on).
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import bpmf_amd
from bpmf_amd import _lib, engine
from tests import link_ref as ref
from tests import link_sparse_ref as sref
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
EINVAL, ENODEV = -1, -2

NEW = ("bpmf_hip_side_set_features_sparse", "bpmf_hip_side_link_cg_set", "bpmf_hip_side_link_cg_stats", "bpmf_hip_link_spmm_nn",
       "bpmf_hip_link_spmm_tn", "bpmf_hip_link_cg_solve", "bpmf_hip_link_noise_rows")


def run(args, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=e)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_sparse_link_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    sigs = _lib.exported_signatures()
    for name in NEW:
        assert hasattr(raw, name) and name in sigs, name
    assert _lib.load_library().bpmf_hip_abi_version() == 1


# ---- streams -------------------------------------------------------------------------------------------------------------------------

def test_row_stream_special_case_is_the_keyed_stream():
    """counter = {i, 0, 0, attempt}: row i at iteration 0 is randn_tag(i, key, K), the polar restatement pinned against the oracle"""
    for key in (5, 3 + sref.KEY_Z1, 4 + sref.KEY_Z2):
        rows = sref.randn_rows(4, 37, 0, key, row0=9)
        for i in range(4):
            assert np.array_equal(rows[i], ref.randn_tag(9 + i, key, 37))
    # a prefix of a longer row, and independent of the rows drawn beside it
    assert np.array_equal(sref.randn_rows(2, 8, 6, 77)[1], sref.randn_rows(1, 20, 6, 77, row0=1)[0, :8])


def test_row_streams_are_disjoint_from_the_other_streams():
    K, it = 64, 2
    z1 = sref.randn_rows(3, K, it, ref.TAG_MOVIES + sref.KEY_Z1)
    z2 = sref.randn_rows(3, K, it, ref.TAG_MOVIES + sref.KEY_Z2)
    zu = sref.randn_rows(3, K, it, ref.TAG_USERS + sref.KEY_Z1)
    others = [sref.randn_rows(3, K, it, key) for key in (0, ref.TAG_MOVIES, ref.TAG_USERS)]
    every = [z1, z2, zu] + others
    for a in range(len(every)):
        for b in range(a + 1, len(every)):
            assert not np.any(every[a] == every[b])
    assert not np.any(z1 == sref.randn_rows(3, K, it + 1, ref.TAG_MOVIES + sref.KEY_Z1))     # another iteration
    assert not np.any(z1[0] == z1[1])                                                        # another row
    # rows at iteration `it` are not the dense link's stream of counter `it` either
    assert not np.any(np.isin(z1.ravel(), ref.randn_tag(it, ref.TAG_MOVIES, 3 * K)))
    big = sref.randn_rows(400, 64, 1, 4 + sref.KEY_Z2)
    assert abs(big.mean()) < 0.03 and abs(big.std() - 1.0) < 0.02


# ---- the exact draw ------------------------------------------------------------------------------------------------------------------

def test_restated_draw_has_the_conditional_mean_and_covariance():
    """N = 40, D = 5, K = 3, fixed U, mu, Lambda; beta over it = 0 .. 2999 by the restated step 2' (CG at 1e-12: D = 5 converges in 5
    iterations).  Per entry, 5 standard errors: of the mean sqrt(C_ee / n), of the covariance sqrt((C_ee C_ff + C_ef^2) / n) with
    C = G^-1 (x) Lambda^-1.  The streams are deterministic: measured at n = 3000 the largest |z| is 2.55 over the 15 means and 2.82
    over the 225 covariances (2000: 3.07 / 2.97, 4000: 1.86 / 2.88)."""
    n = 3000
    rng = np.random.default_rng(5)
    N, D, K = 40, 5, 3
    F = sref.random_sparse(N, D, 0.4, 7)
    U, mu = rng.standard_normal((N, K)), rng.standard_normal(K)
    A = rng.standard_normal((K, K))
    Lam = A @ A.T + K * np.eye(K)
    R = np.linalg.cholesky(Lam).T
    link = sref.SparseLink(F, 2.0, 1e-12, 1000)
    B = np.empty((n, D * K))
    for it in range(n):
        B[it] = sref.draw_beta(link, U, mu, R, it, 3).ravel()
    Ginv = np.linalg.inv(link.G)
    mean = (Ginv @ (F.T @ (U - mu))).ravel()
    cov = np.kron(Ginv, np.linalg.inv(Lam))
    zm = (B.mean(axis=0) - mean) / np.sqrt(np.diag(cov) / n)
    Cn = (B - mean).T @ (B - mean) / n
    zc = (Cn - cov) / np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / n)
    print("n %d: max |z| mean %.2f covariance %.2f, CG iterations <= %d" % (n, np.abs(zm).max(), np.abs(zc).max(), max(link.iters)))
    assert np.abs(zm).max() <= 5.0 and np.abs(zc).max() <= 5.0
    assert max(link.iters) <= D + 1 and not link.hit


# ---- the restated CG -----------------------------------------------------------------------------------------------------------------

def test_restated_cg_freezes_columns():
    F = sref.random_sparse(300, 40, 0.1, 3)
    Ft = F.T.tocsr()
    rng = np.random.default_rng(4)
    RHS = rng.standard_normal((40, 6))
    RHS[:, 2] = 0.0
    RHS[:, 4] *= 1e-30
    G = (Ft @ F).toarray() + 3.0 * np.eye(40)
    x, iters, hit = sref.cg_lockstep(F, Ft, 3.0, RHS, 1e-12, 1000)
    want = np.linalg.solve(G, RHS)
    assert not hit and iters[2] == 0 and np.all(x[:, 2] == 0.0) and np.all(iters[[0, 1, 3, 4, 5]] > 0)
    kappa = np.linalg.cond(G)
    for k in range(6):
        assert np.linalg.norm(x[:, k] - want[:, k]) <= 4.0 * kappa * 1e-12 * np.linalg.norm(want[:, k])
    x3, it3, hit3 = sref.cg_lockstep(F, Ft, 3.0, RHS, 1e-12, 3)
    assert hit3 and np.all(it3[[0, 1, 3, 4, 5]] == 3) and it3[2] == 0
    # the same draw by CG and by the dense solve: what a chain pays for the tolerance
    link = sref.SparseLink(F, 3.0, 1e-12)
    assert np.abs(link.solve(RHS) - want).max() <= 4.0 * kappa * 1e-12 * np.abs(want).max()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_null_and_bad_arguments_are_refused():
    lib = _lib.load_library()
    one = np.zeros(8)
    p = one.ctypes.data
    ptr = np.array([0, 1, 2], np.int64)
    idx = np.array([0, 1], np.int32)
    rp, ci = ptr.ctypes.data, idx.ctypes.data
    bad_ptr0 = np.array([1, 1, 2], np.int64).ctypes
    down = np.array([0, 2, 1], np.int64)
    unsorted = (np.array([0, 2, 2], np.int64), np.array([1, 0], np.int32))
    dup = (np.array([0, 2, 2], np.int64), np.array([1, 1], np.int32))
    out_of_range = np.array([0, 2], np.int32)
    negative = np.array([-1, 1], np.int32)
    nan = np.array([1.0, np.nan])
    hit = C.c_int()
    calls = [
        lambda: lib.bpmf_hip_side_set_features_sparse(None, 2, rp, ci, None, 5.0, 3),
        lambda: lib.bpmf_hip_side_link_cg_set(None, 1e-6, 10),
        lambda: lib.bpmf_hip_side_link_cg_stats(None, None, None, None, None),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, None, ci, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, rp, None, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, rp, ci, None, None, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, rp, ci, None, p, 1, None),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 0, 2, rp, ci, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 0, rp, ci, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, rp, ci, None, p, 129, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, rp, ci, None, p, 0, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, bad_ptr0.data, ci, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, down.ctypes.data, ci, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, unsorted[0].ctypes.data, unsorted[1].ctypes.data, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, dup[0].ctypes.data, dup[1].ctypes.data, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, rp, out_of_range.ctypes.data, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, rp, negative.ctypes.data, None, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_nn(0, 2, 2, rp, ci, nan.ctypes.data, p, 1, p),
        lambda: lib.bpmf_hip_link_spmm_tn(0, 2, 2, rp, ci, None, None, 1, 0.0, None, p),
        lambda: lib.bpmf_hip_link_spmm_tn(0, 2, 2, rp, ci, None, p, 1, 0.0, None, None),
        lambda: lib.bpmf_hip_link_spmm_tn(0, 2, 2, rp, ci, None, p, 129, 0.0, None, p),
        lambda: lib.bpmf_hip_link_spmm_tn(0, 2, 2, rp, out_of_range.ctypes.data, None, p, 1, 0.0, None, p),
        lambda: lib.bpmf_hip_link_cg_solve(0, 2, 2, rp, ci, None, 1.0, None, 1, 1e-6, 10, p, None, C.byref(hit)),
        lambda: lib.bpmf_hip_link_cg_solve(0, 2, 2, rp, ci, None, 1.0, p, 1, 1e-6, 10, None, None, C.byref(hit)),
        lambda: lib.bpmf_hip_link_cg_solve(0, 2, 2, rp, ci, None, 0.0, p, 1, 1e-6, 10, p, None, C.byref(hit)),
        lambda: lib.bpmf_hip_link_cg_solve(0, 2, 2, rp, ci, None, 1.0, p, 1, 0.0, 10, p, None, C.byref(hit)),
        lambda: lib.bpmf_hip_link_cg_solve(0, 2, 2, rp, ci, None, 1.0, p, 1, 1.0, 10, p, None, C.byref(hit)),
        lambda: lib.bpmf_hip_link_cg_solve(0, 2, 2, rp, ci, None, 1.0, p, 1, 1e-6, 0, p, None, C.byref(hit)),
        lambda: lib.bpmf_hip_link_cg_solve(0, 2, 2, rp, ci, None, 1.0, p, 129, 1e-6, 10, p, None, C.byref(hit)),
        lambda: lib.bpmf_hip_link_cg_solve(0, 2, 2, rp, ci, None, 1.0, nan.ctypes.data, 1, 1e-6, 10, p, None, C.byref(hit)),
        lambda: lib.bpmf_hip_link_cg_solve(0, 2, 2, unsorted[0].ctypes.data, unsorted[1].ctypes.data, None, 1.0, p, 1, 1e-6, 10, p, None, C.byref(hit)),
        lambda: lib.bpmf_hip_link_noise_rows(0, 2, 2, 0, 5, None, None),
        lambda: lib.bpmf_hip_link_noise_rows(0, 0, 2, 0, 5, None, p),
        lambda: lib.bpmf_hip_link_noise_rows(0, 2, 0, 0, 5, None, p),
        lambda: lib.bpmf_hip_link_noise_rows(0, 2, 129, 0, 5, None, p),
        lambda: lib.bpmf_hip_link_noise_rows(0, 1, 1, 0, 5, np.array([np.inf]).ctypes.data, p),
    ]
    for i, fn in enumerate(calls):
        assert fn() == EINVAL, i
        assert lib.bpmf_hip_last_error()


def test_sparse_pieces_need_a_device():
    """Without a HIP device every piece reports BPMF_HIP_ENODEV: no crash, no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    F = sp.csr_matrix(np.array([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]]))
    for fn in (lambda: engine.link_spmm_nn(F, np.ones((2, 3))), lambda: engine.link_spmm_tn(F, np.ones((3, 3))),
               lambda: engine.link_cg_solve(F, 1.0, np.ones((2, 3))), lambda: engine.link_noise_rows(2, 3, 0, 5)):
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            fn()
        assert e.value.code == ENODEV


def test_csr_arrays_are_canonical():
    coo = sp.coo_matrix((np.array([1.0, 2.0, 3.0, 4.0]), (np.array([1, 0, 1, 1]), np.array([2, 1, 0, 2]))), shape=(3, 4))
    rowptr, colidx, vals = engine.csr_arrays(coo)
    assert rowptr.dtype == np.int64 and colidx.dtype == np.int32
    assert list(rowptr) == [0, 1, 3, 3] and list(colidx) == [1, 0, 2] and list(vals) == [2.0, 3.0, 5.0]
    assert engine.csr_arrays(sp.csr_matrix(np.array([[1.0, 0.0], [1.0, 1.0]])))[2] is None       # all ones: no values
    assert engine._is_sparse(coo) and not engine._is_sparse(np.zeros((2, 2)))


def test_gibbs_takes_a_sparse_matrix_up_to_the_device():
    F = sp.csr_matrix(np.ones((1, 1)))
    with pytest.raises(ValueError, match="pipelined=True"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, row_features=F, pipelined=True)
    with pytest.raises(ValueError, match="link_tol"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, row_features=F, link_tol=0.0)
    with pytest.raises(ValueError, match="link_tol"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, col_features=F, link_max_iter=0)
    with pytest.raises(AttributeError):                                     # the arguments passed: the engine is what is missing
        bpmf_amd.gibbs(None, np.zeros(2, np.int64), np.zeros(2, np.int64), None, 1, 1, row_features=F, link_tol=1e-8, link_max_iter=5)


# ---- the executable ------------------------------------------------------------------------------------------------------------------

def _write_features(path, F):
    from bpmf_amd import io
    Fc = sp.csc_matrix(F)
    Fc.sort_indices()
    io.write_sparse(path, F.shape[0], F.shape[1], (Fc.indptr, Fc.indices, Fc.data))


def test_feature_files_round_trip(tmp_path):
    from bpmf_amd import io
    F = sref.random_sparse(37, 50, 0.1, 3)
    B = sref.skewed_bits(37, 50, 6, 4)
    for name, A in (("f.sdm", F), ("f.sbm", B), ("f.mtx", F), ("f.sdm.gz", F)):
        _write_features(tmp_path / name, A)
        nr, nc, (colptr, rowidx, vals) = io.read_sparse(tmp_path / name)
        back = sp.csc_matrix((vals, rowidx, colptr), shape=(nr, nc))
        assert (nr, nc) == A.shape
        if name.endswith(".mtx"):
            assert np.allclose(back.toarray(), A.toarray(), rtol=1e-5, atol=1e-8)     # (the text writer prints fewer digits)
        else:
            assert np.array_equal(back.toarray(), A.toarray())
    assert np.all(io.read_sparse(tmp_path / "f.sbm")[2][2] == 1.0)


def test_cli_sparse_feature_refusals(tmp_path):
    from bpmf_amd import io
    nu, nm = util.tiny()[4:6]
    io.write_dense(tmp_path / "rows.ddm", ref.features(nu, 3, 1))
    _write_features(tmp_path / "rows.sbm", sref.skewed_bits(nu, 40, 4, 1))
    _write_features(tmp_path / "short.sdm", sref.random_sparse(nu - 1, 40, 0.1, 1))
    _write_features(tmp_path / "short.mtx", sref.random_sparse(nu - 1, 40, 0.1, 1))
    rows = ["--row-features", "rows.sbm"]
    cases = [
        (["--link-tol", "1e-8"], None, "need a sparse feature file"),
        (["--link-max-iter", "10"], None, "need a sparse feature file"),
        (["--row-features", "rows.ddm", "--link-tol", "1e-8"], None, "need a sparse feature file"),
        (["--col-features", "rows.ddm", "--link-max-iter", "10"], None, "need a sparse feature file"),
        (rows + ["--link-tol", "0"], None, "--link-tol expects a number 0 < F < 1"),
        (rows + ["--link-tol", "x"], None, "--link-tol expects a number 0 < F < 1"),
        (rows + ["--link-tol", "2"], None, "--link-tol expects a number 0 < F < 1"),
        (rows + ["--link-max-iter", "0"], None, "--link-max-iter expects an integer"),
        (rows + ["--link-max-iter", "1.5"], None, "--link-max-iter expects an integer"),
        (["--row-features", "short.sdm"], None, "rows, the side has"),
        (["--row-features", "short.mtx"], None, "rows, the side has"),
        (["--col-features", "rows.sbm"], None, "rows, the side has"),
        (["--row-features", "missing.sbm"], None, "missing.sbm"),
        (rows + ["-g", "2"], None, "run on one GPU without -g"),
        (rows + ["--probit"], None, "do not go together with --probit"),
        (rows + ["--noise", "adaptive"], None, "do not go together with --noise adaptive"),
        (rows + ["--fp32", "-d", "128"], None, "do not go together with --fp32"),
        (rows, {"BPMF_REDUCE": "1"}, "do not go together with BPMF_REDUCE=1"),
    ]
    for extra, env, msg in cases:
        r = run(data_args() + extra + ["-o", str(tmp_path)], tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert "num_latent" not in r.stdout
        assert not (tmp_path / "U-link.ddm").exists() and not (tmp_path / "V-link.ddm").exists()


def test_cli_usage_names_the_sparse_flags(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "--link-tol F" in text and "--link-max-iter N" in text
    assert ".sbm" in text and "conjugate gradients" in text
