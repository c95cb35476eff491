"""Fold-in: what can be checked without a GPU.

  * the new entry points are exported and bound, the ABI version is unchanged; NULL handles are refused
  * the normals of tests/foldin_ref.py: the Philox blocks are the oracle's for the counter (i lo, i hi, s, n) and the key (42, tag),
    the pairing is Box-Muller on (1 - canonical53(w3, w2), canonical53(w1, w0)), the moments are a standard normal's; and the margin
    the GPU cases rely on: no u1 they draw is within 1e-300 of 0 (ln u1 is finite) -- u1 >= 2^-53 by construction, asserted on
    every block of every case
  * gibbs(foldin=True) / fold_in ValueErrors, raised before the engine is used
  * every refusal of `bpmf --fold-in-rows / --fold-in-cols` and the file-format errors, each with its one-line reason, before a
    device is opened
  * the planted experiment on the restated CPU chain: 600 x 300, rank 4, K = 8, 100 users held out of the matrix and folded in from
    12 ratings each, alpha = 4, 60 iterations, 30 burn-in; fold-in beats the mean predictor by at least half the measured margin

Fails on the commit before the feature: every test but the two that pin the reference (normals, planted experiment).
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import bpmf_amd
from bpmf_amd import _lib
from tests import foldin_ref as fr
from tests import probit_ref
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
EINVAL = -1

NEW = ("bpmf_hip_side_hyper_reserve", "bpmf_hip_side_hyper_add", "bpmf_hip_side_hyper_count", "bpmf_hip_side_hyper_get", "bpmf_hip_foldin",
       "bpmf_hip_foldin_count", "bpmf_hip_foldin_samples", "bpmf_hip_foldin_get", "bpmf_hip_foldin_get_padded", "bpmf_hip_foldin_predict",
       "bpmf_hip_foldin_topn", "bpmf_hip_foldin_last_ms", "bpmf_hip_foldin_chunk")


def test_foldin_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    sigs = _lib.exported_signatures()
    for name in NEW:
        assert hasattr(raw, name) and name in sigs, name
    assert _lib.load_library().bpmf_hip_abi_version() == 1
    for m in ("hyper_reserve", "hyper_add", "hyper_count", "hyper_get", "foldin", "foldin_get", "foldin_predict", "foldin_topn"):
        assert callable(getattr(bpmf_amd.HipEngine, m)), m
    assert callable(bpmf_amd.fold_in)
    assert 1 <= _lib.load_library().bpmf_hip_foldin_chunk() <= 64


def test_null_handles_are_refused():
    lib = _lib.load_library()
    out = np.zeros(4)
    idx = np.zeros(4, np.int32)
    ptr = np.zeros(2, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.bpmf_hip_side_hyper_reserve(None, 1) == EINVAL
    assert lib.bpmf_hip_side_hyper_add(None, 2.0, None, None) == EINVAL
    assert lib.bpmf_hip_side_hyper_count(None) == 0
    assert lib.bpmf_hip_side_hyper_get(None, None, None, None) == EINVAL
    assert lib.bpmf_hip_foldin(None, None, 0.0, 1, p(ptr), p(idx), p(out), 7, 1) == EINVAL
    assert lib.bpmf_hip_foldin_count(None) == 0 and lib.bpmf_hip_foldin_samples(None) == 0
    assert lib.bpmf_hip_foldin_get(None, p(out)) == EINVAL
    assert lib.bpmf_hip_foldin_get_padded(None, p(out)) == EINVAL
    assert lib.bpmf_hip_foldin_predict(None, None, 0.0, 0, 1, 0, 1, p(out), p(out)) == EINVAL
    assert lib.bpmf_hip_foldin_topn(None, None, 0.0, 1, 1, p(idx), p(out), p(out)) == EINVAL
    assert b"NULL" in lib.bpmf_hip_last_error()


# ---- the normals ------------------------------------------------------------------------------------------------------------------------

def test_normals_are_box_muller_on_the_oracles_philox(oracle):
    n_rows, S, K, tag = 5, 3, 7, fr.TAG_ROWS
    z = fr.normals(n_rows, S, K, tag, row0=2 ** 32 - 2)                       # rows 2^32 - 2 .. 2^32 + 2: the second counter word counts
    for i in range(n_rows):
        row = 2 ** 32 - 2 + i
        for s in range(S):
            for n in range((K + 1) // 2):
                w = [int(x) for x in oracle.philox([row & 0xFFFFFFFF, row >> 32, s, n], [42, tag])]
                u1 = 1.0 - min((w[3] + w[2] * 4294967296.0) * 2.0 ** -64, 1.0 - 2.0 ** -53)
                u2 = min((w[1] + w[0] * 4294967296.0) * 2.0 ** -64, 1.0 - 2.0 ** -53)
                rho = math.sqrt(-2.0 * math.log(u1))
                assert abs(z[i, s, 2 * n] - rho * math.cos(2.0 * math.pi * u2)) <= 1e-14
                if 2 * n + 1 < K:
                    assert abs(z[i, s, 2 * n + 1] - rho * math.sin(2.0 * math.pi * u2)) <= 1e-14
    # a row's normals depend on its index, the slot and the tag alone
    assert np.array_equal(fr.normals(3, 2, 8, 7)[1], fr.normals(1, 2, 8, 7, row0=1)[0])
    assert not np.array_equal(fr.normals(3, 2, 8, 7), fr.normals(3, 2, 8, 8))
    # a standard normal: mean, variance, fourth moment and the correlation of a pair within four standard errors
    big = fr.normals(20000, 5, 10, 7).ravel()
    N = len(big)
    assert abs(big.mean()) <= 4 / math.sqrt(N) and abs(big.var() - 1) <= 4 * math.sqrt(2 / N) and abs((big ** 4).mean() - 3) <= 4 * math.sqrt(96 / N)
    pairs = fr.normals(20000, 5, 10, 7)
    assert abs((pairs[:, :, 0] * pairs[:, :, 1]).mean()) <= 4 / math.sqrt(100000)


def test_no_uniform_of_the_gpu_cases_is_marginal():
    """What tests/test_gpu_foldin.py relies on: ln u1 is finite for every block its batches draw (u1 = 1 - canonical53 >= 2^-53)."""
    worst = 1.0
    for K in (8, 10, 32, 64, 100, 128):
        for S in (1, 3):
            u1, u2 = fr.uniforms(10, S, K, fr.TAG_ROWS)
            assert u1.shape == (10, S, (K + 1) // 2) and (u1 > 1e-300).all() and (u1 <= 1.0).all() and (u2 >= 0).all() and (u2 < 1).all()
            worst = min(worst, float(u1.min()))
    u1 = fr.uniforms(fr.PLANTED["held"], fr.PLANTED["nsims"] - fr.PLANTED["burnin"], fr.PLANTED["K"], fr.TAG_ROWS)[0]
    assert (u1 > 1e-300).all()
    print("smallest u1 over the GPU cases: %.3g" % min(worst, float(u1.min())))
    # and the clamp of canonical53 is what keeps it so: words of all ones give u1 = 2^-53
    ones = np.array([0xFFFFFFFF], np.uint64)
    assert 1.0 - probit_ref.canonical53(ones, ones)[0] == 2.0 ** -53


# ---- gibbs / fold_in --------------------------------------------------------------------------------------------------------------------

def test_gibbs_and_fold_in_refusals():
    F = np.ones((3, 2))
    g = lambda **kw: bpmf_amd.gibbs(None, None, None, None, 3, 3, **kw)
    with pytest.raises(ValueError, match="foldin=True does not go together with probit=True"):
        g(foldin=True, probit=True)
    with pytest.raises(ValueError, match="both sides have features"):
        g(foldin=True, row_features=F, col_features=F)
    with pytest.raises(ValueError, match="post-burn-in"):
        g(foldin=True, nsims=5, burnin=5)
    with pytest.raises(ValueError, match="post-burn-in"):
        g(foldin=True, nsims=4, burnin=5)
    R = sp.csr_matrix(np.ones((2, 3)))
    with pytest.raises(ValueError, match=r"gibbs\(\.\.\., foldin=True\)"):
        bpmf_amd.fold_in(dict(users=None, movies=None), new_rows=R)
    with pytest.raises(ValueError, match=r"gibbs\(\.\.\., foldin=True\)"):
        bpmf_amd.fold_in(None, new_rows=R)

    class Reached(Exception):
        pass

    class Side:                                                             # stands where a Sys does: any use of its engine says so
        def __init__(self, n, linked):
            self._n, self.linked_features = n, linked

        def num(self):
            return self._n

        def __getattr__(self, name):
            raise Reached(name)
    res = dict(foldin=True, users=Side(4, True), movies=Side(3, False))
    with pytest.raises(ValueError, match="new_rows and / or new_cols"):
        bpmf_amd.fold_in(res)
    with pytest.raises(ValueError, match="the users have features"):
        bpmf_amd.fold_in(res, new_rows=R)
    with pytest.raises(ValueError, match="scipy.sparse"):
        bpmf_amd.fold_in(res, new_cols=np.ones((4, 2)))
    with pytest.raises(ValueError, match=r"\[4, n_new >= 1\]"):
        bpmf_amd.fold_in(res, new_cols=sp.csr_matrix(np.ones((5, 2))))
    bad = sp.csr_matrix(np.array([[1.0, np.inf], [0, 0], [0, 0], [0, 0]]))
    with pytest.raises(ValueError, match="not finite"):
        bpmf_amd.fold_in(res, new_cols=bad)
    with pytest.raises(ValueError, match="topn must be >= 1"):
        bpmf_amd.fold_in(res, new_cols=sp.csr_matrix(np.ones((4, 2))), topn=0)
    with pytest.raises(Reached):                                            # valid arguments are refused by nothing before the engine is used
        bpmf_amd.fold_in(res, new_cols=sp.csr_matrix(np.ones((4, 2))))

    class Engine:
        def __getattr__(self, name):
            raise Reached(name)
    with pytest.raises(Reached):
        bpmf_amd.gibbs(Engine(), np.zeros(2, np.int64), np.zeros(2, np.int64), None, 1, 1, foldin=True)


def test_foldin_csr_keeps_duplicates_and_sorts():
    from bpmf_amd.engine import foldin_csr
    R = sp.csr_matrix((np.array([1.0, 2.0, 3.0, 0.0]), np.array([4, 1, 1, 2], np.int32), np.array([0, 3, 4], np.int64)), shape=(2, 5))
    rowptr, colidx, vals = foldin_csr(R, 5)
    assert rowptr.tolist() == [0, 3, 4] and colidx.tolist() == [1, 1, 4, 2] and sorted(vals[:3].tolist()) == [1.0, 2.0, 3.0] and vals[3] == 0.0
    with pytest.raises(ValueError, match=r"\[n_new, 6\]"):
        foldin_csr(R, 6)
    with pytest.raises(ValueError, match="CSR triple"):
        foldin_csr((np.array([0, 2]), np.array([1]), np.array([1.0])), 5)
    rowptr, colidx, vals = foldin_csr(sp.csr_matrix((3, 5)), 5)              # rows without a rating
    assert rowptr.tolist() == [0, 0, 0, 0] and len(colidx) == len(vals) == 1


# ---- the executable ---------------------------------------------------------------------------------------------------------------------

def run(args, cwd, env=None):
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                          env=dict(os.environ, **(env or {})))


def _write(path, A):
    from bpmf_amd import io
    Ac = sp.csc_matrix(A)
    Ac.sort_indices()
    io.write_sparse(path, A.shape[0], A.shape[1], (Ac.indptr.astype(np.int64), Ac.indices.astype(np.int32), Ac.data.astype(np.float64)))


def test_cli_refusals(tmp_path):
    from bpmf_amd import io
    nu, nm = util.tiny()[4:6]
    rng = np.random.default_rng(1)
    pick = lambda r, c: sp.csr_matrix(np.where(rng.random((r, c)) < 0.3, rng.integers(1, 6, (r, c)), 0).astype(float))
    _write(tmp_path / "rows.sdm", pick(4, nm))
    _write(tmp_path / "cols.sdm", pick(nu, 3))
    _write(tmp_path / "rows_wrong.sdm", pick(4, nm + 1))
    _write(tmp_path / "cols_wrong.sdm", pick(nu + 2, 3))
    bad = pick(4, nm).tolil(); bad[0, 0] = np.nan
    _write(tmp_path / "bad.sdm", bad.tocsr())
    io.write_dense(tmp_path / "dense.ddm", np.ones((4, nm)))
    io.write_dense(tmp_path / "feat_u.ddm", np.ones((nu, 2))); io.write_dense(tmp_path / "feat_m.ddm", np.ones((nm, 2)))
    (tmp_path / "twice.mtx").write_text("%%%%MatrixMarket matrix coordinate real general\n2 %d 3\n1 1 3.0\n2 2 4.0\n1 1 5.0\n" % nm)
    (tmp_path / "twice_cols.mtx").write_text("%%%%MatrixMarket matrix coordinate real general\n%d 2 3\n3 2 3.0\n2 1 4.0\n3 2 5.0\n" % nu)
    # the cap of 2^28 cells per file, on a matrix of 3 users x 4 096 movies
    wide_nu, wide_nm = 3, 4096
    _write(tmp_path / "wide.sdm", sp.csc_matrix((np.array([4.0, 2.0, 5.0]), (np.array([0, 1, 2]), np.array([0, 7, 4095]))), shape=(wide_nu, wide_nm)))
    many = (1 << 28) // wide_nm + 1
    _write(tmp_path / "many.sdm", sp.csc_matrix((np.array([3.0]), (np.array([many - 1]), np.array([5]))), shape=(many, wide_nm)))
    data = ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]
    o = ["-o", str(tmp_path)]
    rows, cols = ["--fold-in-rows", "rows.sdm"], ["--fold-in-cols", "cols.sdm"]
    cases = [
        (rows, None, "--fold-in-rows needs -o DIR"),
        (cols, None, "--fold-in-cols needs -o DIR"),
        (rows + o + ["-i", "4", "-b", "4"], None, "--fold-in-rows needs at least one post-burn-in sample (-i > -b)"),
        (cols + o + ["-i", "3", "-b", "4"], None, "--fold-in-cols needs at least one post-burn-in sample (-i > -b)"),
        (rows + o + ["-g", "1"], None, "--fold-in-rows runs on one GPU without -g"),
        (cols + o + ["-g", "2"], None, "--fold-in-cols runs on one GPU without -g"),
        (rows + o + ["--probit"], None, "--fold-in-rows does not go together with --probit"),
        (rows + o + ["-m", "a.ddm,b.ddm"], None, "--fold-in-rows does not go together with a propagated posterior (-m / -l)"),
        (cols + o + ["-l", "a.ddm,b.ddm"], None, "--fold-in-cols does not go together with a propagated posterior (-m / -l)"),
        (rows + o, {"BPMF_REDUCE": "1"}, "--fold-in-rows does not go together with BPMF_REDUCE=1"),
        (rows + o + ["--row-features", "feat_u.ddm"], None, "--fold-in-rows does not go together with --row-features"),
        (cols + o + ["--col-features", "feat_m.ddm"], None, "--fold-in-cols does not go together with --col-features"),
        (rows + o + ["--topn", "3", "--topn-score", "ucb"], None, "--fold-in-rows does not go together with --topn-score ucb"),
        (cols + o + ["--topn", "3", "--topn-score", "ei", "--topn-threshold", "3"], None, "--fold-in-cols does not go together with --topn-score ei"),
        (["--fold-in-rows", "rows_wrong.sdm"] + o, None, "rows_wrong.sdm is 4 x %d, the training matrix has %d columns" % (nm + 1, nm)),
        (["--fold-in-cols", "cols_wrong.sdm"] + o, None, "cols_wrong.sdm is %d x 3, the training matrix has %d rows" % (nu + 2, nu)),
        (["--fold-in-rows", "twice.mtx"] + o, None, "twice.mtx lists cell (1, 1) twice"),
        (["--fold-in-cols", "twice_cols.mtx"] + o, None, "twice_cols.mtx lists cell (3, 2) twice"),
        (["--fold-in-rows", "bad.sdm"] + o, None, "bad.sdm holds a value that is not finite"),
        (["--fold-in-rows", "dense.ddm"] + o, None, "dense.ddm is not a sparse matrix file"),
        (["--fold-in-rows", "missing.sdm"] + o, None, "missing.sdm"),
        (["-n", "wide.sdm", "-p", "wide.sdm", "--fold-in-rows", "many.sdm"] + o, None, "more than 2^28 cells per file: ask for the best N of every query with --topn"),
    ]
    for extra, env, msg in cases:
        r = run((data if extra[:1] != ["-n"] else []) + extra, tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr             # a one-line reason
        assert "num_latent" not in r.stdout                                  # before a device is opened
        assert not list(tmp_path.glob("foldin-*"))


def test_cli_usage_names_the_flags(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "--fold-in-rows FILE" in text and "--fold-in-cols FILE" in text and "foldin-rows-mean.ddm" in text and "foldin-cols-topn.csv" in text


# ---- the planted experiment -------------------------------------------------------------------------------------------------------------

def test_planted_fold_in_beats_the_mean_predictor(oracle):
    """foldin_ref.PLANTED on the restated CPU chain (foldin_ref.PLANTED_MEASURED): RMSE at the 1 200 held-out cells of the 100 held-out
    users
        by fold-in from 12 ratings each     0.6973
        with the same users in the matrix   0.6914
        by the mean predictor               2.0516
    (the noise floor sqrt(1 / alpha) is 0.5).  Fold-in is within 0.006 of having had the users in the matrix; asserted: it beats the
    mean predictor by at least half the measured margin (0.677)."""
    folded, inside, flat = fr.planted_measure(oracle)
    print("planted: fold-in %.4f, in the matrix %.4f, mean predictor %.4f" % (folded, inside, flat))
    for got, want in zip((folded, inside, flat), fr.PLANTED_MEASURED):
        assert abs(got - want) <= 1e-3                                       # the recorded numbers are this experiment's
    assert abs(fr.PLANTED_HALF_MARGIN - 0.5 * (2.051592827616552 - 0.6973206287420437)) < 1e-12
    assert flat - folded >= fr.PLANTED_HALF_MARGIN
    assert abs(folded - inside) <= 0.05
