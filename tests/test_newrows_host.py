"""Rows unseen in training: what can be checked without a GPU.

  * the new entry points are exported and bound, the ABI version is unchanged
  * every refusal of `bpmf --new-row-features / --new-col-features`, each with its reason, before a GPU is touched: a flag without
    its partner, a D mismatch, dense against sparse, a missing -o, -i <= -b, non-finite features, a file of more than 2^28 cells
    without --topn
  * the same for gibbs()'s ValueErrors
  * NULL handles at the C ABI
  * tests/newrows_ref.py against the 6 x 5 case worked by hand in its docstring, exactly; the naive sum p / sum p^2 form it carries
    loses the variance under cancellation, the restatement does not

Fails on the commit before the feature: every test but test_reference_reproduces_the_hand_case and
test_naive_moments_cancel (they pin the reference the GPU tests are judged by).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import bpmf_amd
from bpmf_amd import _lib
from tests import link_ref as ref
from tests import newrows_ref as nr
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
EINVAL = -1

NEW = ("bpmf_hip_predict_block", "bpmf_hip_side_newrows_set", "bpmf_hip_side_newrows_set_sparse", "bpmf_hip_side_newrows_add",
       "bpmf_hip_side_newrows_count", "bpmf_hip_side_newrows_get", "bpmf_hip_newrows_predict", "bpmf_hip_newrows_topn")


def run(args, cwd):
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_newrows_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    sigs = _lib.exported_signatures()
    for name in NEW:
        assert hasattr(raw, name) and name in sigs, name
    assert _lib.load_library().bpmf_hip_abi_version() == 1
    for m in ("newrows_set", "newrows_add", "newrows_count", "newrows_get", "newrows_predict", "newrows_topn", "predict_block"):
        assert callable(getattr(bpmf_amd.HipEngine, m)), m


def test_null_handles_are_refused():
    lib = _lib.load_library()
    out = np.zeros(4)
    idx = np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.bpmf_hip_side_newrows_set(None, 1, p(out), 1) == EINVAL
    assert lib.bpmf_hip_side_newrows_set_sparse(None, 1, None, None, None, 1) == EINVAL
    assert lib.bpmf_hip_side_newrows_add(None, None) == EINVAL
    assert lib.bpmf_hip_side_newrows_count(None) == 0
    assert lib.bpmf_hip_side_newrows_get(None, None, None) == EINVAL
    assert lib.bpmf_hip_newrows_predict(None, None, 0.0, 0, 1, 0, 1, p(out), p(out)) == EINVAL
    assert lib.bpmf_hip_predict_block(None, None, 0.0, 0, 1, 0, 1, p(out), p(out)) == EINVAL
    assert lib.bpmf_hip_newrows_topn(None, None, 0.0, 1, 1, p(idx), p(out), p(out)) == EINVAL
    assert b"NULL" in lib.bpmf_hip_last_error()


def test_gibbs_refusals():
    F = np.ones((3, 2))
    Fs = sp.csr_matrix(F)
    g = lambda **kw: bpmf_amd.gibbs(None, None, None, None, 3, 3, **kw)
    with pytest.raises(ValueError, match="new_row_features needs row_features"):
        g(new_row_features=F)
    with pytest.raises(ValueError, match="new_col_features needs col_features"):
        g(new_col_features=F, row_features=F)
    with pytest.raises(ValueError, match="same kind"):
        g(new_row_features=Fs, row_features=F)
    with pytest.raises(ValueError, match="same kind"):
        g(new_col_features=F, col_features=Fs)
    with pytest.raises(ValueError, match=r"n_new >= 1, 2\]"):
        g(new_row_features=np.ones((4, 3)), row_features=F)
    with pytest.raises(ValueError, match=r"n_new >= 1, 2\]"):
        g(new_col_features=sp.csr_matrix(np.ones((4, 5))), col_features=Fs)
    with pytest.raises(ValueError, match="n_new >= 1"):
        g(new_row_features=np.ones((0, 2)), row_features=F)
    bad = np.ones((4, 2)); bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        g(new_row_features=bad, row_features=F)
    with pytest.raises(ValueError, match="not finite"):
        g(new_col_features=sp.csr_matrix(np.where(np.isnan(bad), np.inf, bad)), col_features=Fs)
    with pytest.raises(ValueError, match="post-burn-in"):
        g(new_row_features=np.ones((4, 2)), row_features=F, nsims=5, burnin=5)
    with pytest.raises(ValueError, match="pipelined"):                      # and whatever the features refuse stays refused
        g(new_row_features=np.ones((4, 2)), row_features=F, pipelined=True)

    class Reached(Exception):
        pass

    class Engine:                                                           # stands where the engine does: any use of it says so
        def __getattr__(self, name):
            raise Reached(name)
    with pytest.raises(Reached):                                            # valid arguments are refused by nothing before the engine is used
        bpmf_amd.gibbs(Engine(), np.zeros(2, np.int64), np.zeros(2, np.int64), None, 1, 1, row_features=np.ones((1, 2)), new_row_features=np.ones((4, 2)))


def _write_sparse(path, F):
    from bpmf_amd import io
    Fc = sp.csc_matrix(F)
    Fc.sort_indices()
    io.write_sparse(path, F.shape[0], F.shape[1], (Fc.indptr, Fc.indices, Fc.data))


def test_cli_refusals(tmp_path):
    from bpmf_amd import io
    nu, nm = util.tiny()[4:6]
    rng = np.random.default_rng(1)
    io.write_dense(tmp_path / "rows.ddm", ref.features(nu, 3, 1))
    io.write_dense(tmp_path / "cols.ddm", ref.features(nm, 3, 2))
    io.write_dense(tmp_path / "new3.ddm", ref.features(5, 3, 3))
    io.write_dense(tmp_path / "new4.ddm", ref.features(5, 4, 4))
    bad = ref.features(5, 3, 5); bad[4, 2] = np.inf
    io.write_dense(tmp_path / "bad.ddm", bad)
    Srows = sp.csr_matrix((rng.random((nu, 40)) < 0.1).astype(float))
    _write_sparse(tmp_path / "rows.sdm", Srows)
    _write_sparse(tmp_path / "new40.sdm", sp.csr_matrix((rng.random((5, 40)) < 0.1).astype(float)))
    _write_sparse(tmp_path / "new41.sdm", sp.csr_matrix((rng.random((5, 41)) < 0.1).astype(float)))
    sbad = sp.csr_matrix((rng.random((5, 40)) < 0.2).astype(float)); sbad.data[0] = np.nan
    _write_sparse(tmp_path / "sbad.sdm", sbad)
    # the cap of 2^28 cells per file, on a matrix of 3 users x 4 096 movies so that the feature file past it stays at 512 KiB
    wide_nu, wide_nm = 3, 4096
    wide = sp.csc_matrix((np.array([4.0, 2.0, 5.0]), (np.array([0, 1, 2]), np.array([0, 7, 4095]))), shape=(wide_nu, wide_nm))
    io.write_sparse(tmp_path / "wide.sdm", wide_nu, wide_nm, (wide.indptr.astype(np.int64), wide.indices.astype(np.int32), wide.data))
    io.write_dense(tmp_path / "huge.ddm", np.zeros(((1 << 28) // wide_nm + 1, 1)))
    io.write_dense(tmp_path / "rows1.ddm", ref.features(wide_nu, 1, 6))
    wide_args = ["-n", "wide.sdm", "-p", "wide.sdm"]
    o = ["-o", str(tmp_path)]
    rows, cols = ["--row-features", "rows.ddm"], ["--col-features", "cols.ddm"]
    cases = [
        (["--new-row-features", "new3.ddm"] + o, "--new-row-features needs --row-features"),
        (["--new-col-features", "new3.ddm"] + o, "--new-col-features needs --col-features"),
        (rows + ["--new-col-features", "new3.ddm"] + o, "--new-col-features needs --col-features"),
        (cols + ["--new-row-features", "new3.ddm"] + o, "--new-row-features needs --row-features"),
        (rows + ["--new-row-features", "new4.ddm"] + o, "has 4 feature columns, --row-features has 3"),
        (cols + ["--new-col-features", "new4.ddm"] + o, "has 4 feature columns, --col-features has 3"),
        (["--row-features", "rows.sdm", "--new-row-features", "new41.sdm"] + o, "has 41 feature columns, --row-features has 40"),
        (rows + ["--new-row-features", "new40.sdm"] + o, "both files must be of the same kind"),
        (["--row-features", "rows.sdm", "--new-row-features", "new3.ddm"] + o, "both files must be of the same kind"),
        (rows + ["--new-row-features", "new3.ddm"], "--new-row-features needs -o DIR"),
        (cols + ["--new-col-features", "new3.ddm"], "--new-col-features needs -o DIR"),
        (rows + ["--new-row-features", "new3.ddm", "-i", "4", "-b", "4"] + o, "needs at least one post-burn-in sample (-i > -b)"),
        (rows + ["--new-row-features", "new3.ddm", "-i", "3", "-b", "4"] + o, "needs at least one post-burn-in sample (-i > -b)"),
        (rows + ["--new-row-features", "bad.ddm"] + o, "holds a value that is not finite"),
        (["--row-features", "rows.sdm", "--new-row-features", "sbad.sdm"] + o, "holds a value that is not finite"),
        (rows + ["--new-row-features", "missing.ddm"] + o, "missing.ddm"),
        (wide_args + ["--row-features", "rows1.ddm", "--new-row-features", "huge.ddm"] + o, "more than 2^28 cells per file: ask for the best N of every query with --topn"),
        (rows + ["--new-row-features", "new3.ddm", "--probit"] + o, "do not go together with --probit"),      # what the features refuse
        (rows + ["--new-row-features", "new3.ddm", "-g", "2"] + o, "run on one GPU without -g"),
    ]
    for extra, msg in cases:
        r = run((data_args() if extra[:1] != ["-n"] else []) + extra, tmp_path)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr             # a one-line reason
        assert "num_latent" not in r.stdout
        assert not list(tmp_path.glob("new-*"))


def test_cli_usage_names_the_flags(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "--new-row-features FILE" in text and "--new-col-features FILE" in text and "new-rows-mean.ddm" in text


# ---- the reference --------------------------------------------------------------------------------------------------------------------

def test_reference_reproduces_the_hand_case():
    h = nr.hand_case()
    Es = np.stack([np.asarray(nr.project(h["F"], b, m)[0], float) for b, m in zip(h["betas"], h["mus"])])
    assert np.array_equal(Es, h["E"])
    w = nr.w_of(h["Vs"], h["Lambdas"])
    assert np.array_equal(np.asarray(w, float), h["w"])
    out = nr.predict(Es, np.stack(h["Vs"]), h["mean_rating"], w)
    assert out["mean"].shape == (6, 5)
    assert np.array_equal(np.asarray(out["mean"], float), h["mean"]) and np.array_equal(np.asarray(out["var"], float), h["var"])
    assert float(out["mean"][2, 2]) == 8.0 and float(out["var"][2, 2]) == 11.25          # the entry worked out in the docstring
    # one sample: no spread between the samples, w alone
    one = nr.predict(Es[:1], np.stack(h["Vs"])[:1], 3.0, nr.w_of(h["Vs"][:1], h["Lambdas"][:1]))
    assert np.array_equal(np.asarray(one["var"], float), np.arange(5.0) ** 2 + 1.0 + np.zeros((6, 1)))
    # sparse features project like dense ones; the top-N helper orders by (mean descending, id ascending) and pads with -1
    assert np.array_equal(np.asarray(nr.project(sp.csr_matrix(h["F"]), h["betas"][1], h["mus"][1])[0], float), h["E"][1])
    m = np.array([[1.0, 3.0, 3.0, 2.0]])
    assert nr.topn_of(m, 3).tolist() == [[1, 2, 3]] and nr.topn_of(m, 6).tolist() == [[1, 2, 3, 0, -1, -1]]
    # the dense naive form agrees where nothing cancels
    nm, nv = nr.predict_naive(Es, np.stack(h["Vs"]), 3.0)
    assert np.array_equal(nm, h["mean"]) and np.array_equal(nv + h["w"], h["var"])


def cancelling_case(nq, nc, K, S, seed):
    """p_s = P + delta_s with |delta_s| ~ 1e-7 |P|, carried by the factors themselves: e_s = (a_q, 1e-2 g_qs), v_s = (b_c, 1e-2 h_cs),
    a, b in [30, 31), g, h ~ N(0, 1)"""
    rng = np.random.default_rng(seed)
    Es = 1e-2 * rng.standard_normal((S, nq, K)); Vs = 1e-2 * rng.standard_normal((S, nc, K))
    Es[:, :, 0] = 30.0 + rng.random(nq); Vs[:, :, 0] = 30.0 + rng.random(nc)
    return Es, Vs


def test_naive_moments_cancel():
    Es, Vs = cancelling_case(9, 7, 8, 5, 3)
    good = nr.predict(Es, Vs, 0.0)
    P = np.asarray(good["mean"], float)
    spread = np.sqrt(np.asarray(good["var"], float))
    assert (np.abs(P) > 800).all() and (spread / np.abs(P) < 1e-6).all() and (spread / np.abs(P) > 1e-9).all()
    bound = np.asarray(nr.var_bound(good, 8), float)
    _, nv = nr.predict_naive(Es, Vs, 0.0)
    assert (np.abs(nv - np.asarray(good["var"], float)) > bound).any()       # the naive form breaks the bound on this input
    # Welford's update on the sum, in fp64 (what the kernel does), keeps it
    s = np.zeros_like(P); m2 = np.zeros_like(P)
    for i in range(5):
        p = Es[i] @ Vs[i].T
        d = p - s * (1.0 / i if i else 0.0)
        m2 += d * d * (i / (i + 1.0)); s += p
    assert (np.abs(m2 / 4.0 - np.asarray(good["var"], float)) <= bound).all()
