"""Sparse tensor factorisation, the part that needs no GPU:

  * tests/tensor_ref.py: the expanded-rows call on the unchanged oracle against the plain numpy statement of one row's conditional,
    every row of every mode of a 7 x 5 x 3 tensor at K = 8 and 10, to 1e-10 max|x|
  * FROSTT .tns files: the round trip (plain and .gz) and the refusals -- a 0-based index, a short line, a value that is not finite,
    a cell listed twice (named 1-based)
  * bpmf_hip_tensor_create: its refusals come before anything touches a device; without a device a context is BPMF_HIP_ENODEV
  * the `bpmf` flags: every refusal of --tensor, each with one line before a GPU is touched
  * the planted experiment on the reference alone: tensor chain < unfolded matrix < mean predictor on posterior-mean test RMSE
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bpmf_amd
from bpmf_amd import _lib
from bpmf_amd import io as bio
from tests import tensor_ref as ref
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")


# ---- 1. the reference against the definition ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [8, 10])
def test_expanded_rows_equal_the_plain_statement(oracle, K):
    dims = (7, 5, 3)
    rng = np.random.default_rng(70 + K)
    cells = rng.choice(7 * 5 * 3, size=60, replace=False)
    idx = np.stack(np.unravel_index(cells, dims), axis=1).astype(np.int32)
    vals = rng.integers(1, 6, len(idx)).astype(np.float64)
    mean, alpha, it = float(vals.mean()), 1.7, 3
    F = ref.factors(K, dims, 90 + K)
    worst = 0.0
    for m in range(3):
        assert (np.bincount(idx[:, m], minlength=dims[m]) > 0).all()
        mu, LU, LF = oracle.hyper_sample(K, dims[m], np.eye(K) * 0.2, it)
        got = [f.copy() for f in F]
        ref.sample_mode(oracle, K, idx, vals, dims, mean, alpha, got, m, it, mu, LF)
        for k in ref.others(m):
            assert np.array_equal(got[k], F[k])                      # only the mode's own factors move
        for c in range(dims[m]):
            want = ref.plain_row(oracle, K, idx.tolist(), vals, mean, alpha, F, m, c, it, mu, LF)
            err = np.abs(got[m][c] - want).max() / np.abs(want).max()
            worst = max(worst, err)
            assert err <= 1e-10, (m, c, err)
    print("K %d: expanded rows against the plain statement, worst %.3g of max|x|" % (K, worst))


# ---- 2. .tns files --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", [".tns", ".tns.gz"])
def test_tns_round_trip(tmp_path, ext):
    rng = np.random.default_rng(3)
    idx = np.stack(np.unravel_index(rng.choice(6 * 4 * 5, size=40, replace=False), (6, 4, 5)), axis=1).astype(np.int32)
    vals = rng.standard_normal(40) * 10.0 ** rng.integers(-8, 8, 40)
    path = tmp_path / ("a" + ext)
    bio.write_tns(path, idx, vals)
    i2, v2, dims = bpmf_amd.read_tns(path)
    assert np.array_equal(i2, idx) and i2.dtype == np.int32
    assert np.array_equal(v2, vals)                                  # %.17g: exact
    assert dims == tuple(int(x) + 1 for x in idx.max(axis=0))
    if ext == ".tns":
        first = open(path).readline().split()
        assert [int(x) for x in first[:3]] == [int(x) + 1 for x in idx[0]]      # 1-based on disk


def test_tns_comments_blank_lines_and_whitespace(tmp_path):
    p = tmp_path / "c.tns"
    p.write_text("# a FROSTT file\n\n1 2 3 4.5\n  2\t1   1  -1e-3\r\n# end\n")
    idx, vals, dims = bpmf_amd.read_tns(p)
    assert idx.tolist() == [[0, 1, 2], [1, 0, 0]] and vals.tolist() == [4.5, -1e-3] and dims == (2, 2, 3)
    p.write_text("# nothing\n")
    idx, vals, dims = bpmf_amd.read_tns(p)
    assert idx.shape == (0, 3) and len(vals) == 0 and dims == (0, 0, 0)


@pytest.mark.parametrize("text,what", [("1 1 1 2.0\n0 1 1 2.0\n", "line 2: index 0 in mode 1: the indices of a .tns file are 1-based"),
                                       ("1 1 2.0\n", "line 1: three indices and a value expected"),
                                       ("1 1 1\n", "line 1: three indices and a value expected"),
                                       ("1 1 1 nan\n", "line 1: the value is not finite"),
                                       ("1 1 1 inf\n", "line 1: the value is not finite"),
                                       ("1 1 1 1 2.0\n", "line 1: more than three indices"),
                                       ("1 2 3 1.0\n# c\n2 2 3 1.0\n1 2 3 4.0\n", "cell (1, 2, 3) is listed twice (lines 1 and 4)")])
def test_tns_refusals(tmp_path, text, what):
    p = tmp_path / "bad.tns"
    p.write_text(text)
    with pytest.raises(bio.BpmfIoError) as e:
        bpmf_amd.read_tns(p)
    assert what in str(e.value), str(e.value)


def test_tns_unknown_extension_and_missing_file(tmp_path):
    with pytest.raises(bio.BpmfIoError):
        bpmf_amd.read_tns(tmp_path / "a.mtx")
    with pytest.raises(bio.BpmfIoError) as e:
        bpmf_amd.read_tns(tmp_path / "nothing.tns")
    assert "not found" in str(e.value)


# ---- 3. bpmf_hip_tensor_create ---------------------------------------------------------------------------------------------------------

def _create(nmodes, dims, idx, vals, mean=0.0):
    lib = _lib.load_library()
    d = np.ascontiguousarray(dims, np.int64)
    idx = np.asarray(idx, np.int32).reshape(-1, 3)
    cols = [np.ascontiguousarray(idx[:, m]) if len(idx) else np.zeros(1, np.int32) for m in range(3)]
    v = np.ascontiguousarray(vals, np.float64) if len(idx) else np.zeros(1)
    h = C.c_void_p()
    rc = lib.bpmf_hip_tensor_create(None, nmodes, d.ctypes.data, len(idx), cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data,
                                    v.ctypes.data, mean, C.byref(h))
    assert not h.value
    return rc, lib.bpmf_hip_last_error().decode()


@pytest.mark.parametrize("nmodes,dims,idx,vals,what", [
    (2, (3, 3, 3), [[0, 0, 0]], [1.0], "2 modes given, tensors of order 3 only"),
    (4, (3, 3, 3), [[0, 0, 0]], [1.0], "4 modes given, tensors of order 3 only"),
    (3, (3, 0, 3), [[0, 0, 0]], [1.0], "mode 2 has size 0"),
    (3, (3, 3, 2 ** 31), [[0, 0, 0]], [1.0], "mode 3 has size 2147483648"),
    (3, (3, 3, 3), [[0, 0, 0], [1, 3, 0]], [1.0, 2.0], "entry 2 has index 4 in mode 2 of size 3"),
    (3, (3, 3, 3), [[0, 0, 0], [-1, 2, 0]], [1.0, 2.0], "entry 2 has index 0 in mode 1 of size 3"),
    (3, (3, 3, 3), [[0, 0, 0], [1, 2, 0]], [1.0, np.inf], "the value of entry 2 is not finite"),
    (3, (3, 3, 3), [[0, 1, 2], [2, 2, 2], [0, 1, 2]], [1.0, 2.0, 3.0], "cell (1, 2, 3) is listed twice (entries 1 and 3)"),
    (3, (3, 3, 3), [[0, 1, 2]], [1.0], "ctx is NULL")])
def test_tensor_create_refusals_come_before_the_device(nmodes, dims, idx, vals, what):
    rc, msg = _create(nmodes, dims, idx, vals)
    assert rc == -1 and msg.startswith("tensor_create: ") and what in msg, msg


def test_tensor_entry_points_refuse_null():
    lib = _lib.load_library()
    out = np.zeros(4)
    assert lib.bpmf_hip_tensor_sample(None, 0, 0, 2.0, None, None, None, None, None) == -1
    assert lib.bpmf_hip_tensor_product(None, 0, out.ctypes.data) == -1
    assert lib.bpmf_hip_tensor_side(None, 0) is None
    h = C.c_void_p()
    assert lib.bpmf_hip_tensor_test_create(None, 0, None, None, None, None, C.byref(h)) == -1 and not h.value
    assert lib.bpmf_hip_tensor_predict(None, 0, None, None, None) == -1
    assert lib.bpmf_hip_tensor_destroy(None) == 0 and lib.bpmf_hip_tensor_test_destroy(None) == 0


def test_no_device_is_enodev():
    """A tensor needs a context, and without a HIP device there is none: BPMF_HIP_ENODEV, never a CPU fallback."""
    try:
        eng = bpmf_amd.HipEngine(8)
    except bpmf_amd.BpmfHipError as e:
        assert e.code == -2
        return
    eng.close()


def test_tensor_gibbs_refuses_before_the_engine():
    class F32:
        dtype, K = "f32", 128
    with pytest.raises(ValueError):
        bpmf_amd.tensor_gibbs(F32(), np.zeros((1, 3), np.int32), np.ones(1), (2, 2, 2))


# ---- 4. the executable -----------------------------------------------------------------------------------------------------------------

def _files(tmp_path):
    idx, vals, tidx, tvals = ref.planted((6, 5, 4), 2, 0.5, 0.1, 1)
    bio.write_tns(tmp_path / "tr.tns", idx, vals)
    bio.write_tns(tmp_path / "te.tns", tidx, tvals)
    return str(tmp_path / "tr.tns"), str(tmp_path / "te.tns")


CLI_REFUSALS = [(["--fp32"], "--tensor does not go together with --fp32"),
                (["-g", "1"], "--tensor runs on one GPU without -g"),
                (["-g", "2"], "--tensor runs on one GPU without -g"),
                (["-m", "a.ddm,b.ddm"], "--tensor does not go together with a propagated posterior"),
                (["-l", "a.ddm,b.ddm"], "--tensor does not go together with a propagated posterior"),
                (["--probit"], "--tensor does not go together with --probit"),
                (["--censored", "c.sdm"], "--tensor does not go together with --censored"),
                (["--weights", "w.sdm"], "--tensor does not go together with --weights"),
                (["--robust", "4"], "--tensor does not go together with --robust"),
                (["--noise", "adaptive"], "--tensor does not go together with --noise adaptive"),
                (["--row-features", "f.ddm"], "--tensor does not go together with --row-features / --col-features"),
                (["--col-features", "f.ddm"], "--tensor does not go together with --row-features / --col-features"),
                (["-n", "m.mtx"], "--tensor takes the place of the matrix files"),
                (["-p", "m.mtx"], "--tensor takes the place of the matrix files"),
                (["--tensor-dims", "5,5,4"], "--tensor-dims 5,5,4: mode 1 has size 5, the files hold the index 6"),
                (["--tensor-dims", "6,5"], "--tensor-dims expects I,J,T"),
                (["-d", "129"], "unsupported number of latent dimensions 129")]


@pytest.mark.parametrize("extra,what", CLI_REFUSALS, ids=[" ".join(c[0]) for c in CLI_REFUSALS])
def test_cli_refusals(tmp_path, extra, what):
    tr, te = _files(tmp_path)
    r = subprocess.run([BPMF, "--tensor", tr, "--tensor-test", te] + extra, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("bpmf: ") and what in lines[0], r.stderr
    assert "HIP" not in r.stderr                                     # refused before a GPU is touched


def test_cli_reduce_environment_is_refused(tmp_path):
    tr, te = _files(tmp_path)
    r = subprocess.run([BPMF, "--tensor", tr], capture_output=True, text=True, cwd=tmp_path, env=dict(os.environ, BPMF_REDUCE="1"))
    assert r.returncode == 1 and r.stderr.strip() == "bpmf: --tensor does not go together with BPMF_REDUCE=1"


@pytest.mark.parametrize("flag", ["--tensor-test", "--tensor-dims"])
def test_cli_tensor_flags_need_tensor(tmp_path, flag):
    tr, te = _files(tmp_path)
    r = subprocess.run([BPMF, flag, te if flag == "--tensor-test" else "6,5,4"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and r.stderr.strip() == "bpmf: %s needs --tensor FILE.tns" % flag


def test_cli_bad_tensor_file_is_named(tmp_path):
    (tmp_path / "bad.tns").write_text("1 1 1 2.0\n1 1 1 3.0\n")
    r = subprocess.run([BPMF, "--tensor", "bad.tns"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "cell (1, 1, 1) is listed twice (lines 1 and 2)" in r.stderr


def test_cli_usage_names_the_tensor_flags(tmp_path):
    r = subprocess.run([BPMF, "-h"], capture_output=True, text=True, cwd=tmp_path)
    for flag in ("--tensor FILE.tns", "--tensor-test FILE.tns", "--tensor-dims I,J,T"):
        assert flag in r.stdout


# ---- 5. the model pays: the planted experiment on the reference ---------------------------------------------------------------------

def test_planted_tensor_beats_the_unfolded_matrix(oracle):
    """A planted rank-4 tensor, 60 x 40 x 8, a quarter of the cells observed with noise sd 0.3, K = 8, 60 iterations with 20 of
    burn-in; posterior-mean RMSE over the 960 held-out entries.  Measured: tensor chain 0.3252, unfolded
    users x (movie, time) matrix 0.5354, mean predictor 2.1675; the collapsed matrix (third index ignored) 2.5748.  Only the
    ordering is asserted."""
    tensor, unfolded, collapsed, mean = ref.planted_measure(oracle)
    print("planted: tensor %.4f, unfolded %.4f, collapsed %.4f, mean predictor %.4f" % (tensor, unfolded, collapsed, mean))
    assert tensor < unfolded < mean
