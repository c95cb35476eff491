"""Top-N by an acquisition score: what can be checked without a GPU.

  * bpmf_hip_topn_scored is exported and bound with its 14 arguments, the ABI version is unchanged
  * NULL sides at the C ABI
  * every refusal of `bpmf --topn-score / --topn-kappa / --topn-threshold`, each with its one-line reason, before a GPU is touched
    and without an output file; the usage text names the flags
  * gibbs()'s ValueErrors, before the engine is used
  * tests/topn_score_ref.py on a case small enough to work by hand

Fails on the commit before the feature: every test but test_reference_on_a_hand_case.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bpmf_amd
from bpmf_amd import _lib
from tests import topn_score_ref as tr
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
EINVAL = -1


def run(args, cwd):
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_symbol_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    sigs = _lib.exported_signatures()
    assert hasattr(raw, "bpmf_hip_topn_scored") and "bpmf_hip_topn_scored" in sigs
    restype, argtypes = sigs["bpmf_hip_topn_scored"]
    assert restype is C.c_int and len(argtypes) == 14
    assert argtypes[7] is C.c_int and argtypes[8] is C.c_double and argtypes[9] is C.c_double
    assert _lib.load_library().bpmf_hip_abi_version() == 1
    assert callable(bpmf_amd.HipEngine.topn_scored)
    assert bpmf_amd.HipEngine.SCORE_KINDS == {"ucb": 0, "prob": 1, "ei": 2}


def test_null_sides_are_refused():
    lib = _lib.load_library()
    out = np.zeros(4)
    idx = np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for kind in (0, 1, 2):
        assert lib.bpmf_hip_topn_scored(None, None, 0.0, 1, 0, 1, 1, kind, 0.0, 1.0, p(idx), p(out), p(out), p(out)) == EINVAL
        assert b"NULL side" in lib.bpmf_hip_last_error()


def test_gibbs_refusals():
    g = lambda **kw: bpmf_amd.gibbs(None, None, None, None, 3, 3, **kw)
    with pytest.raises(ValueError, match="topn_score needs topn"):
        g(topn_score=("ucb", 1.0))
    with pytest.raises(ValueError, match="unknown kind 'mean'"):
        g(topn=5, topn_score=("mean", 1.0))
    with pytest.raises(ValueError, match="pair"):
        g(topn=5, topn_score="ucb")
    with pytest.raises(ValueError, match="finite"):
        g(topn=5, topn_score=("prob", float("nan")))
    for kind in ("prob", "ei"):
        with pytest.raises(ValueError, match="noise='adaptive'"):
            g(topn=5, topn_score=(kind, 3.0), noise="adaptive")

    class Reached(Exception):
        pass

    class Engine:                                                           # stands where the engine does: any use of it says so
        def __getattr__(self, name):
            raise Reached(name)
    for kw in (dict(topn_score=("ucb", -1.0), noise="adaptive"), dict(topn_score=("prob", 3.0)), dict(topn_score=("ei", 3.0), probit=True)):
        with pytest.raises(Reached):                                        # valid arguments are refused by nothing before the engine is used
            bpmf_amd.gibbs(Engine(), np.zeros(2, np.int64), np.zeros(2, np.int64), None, 1, 1, topn=1, **kw)


def test_cli_refusals(tmp_path):
    from bpmf_amd import io
    nu = util.tiny()[4]
    io.write_dense(tmp_path / "rows.ddm", np.ones((nu, 2)))
    io.write_dense(tmp_path / "new.ddm", np.ones((3, 2)))
    o = ["-o", str(tmp_path)]
    top = ["--topn", "3"] + o
    cases = [
        (["--topn-score", "ucb"] + o, "--topn-score ucb needs --topn N"),
        (["--topn-score", "prob", "--topn-threshold", "3"] + o, "--topn-score prob needs --topn N"),
        (top + ["--topn-score", "best"], "--topn-score expects mean, ucb, prob or ei, not 'best'"),
        (top + ["--topn-score", "prob"], "--topn-score prob needs --topn-threshold F"),
        (top + ["--topn-score", "ei"], "--topn-score ei needs --topn-threshold F"),
        (top + ["--topn-score", "prob", "--topn-threshold", "nan"], "--topn-threshold expects a finite number, not 'nan'"),
        (top + ["--topn-score", "ei", "--topn-threshold", "inf"], "--topn-threshold expects a finite number, not 'inf'"),
        (top + ["--topn-score", "ei", "--topn-threshold", "3x"], "--topn-threshold expects a finite number, not '3x'"),
        (top + ["--topn-score", "ucb", "--topn-kappa", "nan"], "--topn-kappa expects a finite number, not 'nan'"),
        (top + ["--topn-score", "ucb", "--topn-kappa", ""], "--topn-kappa expects a finite number, not ''"),
        (top + ["--topn-kappa", "2"], "--topn-kappa goes with --topn-score ucb only"),
        (top + ["--topn-score", "prob", "--topn-threshold", "3", "--topn-kappa", "2"], "--topn-kappa goes with --topn-score ucb only"),
        (top + ["--topn-threshold", "3"], "--topn-threshold goes with --topn-score prob or ei only"),
        (top + ["--topn-score", "mean", "--topn-threshold", "3"], "--topn-threshold goes with --topn-score prob or ei only"),
        (top + ["--topn-score", "ucb", "--topn-threshold", "3"], "--topn-threshold goes with --topn-score prob or ei only"),
        (top + ["--topn-score", "prob", "--topn-threshold", "3", "--noise", "adaptive"], "--topn-score prob does not go together with --noise adaptive"),
        (top + ["--topn-score", "ei", "--topn-threshold", "3", "--noise", "adaptive"], "--topn-score ei does not go together with --noise adaptive"),
        (top + ["--topn-score", "ucb", "--row-features", "rows.ddm", "--new-row-features", "new.ddm"],
         "--topn-score ucb does not go together with --new-row-features / --new-col-features"),
        (top + ["--topn-score", "prob", "--topn-threshold", "3", "--col-features", "rows.ddm", "--new-col-features", "new.ddm"],
         "--topn-score prob does not go together with --new-row-features / --new-col-features"),
    ]
    for extra, msg in cases:
        r = run(data_args() + extra, tmp_path)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr             # a one-line reason
        assert "num_latent" not in r.stdout
        assert not list(tmp_path.glob("*.csv")) and not list(tmp_path.glob("U-*")), extra


def test_cli_usage_names_the_flags(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "--topn-score mean|ucb|prob|ei" in text and "--topn-kappa F" in text and "--topn-threshold F" in text
    assert "query,rank,candidate,score,mean,std" in text


# ---- the reference --------------------------------------------------------------------------------------------------------------------

def test_reference_on_a_hand_case():
    """one query, two candidates, S = 2, K = 1, mean_rating = 1: p(c = 0) = (1 + 1, 1 + 3) = (2, 4), p(c = 1) = (3, 3)"""
    from scipy.special import ndtr
    Es = np.array([[[1.0]], [[1.0]]]); Vs = np.array([[[1.0], [2.0]], [[3.0], [2.0]]])
    f = lambda kind, param, sigma=0.0: np.asarray(tr.reference(Es, Vs, 1.0, 4, kind, param, sigma)["score"], float)[0]
    assert f("ucb", 2.0).tolist() == [3.0 + 2.0 * np.sqrt(2.0), 3.0]
    assert f("ucb", -1.0).tolist() == [3.0 - np.sqrt(2.0), 3.0]
    assert f("prob", 3.0).tolist() == [0.5, 0.0]                               # p == t does not count: strict
    assert f("prob", 2.5).tolist() == [0.5, 1.0]
    assert f("ei", 3.0).tolist() == [0.5, 0.0] and f("ei", 1.0).tolist() == [2.0, 2.0]
    np.testing.assert_allclose(f("prob", 3.0, 1.0), [(ndtr(-1.0) + ndtr(1.0)) / 2, 0.5], rtol=1e-15)
    phi = lambda z: np.exp(-z * z / 2) / np.sqrt(2 * np.pi)
    np.testing.assert_allclose(f("ei", 3.0, 2.0), [(-ndtr(-0.5) + ndtr(0.5) + 4 * phi(0.5)) / 2, 2 * phi(0.0)], rtol=1e-15)
    # the exact restatement and the ranking helper: (score descending, id ascending), padding -1 / 0
    assert tr.exact_scores(Es, Vs, 1.0, "prob", 3.0).tolist() == [[0.5, 0.0]] and tr.exact_scores(Es, Vs, 1.0, "ei", 1.0).tolist() == [[2.0, 2.0]]
    idx, sc = tr.ranked(np.array([[1.0, 3.0, 3.0, 2.0]]), 3)
    assert idx.tolist() == [[1, 2, 3]] and sc.tolist() == [[3.0, 3.0, 2.0]]
    idx, sc = tr.ranked(np.array([[1.0, 3.0, 3.0, 2.0]]), 5, rated=[{2}])
    assert idx.tolist() == [[1, 3, 0, -1, -1]] and sc.tolist() == [[3.0, 2.0, 1.0, 0.0, 0.0]]
    # a device list that is right passes check_lists; one with a better candidate left out does not
    ref = dict(score=np.array([[1.0, 3.0, 3.0, 2.0]], tr.LD), bound=np.full((1, 4), 1e-15, tr.LD))
    tr.check_lists(np.array([[1, 2]], np.int32), np.array([[3.0, 3.0]]), ref, 2)
    with pytest.raises(AssertionError):
        tr.check_lists(np.array([[1, 3]], np.int32), np.array([[3.0, 2.0]]), ref, 2)
    with pytest.raises(AssertionError):
        tr.check_lists(np.array([[2, 1]], np.int32), np.array([[3.0, 3.0]]), ref, 2)
