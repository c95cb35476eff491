"""Posterior top-N ranking, CPU part: the four entry points are exported and bound, and the `bpmf` flags
--topn / --topn-by are checked before anything touches a GPU."""
import ctypes as C
import os
import subprocess

import bpmf_amd
from bpmf_amd import _lib
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
NEW = ("bpmf_hip_side_samples_reserve", "bpmf_hip_side_samples_add", "bpmf_hip_side_samples_count", "bpmf_hip_topn")


def run(args, cwd):
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_topn_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    lib = _lib.load_library()
    sigs = _lib.exported_signatures()
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in sigs
        assert getattr(lib, name).argtypes == sigs[name][1]
    assert sigs["bpmf_hip_topn"][0] is C.c_int and len(sigs["bpmf_hip_topn"][1]) == 10
    assert lib.bpmf_hip_abi_version() == 1
    assert lib.bpmf_hip_side_samples_count(None) == 0


def test_topn_needs_output_dir(tmp_path):
    r = run(data_args() + ["--topn", "5"], tmp_path)
    assert r.returncode != 0 and "--topn needs -o DIR" in r.stderr
    assert not (tmp_path / "topn.csv").exists()


def test_topn_refuses_several_gpus(tmp_path):
    r = run(data_args() + ["--topn", "5", "-o", str(tmp_path), "-g", "2"], tmp_path)
    assert r.returncode != 0 and "--topn runs on one GPU" in r.stderr
    assert "num_latent" not in r.stdout                       # stopped before Sys::init printed anything
    assert not (tmp_path / "topn.csv").exists() and not (tmp_path / "bpmf_0.out").exists()


def test_topn_by_parsing(tmp_path):
    for by in ("rows", "cols"):                              # accepted: the run then stops at the missing -o
        r = run(data_args() + ["--topn", "3", "--topn-by", by], tmp_path)
        assert r.returncode != 0 and "--topn needs -o DIR" in r.stderr, by
    r = run(data_args() + ["--topn", "3", "--topn-by", "users", "-o", str(tmp_path)], tmp_path)
    assert r.returncode != 0 and "--topn-by expects rows or cols" in r.stderr
    r = run(data_args() + ["--topn", "0", "-o", str(tmp_path)], tmp_path)
    assert r.returncode != 0 and "--topn expects N >= 1" in r.stderr
    r = run(data_args() + ["--topn", "3", "-o", str(tmp_path), "-i", "4", "-b", "4"], tmp_path)
    assert r.returncode != 0 and "post-burn-in sample" in r.stderr


def test_usage_names_the_flags(tmp_path):
    r = run([], tmp_path)
    assert r.returncode != 0 and "--topn N" in r.stdout and "--topn-by rows|cols" in r.stdout
