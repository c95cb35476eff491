"""bpmf --similar: every refusal comes back in one line with a non-zero status before a GPU is touched, and so
do those of gibbs(similar=).  These fail on the commit before the feature (an unknown option prints the usage)."""
import os
import subprocess

import numpy as np
import pytest

import bpmf_amd
from tests import model_ref as mr
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")


def refused(args, reason, cwd, env=None):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 1 and p.stdout == "", (args, p.stdout, p.stderr)
    lines = p.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("bpmf: ") and reason in lines[0], (args, p.stderr)


def test_similar_refusals(tmp_path):
    files = ["-n", "train.sdm", "-p", "test.sdm"]
    base = files + ["--similar", 5, "-o", "out"]
    refused(base + ["-g", 1], "--similar runs on one GPU without -g", tmp_path)
    refused(base + ["-g", 2], "--similar runs on one GPU without -g", tmp_path)
    refused(["--tensor", "x.tns", "--similar", 5, "-o", "out"], "--similar does not go together with --tensor", tmp_path)
    refused(base, "--similar does not go together with BPMF_REDUCE=1", tmp_path, {"BPMF_REDUCE": "1"})
    refused(base + ["-m", "a.ddm,b.ddm"], "--similar does not go together with a propagated posterior (-m / -l)", tmp_path)
    refused(base + ["-l", "a.ddm,b.ddm"], "--similar does not go together with a propagated posterior (-m / -l)", tmp_path)
    refused(files + ["--similar", 5], "--similar needs -o DIR", tmp_path)
    refused(base + ["-i", 5, "-b", 5], "--similar needs at least one post-burn-in sample (-i > -b)", tmp_path)
    refused(base + ["-i", 3, "-b", 5], "--similar needs at least one post-burn-in sample (-i > -b)", tmp_path)
    for n in (0, 33, -1, "ten", "5x"):
        refused(files + ["--similar", n, "-o", "out"], "--similar expects 1 <= N <= 32", tmp_path)
    refused(base + ["--similar-kind", "pearson"], "--similar-kind expects cosine or euclid, not 'pearson'", tmp_path)
    refused(base + ["--similar-by", "items"], "--similar-by expects cols or rows, not 'items'", tmp_path)
    for kappa in (-0.5, "nan", "inf", "-inf", "much", ""):
        refused(base + ["--similar-kappa", kappa], "--similar-kappa expects a finite number >= 0", tmp_path)
    for m in (-1, "few", 1.5):
        refused(base + ["--similar-min-ratings", m], "--similar-min-ratings expects an integer >= 0", tmp_path)
    for flag, arg in (("--similar-by", "rows"), ("--similar-kind", "euclid"), ("--similar-kappa", 1), ("--similar-min-ratings", 3)):
        refused(files + [flag, arg, "-o", "out"], flag + " needs --similar N", tmp_path)
    assert not os.path.exists(tmp_path / "out")


def test_similar_refusals_with_a_model(tmp_path):
    bpmf_amd.write_model(tmp_path / "model", mr.random_model(3, 4, 5, 2, 1))
    base = ["--model", "model", "--similar", 3]
    refused(base, "--similar needs -o DIR", tmp_path)
    refused(base + ["-o", "out", "--similar-min-ratings", 2], "--similar-min-ratings with --model needs -n TRAIN", tmp_path)
    refused(base + ["-o", "out", "-i", 9], "--model does not go together with -i", tmp_path)
    refused(base + ["-o", "out", "-g", 1], "--similar runs on one GPU without -g", tmp_path)
    refused(["--model", "model", "--similar-kappa", 1, "-o", "out"], "--similar-kappa needs --similar N", tmp_path)


def test_gibbs_similar_refusals():
    M = (np.array([0, 1, 2], np.int64), np.array([0, 1], np.int32), np.array([1.0, 2.0]))
    for kw, what in ((dict(similar=0), "similar = 0"), (dict(similar=33), "similar = 33"), (dict(similar=2.5), "similar = 2.5"),
                     (dict(similar=3, similar_by="items"), "similar_by must be 'cols' or 'rows'"),
                     (dict(similar=3, similar_kind="pearson"), "similar_kind must be 'cosine' or 'euclid'"),
                     (dict(similar=3, similar_kappa=-1.0), "similar_kappa = -1.0 must be finite and >= 0"),
                     (dict(similar=3, similar_kappa=float("nan")), "similar_kappa = nan must be finite and >= 0"),
                     (dict(similar=3, similar_min_ratings=-2), "similar_min_ratings = -2 must be an integer >= 0"),
                     (dict(similar=3, nsims=4, burnin=4), "similar needs at least one post-burn-in sample")):
        with pytest.raises(ValueError) as e:
            bpmf_amd.gibbs(None, M, M, None, 2, 2, **kw)
        assert what in str(e.value), (kw, str(e.value))


def test_library_exports_the_symbols():
    from bpmf_amd import _lib
    lib = _lib.load_library()
    for name in ("bpmf_hip_similar", "bpmf_hip_similar_block", "bpmf_hip_similar_last_ms"):
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None
    for name in ("similar", "similar_block", "similar_last_ms"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
