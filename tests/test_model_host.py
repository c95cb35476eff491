"""Saved models without a GPU: the format through the Python writer and reader, every refusal of the reader, the
committed model tests/golden/model_v1 that pins format version 1, and every refusal of `bpmf --save-model` / `bpmf --model` and of
gibbs(save_model=), each by its one-line reason (they come before a GPU is touched).

Every test of this file fails on the commit before the feature (missing entry points / flags).
"""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import bpmf_amd
from bpmf_amd import _lib
from bpmf_amd import io as bio
from bpmf_amd.io import BpmfIoError
from tests import model_ref as mr
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
GOLDEN = os.path.join(ROOT, "tests", "golden", "model_v1")
FILES = ["U-hyper.ddm", "U-samples.ddm", "V-hyper.ddm", "V-samples.ddm", "model.txt"]


def same_model(a, b):
    for key in ("num_latent", "rows", "cols", "samples", "mean_rating", "alpha", "probit", "probit_threshold", "dtype"):
        assert a[key] == b[key], key
    for key in ("U", "V"):
        assert a[key].shape == b[key].shape and a[key].tobytes() == np.ascontiguousarray(b[key], np.float64).tobytes(), key
    for key in ("U_hyper", "V_hyper"):
        assert (a[key] is None) == (b[key] is None), key
        if a[key] is not None:
            for x, y in zip(a[key], b[key]):
                assert x.shape == np.shape(y) and x.tobytes() == np.ascontiguousarray(y, np.float64).tobytes(), key


# ---- the format ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,rows,cols,S,hyper,probit", [(1, 3, 2, 1, True, False), (3, 4, 5, 2, True, False), (8, 7, 9, 3, False, True),
                                                       (10, 5, 1, 4, True, False), (32, 2, 3, 2, False, False)])
def test_round_trip(tmp_path, K, rows, cols, S, hyper, probit):
    m = mr.random_model(K, rows, cols, S, 7 * K + S, hyper, probit)
    m["mean_rating"] = 0.1 + 1.0 / 3.0 if not probit else 0.0               # not a short decimal: %.17g must bring it back
    m["dtype"] = "f32" if K == 32 else "f64"
    d = tmp_path / "m"
    bpmf_amd.write_model(d, m)
    assert sorted(os.listdir(d)) == (FILES if hyper else ["U-samples.ddm", "V-samples.ddm", "model.txt"])
    same_model(bpmf_amd.read_model(d), m)
    lines = (d / "model.txt").read_text().splitlines()
    assert lines[0] == "bpmf_model 1" and [ln.split(" ")[0] for ln in lines[1:]] == [
        "num_latent", "rows", "cols", "samples", "mean_rating", "alpha", "likelihood", "probit_threshold", "dtype", "hyper"]
    assert lines[7] == ("likelihood probit" if probit else "likelihood gaussian") and lines[10] == "hyper %d" % hyper
    # the matrices are what the .ddm reader gives: (S K) x rows with sample s of column c at rows s K .. s K + K - 1
    U = bio.read_dense(d / "U-samples.ddm")
    assert U.shape == (S * K, rows) and np.array_equal(U[:, rows - 1].reshape(S, K), m["U"][rows - 1])
    if hyper:
        H = bio.read_dense(d / "V-hyper.ddm")
        alpha, mu, lam = m["V_hyper"]
        assert H.shape == (1 + K + K * K, S) and np.array_equal(H[0], alpha) and np.array_equal(H[1:1 + K].T, mu)
        assert np.array_equal(H[1 + K:, S - 1].reshape(K, K).T, lam[S - 1])                     # column-major, as hyper_get gives it
    bpmf_amd.write_model(tmp_path / "again", bpmf_amd.read_model(d))
    for name in os.listdir(d):
        assert (d / name).read_bytes() == (tmp_path / "again" / name).read_bytes(), name


def test_writer_refusals(tmp_path):
    m = mr.random_model(3, 4, 5, 2, 1)
    bad = dict(m, U=m["U"][:, :1])
    with pytest.raises(ValueError, match="U must be"):
        bpmf_amd.write_model(tmp_path / "m", bad)
    with pytest.raises(ValueError, match="together"):
        bpmf_amd.write_model(tmp_path / "m", dict(m, V_hyper=None))
    bad = dict(m, V=m["V"].copy()); bad["V"][2, 1, 0] = np.inf
    with pytest.raises(BpmfIoError, match="not finite"):
        bpmf_amd.write_model(tmp_path / "m", bad)


def refusal(d, match):
    with pytest.raises(BpmfIoError, match=match) as e:
        bpmf_amd.read_model(d)
    assert "\n" not in str(e.value)
    return str(e.value)


def test_reader_refusals(tmp_path):
    K, rows, cols, S = 3, 4, 5, 2
    good = tmp_path / "good"
    bpmf_amd.write_model(good, mr.random_model(K, rows, cols, S, 2))
    txt = (good / "model.txt").read_text()

    def variant(name):
        d = tmp_path / name
        shutil.copytree(good, d)
        return d
    # an unknown version, a first line of another kind
    d = variant("version"); (d / "model.txt").write_text(txt.replace("bpmf_model 1", "bpmf_model 2"))
    assert "model.txt" in refusal(d, "unknown format version '2'")
    d = variant("other"); (d / "model.txt").write_text(txt.replace("bpmf_model 1\n", ""))
    refusal(d, "model.txt: not a saved model")
    d = variant("key"); (d / "model.txt").write_text(txt.replace("alpha 2\n", ""))
    refusal(d, "model.txt: the key 'alpha' is missing")
    # a missing file, each of the five
    for name in FILES:
        d = variant("missing-" + name); os.remove(d / name)
        assert name in refusal(d, "not found")
    refusal(tmp_path / "nowhere", "model.txt' not found")
    # a row count that is not S K
    d = variant("rows"); bio.write_dense(d / "U-samples.ddm", np.zeros((S * K + 1, rows)))
    refusal(d, r"U-samples.ddm: 7 rows are not samples x num_latent")
    d = variant("hrows"); bio.write_dense(d / "U-hyper.ddm", np.zeros((K + K * K, S)))
    refusal(d, r"U-hyper.ddm: 12 rows, not 1 \+ num_latent \+ num_latent\^2 = 13")
    d = variant("cols"); bio.write_dense(d / "V-samples.ddm", np.zeros((S * K, cols + 1)))
    refusal(d, r"V-samples.ddm: 6 columns, .*model.txt says 5")
    # unequal S between the files
    d = variant("s-samples"); bio.write_dense(d / "V-samples.ddm", np.zeros(((S + 1) * K, cols)))
    refusal(d, r"V-samples.ddm: holds 3 samples, .*model.txt says 2")
    d = variant("s-hyper"); bio.write_dense(d / "V-hyper.ddm", np.ones((1 + K + K * K, S - 1)))
    refusal(d, r"V-hyper.ddm: holds 1 samples, .*model.txt says 2")
    d = variant("s-txt"); (d / "model.txt").write_text(txt.replace("samples 2", "samples 3"))
    refusal(d, r"U-samples.ddm: holds 2 samples, .*model.txt says 3")
    # a value that is not finite
    for name, shape in (("U-samples.ddm", (S * K, rows)), ("V-hyper.ddm", (1 + K + K * K, S))):
        for v in (np.nan, -np.inf):
            A = np.ones(shape); A[2, 1] = v
            d = variant("nan-%s-%s" % (name, v)); bio.write_dense(d / name, A)
            refusal(d, name + ": the value of row 3, column 2 is not finite")
    d = variant("nan-txt"); (d / "model.txt").write_text(txt.replace("mean_rating 3.25", "mean_rating nan"))
    refusal(d, "model.txt: the value of mean_rating is not finite")
    d = variant("short"); (d / "V-samples.ddm").write_bytes((d / "V-samples.ddm").read_bytes()[:-8])
    refusal(d, "V-samples.ddm: unexpected end of file")
    same_model(bpmf_amd.read_model(good), mr.random_model(K, rows, cols, S, 2))


def test_golden_model_pins_version_1(tmp_path):
    """tests/golden/model_v1 was written once by bpmf_amd.write_model(model_ref.golden_model()); it reads back to the numbers stated
    there, and writing them again gives the committed bytes"""
    assert sorted(os.listdir(GOLDEN)) == FILES
    with open(os.path.join(GOLDEN, "model.txt")) as f:
        assert f.read() == mr.GOLDEN_TXT
    want = mr.golden_model()
    got = bpmf_amd.read_model(GOLDEN)
    same_model(got, want)
    assert got["U"][2, 1, 1] == 3.75 and got["V"][4, 0, 2] == -1.625 and got["V_hyper"][2][1, 0, 2] == 1.125 and got["U_hyper"][0][1] == 2.5
    bpmf_amd.write_model(tmp_path / "m", want)
    for name in FILES:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            assert f.read() == (tmp_path / "m" / name).read_bytes(), name
    # the layout of the .ddm files, stated without the reader: two uint64 (rows, columns), then the columns
    raw = np.fromfile(os.path.join(GOLDEN, "U-samples.ddm"), np.uint8)
    assert raw[:16].view(np.uint64).tolist() == [6, 4] and np.array_equal(raw[16:].view(np.float64), want["U"].ravel())


# ---- the interfaces --------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_symbols():
    lib = _lib.load_library()
    for name in ("bpmf_hip_side_samples_get", "bpmf_hip_side_samples_set", "bpmf_hip_predict_cells", "bpmf_hip_predict_cells_last_ms",
                 "bpmf_io_write_model", "bpmf_io_read_model"):
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None
    for name in ("samples_get", "samples_set", "predict_cells"):
        assert callable(getattr(bpmf_amd.HipEngine, name))


def test_python_refusals(tmp_path):
    M = (np.array([0, 1, 2], np.int64), np.array([0, 1], np.int32), np.array([1.0, 2.0]))
    for kw, what in ((dict(ordinal=True), "ordinal"), (dict(implicit=0.5), "implicit"), (dict(row_features=np.ones((2, 1))), "row_features"),
                     (dict(col_features=np.ones((2, 1))), "row_features / col_features")):
        with pytest.raises(ValueError, match="save_model does not go together with " + what):
            bpmf_amd.gibbs(None, M, M, None, 2, 2, save_model=str(tmp_path / "m"), **kw)
    with pytest.raises(ValueError, match="save_model needs at least one post-burn-in sample"):
        bpmf_amd.gibbs(None, M, M, None, 2, 2, nsims=3, burnin=3, save_model=str(tmp_path / "m"))
    bpmf_amd.write_model(tmp_path / "m", mr.random_model(3, 4, 5, 2, 1))
    with pytest.raises(ValueError, match="the engine has num_latent 8, the model 3"):
        bpmf_amd.load_model(types.SimpleNamespace(K=8), tmp_path / "m")
    with pytest.raises(ValueError, match="does not have the model's shape 4 x 5"):
        bpmf_amd.load_model(types.SimpleNamespace(K=3), tmp_path / "m", M)
    with pytest.raises(ValueError, match="save_model needs the result of gibbs"):
        bpmf_amd.save_model({}, tmp_path / "x")
    assert not os.path.exists(tmp_path / "x")


# ---- the executable: every refusal comes before a GPU is touched ---------------------------------------------------------------------------

def refused(args, reason, cwd, env=None):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 1 and p.stdout == "", (args, p.stdout, p.stderr)
    lines = p.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("bpmf: ") and reason in lines[0], (args, p.stderr)


def test_save_model_refusals(tmp_path):
    base = ["-n", "train.sdm", "-p", "test.sdm", "--save-model", "model"]
    refused(base + ["-i", 5, "-b", 5], "--save-model needs at least one post-burn-in sample (-i > -b)", tmp_path)
    refused(base + ["-g", 1], "--save-model runs on one GPU without -g", tmp_path)
    refused(base + ["-g", 2], "--save-model runs on one GPU without -g", tmp_path)
    refused(base, "--save-model does not go together with BPMF_REDUCE=1", tmp_path, {"BPMF_REDUCE": "1"})
    refused(["--tensor", "x.tns", "--save-model", "model"], "--save-model does not go together with --tensor", tmp_path)
    refused(base + ["--ordinal"], "--save-model does not go together with --ordinal", tmp_path)
    refused(base + ["--implicit", 0.1], "--save-model does not go together with --implicit", tmp_path)
    refused(base + ["--row-features", "f.ddm"], "--save-model does not go together with --row-features / --col-features", tmp_path)
    refused(base + ["--col-features", "f.sdm"], "--save-model does not go together with --row-features / --col-features", tmp_path)
    refused(base + ["-m", "a.ddm,b.ddm"], "--save-model does not go together with a propagated posterior (-m / -l)", tmp_path)
    refused(base + ["-l", "a.ddm,b.ddm"], "--save-model does not go together with a propagated posterior (-m / -l)", tmp_path)
    assert not os.path.exists(tmp_path / "model")


def test_model_refusals(tmp_path):
    bpmf_amd.write_model(tmp_path / "model", mr.random_model(3, 4, 5, 2, 1))
    bpmf_amd.write_model(tmp_path / "nohyper", mr.random_model(3, 4, 5, 2, 1, hyper=False))
    bpmf_amd.write_model(tmp_path / "probit", mr.random_model(3, 4, 5, 2, 1, hyper=False, probit=True))
    base = ["--model", "model", "--predict", "cells.sdm", "-o", "out"]
    for flag, arg in (("-i", 10), ("-b", 2)):
        refused(base + [flag, arg], "--model does not go together with %s (no chain runs)" % flag, tmp_path)
    refused(base + ["-a", 2.0], "--model does not go together with -a", tmp_path)
    refused(base + ["-g", 1], "--model runs on one GPU without -g", tmp_path)
    refused(base + ["--save-model", "other"], "--model does not go together with --save-model", tmp_path)
    for flags in (["--probit"], ["--probit-threshold", 1], ["--ordinal"], ["--ordinal-levels", "1,2"], ["--implicit", 0.1], ["--robust", 4],
                  ["--censored", "c.sdm"], ["--weights", "w.sdm"], ["--noise", "adaptive"], ["--alpha-prior", "1,1"], ["--alpha-max", 9],
                  ["--row-features", "f.ddm"], ["--col-features", "f.ddm"], ["--new-row-features", "f.ddm"], ["--lambda-beta", 5],
                  ["--lambda-beta-prior", "1,1"], ["--link-tol", 0.1], ["--tensor", "x.tns"], ["--fp32"], ["-m", "a,b"], ["-l", "a,b"], ["-v"], ["-k"],
                  ["-f", 2]):
        refused(base + flags, "--model does not go together with %s (no chain runs" % flags[0], tmp_path)
    refused(base, "--model does not go together with BPMF_REDUCE=1", tmp_path, {"BPMF_REDUCE": "1"})
    refused(base + ["-d", 8], "-d 8 differs from the num_latent 3 of the model model", tmp_path)
    refused(["--model", "model", "--topn", 3, "-o", "out"], "--topn with --model needs -n TRAIN", tmp_path)
    refused(["--model", "model", "--rank-eval", 3, "-p", "test.sdm", "-o", "out"], "--rank-eval with --model needs -n TRAIN", tmp_path)
    refused(["--model", "model", "--rank-eval", 3, "-n", "train.sdm", "-o", "out"], "--rank-eval with --model needs -p TEST", tmp_path)
    refused(["--model", "nohyper", "--fold-in-rows", "new.sdm", "-o", "out"], "--fold-in-rows: nohyper was saved without hyper files", tmp_path)
    refused(["--model", "nohyper", "--fold-in-cols", "new.sdm", "-o", "out"], "--fold-in-cols: nohyper was saved without hyper files", tmp_path)
    refused(["--model", "probit", "--fold-in-rows", "new.sdm", "-o", "out"], "--fold-in-rows: probit is a probit model, which is saved without hyper files",
            tmp_path)
    refused(["--predict", "cells.sdm", "-o", "out"], "--predict needs --model DIR", tmp_path)
    refused(["--model", "model", "--predict-threshold", 3, "--topn", 3, "-n", "train.sdm", "-o", "out"], "--predict-threshold needs --predict FILE", tmp_path)
    refused(base + ["--predict-threshold", "high"], "--predict-threshold expects a finite number", tmp_path)
    refused(["--model", "model", "-o", "out"], "--model: nothing to do", tmp_path)
    refused(["--model", "model", "--predict", "cells.sdm"], "--model needs -o DIR", tmp_path)
    refused(["--model", "absent", "--predict", "cells.sdm", "-o", "out"], "absent/model.txt' not found", tmp_path)
    os.remove(tmp_path / "nohyper" / "V-samples.ddm")
    refused(["--model", "nohyper", "--predict", "cells.sdm", "-o", "out"], "nohyper/V-samples.ddm' not found", tmp_path)
