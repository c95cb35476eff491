"""Adaptive noise precision, CPU part: bpmf_hip_noise_sample is the Gamma draw of the oracle on the stream BPMF_NOISE_COUNTER(iter),
bit for bit; its argument checks; the `bpmf` flags --noise / --alpha-prior / --alpha-max are checked before anything touches a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bpmf_amd
from bpmf_amd import _lib
from bpmf_amd.engine import noise_sample
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
EINVAL = -1


def run(args, cwd):
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_noise_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    lib = _lib.load_library()
    sigs = _lib.exported_signatures()
    for name in ("bpmf_hip_train_sse", "bpmf_hip_noise_sample"):
        assert hasattr(raw, name) and name in sigs
        assert getattr(lib, name).argtypes == sigs[name][1]
    assert lib.bpmf_hip_abi_version() == 1
    assert lib.bpmf_hip_train_sse(None, None, None, None) == EINVAL


@pytest.mark.parametrize("a0,b0,sse,n,it", [(1.0, 1.0, 1000.0, 1000, 0), (1.0, 1.0, 45123.25, 900000, 7), (2.0, 0.5, 0.0, 1, 3),
                                            (0.5, 0.0, 3.5, 2, 1), (10.0, 100.0, 1e-3, 5, 19), (1.0, 1.0, 2.5e6, 10_000_000, 1000)])
def test_noise_sample_is_the_oracle_draw(oracle, a0, b0, sse, n, it):
    g, _ = oracle.gamma_stream(0xFFFFFFFF - it, [a0 + n / 2])
    want = g[0] / (b0 + sse / 2)
    got = noise_sample(a0, b0, sse, n, it)
    assert np.float64(got).tobytes() == np.float64(want).tobytes(), (got, want)
    assert noise_sample(a0, b0, sse, n, it, alpha_max=0.0) == got            # <= 0: no cap


def test_noise_sample_cap_and_errors():
    free = noise_sample(1.0, 1.0, 1000.0, 1000, 0)
    assert 0.5 < free < 2.0
    assert noise_sample(1.0, 1.0, 1000.0, 1000, 0, alpha_max=0.5) == 0.5
    assert noise_sample(1.0, 1.0, 1000.0, 1000, 0, alpha_max=10.0) == free
    lib = _lib.load_library()
    out = C.c_double()
    bad = [(0.0, 1.0, 1.0, 10, 0), (-1.0, 1.0, 1.0, 10, 0), (1.0, -0.5, 1.0, 10, 0), (1.0, 1.0, 1.0, 0, 0), (1.0, 1.0, 1.0, -3, 0),
           (1.0, 1.0, -1.0, 10, 0), (1.0, 1.0, float("nan"), 10, 0), (1.0, 1.0, float("inf"), 10, 0), (1.0, 1.0, 1.0, 10, -1),
           (1.0, 0.0, 0.0, 10, 0), (float("nan"), 1.0, 1.0, 10, 0)]
    for a0, b0, sse, n, it in bad:
        assert lib.bpmf_hip_noise_sample(a0, b0, sse, n, it, 0.0, C.byref(out)) == EINVAL, (a0, b0, sse, n, it)
        assert b"noise_sample" in lib.bpmf_hip_last_error()
    assert lib.bpmf_hip_noise_sample(1.0, 1.0, 1.0, 10, 0, 0.0, None) == EINVAL
    with pytest.raises(_lib.BpmfHipError):
        noise_sample(1.0, 1.0, -1.0, 10, 0)


def test_gibbs_refuses_bad_noise_arguments():
    with pytest.raises(ValueError, match="noise must be"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, noise="probit")
    with pytest.raises(ValueError, match="alpha_prior"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, noise="adaptive", alpha_prior=(0.0, 1.0))


def test_cli_refuses_adaptive_on_several_gpus(tmp_path):
    for g in ("2", "1"):
        r = run(data_args() + ["--noise", "adaptive", "-o", str(tmp_path), "-g", g], tmp_path)
        assert r.returncode != 0 and "--noise adaptive runs on one GPU" in r.stderr, g
        assert "num_latent" not in r.stdout                      # stopped before Sys::init printed anything
        assert not (tmp_path / "alpha.csv").exists() and not (tmp_path / "bpmf_0.out").exists()


def test_cli_noise_parsing(tmp_path):
    r = run(data_args() + ["--noise", "probit"], tmp_path)
    assert r.returncode != 0 and "--noise expects fixed or adaptive" in r.stderr
    for prior in ("1", "1,", ",1", "0,1", "-1,1", "1,-1", "a,b", "1,2,3", "nan,1"):
        r = run(data_args() + ["--noise", "adaptive", "--alpha-prior", prior], tmp_path)
        assert r.returncode != 0 and "--alpha-prior expects" in r.stderr, prior
    for cap in ("0", "-2", "x"):
        r = run(data_args() + ["--noise", "adaptive", "--alpha-max", cap], tmp_path)
        assert r.returncode != 0 and "--alpha-max expects" in r.stderr, cap
    for extra in (["--alpha-prior", "1,1"], ["--alpha-max", "3"], ["--noise", "fixed", "--alpha-max", "3"]):
        r = run(data_args() + extra, tmp_path)
        assert r.returncode != 0 and "need --noise adaptive" in r.stderr, extra
    r = run(data_args() + ["--noise", "adaptive", "-a", "0", "-g", "0"], tmp_path)
    assert r.returncode != 0 and "initial alpha" in r.stderr


def test_usage_names_the_noise_flags(tmp_path):
    r = run([], tmp_path)
    assert r.returncode != 0
    for flag in ("--noise fixed|adaptive", "--alpha-prior A0,B0", "--alpha-max F"):
        assert flag in r.stdout, flag
