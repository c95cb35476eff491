"""Side information: what can be checked without a GPU.

  * the new entry points are exported, bound, and the ABI version is unchanged
  * the extended hyper-parameter draw: (a) NULL scatter / 0 extra degrees of freedom are the bits of bpmf_hyper_sample, (b) with a
    scatter S and D extra degrees of freedom it is the oracle's draw for N + D points of covariance (N cov + S) / (N + D), with mu
    rescaled by sqrt((2 + N + D) / (2 + N)) -- the bound of tests/test_capi_host.py::test_hyper_sample_matches_oracle
  * the keyed normal stream of the link draw against its numpy restatement and against the oracle (tag 0: the oracle's stream)
  * argument refusals of every new entry point; BPMF_HIP_ENODEV, not a crash, where a device is needed and there is none
  * the `bpmf` flag refusals and the .ddm round trip of a feature file

Fails on the commit before the feature: every test but test_restated_keyed_block_is_the_oracles and test_feature_file_round_trip
(they pin pieces the feature builds on).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bpmf_amd
from bpmf_amd import _lib, engine
from tests import link_ref as ref
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
EINVAL, ENODEV = -1, -2

NEW = ("bpmf_hip_side_set_features", "bpmf_hip_link_sample", "bpmf_hip_side_link_get", "bpmf_hip_side_link_set", "bpmf_hip_side_link_add",
       "bpmf_hip_side_link_mean", "bpmf_hip_side_link_residual", "bpmf_hip_side_link_shift", "bpmf_hip_link_gemm_tn", "bpmf_hip_link_gemm_nn",
       "bpmf_hyper_sample_ex", "bpmf_hyper_draws_ex", "bpmf_hyper_finish_ex", "bpmf_randn_stream_tag")


def run(args, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([BPMF] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=e)


def data_args():
    return ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]


def test_link_symbols_exported_and_bound():
    raw = C.CDLL(bpmf_amd.library_path())
    sigs = _lib.exported_signatures()
    for name in NEW:
        assert hasattr(raw, name) and name in sigs, name
    assert _lib.load_library().bpmf_hip_abi_version() == 1
    for name in ("set_features", "link_sample", "link_get", "link_add", "link_mean"):
        assert callable(getattr(bpmf_amd.HipEngine, name))
    assert callable(bpmf_amd.hyper_sample)


def _spd(rng, K, scale=1.0):
    A = rng.standard_normal((K, 3 * K))
    return scale * (A @ A.T) / (3 * K)


@pytest.mark.parametrize("K", [8, 32, 64, 128])
def test_hyper_ex_without_extras_is_hyper_sample(K):
    rng = np.random.default_rng(K)
    cov = _spd(rng, K)
    for it, N in ((0, 50), (7, 1682)):
        a = bpmf_amd.hyper_sample(K, N, cov, it)
        b = bpmf_amd.hyper_sample(K, N, cov, it, extra_scatter=None, extra_dof=0)
        lib = _lib.load_library()
        mu = np.empty(K); LU = np.empty((K, K), order="F"); LF = np.empty((K, K), order="F")
        cm = np.asfortranarray(cov)
        _lib.check(lib.bpmf_hyper_sample_ex(K, N, cm.ctypes.data, None, None, 0, it, mu.ctypes.data, LU.ctypes.data, LF.ctypes.data))
        for x, y, z in zip(a, b, (mu, LU, LF)):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        # the two-step form
        au = np.empty((K, K), order="F"); z = np.empty(K); au0 = np.empty((K, K), order="F"); z0 = np.empty(K)
        _lib.check(lib.bpmf_hyper_draws_ex(K, N, 0, it, au.ctypes.data, z.ctypes.data))
        _lib.check(lib.bpmf_hyper_draws(K, N, it, au0.ctypes.data, z0.ctypes.data))
        assert np.array_equal(au, au0) and np.array_equal(z, z0)
        _lib.check(lib.bpmf_hyper_finish_ex(K, N, cm.ctypes.data, None, None, au.ctypes.data, z.ctypes.data, mu.ctypes.data, LU.ctypes.data, LF.ctypes.data))
        assert np.array_equal(mu, a[0]) and np.array_equal(LU, a[1]) and np.array_equal(LF, a[2])


@pytest.mark.parametrize("K", [8, 32, 64, 128])
def test_hyper_ex_matches_oracle(oracle, K):
    rng = np.random.default_rng(100 + K)
    for it, N, D in ((0, 50, 7), (3, 1682, 16), (11, 943, 1024)):
        cov = _spd(rng, K)
        S = _spd(rng, K, 5.0 * D)
        mu, LU, LF = bpmf_amd.hyper_sample(K, N, cov, it, extra_scatter=S, extra_dof=D)
        omu, oLU, oLF = oracle.hyper_sample(K, N + D, (N * cov + S) / (N + D), it)
        atol = 1e-12 * np.abs(oLF).max()
        assert np.allclose(LF, oLF, rtol=1e-10, atol=atol)
        assert np.allclose(LU, oLU, rtol=1e-10, atol=atol)
        assert np.allclose(mu, omu * np.sqrt((2.0 + N + D) / (2.0 + N)), rtol=1e-10, atol=1e-12)
        # the two-step form is the one-step form
        lib = _lib.load_library()
        au = np.empty((K, K), order="F"); z = np.empty(K)
        m2 = np.empty(K); U2 = np.empty((K, K), order="F"); F2 = np.empty((K, K), order="F")
        cm, sm = np.asfortranarray(cov), np.asfortranarray(S)
        _lib.check(lib.bpmf_hyper_draws_ex(K, N, D, it, au.ctypes.data, z.ctypes.data))
        _lib.check(lib.bpmf_hyper_finish_ex(K, N, cm.ctypes.data, None, sm.ctypes.data, au.ctypes.data, z.ctypes.data, m2.ctypes.data, U2.ctypes.data,
                                            F2.ctypes.data))
        assert np.array_equal(m2, mu) and np.array_equal(U2, LU) and np.array_equal(F2, LF)


def test_restated_keyed_block_is_the_oracles(oracle):
    rng = np.random.default_rng(19)
    for tag in (0, 3, 4):
        for c, n in zip(rng.integers(0, 2 ** 32, 16), rng.integers(0, 2 ** 20, 16)):
            w = ref.philox4x32_10(np.array([c]), 0, 0, np.array([n]), 42, tag)
            assert [int(x[0]) for x in w] == [int(x) for x in oracle.philox([c, 0, 0, n], [42, tag])]


def test_keyed_normal_stream(oracle):
    for c in (0, 1, 8, 2 ** 32 - 1):
        assert np.array_equal(ref.randn_tag(c, 0, 500), oracle.randn(c, 500))             # tag 0: the reference's stream
        assert np.array_equal(engine.randn_host(c, 500, tag=0), oracle.randn(c, 500))
        for tag in (ref.TAG_MOVIES, ref.TAG_USERS):
            got = engine.randn_host(c, 500, tag=tag)
            assert np.array_equal(got, ref.randn_tag(c, tag, 500))
            assert not np.array_equal(got, oracle.randn(c, 500))
    a, b = engine.randn_host(5, 4000, tag=3), engine.randn_host(5, 4000, tag=4)
    assert abs(a.mean()) < 0.1 and abs(a.std() - 1) < 0.05 and abs(np.corrcoef(a, b)[0, 1]) < 0.06


def test_null_arguments_are_refused():
    lib = _lib.load_library()
    one = np.zeros(4)
    p = one.ctypes.data
    d = C.c_double(); n = C.c_int()
    calls = [
        lambda: lib.bpmf_hip_side_set_features(None, p, 1, 1, 5.0, 3),
        lambda: lib.bpmf_hip_link_sample(None, None, 2.0),
        lambda: lib.bpmf_hip_side_link_get(None, p, p),
        lambda: lib.bpmf_hip_side_link_set(None, p),
        lambda: lib.bpmf_hip_side_link_add(None),
        lambda: lib.bpmf_hip_side_link_mean(None, p, C.byref(n)),
        lambda: lib.bpmf_hip_side_link_residual(None, None, p),
        lambda: lib.bpmf_hip_side_link_shift(None, C.byref(d)),
        lambda: lib.bpmf_hip_link_gemm_tn(0, None, 1, 1, p, 1, None, p),
        lambda: lib.bpmf_hip_link_gemm_tn(0, p, 0, 1, p, 1, None, p),
        lambda: lib.bpmf_hip_link_gemm_tn(0, p, 2, 2, p, 129, None, p),
        lambda: lib.bpmf_hip_link_gemm_tn(0, p, 2, 2, None, 1, None, p),
        lambda: lib.bpmf_hip_link_gemm_nn(0, p, 1, 1, None, 1, p),
        lambda: lib.bpmf_hip_link_gemm_nn(0, p, 1, 1, p, 129, p),
        lambda: lib.bpmf_hyper_sample_ex(0, 10, p, None, None, 0, 0, p, p, p),
        lambda: lib.bpmf_hyper_sample_ex(2, 10, p, None, None, -1, 0, p, p, p),
        lambda: lib.bpmf_hyper_sample_ex(2, 10, None, None, None, 0, 0, p, p, p),
        lambda: lib.bpmf_hyper_draws_ex(2, 10, -1, 0, p, p),
        lambda: lib.bpmf_hyper_draws_ex(2, 0, 0, 0, p, p),
        lambda: lib.bpmf_hyper_finish_ex(2, 10, p, None, None, None, p, p, p, p),
    ]
    for i, fn in enumerate(calls):
        assert fn() == EINVAL, i
        assert lib.bpmf_hip_last_error()


def test_products_need_a_device():
    """Without a HIP device the products report BPMF_HIP_ENODEV: no crash, no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    A = np.ones((4, 2))
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        engine.link_gemm_tn(A, np.ones((4, 3)))
    assert e.value.code == ENODEV
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        engine.link_gemm_nn(A, np.ones((2, 3)))
    assert e.value.code == ENODEV


def test_gibbs_refuses_what_does_not_go_with_features():
    F = np.zeros((1, 1))
    with pytest.raises(ValueError, match="pipelined=True"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, row_features=F, pipelined=True)
    with pytest.raises(ValueError, match="probit=True"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, col_features=F, probit=True)
    with pytest.raises(ValueError, match="noise='adaptive'"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, row_features=F, noise="adaptive")
    with pytest.raises(ValueError, match="lambda_beta"):
        bpmf_amd.gibbs(None, None, None, None, 1, 1, row_features=F, lambda_beta=0.0)


def test_feature_file_round_trip(tmp_path):
    from bpmf_amd import io
    F = ref.features(37, 5, 3)
    for name in ("f.ddm", "f.csv"):
        io.write_dense(tmp_path / name, F)
        back = io.read_dense(tmp_path / name)
        assert back.shape == F.shape
        # (.ddm is binary: bits; the .csv writer prints fewer digits than a double has)
        assert np.array_equal(back, F) if name.endswith(".ddm") else np.allclose(back, F, rtol=1e-5, atol=1e-8)


def test_cli_feature_refusals(tmp_path):
    from bpmf_amd import io
    nu, nm = util.tiny()[4:6]
    io.write_dense(tmp_path / "rows.ddm", ref.features(nu, 3, 1))
    io.write_dense(tmp_path / "cols.ddm", ref.features(nm, 3, 2))
    io.write_dense(tmp_path / "short.ddm", ref.features(nu - 1, 3, 1))
    io.write_dense(tmp_path / "mu.ddm", np.zeros((32, nm)))
    rows, cols = ["--row-features", "rows.ddm"], ["--col-features", "cols.ddm"]
    cases = [
        (rows + ["-g", "2"], None, "run on one GPU without -g"),
        (cols + ["-g", "1"], None, "run on one GPU without -g"),
        (rows + ["--probit"], None, "do not go together with --probit"),
        (rows + ["--noise", "adaptive"], None, "do not go together with --noise adaptive"),
        (cols + ["--fp32", "-d", "128"], None, "do not go together with --fp32"),
        (cols + ["-m", "mu.ddm,mu.ddm"], None, "do not go together with a propagated posterior"),
        (rows + ["-l", "mu.ddm,mu.ddm"], None, "do not go together with a propagated posterior"),
        (rows, {"BPMF_REDUCE": "1"}, "do not go together with BPMF_REDUCE=1"),
        (["--lambda-beta", "5"], None, "--lambda-beta needs --row-features or --col-features"),
        (rows + ["--lambda-beta", "0"], None, "--lambda-beta expects a number F > 0"),
        (rows + ["--lambda-beta", "x"], None, "--lambda-beta expects a number F > 0"),
        (rows + ["--lambda-beta", "inf"], None, "--lambda-beta expects a number F > 0"),
        (["--row-features", "short.ddm"], None, "rows, the side has"),
        (["--col-features", "rows.ddm"], None, "rows, the side has"),
        (["--row-features", "missing.ddm"], None, "missing.ddm"),
    ]
    for extra, env, msg in cases:
        r = run(data_args() + extra + ["-o", str(tmp_path)], tmp_path, env)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
        assert "num_latent" not in r.stdout                              # stopped before Sys::init printed anything
        assert not (tmp_path / "U-link.ddm").exists() and not (tmp_path / "V-link.ddm").exists()


def test_cli_usage_names_the_feature_flags(tmp_path):
    r = run(["-h"], tmp_path)
    text = r.stdout + r.stderr
    assert "--row-features FILE" in text and "--col-features FILE" in text and "--lambda-beta F" in text
    assert "not a tuned number" in text
