"""Per-rating precision weights (`gibbs(..., weights=W)`, `bpmf --weights FILE`) on the GPU.

  * one half-iteration through the weighted form of each sampler family against the expanded-rows reference of tests/weights_ref.py:
    K = 8 (BPMF_HIP_MODE 1 and 3), 10, 32, 64, 100, 128 on the edge side (rating counts on both sides of 4, 16, 64; at
    BPMF_HIP_CHUNK=16 and at the automatic chunk) and on ml-100k; K = 64 also on the product-form side, where no k_sample_pf runs
  * weights that are all 1 give the plain side's factors and statistics bit for bit in every family; two launches are bit-equal;
    replacing seeded weights by ones returns to the plain bits; weights_get is numpy's sqrt(w) and sqrt(w) (r - mean) bit for bit
  * a constant weight c at alpha against the plain side at alpha c, GPU against GPU
  * the coupled chain against the restated chain (K = 32, 64; pipelined and plain loop; BPMF_HIP_FUSED=0 with topn once)
  * arguments, mutual refusals in both orders, the caller's arrays, device memory
  * a planted heteroscedastic experiment in which honouring the weights beats the best single alpha
  * `bpmf --weights` end to end, with a renumbering that moves the weighted columns, and a run without the flag
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import util
from tests import weights_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_parity import RTOL, rel_err
from tests.test_gpu_probit import _from_device, _hip_runtime, _product_form_side, _to_device, _write_mtx

pytestmark = pytest.mark.gpu

EINVAL = -1
ALPHA = 1.7                 # not a power of two
STAT_TOL = 1e-8


class _env:
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _pair(eng, A, nrows, X, Y, w, mean=None):
    """A side over the ratings A (weighted by w; None: no weights) holding the factors X, and a partner without ratings holding Y."""
    ncols = len(A[0]) - 1
    me = eng.side_create(ncols, nrows, *A, util.mean_rating(A) if mean is None else mean)
    ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    if w is not None:
        eng.set_weights(me, w)
    eng.set_items(me, X)
    eng.set_items(ot, Y)
    return me, ot


def _factors(K, ncols, nrows, seed):
    rng = np.random.default_rng(seed)
    sigma = (2.0 / K) ** 0.25
    return sigma * rng.standard_normal((ncols, K)), sigma * rng.standard_normal((nrows, K))


# (id, num_latent, environment, the kernel a weighted side names, the environment of the plain side of the bit test)
FAMILIES = [("k8-mode1", 8, {"BPMF_HIP_MODE": 1}, r"^k_sample1w<8>$", {"BPMF_HIP_MODE": 1}),
            ("k8-mode3", 8, {"BPMF_HIP_MODE": 3}, r"^k_sample4w<8>$", {"BPMF_HIP_MODE": 3}),
            ("k10", 10, {}, r"^k_sample1w<16>$", {}),
            ("k32", 32, {}, r"^k_sample1w<32>$", {}),
            ("k64", 64, {}, r"^k_sample(1s|_slab)w<64>$", {"BPMF_HIP_PF": 0}),
            ("k100", 100, {}, r"^k_sample_wg2w<128,4,double>$", {}),
            ("k128", 128, {}, r"^k_sample_wg2w<128,4,double>$", {})]


def _half_iteration(oracle, eng, K, A, nrows, w, it, expect_kernel, seed):
    """one weighted half-iteration against the reference at the bars of test_gpu_censored._half_iteration; -> schedule_info"""
    ncols, mean = len(A[0]) - 1, util.mean_rating(A)
    X, Y = _factors(K, ncols, nrows, seed)
    me, ot = _pair(eng, A, nrows, X, Y, w)
    assert re.search(expect_kernel, eng.kernel_name(me)), eng.kernel_name(me)
    info = eng.schedule_info(me)
    res = eng.kernel_resources(me)
    assert len(res) >= 1 and all("w<" in r["kernel"] for r in res), res
    mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, it)
    want = X.copy()
    s_ref, p_ref, n_ref = ref.sample_side_weighted(oracle, K, A, w, mean, ALPHA, Y, want, it, mu, LF)
    s, p, n = eng.sample_side(me, ot, it, ALPHA, mu, LF)
    items = eng.get_items(me)
    eng.side_destroy(me); eng.side_destroy(ot)
    assert np.all(np.isfinite(items))
    err = rel_err(items, want)
    print("K %d: factors %.3g, sum %.3g, prod %.3g" % (K, err, rel_err(s, s_ref), rel_err(p, p_ref)))
    assert err < RTOL, err
    assert rel_err(s, s_ref) < STAT_TOL and rel_err(p, p_ref) < STAT_TOL and abs(n - n_ref) <= STAT_TOL * abs(n_ref)
    return info


# ---- 1. one half-iteration per family against the reference ---------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [16, None])
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_half_iteration_edge_side(oracle, fam, chunk):
    import bpmf_amd
    _, K, env, kern, _ = fam
    A, nrows, w = ref.edge_side()
    with _env(**dict(env, **({"BPMF_HIP_CHUNK": chunk} if chunk else {}))):
        eng = bpmf_amd.HipEngine(K)
        try:
            info = _half_iteration(oracle, eng, K, A, nrows, w, 4, kern, 600 + K)
        finally:
            eng.close()
    if chunk:                                                        # the columns of 17 .. 257 ratings are cut at every 16th rating
        assert info["chunk"] == 16 and info["chunked_columns"] == 8 and info["chunks"] >= 2 + 4 + 4 + 5 + 8 + 8 + 9 + 17, info


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_half_iteration_ml100k(oracle, fam):
    import bpmf_amd
    _, K, env, kern, _ = fam
    M, Mt, T, Tt, nu, nm = util.ml100k()
    with _env(**env):
        eng = bpmf_amd.HipEngine(K)
        try:
            _half_iteration(oracle, eng, K, M, nu, ref.seeded_weights(len(M[2]), 31), 4, kern, 800 + K)
        finally:
            eng.close()


def test_half_iteration_k64_runs_no_product_form(oracle):
    """A side whose plain form launches the product-form kernels for its light columns sends every column through the slab form
    once it has weights; a chunked heavy column rides in the same launch."""
    import bpmf_amd
    K = 64
    rng = np.random.default_rng(864)
    A, nrows = _product_form_side(rng)
    ncols = len(A[0]) - 1
    with _env(BPMF_HIP_CHUNK=16):
        eng = bpmf_amd.HipEngine(K)
        try:
            plain = eng.side_create(ncols, nrows, *A, util.mean_rating(A))
            assert "k_sample_pf" in eng.kernel_name(plain)
            eng.set_weights(plain, np.ones(len(A[2])))
            assert eng.kernel_name(plain) == "k_sample_slabw<64>"
            eng.side_destroy(plain)
            info = _half_iteration(oracle, eng, K, A, nrows, ref.seeded_weights(len(A[2]), 32), 4, r"^k_sample_slabw<64>$", 864)
            assert info["light_columns"] > 0 and info["chunk"] == 16 and info["chunked_columns"] >= 3, info
        finally:
            eng.close()


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------------------

def _launch(eng, A, nrows, X, Y, w, it, mu, LF, replace=None):
    me, ot = _pair(eng, A, nrows, X, Y, w)
    if replace is not None:
        eng.set_weights(me, replace)
    name = eng.kernel_name(me)
    s, p, n = eng.sample_side(me, ot, it, ALPHA, mu, LF)
    out = (eng.get_items(me).tobytes(), np.asarray(s).tobytes(), np.asarray(p).tobytes(), n)
    eng.side_destroy(me); eng.side_destroy(ot)
    return out, name


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_unit_weights_are_the_plain_side_bit_for_bit(oracle, fam):
    import bpmf_amd
    _, K, env, kern, plain_env = fam
    for A, nrows, w, chunk in (ref.edge_side() + (16,), ref.edge_side() + (None,)) + ((util.ml100k()[0], util.ml100k()[4], None, None),):
        if w is None:
            w = ref.seeded_weights(len(A[2]), 33)
        ncols = len(A[0]) - 1
        X, Y = _factors(K, ncols, nrows, 900 + K)
        mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, 5)
        ck = {"BPMF_HIP_CHUNK": chunk} if chunk else {}
        with _env(**dict(plain_env, **ck)):
            eng = bpmf_amd.HipEngine(K)
            try:
                plain, pname = _launch(eng, A, nrows, X, Y, None, 5, mu, LF)
            finally:
                eng.close()
        assert "w<" not in pname and "k_sample_pf" not in pname
        if K <= 32 and plain_env.get("BPMF_HIP_MODE", 1) == 1:
            assert pname.startswith("k_sample1<"), pname             # the plain side in its default gather-stream form
        with _env(**dict(env, **ck)):
            eng = bpmf_amd.HipEngine(K)
            try:
                ones, name = _launch(eng, A, nrows, X, Y, np.ones(len(A[2])), 5, mu, LF)
                again, _ = _launch(eng, A, nrows, X, Y, np.ones(len(A[2])), 5, mu, LF)
                seeded, _ = _launch(eng, A, nrows, X, Y, w, 5, mu, LF)
                seeded2, _ = _launch(eng, A, nrows, X, Y, w, 5, mu, LF)
                back, _ = _launch(eng, A, nrows, X, Y, w, 5, mu, LF, replace=np.ones(len(A[2])))
            finally:
                eng.close()
        assert re.search(kern, name), name
        assert ones == plain, (K, chunk, name, pname)
        assert again == ones and seeded2 == seeded and seeded[0] != plain[0]
        assert back == plain


def test_weights_get_is_numpy_bit_for_bit():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    w = ref.seeded_weights(len(M[2]), 34)
    mean = util.mean_rating(M)
    eng = bpmf_amd.HipEngine(16)
    try:
        me = eng.side_create(nm, nu, *M, mean)
        eng.set_weights(me, w)
        sw, zw = eng.weights_get(me)
        assert sw.tobytes() == np.sqrt(w).tobytes() and zw.tobytes() == (np.sqrt(w) * (M[2] - mean)).tobytes()
        assert eng.weights_count(me) == (len(w), float(w.min()), float(w.max()))
        w2 = np.ones(len(w)); w2[7] = 0.37
        eng.set_weights(me, w2)                                      # a second call replaces both arrays
        sw, zw = eng.weights_get(me)
        assert sw.tobytes() == np.sqrt(w2).tobytes() and zw.tobytes() == (np.sqrt(w2) * (M[2] - mean)).tobytes()
        assert eng.weights_count(me) == (1, 0.37, 1.0)
    finally:
        eng.close()


# ---- 3. a constant weight is a scaled alpha ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [32, 128])
def test_constant_weight_is_a_scaled_alpha(oracle, K):
    import bpmf_amd
    c = 2.5
    M, Mt, T, Tt, nu, nm = util.ml100k()
    X, Y = _factors(K, nm, nu, 1000 + K)
    mu, LU, LF = oracle.hyper_sample(K, nm, np.eye(K) * 0.2, 6)
    eng = bpmf_amd.HipEngine(K)
    try:
        me, ot = _pair(eng, M, nu, X, Y, np.full(len(M[2]), c))
        eng.sample_side(me, ot, 6, ALPHA, mu, LF)
        got = eng.get_items(me)
        pl, ot2 = _pair(eng, M, nu, X, Y, None)
        eng.sample_side(pl, ot2, 6, ALPHA * c, mu, LF)
        want = eng.get_items(pl)
    finally:
        eng.close()
    err = rel_err(got, want)
    print("K %d: weight %g at alpha %g against alpha %g: %.3g" % (K, c, ALPHA, ALPHA * c, err))
    assert err < RTOL


# ---- 4. chains against the CPU restatement ----------------------------------------------------------------------------------------------

CHAIN = dict(nsims=8, burnin=3, alpha=1.5)


@functools.lru_cache(maxsize=None)
def _restated_ml100k(K):
    from oracle.oracle import Oracle
    M, Mt, T, Tt, nu, nm = util.ml100k()
    W = ref.ml100k_weights(M)
    return ref.restate_chain(Oracle(), K, M, Mt, T, W, CHAIN["nsims"], CHAIN["burnin"], CHAIN["alpha"]), W


def _check_chain(res, want, label):
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(res["U"] - want["U"]).max() / scale, np.abs(res["V"] - want["V"]).max() / scale
    et = max(np.abs(np.array(res["rmse"]) - want["rmse"]).max(), np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max())
    ef = abs(res["final_rmse_avg"] - want["final_rmse_avg"])
    print("%s: U %.3g V %.3g traces %.3g final %.3g" % (label, eu, ev, et, ef))
    assert eu < 1e-6 and ev < 1e-6 and et < 1e-6 and ef < 1e-6, (label, eu, ev, et, ef)
    assert tuple(res["weights"]) == want["weights"]


@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("pipelined", [True, False])
def test_weighted_chain_against_cpu(K, pipelined):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want, W = _restated_ml100k(K)
    n, lo, hi = want["weights"]
    assert 0.25 < n / len(M[2]) < 0.35 and (lo, hi) == (0.25, 4.0) and set(np.unique(W[2])) == {0.25, 0.37, 4.0}
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, pipelined=pipelined, weights=W, **CHAIN)
    finally:
        eng.close()
    _check_chain(res, want, "K %d pipelined %s" % (K, pipelined))


def test_weighted_chain_with_the_gate_on_its_own_stream():
    """BPMF_HIP_FUSED=0: the weighted sampler without the gate workgroup and the riders, and the sample rings on top.  Same chain."""
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want, W = _restated_ml100k(32)
    with _env(BPMF_HIP_FUSED=0):
        eng = bpmf_amd.HipEngine(32)
        try:
            res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, pipelined=True, weights=W, topn=5, **CHAIN)
        finally:
            eng.close()
    _check_chain(res, want, "K 32 unfused")
    assert res["topn"][0].shape == (nu, 5)


# ---- 5. arguments, mutual refusals, the caller's arrays, device memory ------------------------------------------------------------------

def test_ratings_are_left_alone_and_arguments_checked(oracle):
    import ctypes as C
    import scipy.sparse as sp
    import bpmf_amd
    from bpmf_amd import BpmfHipError
    K = 32
    M, Mt, T, Tt, nu, nm = util.ml100k()
    nnz = len(M[2])
    rng = np.random.default_rng(4)
    V, U = 0.4 * rng.standard_normal((nm, K)), 0.4 * rng.standard_normal((nu, K))
    w = ref.seeded_weights(nnz, 35)
    w0 = w.copy()
    mean = util.mean_rating(M)
    eng = bpmf_amd.HipEngine(K)
    hip = _hip_runtime()
    d_rows, d_vals = _to_device(hip, M[1]), _to_device(hip, M[2])
    try:
        me = eng.side_create_dev(nm, nu, M[0], d_rows.value, d_vals.value, mean)
        ot = eng.side_create(nu, nm, np.zeros(nu + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
        eng.set_weights(me, w)
        eng.set_items(me, V); eng.set_items(ot, U)
        mu, LU, LF = oracle.hyper_sample(K, nm, np.eye(K) * 0.2, 2)
        eng.sample_side(me, ot, 2, 2.5, mu, LF)
        want = V.copy()
        ref.sample_side_weighted(oracle, K, M, w, mean, 2.5, U, want, 2, mu, LF)
        assert rel_err(eng.get_items(me), want) < RTOL
        # the caller's buffers after the launch
        assert np.array_equal(_from_device(hip, d_vals, M[2]), M[2]) and np.array_equal(_from_device(hip, d_rows, M[1]), M[1])
        assert np.array_equal(w, w0)
        # every refusal of set_weights
        lib = eng.lib

        def raw(side, ws):
            bpmf_amd._lib.check(lib.bpmf_hip_side_set_weights(side.handle if side is not None else None,
                                                              ws.ctypes.data_as(C.c_void_p) if ws is not None else None))
        plain = eng.side_create(nm, nu, *M, mean)
        for args in ((None, w), (plain, None)):
            with pytest.raises(BpmfHipError, match="NULL") as e:
                raw(*args)
            assert e.value.code == EINVAL
        for v in (0.0, -1.5, float("nan"), float("inf")):
            wrong = w.copy(); wrong[nnz // 2] = v; wrong[nnz // 2 + 9] = -1.0        # the first offender is named
            with pytest.raises(BpmfHipError, match=r"of rating %d is not finite and > 0" % (nnz // 2)) as e:
                raw(plain, wrong)
            assert e.value.code == EINVAL
        with pytest.raises(BpmfHipError, match="no weights"):
            eng.weights_get(plain)
        with pytest.raises(BpmfHipError, match="no weights"):
            eng.weights_count(plain)
        with pytest.raises(ValueError, match="weights for a side of"):
            eng.set_weights(plain, w[:-1])
        with pytest.raises(ValueError, match="one array"):
            eng.set_weights(plain, w.reshape(1, -1))
        # either pointer of weights_get may be NULL
        sw = np.empty(nnz)
        bpmf_amd._lib.check(lib.bpmf_hip_side_weights_get(me.handle, sw.ctypes.data_as(C.c_void_p), None))
        zw = np.empty(nnz)
        bpmf_amd._lib.check(lib.bpmf_hip_side_weights_get(me.handle, None, zw.ctypes.data_as(C.c_void_p)))
        assert sw.tobytes() == np.sqrt(w).tobytes() and zw.tobytes() == (np.sqrt(w) * (M[2] - mean)).tobytes()
        # set_weights refuses a side that has another add-on
        pb = eng.side_create(nm, nu, *M, 0.0)
        eng.set_probit(pb, 3.0, 1)
        with pytest.raises(BpmfHipError, match="side_set_weights: not on a probit side"):
            eng.set_weights(pb, w)
        cs = eng.side_create(nm, nu, *M, mean)
        eng.set_censored(cs, np.zeros(nnz, np.int8), 5)
        with pytest.raises(BpmfHipError, match="side_set_weights: not on a censored side"):
            eng.set_weights(cs, w)
        ft = eng.side_create(nm, nu, *M, mean)
        eng.set_features(ft, rng.standard_normal((nm, 3)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="side_set_weights: not together with features"):
            eng.set_weights(ft, w)
        pp = eng.side_create(nm, nu, *M, mean)
        eng.set_prop_posterior(pp, np.tile(np.eye(K).ravel(), (nm, 1)))
        with pytest.raises(BpmfHipError, match="side_set_weights: not together with propagated priors"):
            eng.set_weights(pp, w)
        part = eng.side_create(nm, nu, M[0][:11] - M[0][0], M[1][:M[0][10]], M[2][:M[0][10]], mean, 0, 10)
        with pytest.raises(BpmfHipError, match="side_set_weights: .*whole"):
            eng.set_weights(part, w[:M[0][10]])
        ru, rm = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt)), eng.side_create(nm, nu, *M, mean)
        eng.sys_set_reduce(rm, ru)
        with pytest.raises(BpmfHipError, match="side_set_weights: .*BPMF_REDUCE"):
            eng.set_weights(rm, w)
        # ... and the other add-ons refuse a side with weights
        with pytest.raises(BpmfHipError, match="side_set_probit: not on a side with per-rating weights"):
            eng.set_probit(me, 3.0, 1)
        with pytest.raises(BpmfHipError, match="side_set_censored: not on a side with per-rating weights"):
            eng.set_censored(me, np.zeros(nnz, np.int8), 5)
        with pytest.raises(BpmfHipError, match="not on a side with per-rating weights"):
            eng.set_features(me, rng.standard_normal((nm, 3)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="not on a side with per-rating weights"):
            eng.set_features(me, sp.random(nm, 9, density=0.3, random_state=1, format="csr"), 5.0, 3)
        with pytest.raises(BpmfHipError, match="set_prop_posterior: not on a side with per-rating weights"):
            eng.set_prop_posterior(me, np.tile(np.eye(K).ravel(), (nm, 1)))
        cu = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt))
        with pytest.raises(BpmfHipError, match="train_sse: not with a side with per-rating weights"):
            eng.train_sse(me, cu)
        with pytest.raises(BpmfHipError, match="train_sse: not with a side with per-rating weights"):
            eng.train_sse(cu, me)
        with pytest.raises(BpmfHipError, match="sys_set_reduce: not together with per-rating weights"):
            eng.sys_set_reduce(me, cu)
    finally:
        eng.close()
        hip.hipFree(d_rows); hip.hipFree(d_vals)


def test_set_weights_refuses_an_fp32_context():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = bpmf_amd.HipEngine(128, dtype="f32")
    try:
        side = eng.side_create(nm, nu, *M, util.mean_rating(M))
        with pytest.raises(bpmf_amd.BpmfHipError, match="side_set_weights: not on an fp32 context") as e:
            eng.set_weights(side, np.ones(len(M[2])))
        assert e.value.code == EINVAL
        with pytest.raises(ValueError, match="fp64"):
            bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=2, burnin=0, weights=(M[0], M[1], np.full(len(M[2]), 2.0)))
    finally:
        eng.close()


_COMM_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bpmf_amd
eng = bpmf_amd.HipEngine(8)
eng.comm_init(1, 0, eng.comm_unique_id())
side = eng.side_create(2, 4, np.array([0, 4, 6], np.int64), np.array([0, 1, 2, 3, 0, 2], np.int32), np.array([2., 3., 7., 4., 5., 1.]), 3.0)
try:
    eng.set_weights(side, np.array([1., 2., .5, 1., 4., 1.]))
    print("ACCEPTED")
except bpmf_amd.BpmfHipError as e:
    print("REFUSED %d %s" % (e.code, e))
eng.close()
"""


def test_set_weights_refuses_a_context_with_a_communicator():
    """The other branch of the single-GPU check: a whole side on a context that has a communicator (one rank, as `bpmf -g 1`
    makes one).  In a process of its own: a communicator is process-wide state of the communication library."""
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("BPMF_HIP_RCCL_LIBRARY", None)
    r = subprocess.run([sys.executable, "-c", _COMM_CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert re.search(r"^REFUSED -1 .*side_set_weights: .*communicator", r.stdout, re.M), r.stdout


def test_device_memory_returns():
    import bpmf_amd

    def live():
        return int(bpmf_amd.load_library().bpmf_hip_live_device_bytes())
    M, Mt, T, Tt, nu, nm = util.tiny()
    base = live()
    eng = bpmf_amd.HipEngine(8)
    try:
        movies = eng.side_create(nm, nu, *M, util.mean_rating(M))
        users = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt))
        before = live()
        wm = np.ones(len(M[2])); wm[0], wm[-1] = 2.5, 0.25
        wu = np.ones(len(Mt[2])); wu[1] = 4.0
        # a refused call leaves nothing
        wrong = wm.copy(); wrong[-1] = 0.0
        with pytest.raises(bpmf_amd.BpmfHipError, match="not finite and > 0"):
            eng.set_weights(movies, wrong)
        assert live() == before
        eng.set_weights(movies, wm)
        assert live() - before == 2 * len(wm) * 8                    # sw and zw
        eng.set_weights(movies, wm[::-1].copy())                     # replaced, not added
        assert live() - before == 2 * len(wm) * 8
        eng.set_weights(users, wu)
        held = live()
        for _ in range(2):
            eng.sys_sample(movies, users, 2.0)
            eng.sys_sample(users, movies, 2.0)
        eng.sync()
        assert live() == held
        eng.side_destroy(movies)
        assert before - 2 * len(wu) * 8 < live() < held
        eng.side_destroy(users)
        assert live() == before
    finally:
        eng.close()
    assert live() == base


# ---- 6. planted heteroscedastic experiment ----------------------------------------------------------------------------------------------

def test_planted_weights_are_honoured(oracle):
    """600 x 300, rank 4, 40 training cells per user, half of them with noise sd 2 and the others sd 0.25, 6000 noise-free test cells;
    alpha = 16 and w = 1 / 64 at the noisy cells.  Restated CPU chains, test RMSE of the posterior-mean prediction
    (weights_ref.PLANTED_MEASURED; tests/test_weights_host.py re-measures all four):
        weights honoured                              0.1685
        weights ignored, alpha = 16                   1.3976
        weights ignored, alpha = 1 / mean variance    0.6112   (the best single alpha)
        noisy cells dropped                           0.1714
    Asserted: the GPU chain with the weights beats the best single alpha by at least half the recorded margin (0.2214), lands within
    that half margin of the restated chain with the weights -- and is that chain at the chain bars."""
    import bpmf_amd
    P = ref.PLANTED
    d = ref.planted_data(**P)
    assert d["nnoisy"] == 11880 and len(d["T"][2]) == P["ntest"] and abs(1.0 / d["mean_var"] - 0.4971) < 1e-3
    a = ref.restate_chain(oracle, P["K"], d["M"], d["Mt"], d["T"], d["W"], P["nsims"], P["burnin"], P["alpha"])
    c = ref.restate_chain(oracle, P["K"], d["M"], d["Mt"], d["T"], None, P["nsims"], P["burnin"], 1.0 / d["mean_var"])
    ra, rc = ref.planted_rmse(a["pred"], d["T"][2]), ref.planted_rmse(c["pred"], d["T"][2])
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, d["M"], d["Mt"], d["T"], P["nusers"], P["nmovies"], nsims=P["nsims"], burnin=P["burnin"], Tt=d["Tt"],
                             pipelined=True, alpha=P["alpha"], weights=d["W"])
    finally:
        eng.close()
    # the GPU chain's test RMSE of its running-mean prediction ("avg RMSE" of the last line; the closing evaluation counts the last
    # sample twice, c++/bpmf.cpp:242: 0.1683 for the restated chain against the 0.1685 of the plain mean)
    rg = res["final_rmse_avg"]
    print("test RMSE: GPU honoured %.4f, restated honoured %.4f, restated best single alpha %.4f" % (rg, ra, rc))
    assert rc - rg >= ref.PLANTED_HALF_MARGIN, (rc, rg)
    assert abs(rg - ra) <= ref.PLANTED_HALF_MARGIN, (rg, ra)
    assert abs(ra - ref.PLANTED_MEASURED[0]) < 1e-6 and abs(rc - ref.PLANTED_MEASURED[2]) < 1e-6
    _check_chain(res, a, "planted, weights honoured")


# ---- 7. the executable ------------------------------------------------------------------------------------------------------------------

def _mask(stdout):
    """stdout without what differs between two runs of the same command: the pid and the rates of the iteration lines"""
    out = re.sub(r"^pid: \d+$", "pid: *", stdout, flags=re.M)
    out = re.sub(r"items/sec: .*$", "items/sec: *", out, flags=re.M)
    return re.sub(r"^(Total time|Average items/sec|Average ratings/sec): .*$", r"\1: *", out, flags=re.M)


def test_cli_weights_end_to_end(tmp_path, oracle):
    import scipy.sparse as sp
    import bpmf_amd
    from bpmf_amd import io as bio
    M, Mt, T, Tt, nu, nm = util.tiny()
    # tiny-train.mtx: the cells (1..4, 1), (1, 2), (3, 2); three of them weighted, one with the weight 1
    W = util.csc_arrays(sp.coo_matrix((np.array([2.5, 0.25, 1.0, 4.0]), ([0, 2, 3, 2], [0, 0, 0, 1])), shape=(nu, nm)))
    bio.write_sparse(tmp_path / "W.sdm", nu, nm, W)
    want = ref.restate_chain(oracle, 8, M, Mt, T, W, 6, 2, 3.0)
    eng = bpmf_amd.HipEngine(8)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, alpha=3.0, Tt=Tt, pipelined=True, weights=W)
    finally:
        eng.close()
    assert res["weights"] == (3, 0.25, 4.0) == want["weights"]
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    base = [exe, "-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx"), "-a", "3", "-i", "6",
            "-b", "2", "-d", "8"]
    (tmp_path / "o").mkdir(); (tmp_path / "p").mkdir()

    def run(extra):
        return subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    plain_before = run(["-o", str(tmp_path / "p")])
    runs = [run(["--weights", str(tmp_path / "W.sdm"), "-v", "-o", str(tmp_path / "o")]),       # -o: the plain loop
            run(["--weights", str(tmp_path / "W.sdm")])]                                  # without: the pipelined one
    plain_after = run(["-o", str(tmp_path / "p")])
    for out in runs:
        assert out.returncode == 0, out.stderr
        assert re.search(r"^weights: 3 of 6 training ratings weighted, min 0\.25, max 4$", out.stdout, re.M), out.stdout
        lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", out.stdout)
        assert len(lines) == 6
        got = np.array([[float(a), float(b)] for a, b in lines])
        # the RMSE lines are those of gibbs(weights=W), to half a unit of the four printed decimals
        assert np.abs(got[:, 0] - res["rmse"]).max() <= 5e-5 and np.abs(got[:, 1] - res["rmse_avg"]).max() <= 5e-5
        assert np.abs(got[:, 0] - want["rmse"]).max() <= 1e-6 + 5e-5 and np.abs(got[:, 1] - want["rmse_avg"]).max() <= 1e-6 + 5e-5
        final = re.search(r"^Final Avg RMSE: (\S+)$", out.stdout, re.M)
        assert final and abs(float(final.group(1)) - want["final_rmse_avg"]) <= 1e-6 + 5e-6 * max(1.0, want["final_rmse_avg"])
    # the last sample (-v) at the bar of the chain tests
    U, V = bio.read_dense(tmp_path / "o" / "U-5.ddm").T, bio.read_dense(tmp_path / "o" / "V-5.ddm").T
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(U - want["U"]).max() / scale, np.abs(V - want["V"]).max() / scale
    print("bpmf --weights: U %.3g V %.3g of max|U|" % (eu, ev))
    assert eu < 1e-6 and ev < 1e-6, (eu, ev)
    # without the flag: the same stdout before and after, no weights line, and the lines of the plain chain
    assert plain_before.returncode == 0 and plain_after.returncode == 0, plain_before.stderr + plain_after.stderr
    assert _mask(plain_before.stdout) == _mask(plain_after.stdout) and "weights" not in plain_before.stdout
    plain_want = ref.restate_chain(oracle, 8, M, Mt, T, None, 6, 2, 3.0)
    lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", plain_before.stdout)
    got = np.array([[float(a), float(b)] for a, b in lines])
    assert np.abs(got[:, 0] - plain_want["rmse"]).max() <= 1e-6 + 5e-5
    assert _mask(plain_before.stdout) != _mask(runs[0].stdout)


def test_cli_weights_follow_the_renumbering(tmp_path, oracle):
    """BPMF_TEST_ASSIGN_PARTS=3 renumbers rows and columns as for three ranks and runs on one GPU without -g: the chain is the
    restated chain on the renumbered ratings WITH the renumbered weight matrix (test_gpu_censored.py does the same for the flags)."""
    import scipy.sparse as sp
    from bpmf_amd import io as bio
    from tests.test_assign import greedy
    K, parts, nsims, burnin = 8, 3, 6, 2
    M, Mt, T, Tt, nu, nm = util.ml100k()
    Wm = ref.ml100k_weights(M)
    pm, pu = np.arange(nm), np.arange(nu)
    for _ in range(2):
        for side in (0, 1):
            perm, csc = (pm, M) if side == 0 else (pu, Mt)
            order, _ = greedy(np.concatenate([[0], np.cumsum(np.diff(csc[0])[perm])]), parts)
            if side == 0:
                pm = perm[order]
            else:
                pu = perm[order]
    renum = lambda X: util.csc_arrays(sp.csc_matrix((X[2], X[1], X[0]), shape=(nu, nm))[pu][:, pm].tocsc())
    Mp, Tp, Wp = renum(M), renum(T), renum(Wm)
    assert not np.array_equal(pm, np.arange(nm)) and not np.array_equal(Wp[0], Wm[0])      # the weighted columns moved
    Mpt = util.csc_arrays(sp.csc_matrix((Mp[2], Mp[1], Mp[0]), shape=(nu, nm)).T)
    want = ref.restate_chain(oracle, K, Mp, Mpt, Tp, Wp, nsims, burnin, 2.0)
    bio.write_sparse(tmp_path / "W.sdm", nu, nm, Wm)
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    (tmp_path / "o").mkdir()
    out = subprocess.run([exe, "-i", str(nsims), "-b", str(burnin), "-d", str(K), "-v", "-o", "o/", "-n", os.path.join(util.GOLDEN, "ml100k-train.mtx.gz"),
                          "-p", os.path.join(util.GOLDEN, "ml100k-test.mtx.gz"), "--weights", str(tmp_path / "W.sdm")], cwd=tmp_path,
                         env=dict(os.environ, BPMF_TEST_ASSIGN_PARTS=str(parts)), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "assignment: greedy" in out.stdout
    assert re.search(r"^weights: %d of %d training ratings weighted, min 0\.25, max 4$" % (want["weights"][0], len(M[2])), out.stdout, re.M), out.stdout
    lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", out.stdout)
    got = np.array([[float(a), float(b)] for a, b in lines])
    assert got.shape == (nsims, 2)
    assert np.abs(got[:, 0] - want["rmse"]).max() <= 1e-6 + 5e-5 and np.abs(got[:, 1] - want["rmse_avg"]).max() <= 1e-6 + 5e-5
    final = re.search(r"^Final Avg RMSE: (\S+)$", out.stdout, re.M)
    assert final and abs(float(final.group(1)) - want["final_rmse_avg"]) <= 1e-6 + 5e-6
    # the last sample, written in the ORIGINAL numbering: row pu[j] of the file = row j of the renumbered chain's factor
    U = bio.read_dense(tmp_path / "o" / ("U-%d.ddm" % (nsims - 1))).T; V = bio.read_dense(tmp_path / "o" / ("V-%d.ddm" % (nsims - 1))).T
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(U[pu] - want["U"]).max() / scale, np.abs(V[pm] - want["V"]).max() / scale
    plain = ref.restate_chain(oracle, K, Mp, Mpt, Tp, None, nsims, burnin, 2.0)
    away = np.abs(plain["U"] - want["U"]).max() / scale
    print("renumbered: U %.3g V %.3g; the chain without the weights is %.3g away" % (eu, ev, away))
    assert eu < 1e-6 and ev < 1e-6 and away > 1e-2


def test_fixed_path_is_untouched_by_a_weighted_run():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.tiny()
    Wm = (np.array([0, 2, 3], np.int64), np.array([0, 2, 0], np.int32), np.array([2.5, 0.25, 4.0]))   # (1, 1), (3, 1), (1, 2) of tiny-train.mtx
    eng = bpmf_amd.HipEngine(16)
    try:
        before = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
        ws = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True, weights=Wm)
        after = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
    finally:
        eng.close()
    assert before["U"].tobytes() == after["U"].tobytes() and before["V"].tobytes() == after["V"].tobytes()
    assert before["rmse"] == after["rmse"] and before["rmse_avg"] == after["rmse_avg"]
    assert "weights" not in before and "weights" not in after and ws["weights"] == (3, 0.25, 4.0)
    assert not np.array_equal(ws["U"], before["U"])
