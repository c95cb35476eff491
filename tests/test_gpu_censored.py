"""Censored ratings (`gibbs(..., censored=C)`, `bpmf --censored FILE`) on the GPU.

  * the latent kernel (k_censor_latent) against the CPU restatement of tests/censor_ref.py at every censored position, the ratings
    bit for bit at every other: K = 8, 10, 16, 32, 64, 100, 128 fp64 and 128 fp32 on the matrix with a 50 000-rating column, both
    orientations, alpha 0.5 / 2 / 3
  * list lengths 0, 1, 255, 256, 257 and nnz, all lower bounds / all upper bounds / mixed, two launches bit-equal
  * a side whose flags are all zero samples bit for bit like a side without flags
  * one half-iteration through each sampler family with the latent values in place of the ratings, against oracle.sample_side fed
    the restatement's values
  * the coupled chain against the restated chain (K = 32, 64; pipelined and plain loop; BPMF_HIP_FUSED=0 once)
  * arguments, mutual refusals, the caller's ratings, the failure word, device memory
  * a planted experiment in which honouring the bounds beats taking them for measurements
  * `bpmf --censored` end to end, and a guard that a censored run leaves nothing behind in the fixed path

tests/test_censor_host.py asserts on the CPU that no accept / reject decision of the restatement is within 1e-9 of its threshold
for the inputs of the first two tests: a mismatch here is never a flipped branch.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import censor_ref as ref
from tests import probit_ref
from tests import util
from tests.conftest import ROOT
from tests.test_gpu_parity import RTOL, rel_err
from tests.test_gpu_probit import _from_device, _hip_runtime, _product_form_side, _to_device, _write_mtx

pytestmark = pytest.mark.gpu

NT = ref.NT
ENUM, EINVAL = -5, -1
LATENT_BAR = 1e-12          # |z - z_ref| <= 1e-12 (1 + |b| + |m|): the bar of the probit latent test, which measured 3e-15


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


def _hyper(K, ncols, it, seed):
    import bpmf_amd
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, 3 * K))
    return bpmf_amd.engine.hyper_sample(K, ncols, A @ A.T / (3 * K), it)


def _pair(eng, A, nrows, X, Y, flags, tag, mean=None):
    """A side over the ratings A (censored by `flags`; None: no flags) holding the factors X, and a partner without ratings holding Y."""
    ncols = len(A[0]) - 1
    me = eng.side_create(ncols, nrows, *A, util.mean_rating(A) if mean is None else mean)
    ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    if flags is not None:
        eng.set_censored(me, flags, tag)
    eng.set_items(me, X)
    eng.set_items(ot, Y)
    return me, ot


def _check_latent(z, A, flags, z_ref, pos, m):
    """-> the worst |z - z_ref| / (1 + |b| + |m|) over the censored positions; asserts the exact positions and the half lines"""
    exact = flags == 0
    assert z[exact].tobytes() == A[2][exact].tobytes()
    b, s = A[2][pos], flags[pos].astype(np.float64)
    assert np.all(np.isfinite(z[pos])) and np.all(s * (z[pos] - b) >= 0.0)
    return float((np.abs(z[pos] - z_ref[pos]) / (1.0 + np.abs(b) + np.abs(m))).max()) if len(pos) else 0.0


# ---- 1. the latent kernel against the restatement -----------------------------------------------------------------------------------

@pytest.mark.parametrize("K,dtype", probit_ref.LATENT_CASES)
def test_latent_against_restatement(K, dtype):
    import bpmf_amd
    sides, nu, nm = ref.latent_inputs()
    U, V = probit_ref.latent_factors(K, dtype, nu, nm)
    it = ref.LATENT_ITER
    eng = bpmf_amd.HipEngine(K, dtype=dtype)
    try:
        for A, nrows, side, tag, flags in sides:
            X, Y = (V, U) if side == 0 else (U, V)
            ncols, mean = len(A[0]) - 1, util.mean_rating(A)
            mu, LU, LF = _hyper(K, ncols, it, 70 + K)
            me, ot = _pair(eng, A, nrows, X, Y, flags, tag)
            assert np.array_equal(eng.get_items(me), X) and np.array_equal(eng.get_items(ot), Y)     # fp32: representable values
            assert eng.censored_count(me) == (int((flags > 0).sum()), int((flags < 0).sum()))
            assert eng.censored_latent(me).tobytes() == A[2].tobytes()                             # before any launch: the ratings
            for alpha in ref.LATENT_ALPHAS:
                z_ref, pos, m, attempts, margin, bmargin = ref.latent(A, flags, X, Y, it, tag, alpha, mean, full=True)
                eng.set_items(me, X)
                eng.sample_side(me, ot, it, alpha, mu, LF)
                z = eng.censored_latent(me)
                worst = _check_latent(z, A, flags, z_ref, pos, m)
                print("K %d %s tag %d alpha %g: %d of %d ratings censored, |m| <= %.2f, attempts mean %.3f max %d, worst ratio %.3g, "
                      "closest decision %.3g" % (K, dtype, tag, alpha, len(pos), len(z), np.abs(m).max(), attempts.mean(), attempts.max(),
                                                 worst, min(margin, bmargin)))
                assert worst <= LATENT_BAR, (K, dtype, tag, alpha, worst)
            eng.side_destroy(me); eng.side_destroy(ot)
    finally:
        eng.close()


# ---- 2. list-length edges -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", ref.EDGE_COUNTS)
def test_list_length_edges(count):
    import bpmf_amd
    K, it, alpha, tag = 8, 2, 3.0, ref.TAG_MOVIES
    A, nrows = ref.edge_side()
    ncols, nnz, mean = len(A[0]) - 1, len(A[2]), util.mean_rating(A)
    assert ncols == 33 and np.diff(A[0]).min() == 0 and np.diff(A[0]).max() == 40 and nnz > 257
    rng = np.random.default_rng(5)
    X, Y = 0.6 * rng.standard_normal((ncols, K)), 0.6 * rng.standard_normal((nrows, K))
    mu, LU, LF = _hyper(K, ncols, it, 9)
    eng = bpmf_amd.HipEngine(K)
    try:
        for signs in ref.EDGE_SIGNS:
            flags = ref.edge_flags(A, count, signs)
            n = nnz if count == "nnz" else count
            if n >= 2:
                assert flags[0] != 0 and flags[-1] != 0                                   # the first and the last position of the CSC
            if n >= 255:
                assert np.all(flags[A[0][4]:A[0][5]] != 0) and A[0][5] - A[0][4] == 40    # a column whose every rating is censored
            z_ref, pos, m, _, _, _ = ref.latent(A, flags, X, Y, it, tag, alpha, mean, full=True)
            me, ot = _pair(eng, A, nrows, X, Y, flags, tag)
            assert sum(eng.censored_count(me)) == n
            got = []
            for _ in range(2):
                eng.set_items(me, X)
                eng.sample_side(me, ot, it, alpha, mu, LF)
                got.append(eng.censored_latent(me))
            eng.side_destroy(me); eng.side_destroy(ot)
            worst = _check_latent(got[0], A, flags, z_ref, pos, m)
            print("count %s %s: worst ratio %.3g" % (count, signs, worst))
            assert worst <= LATENT_BAR, (count, signs, worst)
            assert got[1].tobytes() == got[0].tobytes()
            if n == 0:
                assert got[0].tobytes() == A[2].tobytes()
    finally:
        eng.close()


# ---- 3. an all-zero flags array is the plain path -------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,mode", [(8, 1), (8, 3), (64, None), (128, None)])
def test_zero_flags_half_iteration_is_the_plain_one(K, mode):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    rng = np.random.default_rng(30 + K)
    sigma = (2.0 / K) ** 0.25
    V, U = sigma * rng.standard_normal((nm, K)), sigma * rng.standard_normal((nu, K))
    mu, LU, LF = _hyper(K, nm, 3, 4)
    with _env(**({"BPMF_HIP_MODE": mode} if mode else {})):
        eng = bpmf_amd.HipEngine(K)
        try:
            out = []
            for flags in (None, np.zeros(len(M[2]), np.int8)):
                me, ot = _pair(eng, M, nu, V, U, flags, ref.TAG_MOVIES)
                s, p, n = eng.sample_side(me, ot, 3, 1.7, mu, LF)
                out.append((eng.get_items(me), s, p, n))
                if flags is not None:
                    assert eng.censored_count(me) == (0, 0) and eng.censored_latent(me).tobytes() == M[2].tobytes()
                eng.side_destroy(me); eng.side_destroy(ot)
        finally:
            eng.close()
    (i0, s0, p0, n0), (i1, s1, p1, n1) = out
    assert i0.tobytes() == i1.tobytes() and s0.tobytes() == s1.tobytes() and np.asarray(p0).tobytes() == np.asarray(p1).tobytes() and n0 == n1


def test_zero_flags_chain_is_the_plain_one():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    none = (np.zeros(nm + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    eng = bpmf_amd.HipEngine(32)
    try:
        plain = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=4, burnin=1, Tt=Tt, pipelined=True, alpha=1.7)
        zero = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=4, burnin=1, Tt=Tt, pipelined=True, alpha=1.7, censored=none)
    finally:
        eng.close()
    assert zero["censored"] == (0, 0) and "censored" not in plain
    assert plain["U"].tobytes() == zero["U"].tobytes() and plain["V"].tobytes() == zero["V"].tobytes()
    assert plain["rmse"] == zero["rmse"] and plain["rmse_avg"] == zero["rmse_avg"] and plain["norm_u"] == zero["norm_u"]


# ---- 4. one half-iteration per sampler family ---------------------------------------------------------------------------------------

ALPHA = 1.7                 # not a power of two: sqrt(alpha) and 1 / sqrt(alpha) round


def _half_iteration(oracle, eng, K, A, nrows, X, Y, flags, it, tag, tol, stat_tol, expect_kernel):
    ncols, mean = len(A[0]) - 1, util.mean_rating(A)
    me, ot = _pair(eng, A, nrows, X, Y, flags, tag)
    assert re.search(expect_kernel, eng.kernel_name(me)), eng.kernel_name(me)
    info = eng.schedule_info(me)
    X, Y = eng.get_items(me), eng.get_items(ot)                      # (fp32: the stored values, widened)
    z = ref.latent(A, flags, X, Y, it, tag, ALPHA, mean)
    mu, LU, LF = oracle.hyper_sample(K, ncols, np.eye(K) * 0.2, it)
    want = X.copy()
    s_ref, p_ref, n_ref = oracle.sample_side(K, (A[0], A[1], z), mean, ALPHA, Y, want, it, mu, LF, nthreads=NT)
    s, p, n = eng.sample_side(me, ot, it, ALPHA, mu, LF)
    items = eng.get_items(me)
    zg = eng.censored_latent(me)
    eng.side_destroy(me); eng.side_destroy(ot)
    assert np.all(np.isfinite(items))
    err = rel_err(items, want)
    print("K %d %s: factors %.3g, latent %.3g" % (K, eng.dtype, err, np.abs(zg - z).max()))
    assert err < tol, err
    assert rel_err(s, s_ref) < stat_tol and rel_err(p, p_ref) < stat_tol and abs(n - n_ref) <= stat_tol * abs(n_ref)
    return info


@pytest.mark.parametrize("mode", [1, 3])
def test_half_iteration_k8(oracle, mode):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    with _env(BPMF_HIP_MODE=mode):
        eng = bpmf_amd.HipEngine(8)
        try:
            rng = np.random.default_rng(80 + mode)
            _half_iteration(oracle, eng, 8, M, nu, 0.7 * rng.standard_normal((nm, 8)), 0.7 * rng.standard_normal((nu, 8)),
                            ref.seeded_flags(len(M[2]), 41), 3, ref.TAG_MOVIES, RTOL, 1e-8, {1: r"k_sample1", 3: r"k_sample4"}[mode])
        finally:
            eng.close()


@pytest.mark.parametrize("K,dtype", [(10, "f64"), (32, "f64"), (64, "f64"), (100, "f64"), (128, "f64"), (128, "f32")])
def test_half_iteration_families(oracle, K, dtype):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    rng = np.random.default_rng(800 + K)
    sigma = (2.0 / K) ** 0.25
    tol, stat_tol = (2e-3, 1e-3) if dtype == "f32" else (RTOL, 1e-8)
    with _env(**({"BPMF_HIP_CHUNK": 16} if K == 64 else {})):
        eng = bpmf_amd.HipEngine(K, dtype=dtype)
        try:
            if K == 64:                                              # product-form columns + a chunked heavy column in the slab launch
                A, nrows = _product_form_side(rng)
                ncols = len(A[0]) - 1
                flags = ref.seeded_flags(len(A[2]), 42)
                for c in np.flatnonzero(np.diff(A[0]) == 300):       # censored entries on both sides of the first chunk cuts
                    flags[A[0][c] + 15], flags[A[0][c] + 16], flags[A[0][c] + 31], flags[A[0][c] + 32] = 1, -1, -1, 1
                info = _half_iteration(oracle, eng, K, A, nrows, sigma * rng.standard_normal((ncols, K)), sigma * rng.standard_normal((nrows, K)),
                                       flags, 4, ref.TAG_MOVIES, tol, stat_tol, r"k_sample_pf")
                assert info["pf_le3"] > 0 and info["pf_4to6"] > 0 and info["pf_7to16"] > 0 and info["other_items"] > 0, info
                assert info["chunk"] == 16 and info["chunked_columns"] >= 3, info
            else:
                V, U = sigma * rng.standard_normal((nm, K)), sigma * rng.standard_normal((nu, K))
                kern = r"k_sample_wg2" if K > 64 else r"k_sample"
                _half_iteration(oracle, eng, K, M, nu, V, U, ref.seeded_flags(len(M[2]), 43), 4, ref.TAG_MOVIES, tol, stat_tol, kern)
        finally:
            eng.close()


# ---- 5. chains against the CPU restatement ------------------------------------------------------------------------------------------

CHAIN = dict(nsims=8, burnin=3, alpha=1.5)


@functools.lru_cache(maxsize=None)
def _restated_ml100k(K):
    from oracle.oracle import Oracle
    M, Mt, T, Tt, nu, nm = util.ml100k()
    C = ref.ml100k_censoring(M)
    return ref.restate_chain(Oracle(), K, M, Mt, T, C, CHAIN["nsims"], CHAIN["burnin"], CHAIN["alpha"]), C


def _check_chain(res, want, label):
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(res["U"] - want["U"]).max() / scale, np.abs(res["V"] - want["V"]).max() / scale
    et = max(np.abs(np.array(res["rmse"]) - want["rmse"]).max(), np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max())
    ef = abs(res["final_rmse_avg"] - want["final_rmse_avg"])
    print("%s: U %.3g V %.3g traces %.3g final %.3g, closest decision of the restatement %.3g" % (label, eu, ev, et, ef, want["margin"]))
    assert eu < 1e-6 and ev < 1e-6 and et < 1e-6 and ef < 1e-6, (label, eu, ev, et, ef)
    assert tuple(res["censored"]) == want["censored"]


@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("pipelined", [True, False])
def test_censored_chain_against_cpu(K, pipelined):
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want, C = _restated_ml100k(K)
    frac = sum(want["censored"]) / len(M[2])
    assert 0.1 < frac < 0.2 and min(want["censored"]) > 2000         # 20 % drawn, the 3s among them stay exact; both kinds present
    eng = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, pipelined=pipelined, censored=C, **CHAIN)
    finally:
        eng.close()
    _check_chain(res, want, "K %d pipelined %s" % (K, pipelined))


def test_censored_chain_with_the_gate_on_its_own_stream():
    """BPMF_HIP_FUSED=0: the latent kernel is enqueued by bpmf_hip_sys_sample ahead of the samplers' stream's wait for the gate
    event, not by launch_sampler.  Same chain."""
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.ml100k()
    want, C = _restated_ml100k(32)
    with _env(BPMF_HIP_FUSED=0):
        eng = bpmf_amd.HipEngine(32)
        try:
            res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, pipelined=True, censored=C, topn=5, **CHAIN)
        finally:
            eng.close()
    _check_chain(res, want, "K 32 unfused")
    assert res["topn"][0].shape == (nu, 5)


# ---- 6. the ratings are left alone, arguments are checked -----------------------------------------------------------------------------

def test_ratings_are_left_alone_and_arguments_checked():
    import ctypes as C
    import scipy.sparse as sp
    import bpmf_amd
    from bpmf_amd import BpmfHipError
    K = 32
    M, Mt, T, Tt, nu, nm = util.ml100k()
    nnz = len(M[2])
    rng = np.random.default_rng(4)
    V, U = 0.4 * rng.standard_normal((nm, K)), 0.4 * rng.standard_normal((nu, K))
    flags = ref.seeded_flags(nnz, 44)
    mean = util.mean_rating(M)
    eng = bpmf_amd.HipEngine(K)
    hip = _hip_runtime()
    d_rows, d_vals = _to_device(hip, M[1]), _to_device(hip, M[2])
    try:
        me = eng.side_create_dev(nm, nu, M[0], d_rows.value, d_vals.value, mean)
        ot = eng.side_create(nu, nm, np.zeros(nu + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
        eng.set_censored(me, flags, 5)
        eng.set_items(me, V); eng.set_items(ot, U)
        mu, LU, LF = _hyper(K, nm, 2, 5)
        eng.sample_side(me, ot, 2, 2.5, mu, LF)
        z = eng.censored_latent(me)
        z_ref, pos, m, _, _, _ = ref.latent(M, flags, V, U, 2, 5, 2.5, mean, full=True)
        assert _check_latent(z, M, flags, z_ref, pos, m) <= LATENT_BAR
        # the caller's buffers after the launch
        assert np.array_equal(_from_device(hip, d_vals, M[2]), M[2]) and np.array_equal(_from_device(hip, d_rows, M[1]), M[1])
        # a NaN factor row: every draw of its censored ratings runs into the cap -> BPMF_HIP_ENUM; the next healthy launch succeeds
        col = int(np.repeat(np.arange(nm), np.diff(M[0]))[pos[len(pos) // 2]])
        bad = V.copy(); bad[col] = np.nan
        eng.set_items(me, bad)
        with pytest.raises(BpmfHipError, match="rejected 64 times") as e:
            eng.sample_side(me, ot, 3, 2.5, mu, LF)
        assert e.value.code == ENUM
        eng.set_items(me, V)
        eng.sample_side(me, ot, 2, 2.5, mu, LF)
        assert eng.censored_latent(me).tobytes() == z.tobytes()
        # every refusal of set_censored
        lib = eng.lib
        f8 = np.ascontiguousarray(flags)

        def raw(side, fl, tag):
            bpmf_amd._lib.check(lib.bpmf_hip_side_set_censored(side.handle if side is not None else None,
                                                               fl.ctypes.data_as(C.c_void_p) if fl is not None else None, tag))
        plain = eng.side_create(nm, nu, *M, mean)
        for args, msg in (((None, f8, 5), "NULL"), ((plain, None, 5), "NULL"), ((plain, f8, 0), "tag must be >= 1"),
                          ((me, f8, 5), "censored side already")):
            with pytest.raises(BpmfHipError, match=msg) as e:
                raw(*args)
            assert e.value.code == EINVAL
        for v in (2, -2, 127, -128):
            wrong = f8.copy(); wrong[nnz // 2] = v
            with pytest.raises(BpmfHipError, match=r"flag %d of rating %d is not one of -1, 0, \+1" % (v, nnz // 2)) as e:
                raw(plain, wrong, 5)
            assert e.value.code == EINVAL
        with pytest.raises(ValueError, match="-1, 0 or"):
            eng.set_censored(plain, flags.astype(np.int64) * 2, 5)
        with pytest.raises(ValueError, match="flags for a side of"):
            eng.set_censored(plain, flags[:-1], 5)
        pb = eng.side_create(nm, nu, *M, 0.0)
        eng.set_probit(pb, 3.0, 1)
        with pytest.raises(BpmfHipError, match="not on a probit side"):
            eng.set_censored(pb, flags, 5)
        ft = eng.side_create(nm, nu, *M, mean)
        eng.set_features(ft, rng.standard_normal((nm, 3)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="not together with features"):
            eng.set_censored(ft, flags, 5)
        pp = eng.side_create(nm, nu, *M, mean)
        eng.set_prop_posterior(pp, np.tile(np.eye(K).ravel(), (nm, 1)))
        with pytest.raises(BpmfHipError, match="propagated priors"):
            eng.set_censored(pp, flags, 5)
        part = eng.side_create(nm, nu, M[0][:11] - M[0][0], M[1][:M[0][10]], M[2][:M[0][10]], mean, 0, 10)
        with pytest.raises(BpmfHipError, match="whole"):
            eng.set_censored(part, flags[:M[0][10]], 5)
        ru, rm = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt)), eng.side_create(nm, nu, *M, mean)
        eng.sys_set_reduce(rm, ru)
        with pytest.raises(BpmfHipError, match="BPMF_REDUCE"):
            eng.set_censored(rm, flags, 5)
        # ... and the other add-ons refuse a censored side
        with pytest.raises(BpmfHipError, match="not on a censored side"):
            eng.set_probit(me, 3.0, 1)
        with pytest.raises(BpmfHipError, match="not on a censored side"):
            eng.set_features(me, rng.standard_normal((nm, 3)), 5.0, 3)
        with pytest.raises(BpmfHipError, match="not on a censored side"):
            eng.set_features(me, sp.random(nm, 9, density=0.3, random_state=1, format="csr"), 5.0, 3)
        cu = eng.side_create(nu, nm, *Mt, util.mean_rating(Mt))
        with pytest.raises(BpmfHipError, match="train_sse: not with a censored side"):
            eng.train_sse(me, cu)
        with pytest.raises(BpmfHipError, match="train_sse: not with a censored side"):
            eng.train_sse(cu, me)
        with pytest.raises(BpmfHipError, match="censored ratings"):
            eng.sys_set_reduce(me, cu)
        with pytest.raises(BpmfHipError, match="not a censored side"):
            eng.censored_latent(plain)
        with pytest.raises(BpmfHipError, match="not a censored side"):
            eng.censored_count(plain)
        with pytest.raises(BpmfHipError, match="alpha > 0"):
            eng.sample_side(me, ot, 3, 0.0, mu, LF)
    finally:
        eng.close()
        hip.hipFree(d_rows); hip.hipFree(d_vals)


_COMM_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bpmf_amd
eng = bpmf_amd.HipEngine(8)
eng.comm_init(1, 0, eng.comm_unique_id())
side = eng.side_create(2, 4, np.array([0, 4, 6], np.int64), np.array([0, 1, 2, 3, 0, 2], np.int32), np.array([2., 3., 7., 4., 5., 1.]), 3.0)
try:
    eng.set_censored(side, np.array([1, 0, 0, 0, -1, 0], np.int8), 5)
    print("ACCEPTED")
except bpmf_amd.BpmfHipError as e:
    print("REFUSED %d %s" % (e.code, e))
eng.close()
"""


def test_set_censored_refuses_a_context_with_a_communicator():
    """The other branch of the single-GPU check: a whole side on a context that has a communicator (one rank, as `bpmf -g 1`
    makes one).  In a process of its own: a communicator is process-wide state of the communication library."""
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("BPMF_HIP_RCCL_LIBRARY", None)
    r = subprocess.run([sys.executable, "-c", _COMM_CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert re.search(r"^REFUSED -1 .*side_set_censored: .*communicator", r.stdout, re.M), r.stdout


# ---- 7. lifetime --------------------------------------------------------------------------------------------------------------------

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
        fm = np.zeros(len(M[2]), np.int8); fm[0], fm[-1] = 1, -1
        fu = np.zeros(len(Mt[2]), np.int8); fu[1] = 1
        # a refused call that had its arrays half built leaves nothing
        wrong = fm.copy(); wrong[-1] = 3
        with pytest.raises(bpmf_amd.BpmfHipError, match="not one of"):
            eng.set_censored(movies, wrong, 5)
        assert live() == before
        eng.set_censored(movies, fm, 5)
        assert live() - before == len(fm) * 8 + 2 * (8 + 4 + 4 + 1)      # z; position, column, row, sign of two entries
        eng.set_censored(users, fu, 6)
        held = live()
        for _ in range(2):
            eng.sys_sample(movies, users, 2.0)
            eng.sys_sample(users, movies, 2.0)
        eng.sync()
        assert live() == held
        eng.side_destroy(movies)
        assert before - len(fu) * 8 < live() < held
        eng.side_destroy(users)
        assert live() == before
    finally:
        eng.close()
    assert live() == base


# ---- 8. planted experiment ----------------------------------------------------------------------------------------------------------

def test_planted_bounds_are_honoured(oracle):
    """600 x 300, rank 4, noise variance 1/4 (alpha = 4), 40 training cells per user; every training value above the 70th percentile
    q is recorded as the lower bound q.  Restated CPU chains, scored by the posterior-mean prediction on the test cells whose true
    value is above q | on all test cells (censor_ref.PLANTED_MEASURED):
        (a) flags honoured                 0.8178 | 0.6577
        (b) bounds taken as measurements   1.7018 | 1.1087
        (c) censored cells dropped         1.4404 | 0.9783
    Asserted in the restatement: (a) beats (b) above q by at least half the measured margin (0.442); and the GPU chain (a) is the
    restated chain (a) at the chain bars."""
    import bpmf_amd
    P = ref.PLANTED
    d = ref.planted_data(**P)
    assert d["ncens"] == 7200 and len(d["T"][2]) == P["ntest"]
    a = ref.restate_chain(oracle, P["K"], d["M"], d["Mt"], d["T"], d["C"], P["nsims"], P["burnin"], P["alpha"])
    b = ref.restate_chain(oracle, P["K"], d["M"], d["Mt"], d["T"], None, P["nsims"], P["burnin"], P["alpha"])
    c = ref.restate_chain(oracle, P["K"], d["Md"], d["Mdt"], d["T"], None, P["nsims"], P["burnin"], P["alpha"])
    sa, sb, sc = (ref.planted_scores(r["pred"], d["T"][2], d["above"]) for r in (a, b, c))
    print("RMSE above q | all: (a) %.4f | %.4f  (b) %.4f | %.4f  (c) %.4f | %.4f" % (sa + sb + sc))
    assert sb[0] - sa[0] >= ref.PLANTED_HALF_MARGIN and sa[1] < sb[1]
    eng = bpmf_amd.HipEngine(P["K"])
    try:
        res = bpmf_amd.gibbs(eng, d["M"], d["Mt"], d["T"], P["nusers"], P["nmovies"], nsims=P["nsims"], burnin=P["burnin"], Tt=d["Tt"],
                             pipelined=True, alpha=P["alpha"], censored=d["C"])
    finally:
        eng.close()
    _check_chain(res, a, "planted (a)")


# ---- 9. the executable --------------------------------------------------------------------------------------------------------------

def _mask(stdout):
    """stdout without what differs between two runs of the same command: the pid and the rates of the iteration lines"""
    out = re.sub(r"^pid: \d+$", "pid: *", stdout, flags=re.M)
    out = re.sub(r"items/sec: .*$", "items/sec: *", out, flags=re.M)
    return re.sub(r"^(Total time|Average items/sec|Average ratings/sec): .*$", r"\1: *", out, flags=re.M)


def test_cli_censored_end_to_end(tmp_path, oracle):
    import scipy.sparse as sp
    from bpmf_amd import io as bio
    rng = np.random.default_rng(78)
    nu, nm, n = 300, 200, 14000
    cells = rng.permutation(nu * nm)[:n]
    r, c = cells // nm, cells % nm
    Ut, Vt = rng.standard_normal((nu, 2)), rng.standard_normal((nm, 2))
    y = np.einsum("ij,ij->i", Ut[r], Vt[c]) + 0.5 * rng.standard_normal(n)
    tr, te = np.arange(n) < 12500, np.arange(n) >= 12500
    hi, lo = np.percentile(y[tr], 80), np.percentile(y[tr], 10)
    flag = np.where(tr & (y > hi), 1.0, np.where(tr & (y < lo), -1.0, 0.0))
    rec = np.round(np.where(flag > 0, hi, np.where(flag < 0, lo, y)), 3)            # (%g below writes six significant digits)
    rec[rec == 0.0] = 0.001
    _write_mtx(tmp_path / "train.mtx", nu, nm, r[tr], c[tr], rec[tr])
    _write_mtx(tmp_path / "test.mtx", nu, nm, r[te], c[te], rec[te])
    cen = flag != 0
    Cm = util.csc_arrays(sp.coo_matrix((flag[cen], (r[cen], c[cen])), shape=(nu, nm)))
    bio.write_sparse(tmp_path / "C.sdm", nu, nm, Cm)

    def csc(sel):
        m = sp.coo_matrix((rec[sel] + 100.0, (r[sel], c[sel])), shape=(nu, nm)).tocsc()
        A, At = util.csc_arrays(m), util.csc_arrays(m.T)
        return (A[0], A[1], A[2] - 100.0), (At[0], At[1], At[2] - 100.0)
    (M, Mt), (T, Tt) = csc(tr), csc(te)
    want = ref.restate_chain(oracle, 16, M, Mt, T, Cm, 6, 2, 3.0)
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    base = [exe, "-n", str(tmp_path / "train.mtx"), "-p", str(tmp_path / "test.mtx"), "-a", "3", "-i", "6", "-b", "2", "-d", "16"]
    (tmp_path / "o").mkdir(); (tmp_path / "p").mkdir()

    def run(extra):
        return subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    plain_before = run(["-o", str(tmp_path / "p")])
    plain_want = ref.restate_chain(oracle, 16, M, Mt, T, None, 6, 2, 3.0)
    runs = [run(["--censored", str(tmp_path / "C.sdm"), "-v", "-o", str(tmp_path / "o")]),     # -o: the plain loop
            run(["--censored", str(tmp_path / "C.sdm")])]                                # without: the pipelined one
    plain_after = run(["-o", str(tmp_path / "p")])
    for out in runs:
        assert out.returncode == 0, out.stderr
        head = re.search(r"^censored: (\d+) lower bounds, (\d+) upper bounds of (\d+) training ratings$", out.stdout, re.M)
        assert head, out.stdout
        assert tuple(int(x) for x in head.groups()) == (int((flag > 0).sum()), int((flag < 0).sum()), int(tr.sum()))
        assert re.search(r"^alpha: 3$", out.stdout, re.M)
        lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", out.stdout)
        assert len(lines) == 6
        got = np.array([[float(a), float(b)] for a, b in lines])
        # (the lines print four decimals and the final line six significant digits: the 1e-6 of the chain tests on top of half a
        #  unit of the print)
        assert np.abs(got[:, 0] - want["rmse"]).max() <= 1e-6 + 5e-5 and np.abs(got[:, 1] - want["rmse_avg"]).max() <= 1e-6 + 5e-5
        final = re.search(r"^Final Avg RMSE: (\S+)$", out.stdout, re.M)
        assert final and want["final_rmse_avg"] < 10.0 and abs(float(final.group(1)) - want["final_rmse_avg"]) <= 1e-6 + 5e-6
        # ... and the printed lines are those of the censored chain, not of the chain that takes the bounds for measurements
        assert np.abs(got[:, 0] - plain_want["rmse"]).max() > 1e-2
    for name in ("U-mu.ddm", "U-Lambda.ddm", "V-mu.ddm", "V-Lambda.ddm", "Pavg.sdm", "Pm2.sdm", "U-5.ddm", "V-5.ddm"):
        assert (tmp_path / "o" / name).exists(), sorted(p.name for p in (tmp_path / "o").iterdir())
    # the last sample (-v) at the bar of the chain tests: sharper than the four printed decimals
    U, V = bio.read_dense(tmp_path / "o" / "U-5.ddm").T, bio.read_dense(tmp_path / "o" / "V-5.ddm").T
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(U - want["U"]).max() / scale, np.abs(V - want["V"]).max() / scale
    print("bpmf --censored: U %.3g V %.3g of max|U|" % (eu, ev))
    assert eu < 1e-6 and ev < 1e-6, (eu, ev)
    # without the flag: the same stdout before and after, and no censoring line
    assert plain_before.returncode == 0 and plain_after.returncode == 0, plain_before.stderr + plain_after.stderr
    assert _mask(plain_before.stdout) == _mask(plain_after.stdout) and "censored" not in plain_before.stdout
    assert _mask(plain_before.stdout) != _mask(runs[0].stdout)


def test_cli_censored_flags_follow_the_renumbering(tmp_path, oracle):
    """BPMF_TEST_ASSIGN_PARTS=3 renumbers rows and columns as for three ranks and runs on one GPU without -g: the chain is the
    restated chain on the renumbered ratings WITH the renumbered censoring matrix (tests/test_assign.py does the same for the
    ratings alone)."""
    import scipy.sparse as sp
    from bpmf_amd import io as bio
    from tests.test_assign import greedy
    K, parts, nsims, burnin = 8, 3, 6, 2
    M, Mt, T, Tt, nu, nm = util.ml100k()
    Cm = ref.ml100k_censoring(M)
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
    Mp, Tp, Cp = renum(M), renum(T), renum(Cm)
    Mpt = util.csc_arrays(sp.csc_matrix((Mp[2], Mp[1], Mp[0]), shape=(nu, nm)).T)
    want = ref.restate_chain(oracle, K, Mp, Mpt, Tp, Cp, nsims, burnin, 2.0)
    bio.write_sparse(tmp_path / "C.sdm", nu, nm, Cm)
    exe = os.path.join(ROOT, "bpmf_amd", "bpmf")
    (tmp_path / "o").mkdir()
    out = subprocess.run([exe, "-i", str(nsims), "-b", str(burnin), "-d", str(K), "-v", "-o", "o/", "-n", os.path.join(util.GOLDEN, "ml100k-train.mtx.gz"),
                          "-p", os.path.join(util.GOLDEN, "ml100k-test.mtx.gz"), "--censored", str(tmp_path / "C.sdm")], cwd=tmp_path,
                         env=dict(os.environ, BPMF_TEST_ASSIGN_PARTS=str(parts)), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "assignment: greedy" in out.stdout
    assert re.search(r"^censored: %d lower bounds, %d upper bounds of %d training ratings$" % (want["censored"] + (len(M[2]),)), out.stdout, re.M)
    lines = re.findall(r"iteration \d+:\t RMSE: (\S+)\tavg RMSE: (\S+)\tFU\(", out.stdout)
    got = np.array([[float(a), float(b)] for a, b in lines])
    assert got.shape == (nsims, 2)
    assert np.abs(got[:, 0] - want["rmse"]).max() <= 1e-6 + 5e-5 and np.abs(got[:, 1] - want["rmse_avg"]).max() <= 1e-6 + 5e-5
    final = re.search(r"^Final Avg RMSE: (\S+)$", out.stdout, re.M)
    assert final and abs(float(final.group(1)) - want["final_rmse_avg"]) <= 1e-6 + 5e-6
    # the last sample, written in the ORIGINAL numbering: row pu[j] of the file = row j of the renumbered chain's factor.  (Six
    # iterations from zero factors are still near the saddle, where the four printed decimals of the RMSE say little: the factors
    # are the check that every flag sits on its rating.)
    U = bio.read_dense(tmp_path / "o" / ("U-%d.ddm" % (nsims - 1))).T; V = bio.read_dense(tmp_path / "o" / ("V-%d.ddm" % (nsims - 1))).T
    scale = max(np.abs(want["U"]).max(), np.abs(want["V"]).max())
    eu, ev = np.abs(U[pu] - want["U"]).max() / scale, np.abs(V[pm] - want["V"]).max() / scale
    plain = ref.restate_chain(oracle, K, Mp, Mpt, Tp, None, nsims, burnin, 2.0)
    away = np.abs(plain["U"] - want["U"]).max() / scale
    print("renumbered: U %.3g V %.3g; the chain without the flags is %.3g away" % (eu, ev, away))
    assert eu < 1e-6 and ev < 1e-6 and away > 1e-2


# ---- 10. the fixed path is untouched ------------------------------------------------------------------------------------------------

def test_fixed_path_is_untouched_by_a_censored_run():
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.tiny()
    Cm = (np.array([0, 2, 3], np.int64), np.array([0, 2, 0], np.int32), np.array([1.0, -1.0, 1.0]))   # (1, 1), (3, 1), (1, 2) of tiny-train.mtx
    assert not ref.flags_of(M, Cm).all() and ref.flags_of(M, Cm).any()
    eng = bpmf_amd.HipEngine(16)
    try:
        before = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
        cs = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True, censored=Cm)
        after = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=6, burnin=2, Tt=Tt, pipelined=True)
    finally:
        eng.close()
    assert before["U"].tobytes() == after["U"].tobytes() and before["V"].tobytes() == after["V"].tobytes()
    assert before["rmse"] == after["rmse"] and before["rmse_avg"] == after["rmse_avg"]
    assert "censored" not in before and "censored" not in after and cs["censored"] == (2, 1)
    assert not np.array_equal(cs["U"], before["U"])
