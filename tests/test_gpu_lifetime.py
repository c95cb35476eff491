"""Ownership of the device memory of a side's add-ons (probit, side information, sample ring, training residuals):
bpmf_hip_live_device_bytes counts what they hold, so what an entry point allocates and what a destroy or a refused call leaves
behind can be stated in bytes.  (hipMemGetInfo counts the whole card, other processes included.)  The core state of a context, a
side and a test set (blobs, ratings, factors, schedules, aggregates, priors, test entries) is counted on its own by
bpmf_hip_live_core_bytes: the second half of this file.

Shapes: 48 users x 40 movies, about 300 ratings; K = 8 (a kernel size) and K = 20 (runs padded to 32)."""
import numpy as np
import pytest
import scipy.sparse as sp

import bpmf_amd
import util

pytestmark = pytest.mark.gpu

NU, NM = 48, 40


def live():
    return int(bpmf_amd.load_library().bpmf_hip_live_device_bytes())


def core():
    return int(bpmf_amd.load_library().bpmf_hip_live_core_bytes())


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(5)
    at = rng.choice(NU * NM, size=330, replace=False)
    vals = rng.integers(1, 6, size=len(at)).astype(np.float64)
    held = np.arange(len(at)) < 30
    A = sp.coo_matrix((vals[~held], (at[~held] // NM, at[~held] % NM)), shape=(NU, NM)).tocsc()       # users x movies: a column per movie
    T = sp.coo_matrix((vals[held], (at[held] // NM, at[held] % NM)), shape=(NU, NM)).tocsc()
    Fm = rng.standard_normal((NM, 5))
    Fu = sp.random(NU, 70, density=0.1, random_state=7, format="csr")
    Fu.sort_indices()
    return dict(M=util.csc_arrays(A), Mt=util.csc_arrays(A.T), T=util.csc_arrays(T), Tt=util.csc_arrays(T.T), Fm=Fm, Fu=Fu)


def attach_everything(eng, d):
    """model A: probit on both sides, predictive sums, training residuals; model B: dense and sparse features, rings, a ranking"""
    movies = eng.side_create(NM, NU, *d["M"], 0.0)
    users = eng.side_create(NU, NM, *d["Mt"], 0.0)
    eng.set_probit(movies, 3.0, 1)
    eng.set_probit(users, 3.0, 2)
    test = eng.test_create(movies, *d["T"])
    eng.sys_sample(movies, users, 1.0)
    eng.sys_sample(users, movies, 1.0)
    eng.probit_add(test, movies, users)
    sse, n = eng.train_sse(movies, users)
    assert n == d["M"][0][-1] and np.isfinite(sse)
    prob, k = eng.probit_get(test)
    assert k == 1 and np.all((prob >= 0.0) & (prob <= 1.0))

    movies2 = eng.side_create(NM, NU, *d["M"], 0.0)
    users2 = eng.side_create(NU, NM, *d["Mt"], 0.0)
    eng.set_features(movies2, d["Fm"], 5.0, 3)
    eng.set_features(users2, d["Fu"], 5.0, 4)
    for _ in range(3):
        eng.link_sample(movies2, users2, 2.0)
        eng.link_sample(users2, movies2, 2.0)
    for s in (movies2, users2):
        eng.link_add(s)
        eng.samples_reserve(s, 4)
        eng.samples_add(s)
    assert eng.link_cg_stats(users2)["iters_total"] > 0
    idx, mean, std = eng.topn(users2, movies2, 3.0, 5, exclude_rated=True)
    assert idx.shape == (NU, 5) and np.all(np.isfinite(mean))
    return [movies, users, movies2, users2]


@pytest.mark.parametrize("K", [8, 20])
@pytest.mark.parametrize("one_by_one", [False, True])
def test_everything_attached_then_closed(data, K, one_by_one):
    base = live()
    eng = bpmf_amd.HipEngine(K)
    try:
        sides = attach_everything(eng, data)
        assert live() > base
        if one_by_one:
            held = live()
            for s in sides:
                eng.side_destroy(s)
                assert live() < held
                held = live()
            assert held == base
    finally:
        eng.close()
    assert live() == base


@pytest.mark.parametrize("K", [8, 20])
def test_refused_attach_leaves_nothing(data, K):
    eng = bpmf_amd.HipEngine(K)
    try:
        users = eng.side_create(NU, NM, *data["Mt"], 0.0)
        Fd = np.asarray(data["Fu"].todense())[:, :6].copy()
        bad = Fd.copy(); bad[5, 1] = np.inf
        unsorted = data["Fu"].copy()
        row = int(np.argmax(np.diff(unsorted.indptr)))                 # a row with at least two entries, first two swapped
        p = unsorted.indptr[row]
        assert unsorted.indptr[row + 1] - p >= 2
        unsorted.indices[[p, p + 1]] = unsorted.indices[[p + 1, p]]
        rowptr, colidx, vals = (np.ascontiguousarray(unsorted.indptr, np.int64), np.ascontiguousarray(unsorted.indices, np.int32),
                                np.ascontiguousarray(unsorted.data, np.float64))
        lib = eng.lib

        def unsorted_csr():
            bpmf_amd._lib.check(lib.bpmf_hip_side_set_features_sparse(users.handle, 70, rowptr.ctypes.data, colidx.ctypes.data,
                                                                      vals.ctypes.data, 5.0, 4))
        before = live()
        for refused in (lambda: eng.set_features(users, bad),                      # infinite feature
                        lambda: eng.set_features(users, Fd, 0.0),                  # lambda_beta = 0
                        lambda: eng.set_features(users, Fd, 5.0, 0),               # tag 0
                        lambda: eng.set_features(users, np.zeros((NU, 1025))),     # D = 1025
                        unsorted_csr):
            with pytest.raises(bpmf_amd.BpmfHipError) as e:
                refused()
            assert e.value.code == -1, str(e.value)
            assert live() == before
        eng.set_features(users, Fd, 5.0, 4)
        assert live() > before
        beta, offs = eng.link_get(users)
        assert beta.shape == (6, K) and offs.shape == (NU, K)
        assert not beta.any() and not offs.any()
    finally:
        eng.close()


@pytest.mark.parametrize("K", [8, 20])
def test_ring_reserve_and_release(data, K):
    kp = (K + 3) // 4 * 4
    eng = bpmf_amd.HipEngine(K)
    try:
        movies = eng.side_create(NM, NU, *data["M"], 3.0)
        before = live()
        eng.samples_reserve(movies, 4)
        assert live() - before == NM * 4 * kp * 8
        eng.samples_reserve(movies, 0)
        assert live() == before
        eng.samples_reserve(movies, 4)
        eng.samples_reserve(movies, 7)                                  # another size: a new ring in place of the old one
        assert live() - before == NM * 7 * kp * 8
        eng.samples_reserve(movies, 0)
        assert live() == before
    finally:
        eng.close()


@pytest.mark.parametrize("K", [8, 20])
def test_colptr_is_shared(data, K):
    nnz = int(data["M"][0][-1])
    nblk = (nnz + 255) // 256                                           # train_sse_blocks: its cap of 16 blocks per CU is far away
    eng = bpmf_amd.HipEngine(K)
    try:
        movies = eng.side_create(NM, NU, *data["M"], 0.0)
        users = eng.side_create(NU, NM, *data["Mt"], 0.0)
        before = live()
        eng.train_sse(movies, users)
        eng.set_probit(movies, 3.0, 1)
        others = nnz * 8 + max(nnz, 1) + (nblk + 1) * 8                 # z, sign, the partials | sum
        assert live() - before == others + (NM + 1) * 8                 # ... and the column pointers once
    finally:
        eng.close()


# ---- the core state: bpmf_hip_live_core_bytes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,dtype", [(8, "f64"), (20, "f64"), (65, "f32")])
def test_core_state_returns_to_base(data, K, dtype):
    """Everything the core state can hold at once -- the lazily built state of the stateful path, a test set with its twin and
    evaluations in flight, posterior aggregates, a propagated posterior, the BPMF_REDUCE storage of a second pair (fp64 only: the
    fp32 context refuses it) -- goes with the handle that holds it, and none of it is an add-on."""
    base, addons = core(), live()
    eng = bpmf_amd.HipEngine(K, dtype=dtype)
    try:
        assert core() > base and live() == addons                      # the context's blobs
        movies = eng.side_create(NM, NU, *data["M"], 3.0)
        users = eng.side_create(NU, NM, *data["Mt"], 3.0)
        assert live() == addons
        test = eng.test_create(movies, *data["T"])
        twin = eng.test_create(users, *data["Tt"])
        eng.test_set_twin(test, twin)
        assert live() == addons
        for i in range(3):                                             # the pipelined loop: the line of i - 1 is collected behind iteration i
            eng.sys_sample(movies, users, 2.0)
            eng.sys_sample(users, movies, 2.0)
            if i > 0:
                assert eng.predict_finish(test)[2] == 30 and eng.predict_finish(twin)[2] == 30
            eng.predict_launch(test, movies, users, i)
            assert live() == addons
        assert eng.predict_finish(test)[2] == 30 and eng.predict_finish(twin)[2] == 30
        eng.aggr_add(movies)
        eng.aggr_add(users)
        assert live() == addons
        eng.set_prop_posterior(users, np.tile(np.eye(K).ravel(order="F"), (NU, 1)))
        assert live() == addons
        sides = [movies, users]
        if dtype == "f64":
            sides += [eng.side_create(NM, NU, *data["M"], 3.0), eng.side_create(NU, NM, *data["Mt"], 3.0)]
            eng.sys_set_reduce(sides[2], sides[3])
            assert live() == addons
        eng.sync()
        assert live() == addons
        held = core()
        for t in (twin, test):
            eng.test_destroy(t)
            assert core() < held and live() == addons
            held = core()
        for s in sides:
            eng.side_destroy(s)
            assert core() < held and live() == addons
            held = core()
    finally:
        eng.close()
    assert core() == base and live() == addons


_BIND_CHILD = """
import sys
import torch                                                           # (first: the library then runs on the HIP runtime torch brought)
import numpy as np
sys.path.insert(0, sys.argv[1])
import bpmf_amd
NU, NM = 48, 40
lib = bpmf_amd.load_library()
core, live = lib.bpmf_hip_live_core_bytes, lib.bpmf_hip_live_device_bytes
rng = np.random.default_rng(5)
rows = np.stack([np.sort(rng.choice(NU, size=7, replace=False)) for _ in range(NM)])      # 7 ratings per movie
colptr = np.arange(NM + 1, dtype=np.int64) * 7
M = (colptr, np.ascontiguousarray(rows.ravel(), np.int32), rng.integers(1, 6, size=NM * 7).astype(np.float64))
for K in (8, 20):
    base = core()
    eng = bpmf_amd.HipEngine(K)
    movies = eng.side_create(NM, NU, *M, 3.0)
    ld = eng.ld()
    assert ld == (8 if K == 8 else 32)
    addons, before = live(), core()
    buf = torch.full((NM, ld), 0.25, dtype=torch.float64, device="cuda:0")
    eng.bind_items(movies, buf.data_ptr(), keep=buf, ld=ld, nbytes=buf.numel() * 8)
    assert before - core() == 2 * ld * NM * 8, (K, before - core())
    assert live() == addons
    held = core()
    eng.side_destroy(movies)
    assert core() < held and live() == addons
    torch.cuda.synchronize()
    assert bool((buf.cpu() == 0.25).all())                             # the caller's storage was not freed with the side
    assert live() == addons
    eng.close()
    assert core() == base
    print("BOUND K=%d" % K)
"""


def test_bind_items_releases_the_two_factor_copies():
    """The caller's buffer is a torch tensor, so this runs in a process of its own, which imports torch ahead of the library."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("BPMF_HIP_DBUF", None)                                     # (the default: a side keeps two copies of its factors)
    r = subprocess.run([sys.executable, "-c", _BIND_CHILD, root], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "BOUND K=8" in r.stdout and "BOUND K=20" in r.stdout, r.stdout


@pytest.mark.parametrize("K", [8, 20])
def test_prop_posterior_is_exact_in_both_directions(data, K):
    eng = bpmf_amd.HipEngine(K)
    try:
        users = eng.side_create(NU, NM, *data["Mt"], 3.0)
        ld = eng.ld()
        addons, before = live(), core()
        eng.set_prop_posterior(users, np.tile(np.eye(K).ravel(order="F"), (NU, 1)))
        assert core() - before == ld * ld * NU * 8 and live() == addons
        eng.set_prop_posterior(users, None)
        assert core() == before and live() == addons
    finally:
        eng.close()


@pytest.mark.parametrize("K", [8, 20])
def test_aggr_finalize_returns_what_aggr_add_took(data, K):
    eng = bpmf_amd.HipEngine(K)
    try:
        movies = eng.side_create(NM, NU, *data["M"], 3.0)
        users = eng.side_create(NU, NM, *data["Mt"], 3.0)
        for _ in range(3):
            eng.sys_sample(movies, users, 2.0)
            eng.sys_sample(users, movies, 2.0)
        eng.sync()
        addons, before = live(), core()                                # (behind the first sys_sample: it builds core state of its own)
        eng.aggr_add(movies)
        assert core() - before == (K + K * K) * NM * 8                 # aggrMu, aggrLambda: the caller's num_latent
        assert live() == addons
        eng.aggr_add(movies)
        assert core() - before == (K + K * K) * NM * 8 and live() == addons
        mu, lam = eng.aggr_finalize(movies, 2)
        assert mu.shape == (NM, K) and lam.shape == (NM, K * K)
        assert core() == before and live() == addons
    finally:
        eng.close()


@pytest.mark.parametrize("K", [8, 20])
def test_create_dev_borrows_the_ratings(data, K):
    from tests.test_gpu_probit import _from_device, _hip_runtime, _to_device
    colptr, rowidx, vals = data["M"]
    nnz = int(colptr[-1])
    hip = _hip_runtime()
    d_rows, d_vals = _to_device(hip, rowidx), _to_device(hip, vals)
    eng = bpmf_amd.HipEngine(K)
    try:
        addons, c0 = live(), core()
        own = eng.side_create(NM, NU, colptr, rowidx, vals, 3.0)
        c1 = core()
        assert live() == addons
        lent = eng.side_create_dev(NM, NU, colptr, d_rows.value, d_vals.value, 3.0)
        c2 = core()
        assert live() == addons
        assert (c1 - c0) - (c2 - c1) == nnz * (4 + 8)                  # the same side but for its copies of rowidx and vals
        eng.side_destroy(lent)
        assert core() == c1 and live() == addons
        assert np.array_equal(_from_device(hip, d_rows, rowidx), rowidx) and np.array_equal(_from_device(hip, d_vals, vals), vals)
        eng.side_destroy(own)
        assert core() == c0 and live() == addons
    finally:
        eng.close()
        hip.hipFree(d_rows); hip.hipFree(d_vals)
