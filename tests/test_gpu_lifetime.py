"""Ownership of the device memory of a side's add-ons (probit, side information, sample ring, training residuals):
bpmf_hip_live_device_bytes counts what they hold, so what an entry point allocates and what a destroy or a refused call leaves
behind can be stated in bytes.  (hipMemGetInfo counts the whole card, other processes included.)

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
    return dict(M=util.csc_arrays(A), Mt=util.csc_arrays(A.T), T=util.csc_arrays(T), Fm=Fm, Fu=Fu)


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
