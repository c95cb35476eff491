"""Parity of the HIP path (through the C ABI) against the CPU oracle on identical
seeds.  fp64 tolerance: the sampled factors must agree to RTOL = 1e-9 of the
largest factor entry after one half-iteration (differences come from the
summation order of the Gram, 1/sqrt vs divide, and log/sqrt ulps), and RMSE
traces of whole runs to 1e-6 (north-star bar: 1e-3)."""
import math

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

RTOL = 1e-9


@pytest.fixture(params=[None, 1, 3], ids=["auto", "per-item", "four-columns"])
def sampler_mode(request):
    """The two shipped forms of the K <= 32 sampler (BPMF_HIP_MODE, read when a side is created): 1 = one work item per
    single-wave workgroup (k_sample1: what a side with < 20 000 columns runs), 3 = four columns per wave with the factorisation
    on the 4x4x4 MFMA shape (k_sample4: what a bigger side runs).  `auto` picks by size, so the small matrices of these tests
    reach k_sample4 only when it is forced.  K = 64 (slab form + product form) and K = 128 (workgroup form) have one form each:
    the switch does nothing there, and the forced runs check that they still give the oracle's numbers.  (Rounds 1-4 kept seven more forms behind this switch:
    docs/FINDINGS.md.)"""
    import os
    old = os.environ.get("BPMF_HIP_MODE")
    if request.param is None:
        os.environ.pop("BPMF_HIP_MODE", None)
    else:
        os.environ["BPMF_HIP_MODE"] = str(request.param)
    yield request.param
    if old is None:
        os.environ.pop("BPMF_HIP_MODE", None)
    else:
        os.environ["BPMF_HIP_MODE"] = old


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def half_iteration_pair(oracle, eng, K, M, nrows, other_items, it, alpha=2.0, cov=None, chunk_note=""):
    """Runs one Sys::sample(Sys&) on both sides of the fence; returns (hip, ref) tuples."""
    ncols = len(M[0]) - 1
    cov = np.zeros((K, K)) if cov is None else cov
    mu, LU, LF = oracle.hyper_sample(K, ncols, cov, it)
    mean = util.mean_rating(M)
    items_ref = np.zeros((ncols, K))
    s_ref, p_ref, n_ref = oracle.sample_side(K, M, mean, alpha, other_items, items_ref, it, mu, LF)
    me = eng.side_create(ncols, nrows, *M, mean)
    ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_items(ot, other_items)
    s, p, n = eng.sample_side(me, ot, it, alpha, mu, LF)
    items = eng.get_items(me)
    eng.side_destroy(me); eng.side_destroy(ot)
    return (items, s, p, n), (items_ref, s_ref, p_ref, n_ref)


def check_half_iteration(hip, ref):
    items, s, p, n = hip
    items_ref, s_ref, p_ref, n_ref = ref
    assert np.all(np.isfinite(items))
    assert rel_err(items, items_ref) < RTOL
    assert rel_err(s, s_ref) < 1e-8 and rel_err(p, p_ref) < 1e-8 and abs(n - n_ref) <= 1e-8 * abs(n_ref)


@pytest.mark.parametrize("counter", [0, 1, 32, 8 * 5 * 9, 2 ** 32 - 1, 1234567])
def test_device_normal_stream(oracle, hip_engine_factory, counter):
    """draw_normals (ballot-ranked polar attempts) == the sequential stream of randn()."""
    eng = hip_engine_factory(32)
    for n in (1, 8, 32, 64, 128):
        z = eng.randn_device(counter, n)
        ref = oracle.randn(counter, n)
        # identical accept/reject decisions; log/sqrt may differ in the last ulps
        assert np.allclose(z, ref, rtol=4e-16 * 8, atol=0), (counter, n)


@pytest.mark.parametrize("K", [8, 16, 32, 64])
def test_tiny_first_half_iterations(oracle, hip_engine_factory, K, sampler_mode):
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = hip_engine_factory(K)
    rng = np.random.default_rng(K)
    # iteration 0: factors are zero (Sys::init); then with random factors
    for it, U in ((0, np.zeros((nu, K))), (3, rng.standard_normal((nu, K)))):
        check_half_iteration(*half_iteration_pair(oracle, eng, K, M, nu, U, it))
    V = rng.standard_normal((nm, K))
    check_half_iteration(*half_iteration_pair(oracle, eng, K, Mt, nm, V, 2))


def test_low_rank_columns(oracle, hip_engine_factory, monkeypatch):
    """K = 64, a ChEMBL-shaped side (thousands of columns with 0..16 ratings, a few heavy ones): the light columns take the
    product form over the shared factor of LambdaF (k_pf_prepare + k_sample_pf<64, 3 | 6 | 16>: same Cholesky factor, hence
    the reference's sample for the same normals) instead of factorising Lambda*.  Class sizes that are not multiples of four
    (ragged last pass of every class), several launches on the same side; against the oracle every time, and against the
    regular path (BPMF_HIP_PF=0: every column in the slab form)."""
    K = 64
    rng = np.random.default_rng(641)
    nrows = 400
    counts = np.concatenate([np.full(301, 0), np.full(203, 1), np.full(97, 2), np.full(250, 3),                  # 851 = 3 mod 4
                             np.full(333, 4), np.full(334, 5), np.full(335, 6)] +                               # 1 002 = 2 mod 4
                            [np.full(33, n) for n in range(7, 17)] +                                            # 330 = 2 mod 4
                            [np.full(9, 30), np.full(3, 300)])          # (300 ratings: a chunked column of the slab form)
    rng.shuffle(counts)
    ncols = len(counts)
    colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rowidx = np.concatenate([np.sort(rng.choice(nrows, size=c, replace=False)) for c in counts]).astype(np.int32)
    vals = rng.normal(5.0, 1.1, size=len(rowidx))
    M = (colptr, rowidx, vals)
    mean = util.mean_rating(M)
    eng = hip_engine_factory(K)
    A = rng.standard_normal((K, 3 * K)); cov = A @ A.T / (3 * K)

    def run(pf):
        if pf is None:
            monkeypatch.delenv("BPMF_HIP_PF", raising=False)
        else:
            monkeypatch.setenv("BPMF_HIP_PF", pf)
        me = eng.side_create(ncols, nrows, *M, mean)
        ot = eng.side_create(nrows, ncols, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
        name = eng.kernel_name(me)
        info = eng.schedule_info(me)
        out = []
        r = np.random.default_rng(7)
        for it in range(3):
            U = (0.3 + 0.05 * it) * r.standard_normal((nrows, K))
            mu, LU, LF = oracle.hyper_sample(K, ncols, cov * (1.0 + it), it)
            eng.set_items(ot, U)
            s, p, n = eng.sample_side(me, ot, it, 2.0, mu, LF)
            out.append((eng.get_items(me).copy(), s, p, n, U, mu, LF))
        eng.side_destroy(me); eng.side_destroy(ot)
        return out, name, info

    pf, name, info = run(None)
    assert name == "k_sample_pf<64,3> + k_sample_pf<64,6> + k_sample_pf<64,16> + k_sample_slab<64>", name
    assert (info["pf_le3"], info["pf_4to6"], info["pf_7to16"], info["lr_columns"]) == (851, 1002, 330, 0)
    for it, (items, s, p, n, U, mu, LF) in enumerate(pf):
        ref = np.zeros((ncols, K))
        s_ref, p_ref, n_ref = oracle.sample_side(K, M, mean, 2.0, U, ref, it, mu, LF)
        check_half_iteration((items, s, p, n), (ref, s_ref, p_ref, n_ref))
    regular, name0, info0 = run("0")
    assert "k_sample_pf" not in name0 and info0["pf_le3"] == 0
    for a, b in zip(pf, regular):
        assert rel_err(a[0], b[0]) < RTOL


@pytest.mark.parametrize("K", [16, 32, 64])
def test_ml100k_half_iterations(oracle, hip_engine_factory, K, sampler_mode):
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)
    rng = np.random.default_rng(100 + K)
    U = 0.3 * rng.standard_normal((nu, K)); V = 0.3 * rng.standard_normal((nm, K))
    A = rng.standard_normal((K, 3 * K)); cov = A @ A.T / (3 * K)
    # movies side: 32 empty columns (sample from the prior), median 21 ratings
    check_half_iteration(*half_iteration_pair(oracle, eng, K, M, nu, U, 5, cov=cov))
    check_half_iteration(*half_iteration_pair(oracle, eng, K, Mt, nm, V, 7, cov=cov))


def test_heavy_column_is_chunked(oracle, hip_engine_factory, sampler_mode):
    """A column far above the chunk size is cut into chunks; the last-arriving chunk sums the
    partial tiles.  Several launches with different inputs on the same side: a stale partial
    (previous launch's tiles served from another XCD's L2) would show up as a mismatch."""
    K = 32
    M, Mt, T, Tt, nu, nm = util.synthetic(6000, 300, 60000, seed=3, heavy=(7, 5000))
    assert np.diff(M[0]).max() >= 5000
    eng = hip_engine_factory(K)
    rng = np.random.default_rng(5)
    mean = util.mean_rating(M)
    me = eng.side_create(nm, nu, *M, mean)
    ot = eng.side_create(nu, nm, np.zeros(nu + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    for it in range(4):
        U = (0.2 + 0.1 * it) * rng.standard_normal((nu, K))
        mu, LU, LF = oracle.hyper_sample(K, nm, np.eye(K) * (0.5 + it), it)
        ref = np.zeros((nm, K))
        s_ref, p_ref, n_ref = oracle.sample_side(K, M, mean, 2.0, U, ref, it, mu, LF)
        eng.set_items(ot, U)
        s, p, n = eng.sample_side(me, ot, it, 2.0, mu, LF)
        check_half_iteration((eng.get_items(me), s, p, n), (ref, s_ref, p_ref, n_ref))
    eng.side_destroy(me); eng.side_destroy(ot)


@pytest.mark.parametrize("K", [32, 64])
def test_item_order_chunks_of_heavy_columns_start_first(hip_engine_factory, K):
    """The launch order of a side's work items (what `schedule(guided)` over the columns is to c++/sample.cpp:353-356):
    every item of a chunked column is listed ahead of every whole column that is not longer than it -- the last
    arriver of a heavy column still has a chunk sum and a factorisation to do, so its chunks must not start late
    (round 3: with whole columns ahead of them ML-1M K = 64 ran 0.3645 instead of 0.3045 ms per iteration) -- the
    list is in non-increasing length, every rating is covered exactly once, and the chunks of a column are even."""
    M, Mt, T, Tt, nu, nm = util.synthetic(6000, 300, 60000, seed=3, heavy=(7, 5000))
    eng = hip_engine_factory(K)
    me = eng.side_create(nm, nu, *M, util.mean_rating(M))
    info = eng.schedule_info(me)
    col, ln, heavy = eng.schedule_items(me)
    assert len(col) == info["work_items"] and info["chunked_columns"] >= 1 and (heavy >= 0).sum() == info["chunks"]
    counts = np.diff(M[0])
    covered = np.zeros(nm, np.int64)
    np.add.at(covered, col, ln)
    assert np.array_equal(covered, counts)                            # every rating in exactly one item
    # the sort key: ratings + a small constant (32) for "everything after the Gram", shared by the chunks of a column
    nch = np.ones(len(ln), np.int64)
    for h in np.unique(heavy[heavy >= 0]):
        nch[heavy == h] = (heavy == h).sum()
    key = ln.astype(np.int64) + 32 // nch
    assert np.all(np.diff(key) <= 0)
    chunk_pos = np.nonzero(heavy >= 0)[0]
    whole_pos = np.nonzero(heavy < 0)[0]
    assert len(chunk_pos) >= 2
    for p in chunk_pos:                                               # whole columns ahead of a chunk are (almost) as long as it
        ahead = whole_pos[whole_pos < p]
        assert np.all(ln[ahead] >= ln[p] - 32)
    for h in np.unique(heavy[heavy >= 0]):
        lens = ln[heavy == h]
        assert lens.max() - lens.min() <= 16 * len(lens) and (lens == lens.max()).sum() >= len(lens) - 1   # equalised chunks (multiples of 16; the last takes the rest)
        assert len(np.unique(col[heavy == h])) == 1
    eng.side_destroy(me)


def test_ragged_and_empty(oracle, hip_engine_factory):
    """Columns with 0, 1, 2, 3, 4, 5, 15, 16, 17 ratings (MFMA k-step and unroll tails)."""
    K = 32
    counts = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 0, 64, 65]
    nrows = 80
    rng = np.random.default_rng(11)
    colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rowidx = np.concatenate([np.sort(rng.choice(nrows, c, replace=False)) for c in counts]).astype(np.int32)
    vals = rng.integers(1, 6, len(rowidx)).astype(np.float64)
    M = (colptr, rowidx, vals)
    U = rng.standard_normal((nrows, K))
    eng = hip_engine_factory(K)
    check_half_iteration(*half_iteration_pair(oracle, eng, K, M, nrows, U, 4))


def test_counter_wraps_mod_2_32(oracle, hip_engine_factory):
    """(idx+1)*K*(iter+1) is truncated to uint32: use a huge iteration number."""
    K = 8
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = hip_engine_factory(K)
    U = np.random.default_rng(0).standard_normal((nu, K))
    it = 2 ** 29 + 3
    check_half_iteration(*half_iteration_pair(oracle, eng, K, M, nu, U, it))


def test_predict_matches_oracle(oracle, hip_engine_factory):
    K = 32
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)
    rng = np.random.default_rng(9)
    U = 0.3 * rng.standard_normal((nu, K)); V = 0.3 * rng.standard_normal((nm, K))
    mean = util.mean_rating(M)
    movies = eng.side_create(nm, nu, *M, mean)
    users = eng.side_create(nu, nm, *Mt, mean)
    eng.set_items(movies, V); eng.set_items(users, U)
    test = eng.test_create(movies, *T)
    pavg = T[2].copy(); pm2 = T[2].copy()
    for n in (0, 0, 1, 2, 5):                       # Q6: n = iter - burnin, avg is overwritten at n = 0 and n = 1
        se, sea, cnt = eng.predict(test, movies, users, n)
        se_r, sea_r, cnt_r = oracle.predict(K, T, V, U, mean, n, pavg, pm2)
        assert cnt == cnt_r == 20000
        assert abs(se - se_r) < 1e-9 * se_r and abs(sea - sea_r) < 1e-9 * sea_r
        a, b = eng.test_get(test)
        assert np.allclose(a, pavg, rtol=1e-12, atol=1e-12) and np.allclose(b, pm2, rtol=1e-10, atol=1e-12)
        V = V + 0.01 * rng.standard_normal(V.shape); eng.set_items(movies, V)
    eng.side_destroy(movies); eng.side_destroy(users)


def test_full_run_tiny_reference_smoke(oracle, hip_engine_factory):
    """The reference's own (disabled) test: data/tiny, -i 9 -b 0, Final Avg RMSE < 3 (run_test.sh:14-16)."""
    import bpmf_amd
    K = 8
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = hip_engine_factory(K)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=9, burnin=0)
    ref = oracle.gibbs(K, M, Mt, T, Tt, nsims=9, burnin=0)
    assert res["final_rmse_avg"] < 3.0
    assert abs(res["final_rmse_avg"] - ref["final_rmse_avg"]) < 1e-6
    assert np.allclose(res["rmse"], ref["rmse"], atol=1e-6)
    assert rel_err(res["U"], ref["U"]) < 1e-7 and rel_err(res["V"], ref["V"]) < 1e-7


def test_full_run_ml100k_matches_oracle(oracle, hip_engine_factory, sampler_mode):
    """Default run (-i 20 -b 5, K = 32) on the shipped MovieLens-100K split: RMSE trace,
    final averaged RMSE and the sampled factors against the CPU path on identical seeds."""
    import bpmf_amd
    K = 32
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=20, burnin=5)
    ref = oracle.gibbs(K, M, Mt, T, Tt, nsims=20, burnin=5, nthreads=1)
    assert abs(res["rmse"][0] - 1.153676) < 2e-3          # iteration 0 = mean predictor
    assert np.allclose(res["rmse"], ref["rmse"], atol=1e-6)
    assert np.allclose(res["rmse_avg"], ref["rmse_avg"], atol=1e-6)
    assert abs(res["final_rmse_avg"] - ref["final_rmse_avg"]) < 1e-6
    assert 0.94 < res["final_rmse_avg"] < 0.97
    assert np.allclose(res["norm_u"], ref["norm_u"], rtol=1e-7) and np.allclose(res["norm_m"], ref["norm_m"], rtol=1e-7)
    # after 20 coupled iterations the chains are still on top of each other
    assert rel_err(res["U"], ref["U"]) < 1e-6 and rel_err(res["V"], ref["V"]) < 1e-6


def test_pipelined_predict_is_the_same_chain(hip_engine_factory):
    """predict_launch / predict_finish around the next half-iteration (the loop bench.py times)
    gives the RMSE trace and factors of the plain loop: the device runs the kernels in program order."""
    import bpmf_amd
    from bpmf_amd.sys import Sys
    K = 16
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)
    ref = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=8, burnin=3)
    Sys.nsims, Sys.burnin, Sys.alpha = 8, 3, 2.0
    movies = Sys("movs", eng, M, nm, nu, T=T)
    users = Sys("users", eng, Mt, nu, nm)
    rmse, rmse_avg = [], []
    for i in range(8):
        movies.sample(users)
        if i > 0:
            movies.predict_finish(); rmse.append(movies.rmse); rmse_avg.append(movies.rmse_avg)
        users.sample(movies)
        movies.predict_launch(users)
    movies.predict_finish(); rmse.append(movies.rmse); rmse_avg.append(movies.rmse_avg)
    assert rmse == ref["rmse"] and rmse_avg == ref["rmse_avg"]
    assert np.array_equal(users.items(), ref["U"]) or rel_err(users.items(), ref["U"]) < 1e-12
    with pytest.raises(RuntimeError):
        movies.predict_finish()                       # nothing launched


@pytest.mark.parametrize("K", [16, 32])
def test_evaluation_beside_the_samplers_is_the_same_chain(hip_engine_factory, monkeypatch, K):
    """Two copies of every factor matrix (samplers write the copy that is not current) let the
    evaluation of iteration i run beside the samplers of iteration i + 1; its launch is put off to
    the other side's next half-iteration.  Odd call orders must flush it in time: a side sampled
    twice in a row (the second launch overwrites a copy the evaluation reads), predict_finish with
    nothing in between, a raw-pointer request in mid-run (drops the second copy), a test matrix
    destroyed with its evaluation still waiting.  Everything must equal the in-place run
    (BPMF_HIP_DBUF=0) bit for bit."""
    from bpmf_amd.sys import Sys
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)

    def run(dbuf):
        monkeypatch.setenv("BPMF_HIP_DBUF", dbuf)                  # read when the sides / test matrices are created
        Sys.nsims, Sys.burnin, Sys.alpha = 9, 2, 2.0
        movies = Sys("movs", eng, M, nm, nu, T=T)
        users = Sys("users", eng, Mt, nu, nm)
        trace = []
        for i in range(9):
            movies.sample(users)
            if i == 3:
                movies.sample(users)                                # (the evaluation of iteration 2 reads the copy this writes)
            users.sample(movies)
            if i == 6:
                assert eng.items_dev_ptr(users.side)                # raw pointer: users go back to one copy
            if i > 0:
                movies.predict_finish(); trace.append((movies.rmse, movies.rmse_avg))
            movies.predict_launch(users)
            if i == 4:
                movies.predict_finish(); trace.append((movies.rmse, movies.rmse_avg))   # nothing in between
                movies.predict_launch(users)
        # leave the last evaluation waiting: destroying the test matrix must cope
        U, V = users.items().copy(), movies.items().copy()
        eng.test_destroy(movies.test); movies.test = None
        eng.side_destroy(movies.side); eng.side_destroy(users.side)
        return np.asarray(trace), U, V

    t0, U0, V0 = run("0")
    t1, U1, V1 = run("1")
    assert np.array_equal(t0, t1) and np.array_equal(U0, U1) and np.array_equal(V0, V1)


@pytest.mark.parametrize("K", [16, 32])
def test_fused_launch_is_the_same_chain(hip_engine_factory, monkeypatch, K):
    """The fused form of the stateful path (one k_sample1 launch carries its own gate + staging
    workgroup and the column statistics of the previous launch's side) against the unfused one
    (gate kernel and statistics kernel on the side's stream): same hyper-parameters, same samples,
    same norms, bit for bit -- also when the statistics find no launch to ride in (state read
    straight after a sample), when one side is sampled twice in a row, and when a stateless launch
    comes in between."""
    from bpmf_amd.sys import Sys
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)

    def run(fused):
        monkeypatch.setenv("BPMF_HIP_FUSED", fused)
        Sys.nsims, Sys.burnin, Sys.alpha = 8, 2, 2.0
        movies = Sys("movs", eng, M, nm, nu, T=T)
        users = Sys("users", eng, Mt, nu, nm)
        out = []
        for i in range(8):
            movies.sample(users)
            if i == 2:
                out.append(eng.sys_state(movies.side)[1])              # norm: needs this launch's statistics NOW
            if i == 4:
                movies.sample(users)                                    # carries its own previous statistics
            users.sample(movies)
            if i == 5:
                eng.sample_side(users.side, movies.side, 99, 2.0, np.zeros(K), np.eye(K))   # stateless launch in between
            movies.predict(users)
            out += [movies.rmse, movies.rmse_avg]
        st_m, st_u = eng.sys_state(movies.side), eng.sys_state(users.side)
        out += [st_m[1], st_u[1]]
        U, V = users.items().copy(), movies.items().copy()
        cov = np.asarray(st_u[2]).copy()
        eng.side_destroy(movies.side); eng.side_destroy(users.side)
        return np.asarray(out), U, V, cov

    a = run("0")
    b = run("1")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("pipelined", [False, True])
def test_users_predict_rides_with_movies_predict(hip_engine_factory, pipelined):
    """users.predict(movies) of the reference's loop (c++/bpmf.cpp:190): the twin evaluation (bpmf_hip_test_set_twin) runs
    with every movies.predict(users), roles swapped, its own Pavg / Pm2 (Q6's running mean included).  Same predictions
    as the movies side, entry for entry, hence the same sums; and the chain itself is untouched."""
    import scipy.sparse as sp
    from bpmf_amd.sys import Sys
    K = 16
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)
    Sys.nsims, Sys.burnin, Sys.alpha = 7, 2, 2.0
    movies = Sys("movs", eng, M, nm, nu, T=T); users = Sys("users", eng, Mt, nu, nm, T=Tt)
    movies.set_twin(users)
    plain_m = Sys("movs", eng, M, nm, nu, T=T); plain_u = Sys("users", eng, Mt, nu, nm)
    tr = []
    for i in range(7):
        movies.sample(users); users.sample(movies)
        plain_m.sample(plain_u); plain_u.sample(plain_m); plain_m.predict(plain_u)
        if pipelined:
            if i > 0:
                movies.predict_finish(); users.predict_finish()
                tr.append((movies.rmse, movies.rmse_avg, users.rmse, users.rmse_avg))
            movies.predict_launch(users)
        else:
            movies.predict(users); users.predict(movies)
            tr.append((movies.rmse, movies.rmse_avg, users.rmse, users.rmse_avg))
            assert movies.rmse == plain_m.rmse and movies.rmse_avg == plain_m.rmse_avg
    if pipelined:
        movies.predict_finish(); users.predict_finish()
        tr.append((movies.rmse, movies.rmse_avg, users.rmse, users.rmse_avg))
    tr = np.asarray(tr)
    assert len(tr) == 7 and np.all(np.isfinite(tr))
    assert np.allclose(tr[:, 0], tr[:, 2], rtol=1e-12) and np.allclose(tr[:, 1], tr[:, 3], rtol=1e-12)
    assert users.num_predict == movies.num_predict == int(T[0][-1])
    # entry for entry: Pavg / Pm2 of the users' copy are those of the movies' copy, transposed
    pm, qm = eng.test_get(movies.test); pu, qu = eng.test_get(users.test)
    A = sp.csc_matrix((np.arange(len(T[2]), dtype=np.float64) + 1.0, T[1], T[0]), shape=(nu, nm))
    At = A.T.tocsc(); At.sort_indices()
    perm = At.data.astype(np.int64) - 1                     # entry e of Tt is entry perm[e] of T
    assert np.allclose(pu, pm[perm], rtol=1e-13, atol=1e-13) and np.allclose(qu, qm[perm], rtol=1e-12, atol=1e-12)
    assert np.array_equal(movies.items(), plain_m.items()) and np.array_equal(users.items(), plain_u.items())
    for sd in (movies, users, plain_m, plain_u):
        eng.side_destroy(sd.side)


def test_twin_matching_does_not_need_sorted_columns(hip_engine_factory):
    """bpmf_hip_test_set_twin matches the entries of the two test copies with one cursor per user when both arrive in CSC order
    with ascending rows (round 6: O(n)); anything else -- here the twin's rows DESCENDING inside every column -- takes the sorting
    path.  Both give the fused evaluation the same sums, entry for entry."""
    from bpmf_amd.sys import Sys
    K = 16
    M, Mt, T, Tt, nu, nm = util.ml100k()
    cp, ri, va = Tt
    ri2, va2 = ri.copy(), va.copy()
    for c in range(len(cp) - 1):                                      # reverse every column of the users' copy
        ri2[cp[c]:cp[c + 1]] = ri[cp[c]:cp[c + 1]][::-1]; va2[cp[c]:cp[c + 1]] = va[cp[c]:cp[c + 1]][::-1]
    eng = hip_engine_factory(K)
    Sys.nsims, Sys.burnin, Sys.alpha = 5, 1, 2.0
    res = []
    for tt in (Tt, (cp, ri2, va2)):
        movies = Sys("movs", eng, M, nm, nu, T=T); users = Sys("users", eng, Mt, nu, nm, T=tt)
        movies.set_twin(users)
        tr = []
        for i in range(5):
            movies.sample(users); users.sample(movies); movies.predict(users); users.predict(movies)
            tr.append((movies.rmse, movies.rmse_avg, users.rmse, users.rmse_avg))
        pu, qu = eng.test_get(users.test)
        res.append((np.asarray(tr), pu, qu))
        for sd in (movies, users):
            eng.side_destroy(sd.side)
    (tr_a, pu_a, qu_a), (tr_b, pu_b, qu_b) = res
    assert np.array_equal(tr_a[:, :2], tr_b[:, :2]) and np.allclose(tr_a[:, 2:], tr_b[:, 2:], rtol=1e-12)
    assert np.allclose(tr_b[:, 0], tr_b[:, 2], rtol=1e-12) and np.allclose(tr_b[:, 1], tr_b[:, 3], rtol=1e-12)
    for c in range(len(cp) - 1):                                      # the reversed copy holds the same running means, reversed
        assert np.array_equal(pu_b[cp[c]:cp[c + 1]], pu_a[cp[c]:cp[c + 1]][::-1]) and np.array_equal(qu_b[cp[c]:cp[c + 1]], qu_a[cp[c]:cp[c + 1]][::-1])


def test_posterior_moments_of_one_column(hip_engine_factory):
    """Statistical check that does not involve the oracle: many draws of the same column
    (different iter => different streams) have mean Lambda*^-1 b and covariance Lambda*^-1."""
    K = 8
    rng = np.random.default_rng(2)
    nrows, nd = 40, 4000
    rows = np.sort(rng.choice(nrows, 12, replace=False)).astype(np.int32)
    vals = rng.integers(1, 6, 12).astype(np.float64)
    # nd identical columns -> nd independent draws in one call (stream depends on idx)
    colptr = (np.arange(nd + 1) * 12).astype(np.int64)
    M = (colptr, np.tile(rows, nd), np.tile(vals, nd))
    U = rng.standard_normal((nrows, K))
    A = rng.standard_normal((K, 2 * K)); LF = A @ A.T / K + np.eye(K); mu = rng.standard_normal(K)
    eng = hip_engine_factory(K)
    mean, alpha = 3.0, 2.0
    me = eng.side_create(nd, nrows, *M, mean)
    ot = eng.side_create(nrows, nd, np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_items(ot, U)
    eng.sample_side(me, ot, 0, alpha, mu, LF)
    X = eng.get_items(me)
    Y = U[rows]
    Lam = LF + alpha * Y.T @ Y
    b = LF @ mu + alpha * Y.T @ (vals - mean)
    m_true = np.linalg.solve(Lam, b); C_true = np.linalg.inv(Lam)
    se = np.sqrt(np.diag(C_true) / nd)
    assert np.all(np.abs(X.mean(0) - m_true) < 5 * se)
    assert np.abs(np.cov(X.T) - C_true).max() < 6 * np.abs(C_true).max() / math.sqrt(nd)
    eng.side_destroy(me); eng.side_destroy(ot)


def test_cholesky_failure_is_reported(hip_engine_factory):
    """THROWERROR("Cholesky failed") (c++/sample.cpp:308) -> BPMF_HIP_ECHOL + column id."""
    import bpmf_amd
    K = 8
    M, Mt, T, Tt, nu, nm = util.tiny()
    eng = hip_engine_factory(K)
    me = eng.side_create(nm, nu, *M, 3.0)
    ot = eng.side_create(nu, nm, np.zeros(nu + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        eng.sample_side(me, ot, 0, 2.0, np.zeros(K), -np.eye(K))       # negative definite prior precision
    assert e.value.code == -4 and "Cholesky failed in column 0" in str(e.value)
    eng.side_destroy(me); eng.side_destroy(ot)


def test_bad_arguments_are_rejected(hip_engine_factory):
    import bpmf_amd
    eng = hip_engine_factory(8)
    with pytest.raises(bpmf_amd.BpmfHipError):
        eng.side_create(2, 4, np.array([0, 1, 2], np.int64), np.array([0, 9], np.int32), np.ones(2), 1.0)   # row 9 >= nrows
    with pytest.raises(bpmf_amd.BpmfHipError):
        bpmf_amd.HipEngine(129)                                                                             # unsupported K (1 .. 128 run)
    with pytest.raises(bpmf_amd.BpmfHipError):
        bpmf_amd.HipEngine(0)


def test_sharded_path_over_rccl_single_rank(tmp_path):
    """bench.py's N > 1 code paths with world_size 1 (everything except a second GPU): (a) RCCL
    inside the library (bpmf_hip_ctx_comm_init: in-place broadcast of the owned range, device
    all-reduce of the sums, all-reduced RMSE), (b) the same exchange through torch.distributed.
    Both must give the single-process path's RMSE."""
    import json
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    env = dict(os.environ, BPMF_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--no-strong", "--repeats", "1", "--prewarm-ms", "0", "--prewarm-steps", "0"]
    a = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert a.returncode == 0, a.stderr[-2000:]
    t = subprocess.run(cmd, env=dict(env, BPMF_DIST="torch", MASTER_PORT="29534"), cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert t.returncode == 0, t.stderr[-2000:]
    # (one communicator, BPMF_HIP_COMM_STREAMS=1: test_real_rccl_split_parts_and_packed_lists_single_rank[1])
    b = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--no-strong", "--repeats", "1", "--prewarm-ms", "0", "--prewarm-steps", "0"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-2000:]
    pick = lambda out: json.loads([l for l in out.splitlines() if l.startswith('{"metric"')][-1])
    ja, jb, jt = pick(a.stdout), pick(b.stdout), pick(t.stdout)
    assert ja["rccl_comm_streams"] == 2 and jb["rccl_comm_streams"] == 0
    assert abs(jt["rmse"] - jb["rmse"]) < 1e-9 and abs(jt["rmse_avg"] - jb["rmse_avg"]) < 1e-9
    assert abs(ja["rmse"] - jb["rmse"]) < 1e-9 and abs(ja["rmse_avg"] - jb["rmse_avg"]) < 1e-9
    assert ja["value"] > 0 and ja["n_gpus"] == 1


@pytest.mark.parametrize("dataset,K", [("ml100k", 16), ("blocks", 32), ("ml100k", 20)])
def test_two_ranks_share_one_gpu(oracle, tmp_path, dataset, K):
    """Two processes, both driving the HIP kernels on cuda:0, joined by gloo (RCCL refuses two ranks on
    one device): the sharded path with REAL kernels on REAL shards -- nnz-balanced column ranges, CSC
    slices, shard-local launches (col_from / col_to), exchange of the fresh ranges, all-reduced sums
    and RMSE -- must reproduce the single-process chain.  "blocks": the connectivity-aware exchange.
    K = 20: a num_latent that runs on the K = 32 kernels -- the tensor TorchComm binds and exchanges must
    have the DEVICE's leading dimension (HipEngine.items_tensor: [ncols, 32]), ADVICE r4 (high)."""
    import os
    import socket
    import subprocess
    import sys
    from tests.conftest import ROOT
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "res")
    nsims, burnin = 4, 1
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_dist_gpu_worker.py"), dataset, str(K),
                                       str(nsims), str(burnin), out], env=env, cwd=ROOT, stderr=subprocess.PIPE, text=True))
    for p in procs:
        _, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-3000:]
    res = [np.load(out + ".rank%d.npz" % r) for r in range(2)]
    M, Mt, T, Tt, nu, nm = util.ml100k() if dataset == "ml100k" else util.blocks()
    ref = oracle.gibbs(K, M, Mt, T, Tt, nsims=nsims, burnin=burnin)
    for r in res:
        assert np.allclose(r["rmse"], ref["rmse"], atol=1e-7) and np.allclose(r["rmse_avg"], ref["rmse_avg"], atol=1e-7)
        assert np.allclose(r["norm_u"], ref["norm_u"], rtol=1e-8) and np.allclose(r["norm_m"], ref["norm_m"], rtol=1e-8)
        if dataset == "blocks":
            assert r["conn_used"].all()
            for X, Xref, dom in ((r["U"], ref["U"], r["dom_u"]), (r["V"], ref["V"], r["dom_m"])):
                assert rel_err(X[dom[0]:dom[1]], Xref[dom[0]:dom[1]]) < 1e-7        # what the rank owns
        else:
            assert rel_err(r["U"], ref["U"]) < 1e-7 and rel_err(r["V"], ref["V"]) < 1e-7
            assert np.array_equal(r["U"], res[0]["U"]) and np.array_equal(r["V"], res[0]["V"])


@pytest.mark.parametrize("K", [32])
def test_connectivity_exchange_loopback(K):
    """bpmf_hip_side_set_conn / bpmf_hip_side_exchange over a one-rank RCCL
    communicator: tests/_conn_worker.py (own process: the communicator is per process)."""
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_conn_worker.py"), str(K)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and "CONN-OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("K", [64])
def test_sharded_big_side_single_rank(K):
    """A side with > 100 000 columns (workgroup form of the statistics pass, k_colstats_wg): sharded over a one-rank
    communicator == plain, and both against the oracle: tests/_bigside_worker.py."""
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_bigside_worker.py"), str(K)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0 and "BIGSIDE-OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("K", [32, 128])
def test_sharded_parts_single_rank(K):
    """Sharded == plain, and bpmf_hip_side_set_overlap (exchange of part c beside the sampling of part c + 1) ==
    uncut, over a one-rank RCCL communicator: tests/_parts_worker.py; K = 128: the fp32 context, sharded."""
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_parts_worker.py"), str(K)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0 and "PARTS-OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("streams", [2, 1])
def test_real_rccl_split_parts_and_packed_lists_single_rank(streams):
    """The REAL librccl, one rank: second communicator from ncclCommSplit (reported by bpmf_hip_ctx_comm_streams), exchanges cut
    into four parts AND routed through the packed connectivity lists at once, in the pipelined loop with the twin evaluation:
    the NO_COMM chain bit for bit (tests/_rccl1_worker.py).  streams = 1: BPMF_HIP_COMM_STREAMS=1, one communicator."""
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("BPMF_HIP_RCCL_LIBRARY", None)                            # the real library, not the tests' double
    if streams == 1:
        env["BPMF_HIP_COMM_STREAMS"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rccl1_worker.py"), "32"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL1-OK streams=%d" % streams in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("K", [16, 32, 64])
def test_propagated_posterior_priors(oracle, hip_engine_factory, K, sampler_mode):
    """-m / -l of the reference (c++/sample.cpp:157-174,272-277): every column has its own prior
    precision Lambda_i (from a previous run's *-Lambda.ddm); rr = Lambda_i * hp.mu keeps the
    global mu (the loaded per-column mu is never used: SURVEY Q2)."""
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)
    rng = np.random.default_rng(300 + K)
    U = 0.3 * rng.standard_normal((nu, K))
    ncols = len(M[0]) - 1
    B = rng.standard_normal((ncols, K, K)) * 0.2
    prop = np.einsum("nij,nkj->nik", B, B) + 2.0 * np.eye(K)[None]        # SPD per column; symmetric => layout-neutral
    A = rng.standard_normal((K, 3 * K)); cov = A @ A.T / (3 * K)
    it, alpha = 4, 2.0
    mu, LU, LF = oracle.hyper_sample(K, ncols, cov, it)
    mean = util.mean_rating(M)
    items_ref = np.zeros((ncols, K))
    s_ref, p_ref, n_ref = oracle.sample_side(K, M, mean, alpha, U, items_ref, it, mu, LF, prop_lambda=prop)
    me = eng.side_create(ncols, nu, *M, mean)
    ot = eng.side_create(nu, ncols, np.zeros(nu + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_items(ot, U)
    eng.set_prop_posterior(me, prop.reshape(ncols, K * K))
    s1, p1, n1 = eng.sample_side(me, ot, it, alpha, mu, LF)
    items = eng.get_items(me)
    assert rel_err(items, items_ref) < RTOL
    assert rel_err(s1, s_ref) < 1e-8 and rel_err(p1, p_ref) < 1e-8
    # and they can be removed again
    eng.set_prop_posterior(me, None)
    items_ref2 = np.zeros((ncols, K))
    oracle.sample_side(K, M, mean, alpha, U, items_ref2, it, mu, LF)
    eng.sample_side(me, ot, it, alpha, mu, LF)
    assert rel_err(eng.get_items(me), items_ref2) < RTOL
    eng.side_destroy(me); eng.side_destroy(ot)


def test_blocking_fallback_paths_give_the_same_chain():
    """Long kernels (big matrices) make the host threads give up spinning on the result words and
    block on an event instead.  BPMF_HIP_SPIN_MS=0 forces that path for every wait: the chain must
    be the one of the spinning run (single-GPU and sharded forms of bench.py)."""
    import json
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--no-strong", "--repeats", "1", "--prewarm-ms", "0", "--prewarm-steps", "0"]
    pick = lambda out: json.loads([l for l in out.splitlines() if l.startswith('{"metric"')][-1])
    runs = []
    for extra in ({}, {"BPMF_HIP_SPIN_MS": "0"},
                  {"BPMF_HIP_SPIN_MS": "0", "BPMF_BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29541",
                   "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}):
        r = subprocess.run(cmd, env=dict(os.environ, **extra), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append(pick(r.stdout))
    for j in runs[1:]:
        assert abs(j["rmse"] - runs[0]["rmse"]) < 1e-9 and abs(j["rmse_avg"] - runs[0]["rmse_avg"]) < 1e-9


@pytest.mark.parametrize("K", [16, 32, 64])
def test_no_covariance_variant(oracle, hip_engine_factory, K, sampler_mode):
    """BPMF_NO_COVARIANCE (c++/sample.cpp:300-304) as a run-time switch: only the diagonal of
    Lambda* is factorised."""
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)
    rng = np.random.default_rng(500 + K)
    V = 0.3 * rng.standard_normal((nm, K))
    ncols = len(Mt[0]) - 1
    A = rng.standard_normal((K, 3 * K)); cov = A @ A.T / (3 * K)
    it, alpha = 2, 2.0
    mu, LU, LF = oracle.hyper_sample(K, ncols, cov, it)
    mean = util.mean_rating(Mt)
    items_ref = np.zeros((ncols, K))
    s_ref, p_ref, n_ref = oracle.sample_side(K, Mt, mean, alpha, V, items_ref, it, mu, LF, no_covariance=True)
    me = eng.side_create(ncols, nm, *Mt, mean)
    ot = eng.side_create(nm, ncols, np.zeros(nm + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_items(ot, V)
    eng.set_no_covariance(True)
    try:
        s1, p1, n1 = eng.sample_side(me, ot, it, alpha, mu, LF)
        items = eng.get_items(me)
    finally:
        eng.set_no_covariance(False)
    assert rel_err(items, items_ref) < RTOL
    assert rel_err(s1, s_ref) < 1e-8 and rel_err(p1, p_ref) < 1e-8
    eng.side_destroy(me); eng.side_destroy(ot)


def test_stateful_path_reports_a_failed_factorisation_and_does_not_hang(hip_engine_factory):
    """The asynchronous Sys::sample: a half-iteration whose factorisation fails (non-finite factors
    on the other side) surfaces as BPMF_HIP_ECHOL at the next call that needs host state; samplers
    queued behind the failing one still run to completion (their gate is opened regardless)."""
    import bpmf_amd
    K = 16
    M, Mt, T, Tt, nu, nm = util.ml100k()
    eng = hip_engine_factory(K)
    movies = eng.side_create(nm, nu, *M, util.mean_rating(M))
    users = eng.side_create(nu, nm, *Mt, util.mean_rating(M))
    eng.sys_sample(movies, users, 2.0)                       # a healthy half-iteration first
    eng.sys_state(movies)
    bad = np.zeros((nu, K)); bad[::7] = np.nan
    eng.set_items(users, bad)
    eng.sys_sample(movies, users, 2.0)                       # fails on the device ...
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        eng.sys_sample(users, movies, 2.0)                   # ... one more half-iteration may be queued behind it
        eng.sys_sample(movies, users, 2.0)
        eng.sys_state(movies)                                # ... and is reported here at the latest
    assert e.value.code == -4 and "Cholesky failed in column" in str(e.value)
    try:
        eng.sync()                                           # the half-iteration queued behind saw NaN factors: same error once more
    except bpmf_amd.BpmfHipError as e2:
        assert e2.code == -4
    eng.sync()                                               # drained: nothing is left spinning
    eng.side_destroy(movies); eng.side_destroy(users)
