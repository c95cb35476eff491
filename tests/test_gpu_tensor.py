"""Sparse tensor factorisation on the device: k_khatri_rao in front of the unchanged column samplers.

  1. Khatri-Rao bits     engine.tensor_product of every mode equals numpy bit for bit, padding rows zero, at every nnz on both sides
                         of the wave / workgroup boundaries and on the edge tensor; asked in the order 0, 2, 1, 0 so that every
                         launch overwrites another mode's rows of the shared buffer
  2. anchor              dims[2] = 1 and a last-mode factor of ones: tensor_sample of modes 0 and 1 equals sample_side of the matrix
                         sides with the same ratings bit for bit (1.0 v = v, same summation order)
  3. half-iteration      every mode of the edge tensor against tests/tensor_ref.py at the project's half-iteration bars, at the
                         automatic chunk and at 16, both K <= 32 forms; launches A, B, A: the third equals the first bit for bit
  4. prediction          per test entry |Pavg - numpy| <= 2 K 2^-53 sum_k |a b c| over n = 0, 1, 2 with 0, 1 and 65 test entries
  5. chain               tensor_gibbs against restate_chain at the tolerances of test_gpu_chain.py; two device runs bit-identical
  6. failure path        a prior that makes a pivot non-positive: BPMF_HIP_ECHOL with the mode's column, then a healthy launch
  7. lifetime            create / destroy twice: bpmf_hip_live_device_bytes goes back to its starting value
  8. the executable      bpmf --tensor ... --tensor-test ... -o DIR against tensor_gibbs
"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import tensor_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_parity import RTOL, rel_err

pytestmark = pytest.mark.gpu

ALPHA = 1.7                 # not a power of two
STAT_TOL = 1e-8             # sums and norm of a half-iteration (the bar of test_gpu_weights.py, test_gpu_censored.py)
U = 2.0 ** -53


class _env:
    def __init__(self, **kv):
        self.kv, self.old = {k: v for k, v in kv.items() if v is not None}, {}

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


def _random_tensor(nnz, dims, seed):
    rng = np.random.default_rng(seed)
    cells = rng.choice(dims[0] * dims[1] * dims[2], size=nnz, replace=False)
    idx = np.stack(np.unravel_index(cells, dims), axis=1).astype(np.int32)
    return idx, rng.integers(1, 6, nnz).astype(np.float64)


def _padded(P, ld):
    out = np.zeros((P.shape[0], ld))
    out[:, :P.shape[1]] = P
    return out


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _set_factors(eng, T, F):
    for m in range(3):
        eng.set_items(T.sides[m], F[m])


_EDGE = {}


def _edge():
    if not _EDGE:
        _EDGE["t"] = ref.edge_tensor()
    return _EDGE["t"]


# ---- 1. Khatri-Rao bits ----------------------------------------------------------------------------------------------------------------

KR_DIMS = (13, 29, 23)


def _check_products(eng, T, idx, F, K):
    ld = eng.ld()
    first = None
    for step, m in enumerate((0, 2, 1, 0)):
        got = eng.tensor_product(T, m)
        want = _padded(ref.khatri_rao(F, idx, m), ld) if len(idx) else np.zeros((0, ld))
        assert got.shape == want.shape
        assert _bits_equal(got, want), "mode %d (step %d): %d of %d elements differ" % (m, step, int((got != want).sum()), got.size)
        assert not got[:, K:].any()                                  # the padding rows
        if step == 0:
            first = got
    assert _bits_equal(first, got)                                   # two launches of mode 0, three other launches between them


@pytest.mark.parametrize("nnz", [0, 1, 63, 64, 65, 257, 4097])
@pytest.mark.parametrize("K", [8, 10, 32, 64, 100, 128])
def test_khatri_rao_bits(hip_engine_factory, K, nnz):
    eng = hip_engine_factory(K)
    idx, vals = _random_tensor(nnz, KR_DIMS, 1000 * K + nnz)
    F = ref.factors(K, KR_DIMS, 7 * K + nnz)
    T = eng.tensor_create(idx, vals, KR_DIMS, 3.0)
    try:
        _set_factors(eng, T, F)
        _check_products(eng, T, idx, F, K)
    finally:
        eng.tensor_destroy(T)


@pytest.mark.parametrize("K", [8, 10, 32, 64, 100, 128])
def test_khatri_rao_bits_edge_tensor(hip_engine_factory, K):
    eng = hip_engine_factory(K)
    idx, vals, dims = _edge()
    F = ref.factors(K, dims, 31 * K)
    T = eng.tensor_create(idx, vals, dims, float(vals.mean()))
    try:
        _set_factors(eng, T, F)
        _check_products(eng, T, idx, F, K)
    finally:
        eng.tensor_destroy(T)


# ---- 2. anchor to the matrix path -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [16, 64, 128])
def test_anchor_to_the_matrix_path(hip_engine_factory, oracle, K):
    """With one index in the last mode and its factor all ones, P = 1.0 * (the other mode's rows): the tensor's modes 0 and 1 are the
    two sides of the matrix with the same ratings, in the same order."""
    import scipy.sparse as sp
    from tests import util
    eng = hip_engine_factory(K)
    nu, nm = 50, 37
    rng = np.random.default_rng(400 + K)
    dense = rng.random((nu, nm)) < 0.3
    dense[:, 5] = False; dense[7, :] = False                          # a column and a row without ratings
    dense[:, 11] = True; dense[7, 11] = False                         # a heavy column
    rows, cols = np.nonzero(dense.T)[1], np.nonzero(dense.T)[0]      # sorted by (column, row)
    assert np.all(np.diff(cols * nu + rows) > 0)
    vals = rng.integers(1, 6, len(rows)).astype(np.float64)
    mean = float(vals.mean())
    M = util.csc_arrays(sp.coo_matrix((vals, (rows, cols)), shape=(nu, nm)))
    Mt = util.csc_arrays(sp.coo_matrix((vals, (cols, rows)), shape=(nm, nu)))
    idx = np.stack([rows, cols, np.zeros_like(rows)], axis=1).astype(np.int32)
    dims = (nu, nm, 1)
    F = ref.factors(K, dims, 500 + K)
    F[2] = np.ones((1, K))
    T = eng.tensor_create(idx, vals, dims, mean)
    movies = eng.side_create(nm, nu, *M, mean)
    users = eng.side_create(nu, nm, *Mt, mean)
    try:
        for mode, me, ot, n in ((1, movies, users, nm), (0, users, movies, nu)):
            mu, LU, LF = oracle.hyper_sample(K, n, np.eye(K) * 0.2, 4)
            _set_factors(eng, T, F)
            eng.set_items(movies, F[1]); eng.set_items(users, F[0])
            s, prod, nrm = eng.tensor_sample(T, mode, 4, ALPHA, mu, LF)
            s2, prod2, nrm2 = eng.sample_side(me, ot, 4, ALPHA, mu, LF)
            a, b = eng.get_items(T.sides[mode]), eng.get_items(me)
            names = (eng.kernel_name(T.sides[mode]), eng.kernel_name(me))
            print("K %d mode %d: %s | %s, differing factors %d" % (K, mode, names[0], names[1], int((a != b).sum())))
            assert np.all(np.isfinite(a)) and np.abs(a).max() > 0
            assert _bits_equal(a, b), names
            assert _bits_equal(s, s2) and _bits_equal(np.asfortranarray(prod), np.asfortranarray(prod2)) and nrm == nrm2
    finally:
        eng.side_destroy(movies); eng.side_destroy(users)
        eng.tensor_destroy(T)


# ---- 3. one half-iteration per mode ------------------------------------------------------------------------------------------------------

_HALF_REF = {}


def _half_reference(oracle, K):
    """per mode the inputs (it, mu, LF) of launches A and B and what the reference makes of them from the same factors"""
    if K not in _HALF_REF:
        idx, vals, dims = _edge()
        mean = float(vals.mean())
        F = ref.factors(K, dims, 600 + K)
        out = []
        for m in range(3):
            per = []
            for it, scale in ((4, 0.2), (5, 0.35)):
                mu, LU, LF = oracle.hyper_sample(K, dims[m], np.eye(K) * scale, it)
                got = [f.copy() for f in F]
                s, prod, nrm = ref.sample_mode(oracle, K, idx, vals, dims, mean, ALPHA, got, m, it, mu, LF)
                per.append(dict(it=it, mu=mu, LF=LF, items=got[m], s=s, prod=prod, nrm=nrm))
            out.append(per)
        _HALF_REF[K] = (F, mean, out)
    return _HALF_REF[K]


HALF = [(K, chunk, mode) for K in (8, 20, 32) for chunk in (None, 16) for mode in (1, 3)] + [(K, chunk, None) for K in (64, 128) for chunk in (None, 16)]


@pytest.mark.parametrize("K,chunk,mode", HALF, ids=["K%d-chunk%s-mode%s" % (k, c or "auto", m or "auto") for k, c, m in HALF])
def test_half_iteration_per_mode(hip_engine_factory, oracle, K, chunk, mode):
    eng = hip_engine_factory(K)
    idx, vals, dims = _edge()
    F, mean, want = _half_reference(oracle, K)
    with _env(BPMF_HIP_CHUNK=chunk, BPMF_HIP_MODE=mode):
        T = eng.tensor_create(idx, vals, dims, mean)
    try:
        if chunk:
            info = eng.schedule_info(T.sides[0])
            assert info["chunk"] == 16 and info["chunked_columns"] >= 1 and info["chunks"] >= 17, info     # the index with 281 entries
        for m in range(3):
            _set_factors(eng, T, F)
            runs = []
            for w in (want[m][0], want[m][1], want[m][0]):            # A, B, A
                s, prod, nrm = eng.tensor_sample(T, m, w["it"], ALPHA, w["mu"], w["LF"])
                runs.append((eng.get_items(T.sides[m]), s, prod, nrm))
            for (items, s, prod, nrm), w in zip(runs[:2], want[m]):
                assert np.all(np.isfinite(items))
                err = rel_err(items, w["items"])
                print("K %d mode %d it %d (%s): factors %.3g, sum %.3g, prod %.3g" % (K, m, w["it"], eng.kernel_name(T.sides[m]), err,
                                                                                     rel_err(s, w["s"]), rel_err(prod, w["prod"])))
                assert err <= RTOL, (m, err)
                assert rel_err(s, w["s"]) < STAT_TOL and rel_err(prod, w["prod"]) < STAT_TOL and abs(nrm - w["nrm"]) <= STAT_TOL * abs(w["nrm"])
            assert _bits_equal(runs[0][0], runs[2][0]) and _bits_equal(runs[0][1], runs[2][1]) and runs[0][3] == runs[2][3]
            assert not _bits_equal(runs[0][0], runs[1][0])
            for k in ref.others(m):                                   # the other modes' factors are read, never written
                assert _bits_equal(eng.get_items(T.sides[k]), F[k])
    finally:
        eng.tensor_destroy(T)


# ---- 4. prediction ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ntest", [0, 1, 65])
@pytest.mark.parametrize("K", [8, 20, 128])
def test_prediction(hip_engine_factory, K, ntest):
    """Pavg / Pm2 / n as bpmf_hip_predict: n = 0 stores the prediction, n >= 1 moves the average by delta / n.  A prediction is a
    K-term dot product of c_t with a o b: in any order of summation it is within 2 K 2^-53 sum_k |a b c| of numpy's; a running average
    of such predictions stays within the largest of their bounds, plus the two roundings of avg + delta / n."""
    eng = hip_engine_factory(K)
    idx, vals, dims = _edge()
    mean = float(vals.mean())
    taken = set(map(tuple, idx.tolist()))
    free = [(i, j, t) for i in range(dims[0]) for j in range(dims[1]) for t in range(dims[2]) if (i, j, t) not in taken]
    rng = np.random.default_rng(50 + K + ntest)
    tidx = np.array([free[q] for q in rng.choice(len(free), size=ntest, replace=False)], np.int32).reshape(-1, 3)
    tvals = rng.integers(1, 6, ntest).astype(np.float64)
    T = eng.tensor_create(idx, vals, dims, mean)
    try:
        tt = eng.tensor_test(T, tidx, tvals)
        avg = np.zeros(ntest)
        bound = np.zeros(ntest)
        for n in (0, 1, 2):
            F = ref.factors(K, dims, 900 + 10 * K + n)
            _set_factors(eng, T, F)
            a, b, c = F[0][tidx[:, 0]], F[1][tidx[:, 1]], F[2][tidx[:, 2]]
            pred = mean + np.einsum("ik,ik->i", a * b, c)
            bound = np.maximum(bound, 2 * K * U * np.abs(a * b * c).sum(axis=1))
            avg = pred.copy() if n == 0 else avg + (pred - avg) / n
            se, se_avg, cnt = eng.tensor_predict(tt, n)
            pavg, pm2 = eng.tensor_test_get(tt)
            assert cnt == ntest and pavg.shape == (ntest,)
            if ntest == 0:
                assert se == 0.0 and se_avg == 0.0
                continue
            slack = bound + (2 * U * np.abs(avg) if n else 0.0)
            err = np.abs(pavg - avg)
            print("K %d, %d test entries, n = %d: max |Pavg - numpy| / bound %.3g" % (K, ntest, n, float((err / slack).max())))
            assert np.all(err <= slack), (n, err, slack)
            # the sums: se_avg is over the device's own Pavg; se over predictions within `bound` of numpy's
            want_avg = float(((tvals - pavg) ** 2).sum())
            assert abs(se_avg - want_avg) <= 1e-13 * ntest * max(want_avg, 1.0)
            want_se = float(((tvals - pred) ** 2).sum())
            assert abs(se - want_se) <= float((2 * np.abs(tvals - pred) * bound + bound ** 2).sum()) + 1e-13 * ntest * max(want_se, 1.0)
            if n == 0:
                assert se == se_avg
    finally:
        eng.tensor_destroy(T)


# ---- 5. the chain -------------------------------------------------------------------------------------------------------------------------

CHAIN_DIMS = (30, 20, 6)
_CHAIN = {}


def _chain_data():
    if "d" not in _CHAIN:
        _CHAIN["d"] = ref.planted(CHAIN_DIMS, 4, 0.25, 0.3, 7)
    return _CHAIN["d"]


def _chain_ref(oracle, K, nsims, burnin):
    key = (K, nsims, burnin)
    if key not in _CHAIN:
        idx, vals, tidx, tvals = _chain_data()
        _CHAIN[key] = ref.restate_chain(oracle, K, idx, vals, CHAIN_DIMS, tidx, tvals, nsims, burnin, 2.0)
    return _CHAIN[key]


def _check_chain(res, want, label):
    d_rmse = float(np.abs(np.array(res["rmse"]) - want["rmse"]).max())
    d_avg = float(np.abs(np.array(res["rmse_avg"]) - want["rmse_avg"]).max())
    d_final = abs(res["final_rmse_avg"] - want["final_rmse_avg"])
    d_norm = float(np.abs(res["norms"] / want["norms"] - 1).max())
    scale = max(np.abs(f).max() for f in want["factors"])
    d_f = max(float(np.abs(a - b).max()) for a, b in zip(res["factors"], want["factors"])) / scale
    d_p = float(np.abs(res["pavg"] - want["pavg"]).max())
    print("%s: RMSE %.2e, avg RMSE %.2e, final %.2e, norms %.2e, factors %.2e of max|U|, Pavg %.2e" % (label, d_rmse, d_avg, d_final, d_norm, d_f, d_p))
    assert d_rmse < 1e-6 and d_avg < 1e-6 and d_final < 1e-6
    assert d_norm < 1e-7
    assert d_f < 1e-6
    assert d_p < 1e-6 * max(1.0, float(np.abs(want["pavg"]).max()))


@pytest.mark.parametrize("K,nsims,burnin", [(8, 8, 3), (64, 4, 1), (100, 4, 1)])
def test_chain(hip_engine_factory, oracle, K, nsims, burnin):
    import bpmf_amd
    eng = hip_engine_factory(K)
    idx, vals, tidx, tvals = _chain_data()
    want = _chain_ref(oracle, K, nsims, burnin)
    res = bpmf_amd.tensor_gibbs(eng, idx, vals, CHAIN_DIMS, tidx, tvals, nsims=nsims, burnin=burnin, alpha=2.0)
    assert len(res["rmse"]) == nsims and res["norms"].shape == (nsims, 3) and res["mean_rating"] == want["mean_rating"]
    _check_chain(res, want, "tensor chain K=%d -i %d -b %d" % (K, nsims, burnin))
    again = bpmf_amd.tensor_gibbs(eng, idx, vals, CHAIN_DIMS, tidx, tvals, nsims=nsims, burnin=burnin, alpha=2.0)
    for a, b in zip(res["factors"], again["factors"]):
        assert _bits_equal(a, b)
    assert res["rmse"] == again["rmse"] and res["rmse_avg"] == again["rmse_avg"] and _bits_equal(res["norms"], again["norms"])
    assert _bits_equal(res["pavg"], again["pavg"]) and _bits_equal(res["pm2"], again["pm2"])
    if K == 8:
        assert res["rmse_avg"][-1] < res["rmse"][0]                  # the averaged predictor beats iteration 0


# ---- 6. the failure path ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [8, 64, 128])
def test_failed_factorisation_is_an_error_code(hip_engine_factory, oracle, K):
    """A prior precision of -1e6 I makes the first pivot of every column non-positive (the way test_gpu_schedule_edges.py reaches its
    failed factorisation): BPMF_HIP_ECHOL naming a column of the mode, no trap; the launches after it are healthy."""
    import bpmf_amd
    eng = hip_engine_factory(K)
    idx, vals, dims = _edge()
    F, mean, want = _half_reference(oracle, K)
    T = eng.tensor_create(idx, vals, dims, mean)
    try:
        for m in (0, 2):
            _set_factors(eng, T, F)
            w = want[m][0]
            with pytest.raises(bpmf_amd.BpmfHipError) as e:
                eng.tensor_sample(T, m, w["it"], ALPHA, w["mu"], -1e6 * np.eye(K))
            assert e.value.code == -4 and "Cholesky failed in column" in str(e.value)
            col = eng.lib.bpmf_hip_failed_column(T.sides[m].handle)
            assert 0 <= col < dims[m] and ("column %d" % col) in str(e.value)
            _set_factors(eng, T, F)
            s, prod, nrm = eng.tensor_sample(T, m, w["it"], ALPHA, w["mu"], w["LF"])
            assert eng.lib.bpmf_hip_failed_column(T.sides[m].handle) == -1
            assert rel_err(eng.get_items(T.sides[m]), w["items"]) <= RTOL and rel_err(s, w["s"]) < STAT_TOL
    finally:
        eng.tensor_destroy(T)


def test_refusals_on_the_device(hip_engine_factory):
    import bpmf_amd
    eng = hip_engine_factory(8)
    idx, vals, dims = _edge()
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        eng.tensor_create(np.vstack([idx, idx[:1]]), np.append(vals, 1.0), dims, 3.0)
    assert e.value.code == -1 and "is listed twice (entries 1 and %d)" % (len(idx) + 1) in str(e.value)
    T = eng.tensor_create(idx, vals, dims, 3.0)
    try:
        mu, LF = np.zeros(8), np.eye(8)
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            eng.tensor_sample(T, 3, 0, ALPHA, mu, LF)
        assert e.value.code == -1
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            eng.tensor_test(T, np.array([[0, 0, dims[2]]]), np.ones(1))
        assert e.value.code == -1 and "entry 1 has index %d in mode 3" % (dims[2] + 1) in str(e.value)
        eng.set_weights(T.sides[1], np.full(T.nnz, 2.0))             # a mode's side with an add-on is refused, in a line
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            eng.tensor_sample(T, 0, 0, ALPHA, mu, LF)
        assert e.value.code == -1 and "not together with per-rating weights on a mode of a tensor" in str(e.value)
    finally:
        eng.tensor_destroy(T)
    f32 = hip_engine_factory(128, "f32")
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        f32.tensor_create(idx, vals, dims, 3.0)
    assert e.value.code == -1 and "not on an fp32 context" in str(e.value)


# ---- 7. lifetime ---------------------------------------------------------------------------------------------------------------------------

def test_create_destroy_twice_returns_the_device_bytes(hip_engine_factory):
    eng = hip_engine_factory(32)
    idx, vals, dims = _edge()
    start = eng.lib.bpmf_hip_live_device_bytes()
    for _ in range(2):
        T = eng.tensor_create(idx, vals, dims, 3.0)
        tt = eng.tensor_test(T, idx[:10], vals[:10])
        live = eng.lib.bpmf_hip_live_device_bytes()
        # P and Q (ld doubles per entry) and two int32 per entry and mode / test entry
        assert live - start == 8 * 32 * (len(idx) + 10) + 3 * 2 * 4 * len(idx) + 2 * 4 * 10, live - start
        eng.tensor_predict(tt, 0)
        eng.tensor_destroy(T)                                        # (its test sets go first)
        assert eng.lib.bpmf_hip_live_device_bytes() == start


# ---- 8. the executable ---------------------------------------------------------------------------------------------------------------------

def test_cli_tensor_run(tmp_path, hip_engine_factory):
    import bpmf_amd
    from bpmf_amd import io as bio
    K, nsims, burnin = 8, 6, 2
    idx, vals, tidx, tvals = _chain_data()
    bio.write_tns(tmp_path / "train.tns", idx, vals)
    bio.write_tns(tmp_path / "test.tns.gz", tidx, tvals)
    (tmp_path / "o").mkdir()
    out = subprocess.run([os.path.join(ROOT, "bpmf_amd", "bpmf"), "--tensor", "train.tns", "--tensor-test", "test.tns.gz", "-d", str(K), "-i", str(nsims),
                          "-b", str(burnin), "-o", "o"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines()[0] == "tensor: 30 x 20 x 6, %d ratings, %d test" % (len(vals), len(tvals))
    eng = hip_engine_factory(K)
    res = bpmf_amd.tensor_gibbs(eng, idx, vals, CHAIN_DIMS, tidx, tvals, nsims=nsims, burnin=burnin, alpha=2.0, keep_samples=True)
    lines = re.findall(r"^0: (Burnin|Sampling) iteration (\d+):\t RMSE: (\S+)\tavg RMSE: (\S+)\tF1\(\s*(\S+)\)\tF2\(\s*(\S+)\)\tF3\(\s*(\S+)\)\titems/sec:", out.stdout, re.M)
    assert [int(l[1]) for l in lines] == list(range(nsims)) and [l[0] for l in lines] == ["Burnin"] * burnin + ["Sampling"] * (nsims - burnin)
    got = np.array([[float(x) for x in l[2:]] for l in lines])
    assert np.abs(got[:, 0] - res["rmse"]).max() <= 5e-5 and np.abs(got[:, 1] - res["rmse_avg"]).max() <= 5e-5     # four printed decimals
    assert np.abs(got[:, 2:] - np.sqrt(res["norms"])).max() <= 5e-3                                                # two
    final = re.search(r"^Final Avg RMSE: (\S+)$", out.stdout, re.M)
    assert final and abs(float(final.group(1)) - res["final_rmse_avg"]) <= 5e-6 * max(1.0, res["final_rmse_avg"])
    # modeN-mu.ddm: the mean of the post-burn-in samples, through the aggregation kernels
    for m in range(3):
        mu = bio.read_dense(tmp_path / "o" / ("mode%d-mu.ddm" % (m + 1))).T
        want = np.mean([s[m] for s in res["samples"][burnin:]], axis=0)
        assert mu.shape == want.shape and np.abs(mu - want).max() <= 1e-8 * max(1.0, np.abs(want).max())
    # (1e-8, not bits: the executable sums the ratings for their mean in file order, numpy pairwise -- the two chains may start an
    #  ulp of the mean apart)
    pidx, pavg, _ = bpmf_amd.read_tns(tmp_path / "o" / "Pavg.tns")
    assert np.array_equal(pidx, tidx) and np.abs(pavg - res["pavg"]).max() <= 1e-8 * max(1.0, np.abs(res["pavg"]).max())
    pidx, pm2, _ = bpmf_amd.read_tns(tmp_path / "o" / "Pm2.tns")
    assert np.array_equal(pidx, tidx) and np.abs(pm2 - res["pm2"]).max() <= 1e-8 * max(1.0, np.abs(res["pm2"]).max())
