"""Multi-chain rank-normalised convergence diagnostics on the device: bpmf_hip_diag_traces_mc and
bpmf_hip_diag_cells_mc against tests/diag_mc_ref.py.

  1. diag_traces_mc against the longdouble reference at (C, S) in SIZES -- the edges of one wave's width, of the power-of-two padding of
     the sort, of the odd-S drop and of the LDS maximum -- in lists of 0, 1, 63 and 257 traces; iid normal, AR(1) 0.5 / 0.9, one chain
     shifted, one chain scaled (C = 1: the second half), Cauchy, 1e8 + N(0, 1), rounded to one decimal (many ties), two-valued, a monotone
     ramp (every lag summed), alternating signs (the antithetic cap), constant, per-chain constant, one NaN, one inf.  Tolerance per kind
     and size, for each of the three outputs: 8 x the largest relative error of the fp64 restatement against longdouble over that kind's
     traces, not less than 1e-12 (the rule of tests/test_gpu_diag.py); the NaN pattern must be equal.  Refusals.
  2. bits: a trace gives equal bytes at another place in the list, in a list of 1 and of 257 and on a second call; diag_cells_mc with
     batches of 1 cell, 7 cells and automatic gives equal bytes
  3. diag_cells_mc on planted rings (samples_set; 40 queries x 30 candidates): C S = 4 x 16 and 2 x 100, K in {1, 8, 32, 64, 128}, an fp32
     context, a pair of sides with biases; mean and std byte-equal to predict_cells; rhat, ess_bulk and ess_tail within the tolerance of 1
     of the reference on the longdouble traces of samples_get; every refusal
  4. diag_cells_mc against diag_traces_mc on the device's own traces, byte for byte, on rings whose dot products are not exact.  The
     library has no entry point that returns the traces k_cell_traces writes (interval_traces takes traces, it does not return them),
     but predict_cells over a ring of ONE sample with mean_rating = 0 returns that sample's d_s = u_s . v_s to the bit: the walk and the
     order of additions are k_cell_traces's (mean and std are byte-equal for that reason), Welford's first step gives m = d exactly and
     0 + d = d.  So the traces are read back sample by sample and handed to diag_traces_mc.

Every test of this file fails on the commit before the feature (missing entry points).
"""
import ctypes as C_

import numpy as np
import pytest
import bpmf_amd
from tests import diag_ref as dr
from tests import diag_mc_ref as mc
from tests import model_ref as mr

pytestmark = pytest.mark.gpu

ld = np.longdouble
FLOOR = 1e-12
NAMES = ("rhat", "ess_bulk", "ess_tail")

# ---- 1. diag_traces_mc against longdouble -------------------------------------------------------------------------------------------------

SIZES = [(1, 8), (1, 9), (2, 8), (2, 9), (3, 11), (4, 16), (4, 17), (5, 13), (8, 32), (3, 683), (2, 1024), (2, 1025), (64, 64), (1, 4096)]
NAN_KINDS = ("constant", "chain_constant", "nan", "inf")


def traces_of_kinds(C, S, seed):
    """kind -> [m, C S]: the traces of the module docstring (one of each at the long sizes: the reference is a Python loop)"""
    rng = np.random.default_rng(seed)
    L = C * S
    m = 3 if L <= 300 else 1
    n = S // 2
    last = slice((C - 1) * S, L) if C > 1 else slice(S - n, S)          # the last chain; of one chain, its second half
    out = dict(iid=rng.standard_normal((m, L)))
    for rho in (0.5, 0.9):
        out["ar%g" % rho] = mc.chains_ar1(rng, m, C, S, rho)
    shifted = mc.chains_ar1(rng, m, C, S, 0.3); shifted[:, last] += 1.0
    out["shifted"] = shifted
    scaled = mc.chains_ar1(rng, m, C, S, 0.3); scaled[:, last] *= 3.0
    out["scaled"] = scaled
    out["cauchy"] = rng.standard_cauchy((m, L))
    out["offset1e8"] = 1e8 + rng.standard_normal((m, L))
    out["rounded"] = np.round(rng.standard_normal((m, L)), 1)
    out["two_valued"] = rng.integers(0, 2, (m, L)).astype(np.float64)
    out["ramp"] = np.arange(L, dtype=np.float64)[None, :] * (1.0 + np.arange(m))[:, None]
    out["alternating"] = (1.0 - 2.0 * (np.arange(S) % 2))[None, None, :].repeat(C, 1).reshape(1, L) * (1.0 + 0.01 * rng.random((m, L)))
    out["constant"] = np.repeat(np.array([0.0, 3.0, -1e300])[:m, None], L, axis=1)
    out["chain_constant"] = np.repeat(np.repeat(np.arange(C, dtype=np.float64), S)[None, :], m, axis=0) + np.arange(m)[:, None]
    for kind, bad in (("nan", np.nan), ("inf", np.inf)):
        x = rng.standard_normal((m, L))
        for i, at in enumerate((n, 0, L - 1)[:m]):                       # (n: the draw an odd S drops from the half-chains)
            x[i, at] = bad
        out[kind] = x
    return out


def tolerances(X, C, S):
    """(want, tol): the longdouble reference of the traces X, three arrays, and per output 8 x the worst relative error of the fp64
    restatement, not less than FLOOR"""
    want = mc.diag_mc_many(X, C, S)
    f64 = mc.diag_mc_many(X, C, S, True)
    return want, tuple(max(8.0 * dr.relative_error(f64[k], want[k]), FLOOR) for k in range(3))


def check(got, want, tol, tag):
    ratio = []
    for k, name in enumerate(NAMES):
        err = dr.relative_error(got[k], want[k])
        assert err <= tol[k], (tag, name, err, tol[k])
        ratio.append(err / tol[k])
    return ratio


@pytest.mark.parametrize("C,S", SIZES)
def test_diag_traces_mc_against_longdouble(hip_engine_factory, C, S):
    eng = hip_engine_factory(8)
    kinds = traces_of_kinds(C, S, 7000 + 64 * S + C)
    names = list(kinds)
    base = np.concatenate([kinds[k] for k in names])
    kind_of = np.repeat(np.arange(len(names)), [len(kinds[k]) for k in names])
    ref = {k: tolerances(kinds[k], C, S) for k in names}
    want = [np.concatenate([ref[k][0][j] for k in names]) for j in range(3)]
    for k in NAN_KINDS:
        assert all(np.isnan(w).all() for w in ref[k][0]), k
    for k in ("iid", "ar0.5", "cauchy", "offset1e8"):
        assert all(np.isfinite(w).all() for w in ref[k][0]), k
    worst = [0.0, 0.0, 0.0]
    empty = eng.diag_traces_mc(np.zeros((0, C * S)), C)
    assert all(a.shape == (0,) for a in empty)
    for n in (1, 63, 257):
        lists = [np.array([i]) for i in range(len(base))] if n == 1 else [(np.arange(n) * 7 + n) % len(base)]
        for idx in lists:
            got = eng.diag_traces_mc(base[idx], C)
            assert all(a.shape == (n,) for a in got)
            for kk, name in enumerate(names):
                sel = kind_of[idx] == kk
                if sel.any():
                    w = check([g[sel] for g in got], [x[idx][sel] for x in want], ref[name][1], (C, S, n, name))
                    worst = [max(a, b) for a, b in zip(worst, w)]
    print("C %d S %d: worst err / tolerance rhat %.3g ess_bulk %.3g ess_tail %.3g; largest tolerance %.1e" % (C, S, worst[0], worst[1], worst[2],
          max(max(ref[k][1]) for k in names)))
    # what the kinds are there for: the shifted and the scaled chain are flagged where the chains are long enough to tell, the
    # alternating signs sit at the cap N log10 N
    got = eng.diag_traces_mc(base, C)
    if C >= 2 and S >= 64:
        assert (got[0][kind_of == names.index("shifted")] > 1.01).all() and (got[0][kind_of == names.index("scaled")] > 1.01).all()
    N = 2 * C * (S // 2)
    alt = got[1][kind_of == names.index("alternating")]
    assert np.allclose(alt, N * np.log10(N), rtol=1e-12)


def test_diag_traces_mc_shapes_and_refusals(hip_engine_factory):
    eng = hip_engine_factory(8)
    one = eng.diag_traces_mc(np.random.default_rng(1).standard_normal(32), 2)
    assert all(a.shape == (1,) and np.isfinite(a).all() for a in one)
    for Cc, S, what in ((65, 8, "65 chains"), (1, 7, "7 samples per chain"), (2, 7, "7 samples per chain"), (1, 4097, "4097 samples per chain"),
                        (3, 1366, "1366 samples per chain in 3 chains"), (64, 65, "65 samples per chain")):
        with pytest.raises(bpmf_amd.BpmfHipError, match="diag_traces_mc: " + what) as e:
            eng.diag_traces_mc(np.zeros((2, Cc * S)), Cc)
        assert e.value.code == -1
    with pytest.raises(ValueError, match="not 3 chains of one length"):
        eng.diag_traces_mc(np.zeros((2, 32)), 3)
    out = np.zeros(2); x = np.zeros((2, 32))
    ptr = lambda a: a.ctypes.data_as(C_.c_void_p)
    for Cc in (0, -2):
        assert eng.lib.bpmf_hip_diag_traces_mc(eng.ctx, 2, Cc, 16, ptr(x), ptr(out), ptr(out), ptr(out)) == -1
    assert eng.lib.bpmf_hip_diag_traces_mc(None, 2, 2, 16, ptr(x), ptr(out), ptr(out), ptr(out)) == -1
    for args in ((None, ptr(out), ptr(out), ptr(out)), (ptr(x), None, ptr(out), ptr(out)), (ptr(x), ptr(out), None, ptr(out)),
                 (ptr(x), ptr(out), ptr(out), None)):
        assert eng.lib.bpmf_hip_diag_traces_mc(eng.ctx, 2, 2, 16, *args) == -1
    assert eng.lib.bpmf_hip_diag_traces_mc(eng.ctx, 0, 2, 16, None, None, None, None) == 0
    assert np.isfinite(eng.diag_traces_mc(np.random.default_rng(0).standard_normal((3, 32)), 2)[1]).all()    # the context goes on working


def test_rank_rhat_sees_what_split_rhat_misses(hip_engine_factory):
    """one chain of four scaled by 3 (AR(1), rho = 0.3, 4 x 100): the estimator of section 29 on the same values has a median near 1.004,
    the folded rank-normalised Rhat near 1.147 (tests/test_diag_mc_host.py has the figures of the restatement)"""
    eng = hip_engine_factory(8)
    X = mc.chains_ar1(np.random.default_rng(5), 200, 4, 100, 0.3)
    X[:, 300:] *= 3.0
    rhat = eng.diag_traces_mc(X, 4)[0]
    plain = eng.diag_traces(X)[0]
    assert np.median(rhat) > 1.08 and rhat.min() > 1.02 and np.median(plain) < 1.03


# ---- 2. bits -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,S", [(1, 9), (2, 32), (4, 17), (3, 683), (1, 4096)])
def test_trace_bits_depend_on_the_trace_alone(hip_engine_factory, C, S):
    eng = hip_engine_factory(8)
    rng = np.random.default_rng(S)
    X = np.concatenate([mc.chains_ar1(rng, 129, C, S, 0.8), np.round(rng.standard_normal((128, C * S)), 1)])
    X[200, (C * S) // 2:] += 2.0
    base = eng.diag_traces_mc(X, C)
    again = eng.diag_traces_mc(X, C)
    assert len(X) == 257 and all(a.tobytes() == b.tobytes() for a, b in zip(base, again))
    perm = rng.permutation(len(X))
    got = eng.diag_traces_mc(X[perm], C)
    assert all(a[perm].tobytes() == b.tobytes() for a, b in zip(base, got))
    for i in (0, 3, 200, 256):
        alone = eng.diag_traces_mc(X[i], C)
        assert all(a[i:i + 1].tobytes() == b.tobytes() for a, b in zip(base, alone)), i
    for n in (63,):
        part = eng.diag_traces_mc(X[:n], C)
        assert all(a[:n].tobytes() == b.tobytes() for a, b in zip(base, part))


NQ, NC = 40, 30


def chain_rings(rng, C, S, K, rho=0.6):
    """(Es [C S, NQ, K], Vs [C S, NC, K]): every factor entry C independent AR(1) chains of S draws around a level of its own, rounded
    to multiples of 2^-12.  Every product is then a multiple of 2^-24 and every partial sum of a dot product is exact in fp64, so the
    device's traces are numpy's bit for bit whatever the order of additions -- which the comparison needs: the folded values of the two
    middle order statistics are equal in exact arithmetic, and one ulp in a trace decides whether their ranks are 1.5 and 1.5 or 1 and 2"""
    def side(n):
        x = np.transpose(dr.ar1(rng, n * K * C, S, rho).reshape(n, K, C, S), (2, 3, 0, 1)).reshape(C * S, n, K)
        return np.round((0.5 * rng.standard_normal((n, K)) + 0.3 * x) * 4096.0) / 4096.0
    return side(NQ), side(NC)


def load_rings(eng, sq, sc, Es, Vs):
    L = Es.shape[0]
    eng.samples_reserve(sq, L); eng.samples_reserve(sc, L)
    eng.samples_set(sq, np.transpose(Es, (1, 0, 2))); eng.samples_set(sc, np.transpose(Vs, (1, 0, 2)))


def cell_lists(rng):
    q1 = 17
    every = (np.full(3 * NC, q1), np.tile(np.arange(NC), 3))
    rand = (rng.integers(0, NQ, 150), rng.integers(0, NC, 150))
    return dict(empty=(np.zeros(0, int), np.zeros(0, int)), one=(np.array([5]), np.array([7])), every=every,
                last=(np.array([NQ - 1, 0, NQ - 1]), np.array([NC - 1, NC - 1, 0])), random=rand)


KEYS = ("mean", "std", "rhat", "ess_bulk", "ess_tail")


@pytest.mark.parametrize("K", [4, 128])
def test_cell_bits_do_not_depend_on_the_batch(hip_engine_factory, K):
    C, S = 2, 9
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    try:
        rng = np.random.default_rng(K)
        load_rings(eng, sq, sc, *chain_rings(rng, C, S, K))
        lists = cell_lists(rng)
        q, c = (np.concatenate([lists[k][i] for k in ("every", "last", "random")]) for i in (0, 1))
        base = eng.diag_cells_mc(sq, sc, 2.5, q, c, C)
        assert sorted(base) == sorted(KEYS)
        for cells in (1, 7, 0):
            eng.diag_batch_cells(cells)
            got = eng.diag_cells_mc(sq, sc, 2.5, q, c, C)
            assert all(base[k].tobytes() == got[k].tobytes() for k in KEYS), (K, cells)
        perm = rng.permutation(len(q))
        got = eng.diag_cells_mc(sq, sc, 2.5, q[perm], c[perm], C)
        assert all(base[k][perm].tobytes() == got[k].tobytes() for k in KEYS)
        assert eng.diag_last_ms(sq) >= 0.0
    finally:
        eng.diag_batch_cells(0)
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 3. diag_cells_mc on planted rings -----------------------------------------------------------------------------------------------------

def cell_reference(Es, Vs, q, c, C, S, extra=None):
    """the longdouble reference of the unique cells of the list and its tolerance (the fp64 restatement on the fp64 dot products):
    (want, tol) in list order.  extra [C S, n]: added to the dot products of the list's cells"""
    cells, inv = np.unique(np.stack([q, c]), axis=1, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    Tl = np.einsum("sik,sik->is", Es[:, cells[0]].astype(ld), Vs[:, cells[1]].astype(ld))
    T64 = np.einsum("sik,sik->is", Es[:, cells[0]], Vs[:, cells[1]])
    assert np.array_equal(Tl.astype(np.float64), T64)                 # (exact: see chain_rings)
    if extra is not None:
        first = np.array([np.flatnonzero(inv == u)[0] for u in range(cells.shape[1])])
        Tl = Tl + extra.T[first].astype(ld); T64 = T64 + extra.T[first]
    sub = np.arange(0, len(Tl), max(1, len(Tl) // 24))                 # the fp64 restatement is a Python loop: a sample of the cells
    want = mc.diag_mc_many(Tl.astype(np.float64), C, S)                # (the ranked values are fp64 on the device)
    f64 = mc.diag_mc_many(T64[sub], C, S, True)
    tol = tuple(max(8.0 * dr.relative_error(f64[k], want[k][sub]), FLOOR) for k in range(3))
    return [w[inv] for w in want], tol


@pytest.mark.parametrize("K,dtype", [(1, "f64"), (8, "f64"), (32, "f64"), (64, "f64"), (128, "f64"), (72, "f32")])
def test_diag_cells_mc_against_longdouble(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    mean_rating = 3.5
    try:
        for C, S in ((4, 16), (2, 100)):
            rng = np.random.default_rng(100 * K + S)
            Es, Vs = chain_rings(rng, C, S, K)
            load_rings(eng, sq, sc, Es, Vs)
            Eg, Vg = np.transpose(eng.samples_get(sq), (1, 0, 2)), np.transpose(eng.samples_get(sc), (1, 0, 2))
            assert Eg.tobytes() == Es.tobytes() and Vg.tobytes() == Vs.tobytes()
            for name, (q, c) in cell_lists(rng).items():
                got = eng.diag_cells_mc(sq, sc, mean_rating, q, c, C)
                assert sorted(got) == sorted(KEYS) and all(v.shape == (len(q),) for v in got.values())
                mean, std = eng.predict_cells(sq, sc, mean_rating, q, c)
                assert got["mean"].tobytes() == mean.tobytes() and got["std"].tobytes() == std.tobytes(), (K, C, S, name)
                if len(q) == 0:
                    continue
                want, tol = cell_reference(Eg, Vg, q, c, C, S)
                w = check([got[k] for k in NAMES], want, tol, (K, dtype, C, S, name))
                if name == "random":
                    print("K %d %s C %d S %d: err / tolerance rhat %.3g ess_bulk %.3g ess_tail %.3g (tolerance %.1e %.1e %.1e); median "
                          "ess_bulk %.1f" % (K, dtype, C, S, w[0], w[1], w[2], tol[0], tol[1], tol[2], np.median(got["ess_bulk"])))
            # one chain of the same rings: the estimator of one chain, other figures
            if (C, S) == (4, 16):
                q, c = cell_lists(rng)["random"]
                single = eng.diag_cells_mc(sq, sc, mean_rating, q, c, 1)
                want, tol = cell_reference(Eg, Vg, q, c, 1, C * S)
                check([single[k] for k in NAMES], want, tol, (K, dtype, "one chain"))
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def device_traces(eng, Es, Vs, q, c):
    """[n, L]: d_s = u_s(q) . v_s(c) of every cell as the device forms it (module docstring, 4)"""
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    try:
        eng.samples_reserve(sq, 1); eng.samples_reserve(sc, 1)
        out = np.empty((len(q), Es.shape[0]))
        for s in range(Es.shape[0]):
            eng.samples_set(sq, Es[s][:, None, :]); eng.samples_set(sc, Vs[s][:, None, :])
            out[:, s] = eng.predict_cells(sq, sc, 0.0, q, c)[0]
        return out
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


@pytest.mark.parametrize("K,dtype", [(8, "f64"), (32, "f64"), (128, "f64"), (72, "f32")])
def test_diag_cells_mc_is_diag_traces_mc_of_the_device_traces(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    try:
        for C, S in ((4, 16), (2, 100), (1, 9)):
            rng = np.random.default_rng(7 * K + S)
            L = C * S
            Es, Vs = 0.5 * rng.standard_normal((1, NQ, K)) + 0.3 * rng.standard_normal((L, NQ, K)), rng.standard_normal((L, NC, K))   # not on a grid
            load_rings(eng, sq, sc, Es, Vs)
            lists = cell_lists(rng)
            q, c = (np.concatenate([lists[k][i] for k in ("every", "last", "random")]) for i in (0, 1))
            T = device_traces(eng, Es, Vs, q, c)
            assert np.abs(T - np.einsum("sik,sik->is", Es[:, q], Vs[:, c])).max() < 1e-12 * K
            want = eng.diag_traces_mc(T, C)
            for cells in (0, 7):                                         # one batch, and batches of 7 cells: the scatter through orig[]
                eng.diag_batch_cells(cells)
                got = eng.diag_cells_mc(sq, sc, 2.5, q, c, C)
                for k, w in zip(NAMES, want):
                    assert got[k].tobytes() == w.tobytes(), (K, dtype, C, S, cells, k)
            assert C == 1 or np.isfinite(want[0]).all()
            # the same traces through the estimator of one chain, and section 29's beside it
            if C > 1:
                one = eng.diag_cells_mc(sq, sc, 2.5, q, c, 1)
                assert all(one[k].tobytes() == w.tobytes() for k, w in zip(NAMES, eng.diag_traces_mc(T, 1)))
            old = eng.diag_cells(sq, sc, 2.5, q, c)
            r29 = eng.diag_traces(T)
            assert old["rhat"].tobytes() == r29[0].tobytes() and old["ess"].tobytes() == r29[1].tobytes()
    finally:
        eng.diag_batch_cells(0)
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_diag_cells_mc_with_biases(hip_engine_factory):
    K, C, S, nq, nc = 8, 2, 12, 11, 23
    L = C * S
    eng = hip_engine_factory(K)
    A = (np.zeros(nq + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    B = (np.zeros(nc + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    sq, sc = eng.side_create(nq, nc, *A, 0.0), eng.side_create(nc, nq, *B, 0.0)
    try:
        eng.set_bias(sq, 1.0, 14, 1); eng.set_bias(sc, 1.0, 13, 0)
        eng.samples_reserve(sq, L); eng.samples_reserve(sc, L)
        rng = np.random.default_rng(4)
        grid = lambda a: np.round(a * 4096.0) / 4096.0                    # (exact dot products: see chain_rings)
        Es = grid(0.4 * dr.ar1(rng, nq * K, L, 0.6).T.reshape(L, nq, K)); Vs = grid(0.4 * dr.ar1(rng, nc * K, L, 0.6).T.reshape(L, nc, K))
        bq, bc = grid(dr.ar1(rng, nq, L, 0.8).T.copy()), grid(dr.ar1(rng, nc, L, 0.8).T.copy())
        for s in range(L):
            eng.set_items(sq, Es[s]); eng.set_items(sc, Vs[s])
            eng.bias_set(sq, bq[s]); eng.bias_set(sc, bc[s])
            eng.samples_add(sq); eng.samples_add(sc)
        q, c = np.divmod(np.arange(nq * nc), nc)
        got = eng.diag_cells_mc(sq, sc, 1.25, q, c, C)
        mean, std = eng.predict_cells(sq, sc, 1.25, q, c)
        assert got["mean"].tobytes() == mean.tobytes() and got["std"].tobytes() == std.tobytes()
        want, tol = cell_reference(Es, Vs, q, c, C, S, extra=bq[:, q] + bc[:, c])
        w = check([got[k] for k in NAMES], want, tol, "bias")
        print("bias: err / tolerance rhat %.3g ess_bulk %.3g ess_tail %.3g" % tuple(w))
        # without the biases the figures are others: the bias rows of the rings are read
        plain = mc.diag_mc_many(np.einsum("sik,sik->is", Es[:, q], Vs[:, c]), C, S)
        assert dr.relative_error(got["ess_bulk"], plain[1]) > 1e-3
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_diag_cells_mc_refusals(hip_engine_factory):
    K = 8
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    try:
        with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells_mc: no sample ring"):
            eng.diag_cells_mc(sq, sc, 0.0, [0], [0], 1)
        rng = np.random.default_rng(1)
        load_rings(eng, sq, sc, rng.standard_normal((30, NQ, K)), rng.standard_normal((30, NC, K)))
        with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells_mc: the rings hold 30 samples, which is not 4 chains") as e:
            eng.diag_cells_mc(sq, sc, 0.0, [0], [0], 4)
        assert e.value.code == -1
        with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells_mc: 6 samples per chain in 5 chains"):
            eng.diag_cells_mc(sq, sc, 0.0, [0], [0], 5)
        with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells_mc: 6 samples per chain"):
            eng.diag_cells_mc(sq, sc, 0.0, [], [], 5)
        for Cc in (0, -1, 65):
            with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells_mc: %d chains" % Cc):
                eng.diag_cells_mc(sq, sc, 0.0, [0], [0], Cc)
        with pytest.raises(bpmf_amd.BpmfHipError, match="no diagnostics"):
            eng.diag_last_ms(sq)
        eng.samples_set(sc, rng.standard_normal((NC, 29, K)))
        with pytest.raises(bpmf_amd.BpmfHipError, match="same number"):
            eng.diag_cells_mc(sq, sc, 0.0, [0], [0], 1)
        eng.samples_set(sc, rng.standard_normal((NC, 30, K)))
        for q, c, cell in (([0, NQ], [0, 0], "cell 1"), ([0, 1, 2], [0, 1, NC], "cell 2"), ([-1], [0], "cell 0")):
            with pytest.raises(bpmf_amd.BpmfHipError, match="diag_cells_mc: " + cell + " .*out of range") as e:
                eng.diag_cells_mc(sq, sc, 0.0, q, c, 3)
            assert e.value.code == -1
        with pytest.raises(bpmf_amd.BpmfHipError, match="mean_rating is not finite"):
            eng.diag_cells_mc(sq, sc, np.nan, [0], [0], 3)
        ptr = lambda a: a.ctypes.data_as(C_.c_void_p)
        one = np.zeros(1, np.int32); out = np.zeros(1)
        o5 = [ptr(out)] * 5
        assert eng.lib.bpmf_hip_diag_cells_mc(None, sc.handle, 0.0, 1, ptr(one), ptr(one), 3, *o5) == -1
        assert eng.lib.bpmf_hip_diag_cells_mc(sq.handle, sc.handle, 0.0, 1, ptr(one), None, 3, *o5) == -1
        for k in range(5):
            args = list(o5); args[k] = None
            assert eng.lib.bpmf_hip_diag_cells_mc(sq.handle, sc.handle, 0.0, 1, ptr(one), ptr(one), 3, *args) == -1
        other = bpmf_amd.HipEngine(K)
        try:
            oq, oc = mr.pair_of_sides(other, NQ, NC)
            with pytest.raises(bpmf_amd.BpmfHipError, match="different contexts"):
                eng.diag_cells_mc(sq, oc, 0.0, [0], [0], 3)
        finally:
            other.close()
        got = eng.diag_cells_mc(sq, sc, 0.0, [0], [0], 3)
        assert all(np.isfinite(v).all() for v in got.values()) and eng.diag_last_ms(sq) >= 0.0
        # the newest call of either kind is the one timed
        eng.diag_cells(sq, sc, 0.0, [0], [0])
        assert eng.diag_last_ms(sq) >= 0.0
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)
