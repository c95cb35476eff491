"""k_sample1's gather stream against the oracle and against the index-block form it replaces.

A side that runs k_sample1 (K <= 32, one work item per wave) gets a gather stream when it is created: per rating, in the order
the work items consume them, the rated row's offset into the other side's factor matrix and r - mean_rating, every item
padded to a multiple of 16 ratings with records that gather a row of zeros.  The launches that read the side's own ratings
take their Gram from it (k_sample1<K>); BPMF_HIP_GATHER_STREAM=0, read when a side is created, keeps the index-block form
(k_sample1i<K>), which probit, censored and side-information launches always take.  Both forms do the same floating-point
operations in the same order, so their samples must be EQUAL, not close.

The movies side has 48 columns over 64 rows: 0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65 and 129 ratings (every count on both
sides of a group of 16, of the two-group trip of the stream's loop and of the 64-rating index block), 128 and 200 for the
chunk cases, one column whose ratings all sit in the LAST row of the other side (the row next to the end of the factor
matrix), the rest filler.  A column with more ratings than the other side has rows rates rows twice: the sampler and the
oracle both take a CSC as a list of (row, value) pairs per column.  Cases:

  * every column against the oracle (one stateless launch, fp64 RTOL = 1e-9 of max|U| on the factors and 1e-8 on the sums:
    tests/test_gpu_parity.py), K = 8, 16, 32, at the automatic chunk and at BPMF_HIP_CHUNK=64 (columns of 64, 65, 128, 200:
    chunks that end on and off a group boundary), in both forms;
  * a 3-iteration chain (bpmf_amd.gibbs: both sides, hyper-parameter draws, predictions), stream == index blocks bit for bit,
    and against the oracle's chain at the 1e-6 of a coupled run;
  * adaptive noise (the stream in use, alpha changing from iteration to iteration): the same equality, alpha included;
  * a probit side: the index-block form is what the library reports and runs, against the oracle.
"""
import numpy as np
import pytest

from tests import util
from tests.test_gpu_parity import check_half_iteration, rel_err

pytestmark = pytest.mark.gpu

NROWS, NCOLS = 64, 48
COUNTS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 128, 200, 0, 2, 5, 48, 47, 49, 80, 96, 97, 3]
LAST_ROW_COL = 23                                                     # the column of 3 ratings: all in row NROWS - 1
_CACHE = {}


def _matrices():
    """(M, Mt, T, Tt): CSC by column / by row of the same (row, column, value) list, and a small test matrix."""
    if "m" not in _CACHE:
        rng = np.random.default_rng(950)
        counts = np.asarray(COUNTS + [int(c) for c in rng.integers(1, 40, size=NCOLS - len(COUNTS))], np.int64)
        assert len(counts) == NCOLS
        rows, cols = [], []
        for c, n in enumerate(counts):
            if c == LAST_ROW_COL:
                r = np.full(n, NROWS - 1)
            elif n <= NROWS:
                r = np.sort(rng.choice(NROWS, size=int(n), replace=False))
            else:                                                     # more ratings than rows: every row, some twice or more
                r = np.sort(np.concatenate([np.arange(NROWS), rng.integers(0, NROWS, size=int(n) - NROWS)]))
            rows.append(r); cols.append(np.full(n, c))
        rows = np.concatenate(rows).astype(np.int32); cols = np.concatenate(cols).astype(np.int32)
        rows[np.flatnonzero(cols == 1)] = NROWS - 1                   # the single rating of column 1 too
        vals = rng.normal(3.6, 1.1, size=len(rows))

        def csc(major, minor, v, nmajor):
            order = np.argsort(major, kind="stable")
            ptr = np.concatenate([[0], np.cumsum(np.bincount(major, minlength=nmajor))]).astype(np.int64)
            out = (ptr, np.ascontiguousarray(minor[order], np.int32), np.ascontiguousarray(v[order], np.float64))
            for a in out:
                a.setflags(write=False)
            return out

        M, Mt = csc(cols, rows, vals, NCOLS), csc(rows, cols, vals, NROWS)
        tkey = rng.choice(NROWS * NCOLS, size=40, replace=False)
        trow, tcol = (tkey // NCOLS).astype(np.int32), (tkey % NCOLS).astype(np.int32)
        tval = rng.normal(3.6, 1.1, size=40)
        _CACHE["m"] = (M, Mt, csc(tcol, trow, tval, NCOLS), csc(trow, tcol, tval, NROWS), counts)
    return _CACHE["m"]


def _env(monkeypatch, stream, chunk):
    monkeypatch.setenv("BPMF_HIP_MODE", "1")
    monkeypatch.setenv("BPMF_HIP_GATHER_STREAM", "1" if stream else "0")
    if chunk is None:
        monkeypatch.delenv("BPMF_HIP_CHUNK", raising=False)
    else:
        monkeypatch.setenv("BPMF_HIP_CHUNK", str(chunk))


def _reference(oracle, K):
    """Launch inputs and the oracle's half-iteration for them: once per K, shared, never written."""
    if ("ref", K) not in _CACHE:
        M = _matrices()[0]
        rng = np.random.default_rng(4000 + K)
        U = 0.4 * rng.standard_normal((NROWS, K))
        A = rng.standard_normal((K, 3 * K))
        it, alpha = 5, 1.7
        mu, LU, LF = oracle.hyper_sample(K, NCOLS, A @ A.T / (3 * K), it)
        ref = np.zeros((NCOLS, K))
        s, p, n = oracle.sample_side(K, M, util.mean_rating(M), alpha, U, ref, it, mu, LF)
        ref.setflags(write=False)
        _CACHE[("ref", K)] = ((U, it, alpha, mu, LF), (ref, s, p, n))
    return _CACHE[("ref", K)]


def _half_iteration(eng, inp):
    M = _matrices()[0]
    U, it, alpha, mu, LF = inp
    me = eng.side_create(NCOLS, NROWS, *M, util.mean_rating(M))
    ot = eng.side_create(NROWS, NCOLS, np.zeros(NROWS + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    name, info = eng.kernel_name(me), eng.schedule_info(me)
    eng.set_items(ot, U)
    s, p, n = eng.sample_side(me, ot, it, alpha, mu, LF)
    items = eng.get_items(me)
    eng.side_destroy(me); eng.side_destroy(ot)
    return name, info, (items, s, p, n)


@pytest.mark.parametrize("chunk", [None, 64], ids=["chunk-auto", "chunk-64"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_every_column_against_the_oracle_and_the_index_blocks(oracle, hip_engine_factory, monkeypatch, K, chunk):
    counts = _matrices()[4]
    inp, ref = _reference(oracle, K)
    eng = hip_engine_factory(K)
    out = {}
    for stream in (True, False):
        _env(monkeypatch, stream, chunk)
        name, info, hip = _half_iteration(eng, inp)
        assert name == ("k_sample1<%d>" if stream else "k_sample1i<%d>") % K, name
        if chunk == 64:                                               # 65 -> 48 + 17, 128 -> 64 + 64, 129 -> 48 x 2 + 33, 200 -> 64 x 3 + 8
            assert info["chunk"] == 64 and info["chunked_columns"] == (counts > 64).sum() > 0
        print("gather-stream K %d chunk %s %s: factors %.3e sum %.3e prod %.3e"
              % (K, chunk, name, rel_err(hip[0], ref[0]), rel_err(hip[1], ref[1]), rel_err(hip[2], ref[2])))
        check_half_iteration(hip, ref)                                # every column, the empty ones and the last-row one too
        out[stream] = hip
    assert np.array_equal(out[True][0], out[False][0])                # bit for bit
    assert np.array_equal(out[True][1], out[False][1]) and np.array_equal(out[True][2], out[False][2]) and out[True][3] == out[False][3]


def _chain(eng, monkeypatch, stream, chunk, **kw):
    import bpmf_amd
    M, Mt, T, Tt, _ = _matrices()
    _env(monkeypatch, stream, chunk)
    return bpmf_amd.gibbs(eng, M, Mt, T, NROWS, NCOLS, nsims=3, burnin=0, Tt=Tt, **kw)


@pytest.mark.parametrize("chunk", [None, 64], ids=["chunk-auto", "chunk-64"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_three_iteration_chain_is_bit_identical(oracle, hip_engine_factory, monkeypatch, K, chunk):
    M, Mt, T, Tt, _ = _matrices()
    eng = hip_engine_factory(K)
    new = _chain(eng, monkeypatch, True, chunk)
    old = _chain(eng, monkeypatch, False, chunk)
    assert np.array_equal(new["U"], old["U"]) and np.array_equal(new["V"], old["V"])
    assert new["rmse"] == old["rmse"] and new["rmse_avg"] == old["rmse_avg"]
    if ("chain", K) not in _CACHE:
        _CACHE[("chain", K)] = oracle.gibbs(K, M, Mt, T, Tt, nsims=3, burnin=0)
    ref = _CACHE[("chain", K)]
    scale = max(np.abs(ref["U"]).max(), np.abs(ref["V"]).max())
    err = max(np.abs(new["U"] - ref["U"]).max(), np.abs(new["V"] - ref["V"]).max()) / scale
    print("gather-stream chain K %d chunk %s: factors %.3e" % (K, chunk, err))
    assert err < 1e-6
    assert abs(new["final_rmse_avg"] - ref["final_rmse_avg"]) < 1e-6


def test_adaptive_noise_reads_the_stream(hip_engine_factory, monkeypatch):
    """alpha is a multiply in the kernel, not part of the stream: a chain whose alpha changes every iteration is the same."""
    eng = hip_engine_factory(32)
    kw = dict(alpha=1.5, noise="adaptive", alpha_prior=(2.0, 0.5))
    new = _chain(eng, monkeypatch, True, 64, **kw)
    old = _chain(eng, monkeypatch, False, 64, **kw)
    assert len(set(new["alpha"])) == 3 and new["alpha"][0] == 1.5     # alpha does move
    assert new["alpha"] == old["alpha"] and new["train_rmse"] == old["train_rmse"]
    assert np.array_equal(new["U"], old["U"]) and np.array_equal(new["V"], old["V"])
    assert np.all(np.isfinite(new["U"])) and np.all(np.isfinite(new["V"]))


def test_probit_side_keeps_the_index_blocks(oracle, hip_engine_factory, monkeypatch):
    """The latent scores stand in for the ratings: the stream (built from the ratings) must not be read."""
    from tests import probit_ref
    from tests.test_gpu_parity import RTOL
    K = 16
    M = _matrices()[0]
    eng = hip_engine_factory(K)
    _env(monkeypatch, True, 64)
    rng = np.random.default_rng(77)
    X, Y = 0.7 * rng.standard_normal((NCOLS, K)), 0.7 * rng.standard_normal((NROWS, K))
    it, tag, thr = 3, 1, 3.6
    plain = eng.side_create(NCOLS, NROWS, *M, 0.0)
    assert eng.kernel_name(plain) == "k_sample1<%d>" % K              # the same side without the probit add-on: the stream
    eng.side_destroy(plain)
    me = eng.side_create(NCOLS, NROWS, *M, 0.0)
    ot = eng.side_create(NROWS, NCOLS, np.zeros(NROWS + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_probit(me, thr, tag)
    eng.set_items(me, X); eng.set_items(ot, Y)
    assert eng.kernel_name(me) == "k_sample1i<%d>" % K, eng.kernel_name(me)
    z = probit_ref.latent(M, X, Y, it, tag, thr)
    mu, LU, LF = oracle.hyper_sample(K, NCOLS, np.eye(K) * 0.2, it)
    want = X.copy()
    s_ref, p_ref, n_ref = oracle.sample_side(K, (M[0], M[1], z), 0.0, 1.0, Y, want, it, mu, LF)
    s, p, n = eng.sample_side(me, ot, it, 1.0, mu, LF)
    items = eng.get_items(me)
    eng.side_destroy(me); eng.side_destroy(ot)
    print("gather-stream probit K %d: factors %.3e" % (K, rel_err(items, want)))
    assert np.all(np.isfinite(items)) and rel_err(items, want) < RTOL
    assert rel_err(s, s_ref) < 1e-8 and rel_err(p, p_ref) < 1e-8 and abs(n - n_ref) <= 1e-8 * abs(n_ref)
