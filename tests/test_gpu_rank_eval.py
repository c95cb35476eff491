"""Held-out ranks on the device (bpmf_hip_rank_eval, engine.rank_eval).

  * exact: factors that are multiples of 1/8 in [-4, 4] make every score exact in fp64 in any order (and ties frequent), so rank and
    ncand must EQUAL the plain count of tests/implicit_ref.py, tie-break by candidate id included -- over the query / candidate counts
    around the 64-wide tile, several candidate splits, padded and fp32 contexts, 0 / 1 / 5 / 40 held-out entries per query, the first
    and the last candidate, a query that has rated everything but one candidate, with and without the exclusion, and a query slice
  * against bpmf_hip_topn: a held-out entry has rank <= 32 exactly when it is entry rank - 1 of its query's top-32 list -- an
    equality without a tolerance, which holds only if the two kernels give a pair's score the same bits
  * against numpy on Gaussian factors, as an interval: the candidates above s + d <= rank - 1 <= the candidates above s - d
  * refusals: a held-out rated cell, unsorted / repeated / out-of-range candidates, unequal ring counts
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import implicit_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

HELD = (0, 1, 5, 40)


def pattern(nq, nc, seed):
    """(query side, candidate side) as CSC triples: query q has rated a random 0 .. min(nc - 1, 30) candidates; query 0 has rated
    everything but candidate nc // 2"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for q in range(nq):
        if q == 0 and nc > 1:
            picked = [c for c in range(nc) if c != nc // 2]
        else:
            picked = rng.choice(nc, size=int(rng.integers(0, min(nc - 1, 30) + 1)), replace=False).tolist()
        rows += [int(c) for c in picked]; cols += [q] * len(picked)
    A = sp.coo_matrix((np.full(len(rows), 3.0), (rows, cols)), shape=(nc, nq)).tocsc()           # one column per query
    return util.csc_arrays(A), util.csc_arrays(A.T.tocsc())


def held_out(nq, nc, rated, seed):
    """per query 0, 1, 5 or 40 unrated candidates in turn (as many as there are), the first and the last candidate among them
    whenever they are unrated and there is room"""
    rng = np.random.default_rng(seed + 1)
    tptr, tcand = [0], []
    for q in range(nq):
        free = [c for c in range(nc) if c not in rated[q]]
        want = min(HELD[(q + 1) % 4], len(free))
        pick = set()
        for c in (0, nc - 1):
            if c in free and len(pick) < want:
                pick.add(c)
        rest = [c for c in free if c not in pick]
        pick |= set(rng.choice(rest, size=want - len(pick), replace=False).tolist()) if want > len(pick) else set()
        tcand += sorted(int(c) for c in pick)
        tptr.append(len(tcand))
    return np.array(tptr, np.int64), np.array(tcand, np.int32)


def fill(eng, nq, nc, S, seed, draw):
    """two sides over the seeded pattern with S samples in their rings -> (query side, candidate side, Us, Vs, rated)"""
    Q_side, C_side = pattern(nq, nc, seed)
    sq = eng.side_create(nq, nc, *Q_side, 0.0)
    sc = eng.side_create(nc, nq, *C_side, 0.0)
    rng = np.random.default_rng(seed)
    eng.samples_reserve(sq, S + 1); eng.samples_reserve(sc, S)           # (rings of different capacity: the strides differ)
    Us, Vs = draw(rng, (S, nq, eng.K)), draw(rng, (S, nc, eng.K))
    for s in range(S):
        eng.set_items(sq, Us[s]); eng.set_items(sc, Vs[s])
        eng.samples_add(sq); eng.samples_add(sc)
    return sq, sc, Us, Vs, ref.rated_sets(Q_side, nq)


def dyadic(rng, shape):
    return rng.integers(-32, 33, size=shape) / 8.0


EXACT = [(1, 700, 8, 2, "f64"), (1, 1, 3, 1, "f64"), (63, 63, 3, 1, "f64"), (64, 64, 32, 8, "f64"), (65, 65, 8, 2, "f64"),
         (65, 1, 8, 1, "f64"), (130, 200, 100, 2, "f64"), (130, 700, 8, 1, "f64"), (63, 65, 32, 2, "f64"), (64, 200, 128, 2, "f32")]


@pytest.mark.parametrize("nq,nc,K,S,dtype", EXACT, ids=["q%d-c%d-k%d-s%d-%s" % e for e in EXACT])
def test_ranks_exact(hip_engine_factory, nq, nc, K, S, dtype):
    eng = hip_engine_factory(K, dtype)
    sq, sc, Us, Vs, rated = fill(eng, nq, nc, S, 7 * nq + nc + K, dyadic)
    try:
        score = 0.5 + np.einsum("sqk,sck->qc", Us, Vs) / S               # exact: every term is a multiple of 1/64 below 2^53
        tptr, tcand = held_out(nq, nc, rated, nq + nc)
        if nq > 1 and nc > 1:
            assert len(rated[0]) == nc - 1 and set(np.diff(tptr).tolist()) >= {0, 1} and tcand[tptr[0]:tptr[1]].tolist() == [nc // 2]
        for excl in (True, False):
            rank, ncand = eng.rank_eval(sq, sc, tptr, tcand, 0.5, exclude_rated=excl)
            want_r, want_n = ref.count_ranks(score, rated, tptr, tcand, excl)
            assert np.array_equal(ncand, want_n), (excl, np.nonzero(ncand != want_n)[0][:5])
            assert np.array_equal(rank, want_r), (excl, np.nonzero(rank != want_r)[0][:5], rank[:8], want_r[:8])
            if nq >= 3:                                                  # a slice is the matching part of the full call
                a, b = 1, nq - 1
                r2, n2 = eng.rank_eval(sq, sc, tptr[a:b + 1] - tptr[a], tcand[tptr[a]:tptr[b]], 0.5, q_from=a, q_to=b, exclude_rated=excl)
                assert np.array_equal(r2, rank[tptr[a]:tptr[b]]) and np.array_equal(n2, ncand[a:b])
        if nq > 1 and nc > 1:
            assert ncand[0] == nc and rank[0] >= 1                       # (the last call ran without the exclusion)
        ties = sum(int((score[q] == score[q, c]).sum()) > 1 for q in range(nq) for c in tcand[tptr[q]:tptr[q + 1]])
        print("nq %d nc %d K %d S %d: %d entries, %d of them tied with another candidate" % (nq, nc, K, S, len(tcand), ties))
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def gauss(rng, shape):
    return rng.standard_normal(shape)


@pytest.mark.parametrize("nq,nc", [(130, 200), (3, 700)])
def test_ranks_are_the_top_n_lists(hip_engine_factory, nq, nc):
    """S = 3 at K = 8: the stacked inner dimension 24 is no multiple of 16.  No tolerance."""
    eng = hip_engine_factory(8)
    sq, sc, Us, Vs, rated = fill(eng, nq, nc, 3, 900 + nq, gauss)
    try:
        tptr, tcand = held_out(nq, nc, rated, nq)
        for excl in (True, False):
            rank, ncand = eng.rank_eval(sq, sc, tptr, tcand, 0.25, exclude_rated=excl)
            idx, mean, std = eng.topn(sq, sc, 0.25, 32, exclude_rated=excl)
            listed = 0
            for q in range(nq):
                assert ncand[q] == (nc - len(rated[q]) if excl else nc)
                for p in range(tptr[q], tptr[q + 1]):
                    if rank[p] <= 32:
                        assert idx[q, rank[p] - 1] == tcand[p], (q, p, rank[p], idx[q])
                        listed += 1
                    else:
                        assert tcand[p] not in idx[q], (q, p, rank[p])
            assert listed > 0
            # numpy, as an interval: no entry is left out
            score = 0.25 + np.einsum("sqk,sck->qc", Us, Vs) / 3
            d = 1e-12 * np.abs(score).max()
            for q in range(nq):
                ok = np.ones(nc, bool)
                if excl and rated[q]:
                    ok[sorted(rated[q])] = False
                for p in range(tptr[q], tptr[q + 1]):
                    c = tcand[p]
                    ok2 = ok.copy(); ok2[c] = False
                    lo, hi = int((score[q, ok2] > score[q, c] + d).sum()), int((score[q, ok2] > score[q, c] - d).sum())
                    assert lo <= rank[p] - 1 <= hi, (q, c, lo, rank[p], hi)
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_rank_eval_refusals(hip_engine_factory):
    import bpmf_amd
    eng = hip_engine_factory(8)
    nq, nc = 20, 30
    Q_side, C_side = pattern(nq, nc, 3)
    sq = eng.side_create(nq, nc, *Q_side, 0.0)
    sc = eng.side_create(nc, nq, *C_side, 0.0)
    rated = ref.rated_sets(Q_side, nq)
    tptr, tcand = held_out(nq, nc, rated, 3)
    try:
        with pytest.raises(bpmf_amd.BpmfHipError, match="rank_eval: no sample ring"):
            eng.rank_eval(sq, sc, tptr, tcand)
        eng.samples_reserve(sq, 2); eng.samples_reserve(sc, 2)
        with pytest.raises(bpmf_amd.BpmfHipError, match="same number"):
            eng.rank_eval(sq, sc, tptr, tcand)                           # no samples
        eng.samples_add(sq); eng.samples_add(sq); eng.samples_add(sc)
        with pytest.raises(bpmf_amd.BpmfHipError, match="same number .* 2 and 1"):
            eng.rank_eval(sq, sc, tptr, tcand)
        eng.samples_add(sc)
        rank, ncand = eng.rank_eval(sq, sc, tptr, tcand)
        assert len(rank) == len(tcand) and rank.min() >= 1 and np.all(rank <= np.repeat(ncand, np.diff(tptr)))
        # a held-out entry that is a rated cell of its query: named, and fine without the exclusion
        q = next(q for q in range(1, nq) if rated[q])
        c = min(rated[q])
        one_ptr = np.zeros(nq + 1, np.int64); one_ptr[q + 1:] = 1
        with pytest.raises(bpmf_amd.BpmfHipError, match=r"held-out cell \(query %d, candidate %d\) is a rated cell" % (q, c)):
            eng.rank_eval(sq, sc, one_ptr, np.array([c], np.int32))
        eng.rank_eval(sq, sc, one_ptr, np.array([c], np.int32), exclude_rated=False)
        two_ptr = np.zeros(nq + 1, np.int64); two_ptr[nq:] = 2           # the last query (query 0 has one free candidate only)
        free = sorted(set(range(nc)) - rated[nq - 1])
        with pytest.raises(bpmf_amd.BpmfHipError, match="not ascending and distinct"):
            eng.rank_eval(sq, sc, two_ptr, np.array([free[1], free[0]], np.int32))
        with pytest.raises(bpmf_amd.BpmfHipError, match="not ascending and distinct"):
            eng.rank_eval(sq, sc, two_ptr, np.array([free[0], free[0]], np.int32))
        with pytest.raises(bpmf_amd.BpmfHipError, match="out of range"):
            eng.rank_eval(sq, sc, two_ptr, np.array([free[0], nc], np.int32))
        with pytest.raises(bpmf_amd.BpmfHipError, match="query range"):
            eng.rank_eval(sq, sc, np.zeros(2, np.int64), np.zeros(0, np.int32), q_from=nq, q_to=nq + 1)
        with pytest.raises(ValueError, match="tptr must hold"):
            eng.rank_eval(sq, sc, tptr[:-1], tcand)
        # no query at all, and queries without a held-out entry
        r0, n0 = eng.rank_eval(sq, sc, np.zeros(1, np.int64), np.zeros(0, np.int32), q_from=4, q_to=4)
        assert len(r0) == 0 and len(n0) == 0
        r0, n0 = eng.rank_eval(sq, sc, np.zeros(nq + 1, np.int64), np.zeros(0, np.int32))
        assert len(r0) == 0 and np.array_equal(n0, [nc - len(rated[q]) for q in range(nq)])
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)
