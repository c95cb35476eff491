"""What the entry points that read two sample rings refuse, in which order, and what they leave alone: topn, topn_scored, rank_eval,
predict_block, predict_cells, diag_cells and score_cells (one table), the five *_last_ms entry points, and the empty calls.  One K = 8
engine, sides of 6 x 5 and 5 x 6 with a handful of ratings, rings of 2 samples (of DIAG_MIN_SAMPLES where the diagnostics must run).

  1. each fault alone: the message with its "<who>:" prefix and the error code (BPMF_HIP_EINVAL)
  2. two faults at once: the one that is reported
  3. every *_last_ms refuses with its own message before the first timed call and gives a time >= 0 after one
  4. the empty calls return OK and leave the outputs as they were
"""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp
import bpmf_amd
from tests import util

pytestmark = pytest.mark.gpu

K, NQ, NC, MEAN, EINVAL = 8, 6, 5, 3.0, -1
ENTRIES = ("topn", "topn_scored", "rank_eval", "predict_block", "predict_cells", "diag_cells", "score_cells")
RANKINGS = ("topn", "topn_scored")
RANGED = ("topn", "topn_scored", "rank_eval", "predict_block")
ptr = lambda a: a.ctypes.data_as(C.c_void_p)


def pair(eng, S=None, Sc=None, reserve=None):
    """(query side of 6 columns, candidate side of 5) with seven ratings between them; rings of S and Sc samples (None: no ring)"""
    rows, cols = np.array([1, 2, 3, 4, 0, 0, 2]), np.array([0, 1, 2, 3, 4, 5, 5])      # (candidate, query): query 0 has not rated candidate 0
    A = sp.coo_matrix((np.arange(1.0, 8.0), (rows, cols)), shape=(NC, NQ)).tocsc()
    sq, sc = eng.side_create(NQ, NC, *util.csc_arrays(A), MEAN), eng.side_create(NC, NQ, *util.csc_arrays(A.T.tocsc()), MEAN)
    rng = np.random.default_rng(3)
    for side, n in ((sq, S), (sc, S if Sc is None else Sc)):
        if n is not None:
            eng.samples_reserve(side, reserve or max(n, 1))
            eng.samples_set(side, 0.5 * rng.standard_normal((side.ncols, n, K)))
    return sq, sc


@pytest.fixture(scope="module")
def world(hip_engine_factory):
    eng = hip_engine_factory(K)
    other = bpmf_amd.HipEngine(K)
    w = dict(eng=eng, noring=pair(eng), zero=pair(eng, 0), uneven=pair(eng, 2, 1), ok=pair(eng, 2), diag=pair(eng, eng.DIAG_MIN_SAMPLES),
             foreign=pair(other, 2))
    yield w
    for name, sides in w.items():
        if name != "eng":
            for s in sides:
                (other if name == "foreign" else eng).side_destroy(s)
    other.close()


def call(eng, name, sq, sc, n=2, q_to=None, c_to=None, kind="ucb", tptr=None, cells=([0, 1], [1, 2]), alpha=2.0):
    """one call of the entry point `name` with valid arguments, but for the ones given"""
    if name == "topn":
        return eng.topn(sq, sc, MEAN, n, 0, q_to)
    if name == "topn_scored":
        nq = sq.ncols if q_to is None else q_to
        out = [np.empty((nq, max(n, 1)), np.int32)] + [np.empty((nq, max(n, 1))) for _ in range(3)]
        kind = eng.SCORE_KINDS.get(kind, kind)
        return bpmf_amd._lib.check(eng.lib.bpmf_hip_topn_scored(sq.handle, sc.handle, MEAN, n, 0, nq, 1, kind, 1.0, 0.0, *map(ptr, out)))
    if name == "rank_eval":
        nq = sq.ncols if q_to is None else q_to
        if tptr is None:                                         # query 0 holds out candidate 0
            tptr = np.r_[0, np.ones(nq, np.int64)]
        tptr = np.asarray(tptr, np.int64)
        return eng.rank_eval(sq, sc, tptr, np.zeros(int(tptr[-1]), np.int32), MEAN, 0, q_to)
    if name == "predict_block":
        return eng.predict_block(sq, sc, MEAN, 0, q_to, 0, c_to)
    if name == "predict_cells":
        return eng.predict_cells(sq, sc, MEAN, *cells)
    if name == "diag_cells":
        return eng.diag_cells(sq, sc, MEAN, *cells)
    assert name == "score_cells"
    return eng.score_cells(sq, sc, MEAN, *cells, np.ones(len(cells[0])), alpha)


def refused(eng, text, name, sides, **kw):
    with pytest.raises(bpmf_amd.BpmfHipError, match=re.escape(text)) as e:
        call(eng, name, *sides, **kw)
    assert e.value.code == EINVAL, (name, text, e.value.code)
    return str(e.value)


def topn_max_n(world):
    """read from the library: the refusal of n = 0 names the range"""
    m = re.search(r"n = 0 \(1 \.\. (\d+)\)", refused(world["eng"], "topn: n = 0 (1 .. ", "topn", world["ok"], n=0))
    return int(m.group(1))


# ---- 1. each fault alone -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ENTRIES)
def test_each_fault_alone(world, name):
    eng = world["eng"]
    refused(eng, name + ": no sample ring on both sides (bpmf_hip_side_samples_reserve)", name, world["noring"])
    refused(eng, name + ": both sides must hold the same number (>= 1) of samples: 0 and 0", name, world["zero"])
    refused(eng, name + ": both sides must hold the same number (>= 1) of samples: 2 and 1", name, world["uneven"])
    refused(eng, name + ": the two sides belong to different contexts", name, (world["ok"][0], world["foreign"][1]))
    if name in RANKINGS:
        top = topn_max_n(world)
        assert top >= 1
        for n in (0, top + 1):
            refused(eng, "%s: n = %d (1 .. %d)" % (name, n, top), name, world["ok"], n=n)
    if name in RANGED:
        refused(eng, name + ": query range out of bounds", name, world["ok"], q_to=NQ + 1)
    if name == "predict_block":
        refused(eng, "predict_block: candidate range out of bounds", name, world["ok"], c_to=NC + 1)
    call(eng, name, *world["diag" if name == "diag_cells" else "ok"])     # and the valid call is served


def test_diag_cells_needs_its_samples(world):
    eng = world["eng"]
    assert eng.DIAG_MIN_SAMPLES > 2
    refused(eng, "diag_cells: 2 samples: the estimator takes %d .. " % eng.DIAG_MIN_SAMPLES, "diag_cells", world["ok"])


# ---- 2. precedence -------------------------------------------------------------------------------------------------------------------------

def test_precedence(world):
    eng = world["eng"]
    refused(eng, "topn: n = 0 (1 .. ", "topn", world["noring"], n=0)
    refused(eng, "topn_scored: unknown score kind 7 (", "topn_scored", world["ok"], kind=7, n=0)
    refused(eng, "rank_eval: tptr decreases at query 1", "rank_eval", world["noring"], tptr=[0, 2, 1, 1, 1, 1, 1])
    refused(eng, "predict_block: no sample ring on both sides", "predict_block", world["noring"], q_to=NQ + 1)
    refused(eng, "predict_cells: cell 1 (1, 5) is out of range (6 queries x 5 candidates)", "predict_cells", world["noring"], cells=([0, 1], [1, NC]))
    refused(eng, "score_cells: both sides must hold the same number (>= 1) of samples: 2 and 1", "score_cells", world["uneven"], alpha=[1.0, 2.0, 3.0])
    refused(eng, "score_cells: 3 values of alpha for 2 samples (1 or as many)", "score_cells", world["ok"], alpha=[1.0, 2.0, 3.0])


# ---- 3. the timers -------------------------------------------------------------------------------------------------------------------------

def test_every_last_ms(hip_engine_factory):
    eng = hip_engine_factory(K)
    S = eng.DIAG_MIN_SAMPLES
    sq, sc = pair(eng, S)
    cells = ([0, 1, 5], [1, 2, 4])
    one_row = sp.csr_matrix((np.array([4.0, 2.0]), (np.array([0, 0]), np.array([1, 3]))), shape=(1, NC))

    def fold():
        eng.hyper_reserve(sq, S)
        for s in range(S):
            eng.hyper_add(sq, 2.0, np.zeros(K), np.eye(K))
        eng.foldin(sq, sc, MEAN, one_row, 7)
    table = (("predict_cells_last_ms", "no launch with the side as the queries has been timed (bpmf_hip_predict_cells)", eng.predict_cells_last_ms,
              lambda: eng.predict_cells(sq, sc, MEAN, *cells)),
             ("similar_last_ms", "no ranking of the side has been timed (bpmf_hip_similar)", eng.similar_last_ms, lambda: eng.similar(sq, 2)),
             ("diag_last_ms", "no diagnostics with the side as the queries have been timed (bpmf_hip_diag_cells)", eng.diag_last_ms,
              lambda: eng.diag_cells(sq, sc, MEAN, *cells)),
             ("score_last_ms", "no scoring with the side as the queries has been timed (bpmf_hip_score_cells)", eng.score_last_ms,
              lambda: eng.score_cells(sq, sc, MEAN, *cells, np.ones(3), 2.0)),
             ("foldin_last_ms", "no launch of the side has been timed (bpmf_hip_foldin)", eng.foldin_last_ms, fold))
    try:
        for who, text, last_ms, run in table:                  # all of them before any of the calls: no timer answers for another
            with pytest.raises(bpmf_amd.BpmfHipError, match=re.escape(who + ": " + text)) as e:
                last_ms(sq)
            assert e.value.code == EINVAL, who
        for who, text, last_ms, run in table:
            run()
            assert last_ms(sq) >= 0.0, who
        with pytest.raises(bpmf_amd.BpmfHipError, match="predict_cells_last_ms: no launch"):
            eng.predict_cells_last_ms(sc)                      # the candidate side of the calls has timed nothing
        ms = C.c_float()
        for f in ("predict_cells", "similar", "diag", "score", "foldin"):
            fn = getattr(eng.lib, "bpmf_hip_%s_last_ms" % f)
            assert fn(None, C.byref(ms)) == EINVAL and fn(sq.handle, None) == EINVAL
            assert ("%s_last_ms: NULL argument" % f) in eng.lib.bpmf_hip_last_error().decode()
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 4. the empty calls --------------------------------------------------------------------------------------------------------------------

def test_empty_calls_leave_the_outputs_alone(world):
    eng = world["eng"]
    lib = eng.lib
    sq, sc = (s.handle for s in world["diag"])
    f64 = lambda: np.full(4, -7.5)
    i32 = lambda: np.full(4, -77, np.int32)
    hold, al = np.zeros(1, np.int32), np.ones(1)
    tptr = np.zeros(1, np.int64)

    def untouched(rc, *outs):
        assert rc == 0, lib.bpmf_hip_last_error().decode()
        for a in outs:
            assert (a == (-77 if a.dtype == np.int32 else -7.5)).all()
    o = [i32(), f64(), f64()]
    untouched(lib.bpmf_hip_topn(sq, sc, MEAN, 2, 3, 3, 1, *map(ptr, o)), *o)
    o = [i32(), f64(), f64(), f64()]
    untouched(lib.bpmf_hip_topn_scored(sq, sc, MEAN, 2, 3, 3, 1, 0, 1.0, 0.0, *map(ptr, o)), *o)
    o = [i32(), i32()]
    untouched(lib.bpmf_hip_rank_eval(sq, sc, MEAN, 3, 3, 1, ptr(tptr), ptr(hold), *map(ptr, o)), *o)
    o = [f64(), f64(), f64()]
    untouched(lib.bpmf_hip_predict_cells(sq, sc, MEAN, 0, ptr(hold), ptr(hold), 1, 0.5, 0.0, *map(ptr, o)), *o)
    o = [f64(), f64(), f64(), f64()]
    untouched(lib.bpmf_hip_diag_cells(sq, sc, MEAN, 0, ptr(hold), ptr(hold), *map(ptr, o)), *o)
    o = [f64(), f64(), f64(), f64()]
    untouched(lib.bpmf_hip_score_cells(sq, sc, MEAN, 0, ptr(hold), ptr(hold), ptr(al), None, None, 0, 0.0, 1, ptr(al), *map(ptr, o)), *o)
    for ranges in ((2, 2, 0, NC), (0, NQ, 4, 4), (NQ, NQ, NC, NC)):
        o = [f64(), f64()]
        untouched(lib.bpmf_hip_predict_block(sq, sc, MEAN, *ranges, *map(ptr, o)), *o)
    # the empty calls are still checked: the same calls on sides without rings are refused
    sq, sc = (s.handle for s in world["noring"])
    o = [i32(), f64(), f64()]
    assert lib.bpmf_hip_topn(sq, sc, MEAN, 2, 3, 3, 1, *map(ptr, o)) == EINVAL
    assert lib.bpmf_hip_predict_cells(sq, sc, MEAN, 0, ptr(hold), ptr(hold), 0, 0.0, 0.0, ptr(o[1]), ptr(o[2]), None) == EINVAL
    assert lib.bpmf_hip_predict_block(sq, sc, MEAN, 2, 2, 0, NC, ptr(o[1]), ptr(o[2])) == EINVAL
