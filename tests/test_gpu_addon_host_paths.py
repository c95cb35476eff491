"""The host code the likelihood add-ons share (probit, ordinal, censored ratings, Student-t noise, per-rating weights, implicit
feedback), on the GPU: the one check of a side's latent fail word, the refusals the setters give each other, and the one
"the latent kernel is queued already" flag of the stateful path.

A synthetic 40 x 30 matrix with 300 ratings in 1 .. 5: more than one tile of 256 ratings on either side, fewer than one tile of
censored entries.  K = 8 in fp64 and K = 128 in fp32 (the two branches of the launchers' dispatch; Student-t noise is fp64 only).

  * the fail word of every kind: a NaN factor row makes the half-iteration fail with BPMF_HIP_ENUM and that kind's sentence, the
    word is reset, and the same iteration from the restored factors gives the latent array it gave before, byte for byte
    (tests/test_gpu_censored.py::test_ratings_are_left_alone_and_arguments_checked is the model, and keeps its censored case)
  * twelve states of a side x eleven setters: (code, message) or "ok" of every cell against tests/golden/addon_refusals.json,
    which the library wrote before the refusals came from one table
  * one bpmf_hip_sys_sample on every kind against bpmf_hip_sample_side from the same factors and hyper-parameters: latent array
    and factors byte for byte (the latent kernel ran once ahead of the sampler, not twice and not never)
"""
import json
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import util

pytestmark = pytest.mark.gpu

NU, NM, NNZ = 40, 30, 300
ENUM = -5
LEVELS = np.arange(1.0, 6.0)
SENTENCE = {
    "probit": r"probit: the truncated-normal draw of rating \d+ was rejected 64 times \(non-finite factors\?\)",
    "ordinal": r"ordinal: the score of rating \d+ is not finite \(non-finite factors\?\)",
    "censored": r"censored: the truncated-normal draw of rating \d+ was rejected 64 times \(non-finite factors\?\)",
    "robust": r"robust: the weight of rating \d+ could not be drawn: 64 rejections, or a residual that is not finite "
              r"\(non-finite factors\?\)",
}
ALPHA = {"probit": 1.0, "ordinal": 1.0, "censored": 2.5, "robust": 2.5}
CASES = [(kind, 8, "f64") for kind in SENTENCE] + [(kind, 128, "f32") for kind in ("probit", "ordinal", "censored")]


def _matrix():
    """(M, Mt): the ratings by movie (30 columns, 40 rows) and by user"""
    rng = np.random.default_rng(20)
    cells = rng.choice(NU * NM, NNZ, replace=False)
    vals = rng.integers(1, 6, NNZ).astype(np.float64)
    M = sp.coo_matrix((vals, (cells // NM, cells % NM)), shape=(NU, NM))
    return util.csc_arrays(M), util.csc_arrays(M.T)


def _flags(nnz):
    f = np.zeros(nnz, np.int8)
    f[3::7] = 1
    f[5::11] = -1
    return f


def _factors(K, dtype):
    """(V [30, K], U [40, K]), representable in the factors' type"""
    rng = np.random.default_rng(21)
    V, U = 0.4 * rng.standard_normal((NM, K)), 0.4 * rng.standard_normal((NU, K))
    if dtype == "f32":
        V, U = V.astype(np.float32).astype(np.float64), U.astype(np.float32).astype(np.float64)
    return V, U


def _hyper(K, ncols, it):
    import bpmf_amd
    rng = np.random.default_rng(22 + K)
    A = rng.standard_normal((K, 3 * K))
    return bpmf_amd.engine.hyper_sample(K, ncols, A @ A.T / (3 * K), it)


def _make(eng, kind, A, nrows, partner=None):
    """a side over the ratings A with the latent step of `kind` (any other word: none), and its partner: the transposed ratings
    `partner`, or none.  The mean rating is 0 where the model asks for it."""
    ncols = len(A[0]) - 1
    me = eng.side_create(ncols, nrows, *A, 0.0 if kind in ("probit", "ordinal", "implicit") else util.mean_rating(A))
    empty = (np.zeros(nrows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    ot = eng.side_create(nrows, ncols, *(partner or empty), 0.0)
    if kind == "probit":
        eng.set_probit(me, 3.0, 1)
    elif kind == "ordinal":
        eng.set_ordinal(me, LEVELS, None, 11)
    elif kind == "censored":
        eng.set_censored(me, _flags(me.nnz), 5)
    elif kind == "robust":
        eng.set_robust(me, 4.0, 7)
    return me, ot


def _latent(eng, kind, side):
    """the array the kind's latent kernel wrote for the side's newest launch, as bytes"""
    if kind == "probit":
        return eng.probit_latent(side, side.nnz).tobytes()
    if kind == "ordinal":
        return eng.ordinal_latent(side, side.nnz).tobytes()
    if kind == "censored":
        return eng.censored_latent(side).tobytes()
    sw, zw = eng.weights_get(side)
    return sw.tobytes() + zw.tobytes()


# ---- 1. the fail word of every kind ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,K,dtype", CASES)
def test_fail_word_is_reported_once_and_reset(kind, K, dtype):
    import bpmf_amd
    M, _ = _matrix()
    V, U = _factors(K, dtype)
    alpha = ALPHA[kind]
    eng = bpmf_amd.HipEngine(K, dtype=dtype)
    try:
        me, ot = _make(eng, kind, M, NU)
        eng.set_items(me, V); eng.set_items(ot, U)
        mu, LU, LF = _hyper(K, NM, 2)
        eng.sample_side(me, ot, 2, alpha, mu, LF)
        before = _latent(eng, kind, me)
        # a NaN factor row in a column with ratings (censored: with a censored rating): every draw of that column fails
        col_of = np.repeat(np.arange(NM), np.diff(M[0]))
        pos = np.flatnonzero(_flags(me.nnz)) if kind == "censored" else np.arange(me.nnz)
        bad = V.copy(); bad[int(col_of[pos[len(pos) // 2]])] = np.nan
        eng.set_items(me, bad)
        with pytest.raises(bpmf_amd.BpmfHipError) as e:
            eng.sample_side(me, ot, 3, alpha, mu, LF)
        assert e.value.code == ENUM, str(e.value)
        assert re.fullmatch("bpmf_hip error -5: " + SENTENCE[kind], str(e.value)), str(e.value)
        # the word was reset: the same iteration from the restored factors succeeds and draws what it drew before
        eng.set_items(me, V)
        eng.sample_side(me, ot, 2, alpha, mu, LF)
        assert _latent(eng, kind, me) == before
    finally:
        eng.close()


# ---- 2. the refusals of the setters against the recorded table -------------------------------------------------------------------------

STATES = ("plain", "probit", "ordinal", "censored", "robust", "weights", "implicit", "features", "prop_posterior", "reduce",
          "hyper_reserved", "shard")
SETTERS = ("set_probit", "set_ordinal", "set_censored", "set_robust", "set_weights", "set_implicit", "set_features_dense",
           "set_features_sparse", "set_prop_posterior", "sys_set_reduce", "hyper_reserve")


def _state(eng, state, M, Mt):
    """a fresh side in `state` and its partner (the other orientation of the ratings)"""
    F = np.random.default_rng(23).standard_normal((NM, 3))
    if state == "shard":                                             # columns 0 .. 9 of 30
        n = int(M[0][10])
        me = eng.side_create(NM, NU, M[0][:11], M[1][:n], M[2][:n], util.mean_rating(M), 0, 10)
        return me, eng.side_create(NU, NM, *Mt, 0.0)
    me, ot = _make(eng, state, M, NU, Mt)
    if state == "implicit":
        eng.set_implicit(me, 0.1)
    elif state == "weights":
        eng.set_weights(me, np.linspace(0.5, 2.0, me.nnz))
    elif state == "features":
        eng.set_features(me, F, 5.0, 3)
    elif state == "prop_posterior":
        eng.set_prop_posterior(me, np.tile(np.eye(eng.K).ravel(), (NM, 1)))
    elif state == "reduce":
        eng.sys_set_reduce(me, ot)
    elif state == "hyper_reserved":
        eng.hyper_reserve(me, 2)
    return me, ot


def _apply(eng, setter, me, ot):
    F = np.random.default_rng(24).standard_normal((NM, 3))
    if setter == "set_probit":
        eng.set_probit(me, 3.0, 2)
    elif setter == "set_ordinal":
        eng.set_ordinal(me, LEVELS, None, 12)
    elif setter == "set_censored":
        eng.set_censored(me, _flags(me.nnz), 6)
    elif setter == "set_robust":
        eng.set_robust(me, 4.0, 8)
    elif setter == "set_weights":
        eng.set_weights(me, np.linspace(0.5, 2.0, me.nnz))
    elif setter == "set_implicit":
        eng.set_implicit(me, 0.1)
    elif setter == "set_features_dense":
        eng.set_features(me, F, 5.0, 4)
    elif setter == "set_features_sparse":
        eng.set_features(me, sp.csr_matrix(np.where(np.abs(F) > 0.5, F, 0.0)), 5.0, 4)
    elif setter == "set_prop_posterior":
        eng.set_prop_posterior(me, np.tile(np.eye(eng.K).ravel(), (me.col_to - me.col_from, 1)))
    elif setter == "sys_set_reduce":
        eng.sys_set_reduce(me, ot)
    elif setter == "hyper_reserve":
        eng.hyper_reserve(me, 2)


def refusal_table():
    """{"state/setter": "ok" | [code, message]} of every cell, each on a fresh side of one K = 8 fp64 engine"""
    import bpmf_amd
    M, Mt = _matrix()
    table = {}
    eng = bpmf_amd.HipEngine(8)
    try:
        for state in STATES:
            for setter in SETTERS:
                me, ot = _state(eng, state, M, Mt)
                try:
                    _apply(eng, setter, me, ot)
                    cell = "ok"
                except bpmf_amd.BpmfHipError as e:
                    cell = [e.code, str(e).split(": ", 1)[1]]
                table["%s/%s" % (state, setter)] = cell
                eng.side_destroy(me); eng.side_destroy(ot)
    finally:
        eng.close()
    return table


def test_refusals_against_the_recorded_table():
    with open(os.path.join(util.GOLDEN, "addon_refusals.json")) as f:
        want = json.load(f)
    got = refusal_table()
    assert sorted(got) == sorted(want) and len(got) == len(STATES) * len(SETTERS)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


# ---- 3. the stateful path enqueues the latent kernel once -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind,K,dtype", CASES)
def test_sys_sample_draws_what_sample_side_draws(kind, K, dtype):
    import bpmf_amd
    M, Mt = _matrix()
    V, U = _factors(K, dtype)
    alpha = ALPHA[kind]
    eng = bpmf_amd.HipEngine(K, dtype=dtype)
    try:
        me, ot = _make(eng, kind, M, NU, Mt)
        eng.set_items(me, V); eng.set_items(ot, U)
        eng.sys_sample(me, ot, alpha)
        it, _, _, mu, LF, _ = eng.sys_state(me)
        z1, X1 = _latent(eng, kind, me), eng.get_items(me)
        me2, ot2 = _make(eng, kind, M, NU, Mt)
        eng.set_items(me2, V); eng.set_items(ot2, U)
        eng.sample_side(me2, ot2, it, alpha, mu, LF)
        assert _latent(eng, kind, me2) == z1
        assert eng.get_items(me2).tobytes() == X1.tobytes()
        assert np.all(np.isfinite(X1)) and not np.array_equal(X1, V)
    finally:
        eng.close()
