"""The three kernels that share assemble44 -- k_sample1 (gather stream), k_sample1i (index blocks), k_sample1w (per-rating
weights) -- after one stateless half-iteration on the 64 x 48 matrix of tests/test_gpu_gather_stream.py.

K = 8, 16, 32, at the automatic chunk (every column whole: the accumulators go from the Gram straight into assemble44) and at
BPMF_HIP_CHUNK=64 (the columns of 65, 128, 129 and 200 ratings are chunked: the last chunk to arrive adds the parked
accumulators and assembles the sums).  The columns without ratings assemble accumulators that are all zero.

  * stream == index blocks bit for bit, and both against the oracle at the bars of tests/test_gpu_parity.py (1e-9 of max|U|
    on the factors, 1e-8 on the sums);
  * the weighted form, with a seeded Gamma(2, 0.5) weight per rating, against the expanded-rows reference of
    tests/weights_ref.py at the same bars.
"""
import numpy as np
import pytest

from tests import util
from tests import weights_ref
from tests.test_gpu_gather_stream import NCOLS, NROWS, _env, _half_iteration, _matrices, _reference
from tests.test_gpu_parity import check_half_iteration, rel_err

pytestmark = pytest.mark.gpu

_CACHE = {}


def _weighted_reference(oracle, K):
    """The weights and the reference's half-iteration with them: once per K, shared, never written."""
    if K not in _CACHE:
        M = _matrices()[0]
        U, it, alpha, mu, LF = _reference(oracle, K)[0]
        w = weights_ref.seeded_weights(len(M[2]), 440 + K)
        want = np.zeros((NCOLS, K))
        s, p, n = weights_ref.sample_side_weighted(oracle, K, M, w, util.mean_rating(M), alpha, U, want, it, mu, LF)
        w.setflags(write=False); want.setflags(write=False)
        _CACHE[K] = (w, (want, s, p, n))
    return _CACHE[K]


def _weighted_half_iteration(eng, inp, w):
    M = _matrices()[0]
    U, it, alpha, mu, LF = inp
    me = eng.side_create(NCOLS, NROWS, *M, util.mean_rating(M))
    ot = eng.side_create(NROWS, NCOLS, np.zeros(NROWS + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    eng.set_weights(me, w)
    name, info = eng.kernel_name(me), eng.schedule_info(me)
    eng.set_items(ot, U)
    s, p, n = eng.sample_side(me, ot, it, alpha, mu, LF)
    items = eng.get_items(me)
    eng.side_destroy(me); eng.side_destroy(ot)
    return name, info, (items, s, p, n)


@pytest.mark.parametrize("chunk", [None, 64], ids=["chunk-auto", "chunk-64"])
@pytest.mark.parametrize("K", [8, 16, 32])
def test_stream_index_blocks_and_weighted_form(oracle, hip_engine_factory, monkeypatch, K, chunk):
    counts = _matrices()[4]
    assert (counts == 0).sum() >= 2 and (counts > 64).sum() >= 4      # empty columns; columns BPMF_HIP_CHUNK=64 cuts
    inp, ref = _reference(oracle, K)
    eng = hip_engine_factory(K)
    out = {}
    for stream in (True, False):
        _env(monkeypatch, stream, chunk)
        name, info, hip = _half_iteration(eng, inp)
        assert name == ("k_sample1<%d>" if stream else "k_sample1i<%d>") % K, name
        if chunk == 64:
            assert info["chunk"] == 64 and info["chunked_columns"] == (counts > 64).sum(), info
        print("assemble K %d chunk %s %s: factors %.3e sum %.3e prod %.3e"
              % (K, chunk, name, rel_err(hip[0], ref[0]), rel_err(hip[1], ref[1]), rel_err(hip[2], ref[2])))
        check_half_iteration(hip, ref)
        out[stream] = hip
    assert np.array_equal(out[True][0], out[False][0])                # bit for bit
    assert np.array_equal(out[True][1], out[False][1]) and np.array_equal(out[True][2], out[False][2]) and out[True][3] == out[False][3]

    w, wref = _weighted_reference(oracle, K)
    _env(monkeypatch, True, chunk)
    name, info, hip = _weighted_half_iteration(eng, inp, w)
    assert name == "k_sample1w<%d>" % K, name
    if chunk == 64:
        assert info["chunk"] == 64 and info["chunked_columns"] == (counts > 64).sum(), info
    print("assemble K %d chunk %s %s: factors %.3e sum %.3e prod %.3e"
          % (K, chunk, name, rel_err(hip[0], wref[0]), rel_err(hip[1], wref[1]), rel_err(hip[2], wref[2])))
    check_half_iteration(hip, wref)
