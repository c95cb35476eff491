"""Every sampler form at the rating counts and chunk boundaries where its code branches.

The column samplers branch on how many ratings a column has: the Gram loops work in blocks of 64 / 16 ratings with k-steps of
4, build_schedule cuts a column that is longer than the chunk into pieces (multiples of 16, the last takes the rest) whose
partials the last-arriving piece adds in chunk order before it re-arms the column's ticket, and at K = 64 the light columns
leave for the product form when they are at least half of the side.  BPMF_HIP_CHUNK / BPMF_HIP_MODE / BPMF_HIP_PF are read when
a side is created, so the whole matrix of cases runs on sides of a few dozen columns:

  1. the edge side (0 .. 257 ratings per column, three 32s and three 64s) through k_sample1 / k_sample4 at K = 8, 16, 32, the
     slab form, k_sample_wg2 in fp64 and fp32 and the padded sizes 20, 50, 100, at the automatic chunk, at 16, at 40 (rounded to
     48) and at 272 (nothing cut): the schedule's properties, three launches A, B, A on the same side against the oracle, and
     launch 3 == launch 1 bit for bit (a stale partial, a ticket that was not re-armed or a piece added twice breaks that with
     no tolerance involved);
  2. a col_from / col_to slice of it;
  3. the product form's class cuts for BPMF_HIP_PF in {unset, 0, 1, 2, 3, 4, 6, 7, 15}, the exact-half rule, and the fall-back to
     the full item list with per-column priors / the diagonal-only variant on a side that HAS a light / heavy split;
  4. the stateful loop (bpmf_amd.gibbs) on sides whose columns are chunked at 16;
  5. a failed factorisation in chunked columns, after which the side must still give the oracle's sample.

Tolerances are the project's own: fp64 RTOL = 1e-9 of max|U| on the factors and 1e-8 on the sums (tests/test_gpu_parity.py),
fp32 2e-3 of max|U| and 1e-3 on the sums with the other side's factors rounded to fp32 first (tests/test_gpu_f32.py), RMSE
traces and factors of a coupled run 1e-6.

The automatic chunk.  With BPMF_HIP_CHUNK unset the chunk has a floor of 16 K ratings in k_sample1, a quarter of that in
k_sample4 and 256 at K = 64 / 128, so the 257-rating column (and, in k_sample4 at K = 8, every column above 32) IS cut at the
automatic chunk: only k_sample1<32> (floor 512) leaves the edge side uncut.  The side therefore reports its chunk
(schedule_info["chunk"], word 15 of bpmf_hip_side_schedule_info) and the unset case asserts the general rule against it -- a
column is chunked exactly when it is longer than the reported chunk, hence chunked_columns == 0 wherever the chunk is >= 257 --
and the run in which no column of any form is cut is the extra case BPMF_HIP_CHUNK=272.

Observed on an MI355X, worst over all cases of a form (factors relative to max|U| / sums; bars 1e-9 / 1e-8, fp32 2e-3 / 1e-3):
  k_sample1<8 | 16 | 32>        4.2e-16 | 1.0e-15 | 1.3e-15  /  1.3e-15      k_sample4<8 | 16 | 32>   4.2e-16 | 7.0e-16 | 9.5e-16  /  1.1e-15
  slab K = 64                   2.3e-15 / 1.8e-15                             k_sample_wg2 fp64        3.7e-15 / 3.2e-15
  k_sample_wg2 fp32             3.7e-6 / 4.1e-6                               padded 20 | 50 | 100     5.9e-16 | 1.3e-15 | 5.6e-15  /  2.7e-15
  slice (K = 32, 64, 128)       3.7e-15 / 3.5e-15                             product form, K = 64 | 50, every BPMF_HIP_PF   1.8e-15 / 1.6e-15
  half rule                     5.5e-15 / 5.0e-15                             fall-backs               1.8e-15 / 1.5e-15
  after a failed launch         3.7e-15 / 3.0e-15                             gibbs K = 8 | 32 | 64 | 128: RMSE 8.9e-16, factors 1.3e-14
  launch 3 == launch 1 bit for bit in every case.
No defect was found: all 73 cases passed at the first run.  That the net holds was checked once with a library whose four
samplers do not re-arm the ticket (mc_count) of a chunked column: exactly the 42 cases with a chunked column failed (every
form, the slice, the stateful loop, the launch after a failed one), the 31 without one passed.  A second one with a wrong
Gram tail in each sampler (k_sample1: the last 16-rating group of a block dropped; k_sample4: the last block of an even number
of blocks; slab / k_sample_wg2: the last rating of a third index block) failed 20 cases -- k_sample4, the slab form and
k_sample_wg2 only at the automatic chunk and at 272, where whole columns of 63 .. 257 ratings reach the Gram loops.
"""
import re

import numpy as np
import pytest

from tests import util
from tests.test_gpu_parity import RTOL, check_half_iteration, half_iteration_pair, rel_err

pytestmark = pytest.mark.gpu

EDGE_COUNTS = [0, 0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 32, 32, 33, 47, 48, 49, 63, 64, 64, 64, 65, 80, 81, 96, 97, 127, 128, 129,
               145, 193, 257]
EDGE_NROWS = 300
# matrix B: the columns with <= 1 rating are already a majority of its 149 columns
PF_COUNTS = [0] * 41 + [1] * 37 + [2] * 23 + [n for n in range(3, 18) for _ in range(3)] + [33, 33, 65]
PF_NROWS = 120

_CACHE = {}


def _matrix(name, counts, nrows, seed):
    """(counts in column order, CSC triple): rows distinct and ascending within a column, non-integer values."""
    if name not in _CACHE:
        rng = np.random.default_rng(seed)
        counts = np.asarray(counts, np.int64).copy()
        rng.shuffle(counts)
        colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        rowidx = np.concatenate([np.sort(rng.choice(nrows, size=int(c), replace=False)) for c in counts]).astype(np.int32)
        vals = rng.normal(5.0, 1.1, size=len(rowidx))
        for a in (counts, colptr, rowidx, vals):
            a.setflags(write=False)
        _CACHE[name] = (counts, (colptr, rowidx, vals))
    return _CACHE[name]


def _edge():
    return _matrix("edge", EDGE_COUNTS, EDGE_NROWS, 2024)


def _pf_matrix():
    return _matrix("pf", PF_COUNTS, PF_NROWS, 77)


def _inputs(oracle, K, ncols, nrows, seed, f32=False):
    """Two sets of launch inputs (other side's factors, it, alpha, mu, LambdaF): different factors, hyper-parameters drawn by
    the oracle from a random SPD cov, different it, alpha = 2 then 1.5."""
    rng = np.random.default_rng(seed)
    out = []
    for scale, it, alpha in ((0.3, 3, 2.0), (0.45, 8, 1.5)):
        U = scale * rng.standard_normal((nrows, K))
        if f32:
            U = U.astype(np.float32).astype(np.float64)               # the oracle sees the factors the device sees
        A = rng.standard_normal((K, 3 * K))
        mu, LU, LF = oracle.hyper_sample(K, ncols, A @ A.T / (3 * K), it)
        out.append((U, it, alpha, mu, LF))
    return out


def _references(oracle, key, K, M, ncols, nrows, seed, f32=False, **kw):
    """The inputs and the oracle's (items, sum, prod, norm) for them: computed once per key, shared, never written."""
    if key not in _CACHE:
        mean = util.mean_rating(M)
        inputs = _inputs(oracle, K, ncols, nrows, seed, f32)
        refs = []
        for U, it, alpha, mu, LF in inputs:
            ref = np.zeros((ncols, K))
            s, p, n = oracle.sample_side(K, M, mean, alpha, U, ref, it, mu, LF, **kw)
            ref.setflags(write=False)
            refs.append((ref, s, p, n))
        _CACHE[key] = (inputs, refs)
    return _CACHE[key]


def _env(monkeypatch, mode=None, chunk=None, pf=None):
    for name, v in (("BPMF_HIP_MODE", mode), ("BPMF_HIP_CHUNK", chunk), ("BPMF_HIP_PF", pf)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _empty_side(eng, ncols, nrows):
    return eng.side_create(ncols, nrows, np.zeros(ncols + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)


def _report(tag, hip, ref):
    """Every figure before it is asserted (pytest -s / -rP shows them)."""
    (items, s, p, n), (items_ref, s_ref, p_ref, n_ref) = hip, ref
    print("schedule-edges %s: factors %.3e sum %.3e prod %.3e norm %.3e"
          % (tag, rel_err(items, items_ref), rel_err(s, s_ref), rel_err(p, p_ref), abs(n - n_ref) / max(abs(n_ref), 1e-300)))


def _check(tag, hip, ref, f32=False):
    _report(tag, hip, ref)
    if not f32:
        check_half_iteration(hip, ref)
        return
    (items, s, p, n), (items_ref, s_ref, p_ref, n_ref) = hip, ref
    assert np.all(np.isfinite(items))
    assert rel_err(items, items_ref) < 2e-3
    assert rel_err(s, s_ref) < 1e-3 and rel_err(p, p_ref) < 1e-3 and abs(n - n_ref) <= 1e-3 * abs(n_ref)


def _launch(eng, me, ot, inp):
    U, it, alpha, mu, LF = inp
    eng.set_items(ot, U)
    s, p, n = eng.sample_side(me, ot, it, alpha, mu, LF)
    return eng.get_items(me), s, p, n


def _check_schedule(eng, side, counts, chunk_env):
    """The properties of the cut, not its arithmetic.  counts: ratings of the side's local columns.  Returns (info, pieces per
    column, item lengths, heavy ordinals, item columns)."""
    info = eng.schedule_info(side)
    col, ln, heavy = eng.schedule_items(side)
    R = info["chunk"]
    if chunk_env is not None:
        assert R == -(-int(chunk_env) // 16) * 16                      # the variable, rounded up to 16
    assert R >= 16 and R % 16 == 0
    ncols = len(counts)
    assert len(col) == info["work_items"] and info["local_columns"] == ncols and info["local_ratings"] == counts.sum()
    assert col.min() >= 0 and col.max() < ncols
    covered = np.zeros(ncols, np.int64)
    np.add.at(covered, col, ln)
    assert np.array_equal(covered, counts)                            # every rating in exactly one item
    pieces = np.bincount(col, minlength=ncols)
    assert pieces.min() >= 1                                          # every column is sampled, the empty ones too
    chunked = counts > R
    assert np.array_equal(pieces > 1, chunked)                        # cut exactly when longer than the chunk
    assert np.array_equal(heavy >= 0, chunked[col])
    assert info["chunked_columns"] == chunked.sum() and info["chunks"] == (heavy >= 0).sum() == pieces[chunked].sum()
    if R >= counts.max():
        assert info["chunked_columns"] == 0
    assert ln.max() <= R                                              # no piece longer than the chunk
    assert np.all(ln[heavy >= 0] > 0)                                 # no empty piece
    assert np.array_equal(ln == 0, counts[col] == 0)                  # (a zero-length item is a whole empty column)
    for c in np.nonzero(chunked)[0]:
        mine = col == c
        assert (ln[mine] % 16 != 0).sum() <= 1                        # multiples of 16; only the last piece takes the rest
        assert len(np.unique(heavy[mine])) == 1
    assert len(np.unique(heavy[heavy >= 0])) == chunked.sum()         # one ordinal per chunked column
    return info, pieces, ln, heavy, col


# ----------------------------------------------------------------------------------------------------------------------
# 1. the edge side, through every form
# (id, num_latent, dtype, BPMF_HIP_MODE, expected kernel_name)
FORMS = [("k_sample1-%d" % K, K, "f64", 1, r"k_sample1<%d>" % K) for K in (8, 16, 32)] + \
        [("k_sample4-%d" % K, K, "f64", 3, r"k_sample4<%d>" % K) for K in (8, 16, 32)] + \
        [("slab-64", 64, "f64", None, r"k_sample1s<64>|k_sample_slab<64>"),
         ("wg2-f64-128", 128, "f64", None, r"k_sample_wg2<128,4,double>"),
         ("wg2-f32-128", 128, "f32", None, r"k_sample_wg2<128,2>")]
PADDED = [("padded-20-k_sample1", 20, "f64", 1, r"k_sample1<32>"), ("padded-20-k_sample4", 20, "f64", 3, r"k_sample4<32>"),
          ("padded-50", 50, "f64", None, r"k_sample1s<64>|k_sample_slab<64>"),
          ("padded-100", 100, "f64", None, r"k_sample_wg2<128,4,double>")]
# chunk: unset, 16, 40 (rounded up to 48 by the schedule), 272 (longer than every column: see the module docstring)
EDGE_CASES = [pytest.param(f, c, id="%s-chunk-%s" % (f[0], "auto" if c is None else c)) for f in FORMS for c in (None, 16, 40, 272)] + \
             [pytest.param(f, 16, id="%s-chunk-16" % f[0]) for f in PADDED]


@pytest.mark.parametrize("form,chunk", EDGE_CASES)
def test_edge_side_every_form(oracle, hip_engine_factory, monkeypatch, form, chunk):
    """Schedule properties, then three stateless launches A, B, A on the SAME side: each against the oracle, the third equal
    to the first bit for bit (partials are added in chunk order, the draws are counter-based)."""
    tag, K, dtype, mode, kernel = form
    f32 = dtype == "f32"
    counts, M = _edge()
    ncols = len(counts)
    inputs, refs = _references(oracle, ("edge", K, f32), K, M, ncols, EDGE_NROWS, 1000 + K, f32)
    eng = hip_engine_factory(K, dtype)
    _env(monkeypatch, mode=mode, chunk=chunk)
    me = eng.side_create(ncols, EDGE_NROWS, *M, util.mean_rating(M))
    ot = _empty_side(eng, EDGE_NROWS, ncols)
    name = eng.kernel_name(me)
    assert re.fullmatch(kernel, name), name
    assert "k_sample_pf" not in name                                  # the light columns are a minority here
    info, pieces, ln, heavy, col = _check_schedule(eng, me, counts, chunk)
    assert info["light_columns"] == 0
    if chunk == 272:
        assert info["chunked_columns"] == 0
    if chunk == 16:
        assert (ln[heavy >= 0] == 1).any()                            # a last piece of one rating (17, 33, 65, ...)
        assert {2, 3, 5, 9, 13, 17} <= set(pieces[counts > 16].tolist())
        if mode == 3:                                                 # two pieces of one column in one k_sample4 wave
            pad = np.concatenate([col, -1 - np.arange((-len(col)) % 4)]).reshape(-1, 4)
            assert any(len(np.unique(w)) < 4 for w in pad)
    out = []
    for i, j in enumerate((0, 1, 0)):
        hip = _launch(eng, me, ot, inputs[j])
        _check("%s chunk %s launch %d" % (tag, chunk, i), hip, refs[j], f32)
        out.append(hip)
    assert np.array_equal(out[2][0], out[0][0])                       # bit for bit
    assert np.array_equal(out[2][1], out[0][1]) and np.array_equal(out[2][2], out[0][2]) and out[2][3] == out[0][3]
    eng.side_destroy(me); eng.side_destroy(ot)


# ----------------------------------------------------------------------------------------------------------------------
# 2. a slice of the edge side
@pytest.mark.parametrize("K,mode", [(32, 1), (32, 3), (64, None), (128, None)], ids=["k_sample1-32", "k_sample4-32", "slab-64", "wg2-f64-128"])
def test_slice_of_the_edge_side(oracle, hip_engine_factory, monkeypatch, K, mode):
    """A side that owns the columns [7, ncols - 5) only (the local colptr slice, no communicator): its rows of the factor
    matrix are the oracle's (a column's stream id uses its GLOBAL index), the other rows stay zero, the sums are the slice's."""
    from bpmf_amd import synth
    counts, M = _edge()
    ncols = len(counts)
    lo, hi = 7, ncols - 5
    inputs, refs = _references(oracle, ("edge", K, False), K, M, ncols, EDGE_NROWS, 1000 + K)
    eng = hip_engine_factory(K)
    _env(monkeypatch, mode=mode, chunk=16)
    me = eng.side_create(ncols, EDGE_NROWS, *synth.slice_cols(M, lo, hi), util.mean_rating(M), col_from=lo, col_to=hi)
    ot = _empty_side(eng, EDGE_NROWS, ncols)
    info, pieces, ln, heavy, col = _check_schedule(eng, me, counts[lo:hi], 16)
    assert info["chunked_columns"] == (counts[lo:hi] > 16).sum() >= 1
    for j in (0, 1):
        items, s, p, n = _launch(eng, me, ot, inputs[j])
        X = refs[j][0][lo:hi]
        ref = (X, X.sum(0), X.T @ X, float((X * X).sum()))
        _check("slice K=%d mode %s launch %d" % (K, mode, j), (items[lo:hi], s, p, n), ref)
        assert rel_err(items[lo:hi], X) < RTOL
        assert not items[:lo].any() and not items[hi:].any()
    eng.side_destroy(me); eng.side_destroy(ot)


# ----------------------------------------------------------------------------------------------------------------------
# 3. product form: class cuts, the half rule, fall-backs
def _pf_expect(counts, pf):
    """(light columns, <= 3, 4..6, 7..16, kernel_name) from the documented meaning: BPMF_HIP_PF is the largest number of
    ratings in the product form (default and maximum 16, 0: off), the classes are <= 3, 4..6, 7..16 ratings, the split is on
    when the light columns are at least half of the side; kernel_name names the classes that have columns, then the slab form
    if anything is left.  (A light column is never longer than the chunk: chunks are at least 16.)"""
    pfmax = 16 if pf is None else min(int(pf), 16)
    light = counts <= pfmax if pfmax > 0 else np.zeros(len(counts), bool)
    if pfmax <= 0 or 2 * light.sum() < len(counts):
        return 0, 0, 0, 0, None
    cls = [int((light & (counts >= a) & (counts <= b)).sum()) for a, b in ((0, 3), (4, 6), (7, 16))]
    names = ["k_sample_pf<64,%s>" % nb for nb, c in zip(("3", "6", "16"), cls) if c > 0]
    if (~light).any():
        names.append("k_sample_slab<64>")
    return int(light.sum()), cls[0], cls[1], cls[2], " + ".join(names)


def _pf_run(oracle, eng, K, monkeypatch, pf, chunk, tag):
    counts, M = _pf_matrix()
    ncols = len(counts)
    inputs, refs = _references(oracle, ("pf", K), K, M, ncols, PF_NROWS, 3000 + K)
    _env(monkeypatch, pf=pf, chunk=chunk)
    me = eng.side_create(ncols, PF_NROWS, *M, util.mean_rating(M))
    ot = _empty_side(eng, PF_NROWS, ncols)
    info = eng.schedule_info(me)
    name = eng.kernel_name(me)
    light, le3, c46, c716, expect = _pf_expect(counts, pf)
    print("schedule-edges %s: %s  %s" % (tag, name, {k: info[k] for k in ("light_columns", "pf_le3", "pf_4to6", "pf_7to16", "other_items", "chunked_columns")}))
    assert (info["light_columns"], info["pf_le3"], info["pf_4to6"], info["pf_7to16"]) == (light, le3, c46, c716)
    if expect is None:
        assert "k_sample_pf" not in name and re.fullmatch(r"k_sample1s<64>|k_sample_slab<64>", name), name
    else:
        assert name == expect, (name, expect)
    if chunk is not None:
        _check_schedule(eng, me, counts, chunk)
        assert info["chunked_columns"] == (counts > info["chunk"]).sum() >= 1
        assert info["other_items"] == info["work_items"] - light      # the heavy list carries the chunk items
    for j in (0, 1):
        _check("%s launch %d" % (tag, j), _launch(eng, me, ot, inputs[j]), refs[j])
    eng.side_destroy(me); eng.side_destroy(ot)


@pytest.mark.parametrize("pf", [None, 0, 1, 2, 3, 4, 6, 7, 15], ids=lambda v: "pf-unset" if v is None else "pf-%d" % v)
@pytest.mark.parametrize("K", [64, 50])
def test_product_form_class_cuts(oracle, hip_engine_factory, monkeypatch, K, pf):
    """3a.  The classes for every cut of BPMF_HIP_PF that moves a class boundary, at K = 64 and on the padded K = 50."""
    light, le3, c46, c716, expect = _pf_expect(_pf_matrix()[0], pf)
    assert (expect is None) == (pf == 0)                              # matrix B is split at every value but 0
    _pf_run(oracle, hip_engine_factory(K), K, monkeypatch, pf, None, "pf K=%d BPMF_HIP_PF=%s" % (K, pf))


@pytest.mark.parametrize("K", [64, 50])
def test_product_form_beside_chunked_heavy_columns(oracle, hip_engine_factory, monkeypatch, K):
    """3a, one more run: BPMF_HIP_CHUNK=16, so that the heavy list of a split side carries chunk items (17, 33, 65 ratings)."""
    _pf_run(oracle, hip_engine_factory(K), K, monkeypatch, None, 16, "pf K=%d chunk 16" % K)


@pytest.mark.parametrize("extra", [0, 1], ids=["exactly-half", "one-below-half"])
def test_product_form_half_rule(oracle, hip_engine_factory, monkeypatch, extra):
    """3b.  10 columns of 2 ratings + 10 of 20: light x 2 = columns, the split is on; one more column of 20: off."""
    K = 64
    counts, M = _matrix("half-%d" % extra, [2] * 10 + [20] * (10 + extra), PF_NROWS, 5 + extra)
    ncols = len(counts)
    eng = hip_engine_factory(K)
    _env(monkeypatch)
    me = eng.side_create(ncols, PF_NROWS, *M, util.mean_rating(M))
    info, name = eng.schedule_info(me), eng.kernel_name(me)
    eng.side_destroy(me)
    if extra == 0:
        assert info["light_columns"] == 10 and info["pf_le3"] == 10 and info["other_items"] == 10
        assert name == "k_sample_pf<64,3> + k_sample_slab<64>", name
    else:
        assert info["light_columns"] == 0 and info["pf_le3"] == 0 and "k_sample_pf" not in name, name
    rng = np.random.default_rng(40 + extra)
    A = rng.standard_normal((K, 3 * K))
    hip, ref = half_iteration_pair(oracle, eng, K, M, PF_NROWS, 0.35 * rng.standard_normal((PF_NROWS, K)), 6, alpha=1.5, cov=A @ A.T / (3 * K))
    _check("half rule, %d columns" % ncols, hip, ref)


def test_product_form_falls_back_and_returns(oracle, hip_engine_factory, monkeypatch):
    """3c.  Per-column priors and the diagonal-only variant have no product form: a side that HAS the split runs its full item
    list while either is on (kernel_name says so, the sample is the oracle's for that variant) and the split again after."""
    K = 64
    counts, M = _pf_matrix()
    ncols = len(counts)
    mean = util.mean_rating(M)
    inputs, refs = _references(oracle, ("pf", K), K, M, ncols, PF_NROWS, 3000 + K)
    rng = np.random.default_rng(301)
    B = rng.standard_normal((ncols, K, K)) * 0.2
    prop = np.einsum("nij,nkj->nik", B, B) + 2.0 * np.eye(K)[None]    # SPD per column; symmetric => layout-neutral
    U, it, alpha, mu, LF = inputs[0]
    eng = hip_engine_factory(K)
    _env(monkeypatch)
    me = eng.side_create(ncols, PF_NROWS, *M, mean)
    ot = _empty_side(eng, PF_NROWS, ncols)
    split = eng.kernel_name(me)
    assert split == _pf_expect(counts, None)[4] and "k_sample_pf" in split

    def oracle_variant(**kw):
        ref = np.zeros((ncols, K))
        return (ref,) + tuple(oracle.sample_side(K, M, mean, alpha, U, ref, it, mu, LF, **kw))

    eng.set_prop_posterior(me, prop.reshape(ncols, K * K))
    assert "k_sample_pf" not in eng.kernel_name(me)
    _check("fallback: per-column priors", _launch(eng, me, ot, inputs[0]), oracle_variant(prop_lambda=prop))
    eng.set_prop_posterior(me, None)
    assert eng.kernel_name(me) == split
    _check("fallback: priors removed", _launch(eng, me, ot, inputs[0]), refs[0])
    eng.set_no_covariance(True)
    try:
        assert "k_sample_pf" not in eng.kernel_name(me)
        _check("fallback: diagonal only", _launch(eng, me, ot, inputs[0]), oracle_variant(no_covariance=True))
    finally:
        eng.set_no_covariance(False)
    assert eng.kernel_name(me) == split
    _check("fallback: full covariance again", _launch(eng, me, ot, inputs[1]), refs[1])
    eng.side_destroy(me); eng.side_destroy(ot)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the stateful loop on chunked, split sides
@pytest.mark.parametrize("K,mode,kernel", [(8, 3, "k_sample4<8>"), (32, 1, "k_sample1<32>"), (64, None, "<64>"), (128, None, "k_sample_wg2<128,4,double>")],
                         ids=["k_sample4-8", "k_sample1-32-fused", "k64", "wg2-f64-128"])
def test_stateful_loop_on_chunked_sides(oracle, hip_engine_factory, monkeypatch, K, mode, kernel):
    """bpmf_amd.gibbs (the library's own hyper-parameter draws, the fused launch at K = 32, the product form beside the slab
    form at K = 64) with every column above 16 ratings cut: RMSE traces to 1e-6 and factors to 1e-6 of max|U|, the bars of
    test_full_run_ml100k_matches_oracle."""
    import bpmf_amd
    M, Mt, T, Tt, nu, nm = util.synthetic(150, 40, 2500, seed=12, heavy=(3, 140))
    assert np.diff(M[0]).max() >= 140 and np.diff(Mt[0]).max() > 16
    eng = hip_engine_factory(K)
    _env(monkeypatch, mode=mode, chunk=16)
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=4, burnin=1)
    ref = oracle.gibbs(K, M, Mt, T, Tt, nsims=4, burnin=1)
    for sd, mat in ((res["movies"], M), (res["users"], Mt)):
        info, name = eng.schedule_info(sd.side), eng.kernel_name(sd.side)
        print("schedule-edges gibbs K=%d: %s %s" % (K, name, info))
        assert kernel in name, name
        assert info["chunk"] == 16 and info["chunked_columns"] == (np.diff(mat[0]) > 16).sum() >= 1
    if K == 64:                                                       # 88 of the 150 users have <= 16 ratings: a split side
        assert "k_sample_pf" in eng.kernel_name(res["users"].side) and eng.schedule_info(res["users"].side)["light_columns"] == (np.diff(Mt[0]) <= 16).sum()
    print("schedule-edges gibbs K=%d: rmse %.3e U %.3e V %.3e" % (K, np.abs(np.array(res["rmse"]) - np.array(ref["rmse"])).max(),
                                                                  rel_err(res["U"], ref["U"]), rel_err(res["V"], ref["V"])))
    assert np.allclose(res["rmse"], ref["rmse"], atol=1e-6) and np.allclose(res["rmse_avg"], ref["rmse_avg"], atol=1e-6)
    assert abs(res["final_rmse_avg"] - ref["final_rmse_avg"]) < 1e-6
    assert rel_err(res["U"], ref["U"]) < 1e-6 and rel_err(res["V"], ref["V"]) < 1e-6
    eng.side_destroy(res["movies"].side); eng.side_destroy(res["users"].side)


# ----------------------------------------------------------------------------------------------------------------------
# 5. a failed factorisation in a chunked column leaves the side usable
@pytest.mark.parametrize("K,mode", [(32, 1), (128, None)], ids=["k_sample1-32", "wg2-f64-128"])
def test_failed_factorisation_in_chunked_columns_leaves_the_side_usable(oracle, hip_engine_factory, monkeypatch, K, mode):
    """LambdaF = -1e6 I: every column's factorisation fails, the chunked ones' in their last-arriving piece (the reported-error
    path of test_cholesky_failure_is_reported; nothing faults).  The tickets must have been re-armed all the same: the next
    launch on the same side is the oracle's sample."""
    import bpmf_amd
    counts, M = _edge()
    ncols = len(counts)
    inputs, refs = _references(oracle, ("edge", K, False), K, M, ncols, EDGE_NROWS, 1000 + K)
    eng = hip_engine_factory(K)
    _env(monkeypatch, mode=mode, chunk=16)
    me = eng.side_create(ncols, EDGE_NROWS, *M, util.mean_rating(M))
    ot = _empty_side(eng, EDGE_NROWS, ncols)
    assert eng.schedule_info(me)["chunked_columns"] == (counts > 16).sum()
    U, it, alpha, mu, LF = inputs[0]
    eng.set_items(ot, U)
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        eng.sample_side(me, ot, it, alpha, mu, -1e6 * np.eye(K))
    assert e.value.code == -4 and "Cholesky failed in column" in str(e.value)
    for j in (1, 0):
        _check("after a failed launch K=%d launch %d" % (K, j), _launch(eng, me, ot, inputs[j]), refs[j])
    eng.side_destroy(me); eng.side_destroy(ot)
