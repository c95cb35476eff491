"""The two prior variants of the column samplers on every sampler form, and fp32 at the padded sizes 65 .. 127.

Per-column propagated priors (set_prop_posterior: -m / -l, c++/sample.cpp:157-174,272-277) and the diagonal-only precision
(set_no_covariance: BPMF_NO_COVARIANCE, :300-304) have code of their own in every sampler family -- deposit_column and the fused
K <= 32 forms (kernels.h), kernels_q4.inc, kernels_slab.h and three places of kernels_wg2.h: the prior-before-Gram start of a
whole column at a power-of-two alpha, prior(false) after the Gram for chunked columns and other alphas, and the fp32 tile prior
(lf32), which per-column priors switch off (launch_impl.h: a.lf32 = nullptr, so that the fp32 kernel takes the fp64-load branch
with T = float).  The tests of test_gpu_parity.py / test_gpu_latent.py reach them on whole sides of MovieLens-100K in fp64 only.
Here, on the 33-column edge side of tests/test_gpu_schedule_edges.py (its helpers, its references cache, its bars):

  1. every form x {prop, diag} x BPMF_HIP_CHUNK in {16, 272}: the 9 forms of FORMS, the 4 of PADDED and fp32 at num_latent 100 and
     65.  Chunk 16 cuts every column above 16 ratings -- the last-arriving piece adds the partials and THEN takes the column's own
     prior or drops the off-diagonal -- and chunk 272 cuts none; the count of chunked columns is asserted from schedule_info both
     times.  The inputs are one launch at alpha = 2 and one at alpha = 1.5 (_inputs): with chunk 272 they take, in k_sample_wg2,
     the `whole` start (prior before the Gram, times alpha at the end) and the prior-after-Gram branch respectively; in fp32 under
     diag the tiles stay on, so both take the select inside the lf_tiles branch.  Launches A, B, A against the oracle's sample for
     that variant, launch 3 == launch 1 bit for bit, the form's kernel_name while the variant is on, and after the variant is
     removed one more launch that must be the PLAIN reference of test_edge_side_every_form;
  2. fp32 at num_latent 65, 100 and 127 through the unmodified recipe of test_edge_side_every_form (no variant) at the automatic
     chunk, 16 and 272: the widen / narrow of set_items / get_items, the identity-padded tiles of k_lf32_tiles,
     k_colstats_f32<128, float>; the context's answers (supports, ld, num_latent, the shape get_items returns);
  3. a col_from / col_to slice under per-column priors (the kernels index them by the LOCAL column, the oracle by the global one),
     [7, ncols - 5) and [0, 9);
  4. the stateful loop (bpmf_hip_sys_sample: fused launches, gate, riders, second factor copy) with a variant on, against
     tests/variants_ref.gibbs -- the oracle's pieces in the order of oracle.gibbs -- on sides chunked at 16 in fp64, and in fp32 at
     128 and 100 on MovieLens-100K; fp32 num_latent 100 without a variant against oracle.gibbs, from Python and as
     `bpmf -d 100 --fp32`.

Bars, none of them new: fp64 1e-9 of max|U| on the factors and 1e-8 on the sums (check_half_iteration), fp32 2e-3 / 1e-3 with the
other side's factors rounded to fp32 first (tests/test_gpu_f32.py); coupled fp64 runs 1e-6 on RMSE traces and factors
(test_stateful_loop_on_chunked_sides); coupled fp32 runs 1e-3 on every RMSE and on the final average
(test_f32_full_run_rmse_within_1e3_of_fp64, which is why they run on MovieLens-100K); the CLI 2e-3, printed digits
(test_d128_is_fp64_and_fp32_is_an_explicit_opt_in).

Observed on an MI355X, worst over the cases of a form (factors relative to max|U| / sums), prop ; diag:
  k_sample1<8 | 16 | 32>   6.1e-16 | 8.7e-16 | 7.9e-16 / 7.2e-16 ; 3.4e-16 | 6.7e-16 | 4.3e-16 / 4.2e-16
  k_sample4<8 | 16 | 32>   8.9e-16 | 7.2e-16 | 1.0e-15 / 6.9e-16 ; 3.5e-16 | 6.3e-16 | 4.3e-16 / 4.8e-16
  slab K = 64              1.3e-15 / 7.2e-16 ; 4.7e-16 / 3.4e-16          k_sample_wg2 fp64   2.0e-15 / 1.1e-15 ; 8.3e-16 / 4.3e-16
  padded 20 | 50 | 100     6.6e-16 | 1.1e-15 | 2.4e-15 / 1.2e-15 ; 5.3e-16 | 5.6e-16 | 4.7e-16 / 7.2e-16
  k_sample_wg2 fp32 128    9.6e-7 / 3.8e-7 ; 1.9e-7 / 1.0e-7              fp32 100 | 65       7.4e-7 | 5.0e-7 / 5.4e-7 ; 1.8e-7 | 1.6e-7 / 1.5e-7
  fp32 65 | 100 | 127, no variant   9.7e-7 | 2.2e-6 | 2.6e-6 / 9.8e-7 | 1.2e-6 | 2.4e-6
  slices under prop        fp64 2.1e-15 / 1.9e-15, fp32 1.0e-6 / 5.0e-7
  stateful loop fp64 (8, 32, 64, 128, 50)   prop: RMSE 1.3e-15, factors 7.5e-15 ; diag: RMSE 2.2e-16, factors 9.8e-16
  stateful loop fp32 128 | 100   prop: RMSE 3.2e-8 | 4.9e-8, factors 2.6e-6 | 2.0e-6 ; diag: RMSE 8.0e-12 | 1.4e-11, factors 1.0e-7 | 9.5e-8
  gibbs fp32 at 100: RMSE 5.9e-11 ; bpmf -d 100 --fp32: RMSE 4.9e-5 (four printed decimals), final average 9.6e-7
  launch 3 == launch 1 bit for bit in every case.
(The fp32 chains sit far inside their 1e-3 because four iterations at these sizes barely leave the mean predictor: their RMSE
moves in the fourth decimal.  The factor figures, a few fp32 ulps, say more.)
No defect was found: all 96 cases here and the 6 of tests/test_gpu_reduce.py::test_reduce_formulation_variants passed at the
first run.  That the net holds was checked once against two libraries built from a scratch copy, each changing only which valid
data k_sample_wg2 uses:
  (a) the diagonal-only select in the lf_tiles branch removed: exactly the 8 fp32 diag cases failed -- the 6 of the edge side
      (factors 1.8 .. 2.3 of max|U| off) and the 2 stateful fp32 chains, the latter ONLY by the nearer-chain assertion (0.56 / 0.63
      of max|U| from the variant's chain, 4e-7 from the plain one): their RMSE stayed inside 1e-3 -- the other 88 passed;
  (b) column 0's prior read for every column: exactly the 17 prop cases at num_latent 65 .. 128 failed (10 of the edge side, the 4
      slices of k_sample_wg2 -- [0, 9) too, where only column 0 itself is right --, stateful 128 in fp64 and 128 / 100 in fp32),
      the other 79 passed.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import util
from tests import variants_ref
from tests import test_gpu_schedule_edges as edges
from tests.test_gpu_parity import RTOL, rel_err
from tests.test_gpu_schedule_edges import (EDGE_NROWS, FORMS, PADDED, _check, _check_schedule, _edge, _empty_side, _env, _launch,
                                           _references)

pytestmark = pytest.mark.gpu

F32_PADDED = [("wg2-f32-100", 100, "f32", None, r"k_sample_wg2<128,2>"), ("wg2-f32-65", 65, "f32", None, r"k_sample_wg2<128,2>")]
F32_127 = ("wg2-f32-127", 127, "f32", None, r"k_sample_wg2<128,2>")
ALL_FORMS = FORMS + PADDED + F32_PADDED

_CHAINS = {}


def _prop(ncols, K):
    return variants_ref.prop_priors(ncols, K, 300 + K)


def _variant_kw(variant, ncols, K):
    return dict(prop_lambda=_prop(ncols, K)) if variant == "prop" else dict(no_covariance=True)


def _worst(tag, pairs, f32=False):
    """one line per case: the worst factor / sum figures over its launches"""
    fac = max(rel_err(h[0], r[0]) for h, r in pairs)
    sums = max(max(rel_err(h[1], r[1]), rel_err(h[2], r[2]), abs(h[3] - r[3]) / max(abs(r[3]), 1e-300)) for h, r in pairs)
    print("variant-forms %s: worst factors %.3e sums %.3e (%s)" % (tag, fac, sums, "fp32" if f32 else "fp64"))


# ----------------------------------------------------------------------------------------------------------------------
# 1. the edge side: every form x variant x {every column above 16 cut, nothing cut}
VARIANT_CASES = [pytest.param(f, v, c, id="%s-%s-chunk-%d" % (f[0], v, c)) for f in ALL_FORMS for v in ("prop", "diag") for c in (16, 272)]


@pytest.mark.parametrize("form,variant,chunk", VARIANT_CASES)
def test_edge_side_every_form_with_a_variant(oracle, hip_engine_factory, monkeypatch, form, variant, chunk):
    """Launches A (alpha = 2), B (alpha = 1.5), A on the same side with the variant on, each against the oracle's sample for that
    variant; the third equal to the first bit for bit; then the variant off and launch B against the plain reference.  Chunk 272:
    no column is cut, so that in k_sample_wg2 launch A starts whole columns from the prior (`whole`) and launch B adds it after
    the Gram; chunk 16: the last-arriving piece of a column adds the partials before either."""
    tag, K, dtype, mode, kernel = form
    f32 = dtype == "f32"
    counts, M = _edge()
    ncols = len(counts)
    inputs, plain = _references(oracle, ("edge", K, f32), K, M, ncols, EDGE_NROWS, 1000 + K, f32)
    inputs_v, refs = _references(oracle, ("edge", K, f32, variant), K, M, ncols, EDGE_NROWS, 1000 + K, f32, **_variant_kw(variant, ncols, K))
    assert all(np.array_equal(a[0], b[0]) and a[1:3] == b[1:3] for a, b in zip(inputs, inputs_v))      # same launches, another prior
    assert rel_err(refs[0][0], plain[0][0]) > 1e-2                    # (the variant moves the sample far beyond every bar)
    eng = hip_engine_factory(K, dtype)
    _env(monkeypatch, mode=mode, chunk=chunk)
    me = eng.side_create(ncols, EDGE_NROWS, *M, util.mean_rating(M))
    ot = _empty_side(eng, EDGE_NROWS, ncols)
    info = _check_schedule(eng, me, counts, chunk)[0]
    assert info["chunked_columns"] == ((counts > 16).sum() if chunk == 16 else 0) and info["light_columns"] == 0
    out = []
    if variant == "prop":
        eng.set_prop_posterior(me, _prop(ncols, K).reshape(ncols, K * K))
    else:
        eng.set_no_covariance(True)
    try:
        name = eng.kernel_name(me)
        assert re.fullmatch(kernel, name), name
        for i, j in enumerate((0, 1, 0)):
            hip = _launch(eng, me, ot, inputs[j])
            out.append((hip, refs[j]))
            _check("%s %s chunk %d launch %d" % (tag, variant, chunk, i), hip, refs[j], f32)
    finally:
        if variant == "prop":
            eng.set_prop_posterior(me, None)
        else:
            eng.set_no_covariance(False)
    _worst("%s %s chunk %d" % (tag, variant, chunk), out, f32)
    first, third = out[0][0], out[2][0]
    assert np.array_equal(third[0], first[0])                         # bit for bit
    assert np.array_equal(third[1], first[1]) and np.array_equal(third[2], first[2]) and third[3] == first[3]
    assert re.fullmatch(kernel, eng.kernel_name(me))
    _check("%s %s chunk %d variant removed" % (tag, variant, chunk), _launch(eng, me, ot, inputs[1]), plain[1], f32)
    eng.side_destroy(me); eng.side_destroy(ot)


# ----------------------------------------------------------------------------------------------------------------------
# 2. fp32 at padded sizes, no variant
@pytest.mark.parametrize("form,chunk", [pytest.param(f, c, id="%s-chunk-%s" % (f[0], "auto" if c is None else c))
                                        for f in F32_PADDED + [F32_127] for c in (None, 16, 272)])
def test_edge_side_fp32_padded_sizes(oracle, hip_engine_factory, monkeypatch, form, chunk):
    """num_latent 65, 100 and 127 in fp32 (leading dimension 128) through test_edge_side_every_form itself: the schedule's
    properties, three launches against the oracle at the TRUE num_latent, launch 3 == launch 1."""
    edges.test_edge_side_every_form(oracle, hip_engine_factory, monkeypatch, form, chunk)


def test_fp32_padded_context(hip_engine_factory):
    """What the context says about itself at num_latent 100 in fp32, and the shape that crosses the interface."""
    import bpmf_amd
    lib = bpmf_amd._lib.load_library()
    assert lib.bpmf_hip_supports(100, 1) == 1 and lib.bpmf_hip_supports(65, 1) == 1 and lib.bpmf_hip_supports(64, 1) == 0
    eng = hip_engine_factory(100, "f32")
    assert lib.bpmf_hip_ctx_dtype(eng.ctx) == 1 and lib.bpmf_hip_ctx_ld(eng.ctx) == 128 and eng.ld() == 128
    assert lib.bpmf_hip_ctx_num_latent(eng.ctx) == 100
    counts, M = _edge()
    ncols = len(counts)
    side = eng.side_create(ncols, EDGE_NROWS, *M, util.mean_rating(M))
    X = np.random.default_rng(4).standard_normal((ncols, 100))
    eng.set_items(side, X)
    got = eng.get_items(side)
    assert got.shape == (ncols, 100)
    assert np.array_equal(got, X.astype(np.float32).astype(np.float64))   # narrowed once, widened back: the fp32 neighbour, column for column
    eng.side_destroy(side)


# ----------------------------------------------------------------------------------------------------------------------
# 3. a slice of the edge side under per-column priors
SLICE_FORMS = [f for f in FORMS if f[0] in ("k_sample1-32", "k_sample4-32", "slab-64", "wg2-f64-128", "wg2-f32-128")]


@pytest.mark.parametrize("span", ["7-to-28", "0-to-9"])
@pytest.mark.parametrize("form", [pytest.param(f, id=f[0]) for f in SLICE_FORMS])
def test_slice_of_the_edge_side_with_per_column_priors(oracle, hip_engine_factory, monkeypatch, form, span):
    """test_slice_of_the_edge_side with set_prop_posterior: the side owns [lo, hi) and is handed prop[lo:hi] (hi - lo matrices,
    indexed by the local column); the oracle gets the whole array and the whole matrix.  A kernel that indexed the priors by the
    global column, or by the work item, gives other columns' priors here."""
    from bpmf_amd import synth
    tag, K, dtype, mode, kernel = form
    f32 = dtype == "f32"
    counts, M = _edge()
    ncols = len(counts)
    lo, hi = (7, ncols - 5) if span == "7-to-28" else (0, 9)
    assert len(SLICE_FORMS) == 5 and (lo, hi) in ((7, 28), (0, 9))
    prop = _prop(ncols, K)
    inputs, refs = _references(oracle, ("edge", K, f32, "prop"), K, M, ncols, EDGE_NROWS, 1000 + K, f32, prop_lambda=prop)
    eng = hip_engine_factory(K, dtype)
    _env(monkeypatch, mode=mode, chunk=16)
    me = eng.side_create(ncols, EDGE_NROWS, *synth.slice_cols(M, lo, hi), util.mean_rating(M), col_from=lo, col_to=hi)
    ot = _empty_side(eng, EDGE_NROWS, ncols)
    info, pieces, ln, heavy, col = _check_schedule(eng, me, counts[lo:hi], 16)
    assert info["chunked_columns"] == (counts[lo:hi] > 16).sum() >= 1
    assert (counts[lo:hi] <= 16).any()                                # whole columns beside the chunked ones
    eng.set_prop_posterior(me, prop[lo:hi].reshape(hi - lo, K * K))
    assert re.fullmatch(kernel, eng.kernel_name(me)), eng.kernel_name(me)
    out = []
    for j in (0, 1):
        items, s, p, n = _launch(eng, me, ot, inputs[j])
        X = refs[j][0][lo:hi]
        ref = (X, X.sum(0), X.T @ X, float((X * X).sum()))
        out.append(((items[lo:hi], s, p, n), ref))
        _check("slice [%d, %d) %s prop launch %d" % (lo, hi, tag, j), (items[lo:hi], s, p, n), ref, f32)
        assert rel_err(items[lo:hi], X) < (2e-3 if f32 else RTOL)
        assert not items[:lo].any() and not items[hi:].any()
    _worst("slice [%d, %d) %s prop" % (lo, hi, tag), out, f32)
    eng.side_destroy(me); eng.side_destroy(ot)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the stateful loop with a variant on
def _loop(eng, M, Mt, T, nu, nm, nsims, burnin, prop_m=None, prop_u=None, diag=False):
    """movies.sample(users); users.sample(movies); movies.predict(users) as bpmf_amd.gibbs runs it, with the variant set on the
    Sys objects' sides (gibbs has no arguments for the variants).  Returns the trace, the factors and the two sides."""
    from bpmf_amd.sys import Sys
    K = eng.K
    Sys.nsims, Sys.burnin, Sys.alpha = nsims, burnin, 2.0
    movies = Sys("movs", eng, M, nm, nu, T=T); users = Sys("users", eng, Mt, nu, nm)
    if prop_m is not None:
        eng.set_prop_posterior(movies.side, prop_m.reshape(nm, K * K)); eng.set_prop_posterior(users.side, prop_u.reshape(nu, K * K))
    if diag:
        eng.set_no_covariance(True)
    try:
        rmse, rmse_avg = [], []
        for _ in range(nsims):
            movies.sample(users); users.sample(movies); movies.predict(users)
            rmse.append(movies.rmse); rmse_avg.append(movies.rmse_avg)
        movies.predict(users, True)                                   # c++/bpmf.cpp:242
        res = dict(rmse=np.array(rmse), rmse_avg=np.array(rmse_avg), final_rmse_avg=movies.rmse_avg, U=users.items(), V=movies.items(),
                   names=(eng.kernel_name(movies.side), eng.kernel_name(users.side)),
                   infos=(eng.schedule_info(movies.side), eng.schedule_info(users.side)))
    finally:
        if diag:
            eng.set_no_covariance(False)
    return res, movies, users


def _chain_ref(oracle, key, fn):
    if key not in _CHAINS:
        _CHAINS[key] = fn()
    return _CHAINS[key]


LOOP_FORMS = [("k_sample4-8", 8, 3, "k_sample4<8>"), ("k_sample1-32-fused", 32, 1, "k_sample1<32>"), ("k64", 64, None, "<64>"),
              ("wg2-f64-128", 128, None, "k_sample_wg2<128,4,double>"), ("padded-50", 50, None, "<64>")]


@pytest.mark.parametrize("variant", ["prop", "diag"])
@pytest.mark.parametrize("form", [pytest.param(f, id=f[0]) for f in LOOP_FORMS])
def test_stateful_loop_with_a_variant_on_chunked_sides(oracle, hip_engine_factory, monkeypatch, form, variant):
    """The recipe of test_stateful_loop_on_chunked_sides (150 x 40, 2 500 ratings, BPMF_HIP_CHUNK=16, nsims 4, burnin 1) with
    per-column priors on both sides or the diagonal-only precision, against variants_ref.gibbs: RMSE traces 1e-6, factors 1e-6
    of max|U|."""
    tag, K, mode, kernel = form
    M, Mt, T, Tt, nu, nm = util.synthetic(150, 40, 2500, seed=12, heavy=(3, 140))
    assert np.diff(M[0]).max() >= 140 and np.diff(Mt[0]).max() > 16
    kw = dict(prop_m=_prop(nm, K), prop_u=_prop(nu, K)) if variant == "prop" else dict(no_covariance=True)
    ref = _chain_ref(oracle, ("synthetic", K, variant), lambda: variants_ref.gibbs(oracle, K, M, Mt, T, Tt, 4, 1, 2.0, **kw))
    plain = _chain_ref(oracle, ("synthetic", K, None), lambda: oracle.gibbs(K, M, Mt, T, Tt, nsims=4, burnin=1))
    assert rel_err(ref["U"], plain["U"]) > 1e-2                       # (another chain than the plain one)
    eng = hip_engine_factory(K)
    _env(monkeypatch, mode=mode, chunk=16)
    res, movies, users = _loop(eng, M, Mt, T, nu, nm, 4, 1, kw.get("prop_m"), kw.get("prop_u"), variant == "diag")
    for name, info, mat in zip(res["names"], res["infos"], (M, Mt)):
        assert kernel in name and "k_sample_pf" not in name, name
        assert info["chunk"] == 16 and info["chunked_columns"] == (np.diff(mat[0]) > 16).sum() >= 1
    print("variant-forms loop %s %s: rmse %.3e avg %.3e U %.3e V %.3e  %s" % (
        tag, variant, np.abs(res["rmse"] - ref["rmse"]).max(), np.abs(res["rmse_avg"] - ref["rmse_avg"]).max(),
        rel_err(res["U"], ref["U"]), rel_err(res["V"], ref["V"]), res["names"]))
    assert np.allclose(res["rmse"], ref["rmse"], atol=1e-6) and np.allclose(res["rmse_avg"], ref["rmse_avg"], atol=1e-6)
    assert abs(res["final_rmse_avg"] - ref["final_rmse_avg"]) < 1e-6
    assert rel_err(res["U"], ref["U"]) < 1e-6 and rel_err(res["V"], ref["V"]) < 1e-6
    eng.side_destroy(movies.side); eng.side_destroy(users.side)


def _ml100k_priors(n, K, seed):
    """as variants_ref.prop_priors, not kept: 1 682 matrices of 128 x 128 are 220 MB"""
    B = np.random.default_rng(seed).standard_normal((n, K, K)) * 0.2
    P = B @ B.transpose(0, 2, 1) + 2.0 * np.eye(K)[None]
    return np.ascontiguousarray(0.5 * (P + P.transpose(0, 2, 1)))


@pytest.mark.parametrize("variant", ["prop", "diag"])
@pytest.mark.parametrize("K", [128, 100])
def test_stateful_loop_fp32_with_a_variant(oracle, hip_engine_factory, monkeypatch, K, variant):
    """fp32 at 128 and at the padded 100 on MovieLens-100K, nsims 4, burnin 1, against the fp64 chain of variants_ref.gibbs: every
    RMSE and the final average within 1e-3 (the bar test_f32_full_run_rmse_within_1e3_of_fp64 established on this data).
    After four iterations at these sizes the RMSE of the diagonal-only chain is still within 3e-4 of the plain chain's (the
    factors are 0.4 .. 0.5 of max|U| apart), so that bar alone cannot tell whether the switch reached the kernel: the factors must
    also be nearer to the variant's chain than to the plain one, which needs no tolerance."""
    M, Mt, T, Tt, nu, nm = util.ml100k()
    _env(monkeypatch)
    prop_m = prop_u = None
    if variant == "prop":
        prop_m, prop_u = _ml100k_priors(nm, K, 11 * K), _ml100k_priors(nu, K, 13 * K)
    ref = variants_ref.gibbs(oracle, K, M, Mt, T, Tt, 4, 1, 2.0, prop_m=prop_m, prop_u=prop_u, no_covariance=variant == "diag")
    plain = _chain_ref(oracle, ("ml100k", K, None), lambda: oracle.gibbs(K, M, Mt, T, Tt, nsims=4, burnin=1, nthreads=variants_ref.NT))
    assert rel_err(ref["U"], plain["U"]) > 1e-2 and rel_err(ref["V"], plain["V"]) > 1e-2     # (another chain than the plain one)
    eng = hip_engine_factory(K, "f32")
    res, movies, users = _loop(eng, M, Mt, T, nu, nm, 4, 1, prop_m, prop_u, variant == "diag")
    assert all(re.fullmatch(r"k_sample_wg2<128,2>", n) for n in res["names"]), res["names"]
    assert res["U"].shape == (nu, K) and res["V"].shape == (nm, K) and np.all(np.isfinite(res["U"])) and np.all(np.isfinite(res["V"]))
    print("variant-forms loop fp32 K=%d %s: rmse %.3e avg %.3e final %.3e  U %.3e V %.3e (to the plain chain: %.3e %.3e)" % (
        K, variant, np.abs(res["rmse"] - ref["rmse"]).max(), np.abs(res["rmse_avg"] - ref["rmse_avg"]).max(),
        abs(res["final_rmse_avg"] - ref["final_rmse_avg"]), rel_err(res["U"], ref["U"]), rel_err(res["V"], ref["V"]),
        rel_err(res["U"], plain["U"]), rel_err(res["V"], plain["V"])))
    assert np.allclose(res["rmse"], ref["rmse"], atol=1e-3), np.abs(res["rmse"] - ref["rmse"]).max()
    assert abs(res["final_rmse_avg"] - ref["final_rmse_avg"]) < 1e-3
    assert rel_err(res["U"], ref["U"]) < rel_err(res["U"], plain["U"]) and rel_err(res["V"], ref["V"]) < rel_err(res["V"], plain["V"])
    eng.side_destroy(movies.side); eng.side_destroy(users.side)


def test_f32_full_run_at_num_latent_100(oracle, hip_engine_factory, monkeypatch):
    """bpmf_amd.gibbs in fp32 at the padded num_latent 100 (k_sample_wg2<128,2>, k_colstats_f32, k_predict_f32<128>, the
    library's own hyper-parameter draws at the true size) against oracle.gibbs(100): the bar of the K = 128 run."""
    import bpmf_amd
    K = 100
    M, Mt, T, Tt, nu, nm = util.ml100k()
    _env(monkeypatch)
    eng = hip_engine_factory(K, "f32")
    res = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, nsims=4, burnin=1)
    ref = _chain_ref(oracle, ("ml100k", K, None), lambda: oracle.gibbs(K, M, Mt, T, Tt, nsims=4, burnin=1, nthreads=variants_ref.NT))
    assert res["U"].shape == (nu, K) and res["V"].shape == (nm, K)
    print("variant-forms gibbs fp32 K=100: rmse %.3e avg %.3e final %.3e" % (
        np.abs(np.array(res["rmse"]) - ref["rmse"]).max(), np.abs(np.array(res["rmse_avg"]) - ref["rmse_avg"]).max(),
        abs(res["final_rmse_avg"] - ref["final_rmse_avg"])))
    assert np.allclose(res["rmse"], ref["rmse"], atol=1e-3), np.abs(np.array(res["rmse"]) - ref["rmse"]).max()
    assert np.allclose(res["rmse_avg"], ref["rmse_avg"], atol=1e-3)
    assert abs(res["final_rmse_avg"] - ref["final_rmse_avg"]) < 1e-3
    assert abs(res["rmse"][0] - 1.153676) < 2e-3                      # iteration 0 = mean predictor
    eng.side_destroy(res["movies"].side); eng.side_destroy(res["users"].side)


def test_cli_d100_fp32(oracle, tmp_path):
    """bpmf -d 100 --fp32 -i 4 -b 1: says what it runs and prints the oracle's RMSE to 2e-3."""
    from tests.test_cli import BPMF, G
    K = 100
    M, Mt, T, Tt, nu, nm = util.ml100k()
    r = subprocess.run([BPMF, "-d", "100", "--fp32", "-i", "4", "-b", "1", "-n", os.path.join(G, "ml100k-train.mtx.gz"),
                        "-p", os.path.join(G, "ml100k-test.mtx.gz")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "num_latent: 100" in r.stdout and "arithmetic: fp32" in r.stdout
    ref = _chain_ref(oracle, ("ml100k", K, None), lambda: oracle.gibbs(K, M, Mt, T, Tt, nsims=4, burnin=1, nthreads=variants_ref.NT))
    rm = [float(m.group(1)) for m in re.finditer(r"\t RMSE: (\S+)", r.stdout)]
    final = float(re.search(r"Final Avg RMSE: (\S+)", r.stdout).group(1))
    print("variant-forms bpmf -d 100 --fp32: rmse %.3e final %.3e" % (np.abs(np.array(rm) - ref["rmse"]).max(), abs(final - ref["final_rmse_avg"])))
    assert len(rm) == 4 and np.allclose(rm, ref["rmse"], atol=2e-3)
    assert abs(final - ref["final_rmse_avg"]) < 2e-3
