"""Every sampler form on ill-conditioned inputs, against a longdouble restatement of the oracle's column update.

Every other test of the column samplers holds them to 1e-9 of max|U| (fp32 2e-3) on benign inputs -- the other side's factors
0.3 N(0,1), LambdaF from a Wishart-like A A^T / (3K) with a condition number of a few tens -- where an MI355X delivers 1e-15 ..
5e-15.  None of them says how the error GROWS with the condition number of Lambda* = LambdaF + alpha sum u u^T, and none of the
forms is the reference's unblocked LLT: every pivot goes through rsqrt_nr (v_rsq_f64 + one Halley step, a multiply instead of
the divide), the fused forms take 2 x 2 pivot blocks by determinant, the slab form and k_sample_wg2 factor and explicitly invert
4 x 4 / 16 x 16 diagonal blocks and solve by products with the inverse (in fp32: on the fp32 MFMA), the product form never
factors Lambda* but multiplies by a host-computed R0^-1 and scans s_k = 1 + sum p_i^2, and chunked columns add their partials in
chunk order.  Here the inputs are hard (tests/cond_ref.py: families P(kappa), D(s, eps, alpha), S(k); tests/test_cond_host.py
asserts on the CPU that they are what they claim) and the bar is relative to what an honest Cholesky loses on the same input:

    e(c)  = max_k |x(c,k) - x_ld(c,k)| / max_k |x_ld(c,k)|      x_ld: cond_ref.sample_columns(np.longdouble, ...) on the inputs the
    E     = max_c e(c)                                          device saw (fp32: U, mu, LambdaF rounded to fp32 first)
    rho   = E_dev / max(E_ref, 32 eps_dtype)                    E_ref: oracle.sample_side (fp64) / the restatement at np.float32
    rho  <= 16                                                  in every case; never a constant like 1e-9

(16: two honest fp64 implementations -- row-by-row Cholesky and LAPACK's blocked potrf + solve -- differ by 0.23 .. 2.9 x in their
worst column on these families up to kappa_2 = 1e13; 16 is 5 x that spread and the largest diagonal block any form inverts.  The
32 eps floor keeps a lucky reference from turning rounding noise into a failure.)  Also in every case: items and sums finite, no
failure reported, and the device within the bar at the column the reference itself finds hardest (named in the output).

  1. the edge side of tests/test_gpu_schedule_edges.py (33 columns, 0 .. 257 ratings) through FORMS + PADDED in fp64 over P(1e3),
     P(1e6), P(1e9), D(3, 1e-1, 100), D(3, 1e-3, 100), S(-20), S(+20), and through k_sample_wg2 fp32 at 128, 100, 65, 127 over P(1e1)
     .. P(1e4), D(0.3, 0.1, 2), D(1, 0.1, 8), S(-20 | +20) on P(1e2): BPMF_HIP_CHUNK=272 (nothing cut) for every case, and 16 for the D
     family, where the order of the chunk partials meets the cancellation.  kernel_name is asserted per form;
  2. the product form: matrix B at K = 64 and num_latent 50 with BPMF_HIP_PF unset (k_sample_pf<64,3 | 6 | 16> + the slab form) and
     with BPMF_HIP_PF=0 (the same columns through the slab form), light and heavy columns reported and held to the bar apart;
  3. a numerically singular prior, P(1e18), through k_sample1<32>, the slab form and k_sample_wg2 in fp64 and fp32: BpmfHipError -4
     naming a column or finite items, never a silent NaN; then P(1e3) on the same side meets the bar.

Observed on an MI355X: worst rho over the cases of a family (worst E_dev of the family in brackets).  kappa_2(Lambda*) reaches
6.1e9 in fp64 (P(1e9), K = 128) and 1.5e5 in fp32 (D(1, 0.1, 8)); E_ref itself is 6e-15 .. 8e-14 at P(1e3), 1e-12 .. 3e-11 at
P(1e6), 3e-9 .. 2e-8 at P(1e9).
                            P(1e3)           P(1e6)           P(1e9)           D, uncut         D, chunk 16      S(-20 | +20)
  k_sample1<8>              0.95 (6.8e-15)   0.46 (5.6e-13)   0.33 (9.0e-10)   0.74 (8.2e-13)   0.74 (8.2e-13)   0.97 (9.0e-15)
  k_sample1<16>             0.86 (9.4e-15)   1.69 (4.5e-12)   0.31 (1.1e-9)    0.88 (1.5e-12)   0.88 (1.5e-12)   1.19 (3.3e-14)
  k_sample1<32>             1.47 (2.0e-14)   0.59 (4.0e-12)   1.43 (7.9e-9)    0.50 (4.4e-12)   0.46 (4.0e-12)   1.26 (1.8e-14)
  k_sample4<8>              0.68 (4.8e-15)   1.53 (1.8e-12)   0.51 (1.4e-9)    1.05 (2.9e-10)   0.78 (8.7e-13)   1.25 (1.8e-14)
  k_sample4<16>             0.49 (5.4e-15)   1.15 (3.1e-12)   0.48 (1.7e-9)    1.57 (2.8e-12)   1.57 (2.8e-12)   0.89 (2.4e-14)
  k_sample4<32>             1.62 (2.2e-14)   0.91 (6.2e-12)   1.33 (7.3e-9)    1.17 (5.0e-10)   0.42 (3.7e-12)   1.25 (2.7e-14)
  slab K = 64               1.44 (4.6e-14)   0.84 (9.8e-12)   1.06 (7.5e-9)    1.00 (5.5e-10)   0.49 (2.7e-10)   1.54 (4.5e-14)
  k_sample_wg2 fp64 128     0.82 (6.3e-14)   1.32 (4.1e-11)   0.77 (1.3e-8)    0.94 (1.3e-9)    0.41 (7.1e-11)   1.01 (6.0e-14)
  padded 20, k_sample1      0.77 (1.5e-14)   2.06 (7.1e-12)   0.97 (3.2e-9)    0.62 (9.0e-13)   0.62 (9.0e-13)   1.53 (1.4e-14)
  padded 20, k_sample4      0.74 (1.5e-14)   2.99 (1.0e-11)   0.59 (2.0e-9)    0.85 (2.9e-10)   1.01 (1.4e-12)   1.31 (1.2e-14)
  padded 50                 0.79 (3.9e-14)   0.82 (7.3e-12)   0.93 (5.2e-9)    1.10 (2.3e-11)   2.06 (4.4e-11)   1.30 (4.0e-14)
  padded 100                1.04 (5.8e-14)   0.64 (1.9e-11)   0.63 (8.3e-9)    0.97 (9.0e-10)   0.43 (3.9e-10)   1.24 (6.5e-14)
  product form, light  64   0.27 (1.4e-14)   0.54 (8.9e-12)   0.27 (3.7e-9)    0.04 (6.4e-13)   --               1.06 (1.0e-13)
  product form, light  50   0.31 (1.4e-14)   0.39 (7.0e-12)   0.64 (5.1e-9)    0.04 (6.8e-13)   --               1.44 (1.0e-13)
  same columns, slab   64   0.69 (3.6e-14)   1.38 (2.3e-11)   1.01 (1.4e-8)    0.56 (9.5e-12)   --               0.75 (7.3e-14)
  same columns, slab   50   0.82 (3.7e-14)   0.79 (1.4e-11)   1.76 (1.4e-8)    1.07 (3.2e-11)   --               1.09 (7.7e-14)
  heavy columns of B 64|50  0.94 | 0.49      1.37 | 0.72      0.76 | 0.63      1.30 | 1.17      --               1.94 | 0.87
                            P(1e1)           P(1e2)           P(1e3)           P(1e4)           D uncut | 16                 S(-20 | +20)
  k_sample_wg2 fp32 128     0.78 (3.0e-6)    0.75 (9.6e-6)    0.91 (4.4e-5)    0.52 (2.5e-4)    1.21 (1.2e-4) | 0.43 (5.1e-4)   0.89 (2.2e-5)
  k_sample_wg2 fp32 100     0.55 (2.1e-6)    0.99 (5.7e-6)    1.14 (3.5e-5)    0.91 (2.0e-4)    1.09 (9.8e-5) | 0.45 (3.2e-4)   1.12 (1.1e-5)
  k_sample_wg2 fp32 65      0.48 (1.8e-6)    0.93 (3.6e-6)    0.88 (1.4e-5)    0.73 (6.9e-5)    1.05 (5.3e-4) | 0.37 (1.9e-4)   0.89 (3.4e-6)
  k_sample_wg2 fp32 127     0.65 (2.5e-6)    0.85 (8.3e-6)    1.28 (6.1e-5)    0.57 (2.6e-4)    1.12 (9.5e-4) | 0.53 (4.5e-4)   0.95 (7.7e-6)
  P(1e18): k_sample1<32> reports no failure and all its items are finite (its pivots stay positive; with (c) below it reports
  column 9); the slab form and k_sample_wg2 fp64 raise -4 "Cholesky failed in column 2", fp32 "column 0".  P(1e3) afterwards: rho
  1.47 / 1.44 / 0.82 / 0.91.
No defect was found: all 38 tests passed at the first run, worst rho 2.99.  Every form is as accurate as the oracle's Cholesky up
to kappa_2(Lambda*) = 6e9 in fp64 and 1.5e5 in fp32 -- no form carries a condition-number factor of its own; the product form is
25 x MORE accurate than the oracle on the light columns of the D family (it never forms the cancelling Gram).  No form needed a
fix or a gate.

That the net holds was checked once against four libraries built from a scratch copy, each changing arithmetic only:
  (a) rsqrt_nr without its Halley step (v_rsq_f64 alone, 2^-23): all 24 fp64 edge-side tests, both product-form tests and the three
      fp64 P(1e18) tests fail in every case (rho 8e3 .. 1.6e8); the 9 fp32 tests pass (k_sample_wg2<128,2> does not go through rsqrt_nr).  This one
      is NOT beyond the old net: test_edge_side_every_form fails under it too in all 36 fp64 cases (1e-8 .. 1.5e-7 against its 1e-9), as does
      test_product_form_class_cuts;
  (b) the host's S0t (= R0^-1) rounded through fp32: exactly the two product-form tests fail, in the light columns of the
      BPMF_HIP_PF-unset runs only -- every case (rho 2.9e3 .. 1.7e6; 39 at P(1e9), 50) but P(1e9) at K = 64 (rho 13: E_ref is 1.4e-8 there);
      their heavy columns, the BPMF_HIP_PF=0 control and the other 36 tests pass.  test_product_form_class_cuts fails too (5e-8);
  (c) rsqrt_nr with one Newton step in place of the Halley step (3/8 e^2 = 5e-15 relative, ~24 ulp): everything passes, the old
      tests (worst 1.5e-14) and these -- rho rises to at most 6.5 (padded 20 at S(-20); 5.2 k_sample1<32> at P(1e3)).  A pivot
      inverse that is a few tens of ulps off is inside the bar, and its error carries no kappa factor (rho does not grow along P);
  (d) S0t with the low 14 mantissa bits cleared (2^-39): test_product_form_class_cuts PASSES (worst 2.5e-12 against 1e-9); here
      the two product-form tests fail in the light columns at P(1e3), S(-20) and S(+20) (rho 38 .. 67) and pass at P(1e6), P(1e9)
      and D, where the reference's own error has outgrown the perturbation.  This is the contrast the module exists for: a
      product-form error 400 x below the old bar is caught at the benign end of the hard inputs.
"""
import re

import numpy as np
import pytest

from tests import cond_ref, util
from tests.test_gpu_schedule_edges import (EDGE_NROWS, FORMS, PADDED, PF_NROWS, _edge, _empty_side, _env, _launch, _pf_expect,
                                           _pf_matrix)
from tests.test_gpu_variant_forms import F32_127, F32_PADDED

pytestmark = pytest.mark.gpu

BAR = 16.0
FLOOR = 32.0
FP64_FORMS = [f for f in FORMS if f[2] == "f64"] + PADDED
FP32_FORMS = [f for f in FORMS if f[2] == "f32"] + F32_PADDED + [F32_127]
SLAB = r"k_sample1s<64>|k_sample_slab<64>"


def _eps(f32):
    return cond_ref.EPS[np.float32 if f32 else np.float64]


def _figures(tag, items, ref, f32, counts, cols=None):
    """E_dev, E_ref and rho = E_dev / max(E_ref, 32 eps) over the columns `cols` (default: all), printed before anything is
    asserted; also the worst column of either and the device's error at the reference's worst column."""
    cols = np.arange(len(counts)) if cols is None else cols
    e_dev = cond_ref.col_err(items, ref["x_ld"])[cols]
    e_ref = ref["e_ref"][cols]
    floor = FLOOR * _eps(f32)
    cd, cr = int(np.argmax(e_dev)), int(np.argmax(e_ref))
    E_dev, E_ref = float(e_dev[cd]), float(e_ref[cr])
    rho = E_dev / max(E_ref, floor)
    print("conditioning %s: E_dev %.3e (column %d, %d ratings)  E_ref %.3e (column %d, %d ratings)  rho %.2f  | at the reference's worst "
          "column: device %.3e" % (tag, E_dev, cols[cd], counts[cols[cd]], E_ref, cols[cr], counts[cols[cr]], rho, e_dev[cr]))
    return dict(tag=tag, E_dev=E_dev, E_ref=E_ref, rho=rho, at_ref_worst=float(e_dev[cr]) / max(E_ref, floor))


def _run_case(eng, me, ot, ref, tag, f32, counts, subsets=None):
    """One launch.  No failure reported (sample_side raises on BPMF_HIP_ECHOL), items and sums finite; returns the figures of all
    columns and of each named subset."""
    items, s, p, n = _launch(eng, me, ot, ref["inputs"])
    assert ref["ok_ld"].all() and ref["ok_ref"].all()                 # (tests/test_cond_host.py: the references factorise every column)
    finite = bool(np.all(np.isfinite(items)) and np.all(np.isfinite(s)) and np.all(np.isfinite(p)) and np.isfinite(n))
    figs = [_figures(tag, items, ref, f32, counts)]
    for name, cols in (subsets or {}).items():
        figs.append(_figures("%s [%s]" % (tag, name), items, ref, f32, counts, cols))
    return finite, figs


def _assert_all(results):
    """After every case has been printed: finite everywhere, rho <= 16 everywhere, and the device within the bar of the
    reference at the column the reference finds hardest."""
    bad = ["%s: not finite" % figs[0]["tag"] for finite, figs in results if not finite]
    bad += ["%s: rho %.2f (E_dev %.3e, E_ref %.3e)" % (f["tag"], f["rho"], f["E_dev"], f["E_ref"])
            for _, figs in results for f in figs if not f["rho"] <= BAR or not f["at_ref_worst"] <= BAR]
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the edge side through every form
EDGE_COND = [pytest.param(f, c, id="%s-chunk-%d" % (f[0], c)) for f in FP64_FORMS + FP32_FORMS for c in (272, 16)]


@pytest.mark.parametrize("form,chunk", EDGE_COND)
def test_edge_side_conditioned(oracle, hip_engine_factory, monkeypatch, form, chunk):
    """One side, one launch per case of the form's dtype: every case with nothing cut (BPMF_HIP_CHUNK=272), the D family again
    with every column above 16 ratings cut, where the order of the chunk partials meets the cancellation."""
    tag, K, dtype, mode, kernel = form
    f32 = dtype == "f32"
    counts, M = _edge()
    ncols = len(counts)
    mean = util.mean_rating(M)
    eng = hip_engine_factory(K, dtype)
    _env(monkeypatch, mode=mode, chunk=chunk)
    me = eng.side_create(ncols, EDGE_NROWS, *M, mean)
    ot = _empty_side(eng, EDGE_NROWS, ncols)
    name, info = eng.kernel_name(me), eng.schedule_info(me)
    assert re.fullmatch(kernel, name), name
    assert info["chunk"] == chunk and info["chunked_columns"] == ((counts > 16).sum() if chunk == 16 else 0) and info["light_columns"] == 0
    cases = [c for c in cond_ref.cases(f32) if chunk == 272 or cond_ref.is_D(c)]
    assert len(cases) == ((8 if f32 else 7) if chunk == 272 else 2)
    results = []
    for case in cases:
        ref = cond_ref.references("edge", K, M, mean, EDGE_NROWS, case, f32, oracle)
        results.append(_run_case(eng, me, ot, ref, "%s chunk %d %s" % (tag, chunk, case[0]), f32, counts))
    eng.side_destroy(me); eng.side_destroy(ot)
    _assert_all(results)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the product form beside the slab form, and the same columns through the slab form alone
@pytest.mark.parametrize("K", [64, 50])
def test_product_form_conditioned(oracle, hip_engine_factory, monkeypatch, K):
    """Matrix B (light majority) with BPMF_HIP_PF unset -- k_sample_pf<64,3 | 6 | 16> for the columns of <= 16 ratings, the slab
    form for the rest -- and with BPMF_HIP_PF=0, the control: the same columns from the same inputs through the slab form.  The
    light columns' figures are reported and held to the bar apart from the heavy ones'."""
    counts, M = _pf_matrix()
    ncols = len(counts)
    mean = util.mean_rating(M)
    eng = hip_engine_factory(K)
    subsets = {"light": np.nonzero(counts <= 16)[0], "heavy": np.nonzero(counts > 16)[0]}
    assert len(subsets["light"]) == 143 and len(subsets["heavy"]) == 6
    results = []
    for pf in (None, 0):
        _env(monkeypatch, pf=pf, chunk=272)
        me = eng.side_create(ncols, PF_NROWS, *M, mean)
        ot = _empty_side(eng, PF_NROWS, ncols)
        name, info = eng.kernel_name(me), eng.schedule_info(me)
        if pf is None:
            assert name == _pf_expect(counts, None)[4] == "k_sample_pf<64,3> + k_sample_pf<64,6> + k_sample_pf<64,16> + k_sample_slab<64>", name
            assert info["light_columns"] == 143
        else:
            assert re.fullmatch(SLAB, name) and info["light_columns"] == 0, name
        for case in cond_ref.cases(False):
            ref = cond_ref.references("pf", K, M, mean, PF_NROWS, case, False, oracle)
            results.append(_run_case(eng, me, ot, ref, "pf K=%d BPMF_HIP_PF=%s %s" % (K, pf, case[0]), False, counts, subsets))
        eng.side_destroy(me); eng.side_destroy(ot)
    _assert_all(results)


# ----------------------------------------------------------------------------------------------------------------------
# 3. a numerically singular prior is reported or survived, never a silent NaN
SINGULAR_FORMS = [f for f in FORMS if f[0] in ("k_sample1-32", "slab-64", "wg2-f64-128", "wg2-f32-128")]


@pytest.mark.parametrize("form", [pytest.param(f, id=f[0]) for f in SINGULAR_FORMS])
def test_singular_prior_is_reported_or_finite(oracle, hip_engine_factory, monkeypatch, form):
    """P(1e18): kappa_2(Lambda*) of the light columns is beyond 1 / eps of either dtype (the longdouble restatement does not
    factorise them either).  The launch either raises BpmfHipError -4 naming a column -- the handled condition of
    test_cholesky_failure_is_reported -- or gives finite items; then P(1e3) on the same side meets the bar."""
    import bpmf_amd
    tag, K, dtype, mode, kernel = form
    f32 = dtype == "f32"
    counts, M = _edge()
    ncols = len(counts)
    mean = util.mean_rating(M)
    eng = hip_engine_factory(K, dtype)
    _env(monkeypatch, mode=mode, chunk=272)
    me = eng.side_create(ncols, EDGE_NROWS, *M, mean)
    ot = _empty_side(eng, EDGE_NROWS, ncols)
    assert re.fullmatch(kernel, eng.kernel_name(me))
    try:
        items = _launch(eng, me, ot, cond_ref.inputs(cond_ref.SINGULAR, K, EDGE_NROWS, f32))[0]
    except bpmf_amd.BpmfHipError as e:
        print("conditioning %s P(1e18): reported: %s" % (tag, e))
        assert e.code == -4 and re.search(r"Cholesky failed in column \d+", str(e)), str(e)
    else:
        print("conditioning %s P(1e18): no failure reported, %d non-finite entries" % (tag, (~np.isfinite(items)).sum()))
        assert np.all(np.isfinite(items))
    P1e3 = [c for c in cond_ref.cases(f32) if c[0] == "P1e3"][0]
    ref = cond_ref.references("edge", K, M, mean, EDGE_NROWS, P1e3, f32, oracle)
    results = [_run_case(eng, me, ot, ref, "%s P1e3 after P(1e18)" % tag, f32, counts)]
    eng.side_destroy(me); eng.side_destroy(ot)
    _assert_all(results)
