"""The column statistics pass (sum x, sum x x^T, sum |x|^2 of a side's fresh columns) in every form, against longdouble sums of the
very array the device holds (get_items), with a bound derived from the arithmetic (tests/colstats_ref.py: (N + 64) 2^-53 times the
sums of magnitudes) instead of a tolerance.  Neither the oracle nor the sampler has to be right for these tests to mean something:
the sampler only fills the array.

The forms: k_colstats<8 | 16 | 32> (one wave per slice of columns, 16x16x4 MFMA tiles, finisher waves behind a ticket), k_colstats<64>
(products on the 4x4x4 shape in rotated accumulators, brought into the tile layout through LDS), the same body as riders at the head
of the partner's fused k_sample1 / k_sample1w / k_sample1s<64> / k_sample1sw<64> launch, k_colstats_wg (four-wave workgroups, sides
above 100 000 local columns), k_colstats_f32<128, double | float> + k_colstats_f32_final (one wave per slice and upper tile, at
most 32 slices) and colstats_f32_rider inside k_sample_wg2<128, 2, float>.  The column counts are the ones where the code branches
(bpmf_hip_side_stat_info says what a side's pass looks like, so a case named for an empty range fails loudly when the rule that made
the range empty changes): 1 .. 9 columns (one wave, one partial trip), around every multiple of 8 / 16 / 32 / 64, 768 | 769 (769: 24
waves of 36 columns, two of them without columns), 3840 | 3841 (24 -> 25 waves), 19 999 | 20 000 (the clamp ends: 512 waves, twelve
empty; also the first count on k_sample4), 2047 | 2048 | 2049 | 3841 in the tile form (the 32-slice cap; one slice empty),
100 000 | 100 001 | 100 003 (the switch to k_colstats_wg: 124 of 2048 wave ranges empty), col_from / col_to slices that are no
multiple of 4, and a slice of one column.

  a. stateless: sample_side -> (s, p, n) and get_items, three launches A, B, A on one side: every sum inside its bound, p exactly
     symmetric, n the fp64 sum of p's diagonal in index order, launch 3 == launch 1 byte for byte (stale partials, tickets that were
     not re-armed), the form and the empty ranges as stat_info reports them;
  b. stateful: two sides driven by sys_sample for three iterations with BPMF_HIP_FUSED = 1 | 0 (fp32: BPMF_HIP_F32_RIDERS = 1 | 0):
     every norm and cov read byte-identical between the two settings and inside B_n / B_cov of the longdouble reference of the
     factors at that point, rider passes > 0 with the switch on and = 0 with it off (stat_info), plain and with per-rating weights.

Observed on an MI355X, worst error / bound over all cases of a form (s | p | n; stateful cases cov | norm; the bar is 1):
  k_colstats<8 | 16 | 32>          0.022 0.049 0.020 | 0.023 0.049 0.036 | 0.024 0.051 0.031
  k_colstats<64>, PF default | 0   0.026 0.046 0.079 | 0.028 0.051 0.057        padded 10 | 20 | 50   0.023 0.040 0.034 | 0.028 0.056 0.035 | 0.022 0.048 0.054
  tile form fp64 128 | padded 100  0.024 0.057 0.057 | 0.025 0.060 0.071        fp32 128 | padded 100  0 0.052 0.11 | 0 0.060 0.12   (sum x of fp32 values: exact)
  k_colstats_wg<8 | 32 | 64>       8.5e-6 1.8e-5 1.1e-5 | 1.4e-5 2.1e-5 1.8e-5 | 1.3e-5 2.2e-5 2.4e-5
  slices K = 16 | 64 | 128         0.0015 0.015 0.031 | 0.0021 0.015 0.0063 | 0.0036 0.015 0.057        k_colstats_wg<8>, c0 != 0   8.6e-6 1.4e-5 1.8e-5
  riders K = 8 | 16 | 32 | 64 | 20 | 50     0.018 0.016 | 0.024 0.025 | 0.027 0.042 | 0.032 0.033 | 0.034 0.026 | 0.030 0.047
  weighted riders K = 8 | 16 | 32 | 64      0.024 0.021 | 0.025 0.024 | 0.030 0.038 | 0.038 0.051
  fp32 riders K = 128 | 100        0.065 0.036 | 0.051 0.049                    K = 128 fp64 (stand-alone only)   0.024 0.012
  launch 3 == launch 1 byte for byte and riders on == riders off byte for byte in every case; stat_info reported the form, the empty
  ranges (769: 2, 20 000: 12, 2049 and 3841 in the tile form: 1, 100 001: 124) and the split (riders on: 3 + 0 and 2 + 1 passes of
  the two sides as riders + stand-alone, off: 0 + 3) in every case that names them.
No defect was found: all 296 cases passed; the file takes 10.4 s, its longest case (k_colstats_wg<64> at 100 001 columns with its
longdouble reference) 1.9 s.

That the net holds was checked once, with two libraries that each carry one planted defect changing arithmetic only, against this
file and against tests/test_gpu_schedule_edges.py (73 cases) and tests/test_gpu_parity.py -k half_iterations (21 cases) as they were
before this file existed:
  (i)  colstats_accumulate masks slot 1 (columns 4 .. 7) of a wave's last trip whenever that trip is partial -- a range of 8 m + 5, 6
       or 7 columns loses 1 .. 3 of them.  Failed here: 95 of 296 (59 wave-form cases, 5 of the 6 workgroup-form cases, the workgroup
       slice, 30 rider cases; the tile form has a loop of its own).  The older tests catch it too: 60 of 73 and 9 of 21.
  (ii) colstats_body's finisher starts the partial loop of its last quarter one partial late when nwaves % 4 != 0 -- one wave's
       partial is dropped, but only where the last quarter has partials at all.  Failed here: 21 of 296 (3841 columns = 25 waves in
       all 8 wave forms, 19 999 columns = 125 waves at K = 8, 16, 32, the ten rider configurations at (3841, 770)).  The older tests
       pass it: 73 of 73 and 21 of 21 (sides of 33, 149, 943 and 1682 columns run 2, 5, 24 and 24 waves).
"""
import numpy as np
import pytest

from tests import colstats_ref as R

pytestmark = pytest.mark.gpu

NROWS = 7                                                             # rows of the partner of a stateless side
_CACHE = {}
_WORST = {}


def _kdev(Kt):
    return next(k for k in (8, 16, 32, 64, 128) if k >= Kt)


def _matrix(ncols, nrows, seed):
    """CSC triple with 0 .. 3 ratings per column (rows distinct and ascending), values around 3."""
    key = ("M", ncols, nrows, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        counts = rng.integers(0, min(3, nrows) + 1, size=ncols)
        colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        # distinct rows per column: a random start, then consecutive rows modulo nrows, sorted within the column
        start = np.repeat(rng.integers(0, nrows, size=ncols), counts)
        r = (start + np.arange(colptr[-1]) - np.repeat(colptr[:-1], counts)) % nrows
        col = np.repeat(np.arange(ncols), counts)
        rowidx = r[np.lexsort((r, col))].astype(np.int32)
        vals = rng.normal(3.0, 1.0, size=int(colptr[-1]))
        for a in (colptr, rowidx, vals):
            a.setflags(write=False)
        _CACHE[key] = (colptr, rowidx, vals)
    return _CACHE[key]


def _transpose(M, nrows):
    colptr, rowidx, vals = M
    cols = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))
    order = np.lexsort((cols, rowidx))
    tptr = np.concatenate([[0], np.cumsum(np.bincount(rowidx, minlength=nrows))]).astype(np.int64)
    return tptr, cols[order].astype(np.int32), np.ascontiguousarray(vals[order])


def _mean(M):
    return float(M[2].sum()) / max(len(M[2]), 1)


def _inputs(oracle, Kt, ncols, f32):
    """Two sets of launch inputs (partner's factors, it, alpha, mu, LambdaF): mu with entries of order 1, LambdaF drawn by the
    oracle from a random SPD cov (as tests/test_gpu_schedule_edges.py)."""
    key = ("in", Kt, ncols, f32)
    if key not in _CACHE:
        rng = np.random.default_rng(7000 + Kt)
        out = []
        for scale, it, alpha in ((0.3, 3, 2.0), (0.45, 8, 1.5)):
            U = scale * rng.standard_normal((NROWS, Kt))
            if f32:
                U = U.astype(np.float32).astype(np.float64)
            A = rng.standard_normal((Kt, 3 * Kt))
            _, _, LF = oracle.hyper_sample(Kt, ncols, A @ A.T / (3 * Kt), it)
            mu = rng.standard_normal(Kt) + np.where(np.arange(Kt) % 2, 1.0, -1.0)
            out.append((U, it, alpha, mu, LF))
        _CACHE[key] = out
    return _CACHE[key]


def _env(monkeypatch, **kw):
    for name in ("BPMF_HIP_MODE", "BPMF_HIP_CHUNK", "BPMF_HIP_PF", "BPMF_HIP_FUSED", "BPMF_HIP_F32_RIDERS"):
        v = kw.get(name[9:].lower())
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _note(form, tag, r):
    """Every figure before it is asserted (pytest -s / -rP shows them), and the worst of the form so far."""
    w = _WORST.setdefault(form, [0.0, 0.0, 0.0])
    for i in range(3):
        w[i] = max(w[i], r[i])
    print("colstats %-28s %-34s error / bound  s %.3e  p %.3e  n %.3e   (worst of the form so far %.3e %.3e %.3e)" % ((form, tag) + tuple(r) + tuple(w)))


def _check_sums(form, tag, X, s, p, n):
    """X: the local columns as get_items returned them.  The assertions of part a for one launch."""
    Kt = X.shape[1]
    assert s.shape == (Kt,) and p.shape == (Kt, Kt)                   # the caller's size, also on the padded kernels
    ref = R.sums(X)
    r = R.ratios(s, p, n, ref)
    _note(form, tag, r)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(p)) and np.isfinite(n)
    assert r[0] <= 1.0 and r[1] <= 1.0 and r[2] <= 1.0
    assert np.array_equal(p, p.T)                                     # exactly symmetric
    nn = 0.0
    for i in range(Kt):
        nn += p[i, i]
    assert n == nn                                                    # the fp64 sum of the diagonal in index order
    assert np.abs(X).max() > 0.1                                      # (the columns were sampled: not a sum of zeros)


def _stateless(oracle, eng, monkeypatch, form, N, expect_form, dagger, pf=None, ncols=None, col_from=0, col_to=None):
    Kt = eng.K
    f32 = eng.dtype == "f32"
    ncols = N if ncols is None else ncols
    col_to = ncols if col_to is None else col_to
    nloc = col_to - col_from
    assert nloc == N
    _env(monkeypatch, pf=pf)
    M = _matrix(nloc, NROWS, 11 + N % 13)
    me = eng.side_create(ncols, NROWS, *M, _mean(M), col_from=col_from, col_to=col_to)
    ot = eng.side_create(NROWS, ncols, np.zeros(NROWS + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)
    info = eng.stat_info(me)
    print("colstats %-28s N=%d %s  %s" % (form, N, eng.kernel_name(me), info))
    assert info["form"] == expect_form
    assert info["per"] % 4 == 0 and info["per"] == (-(-N // (info["units"] * (4 if expect_form == "workgroups" else 1))) + 3) // 4 * 4
    if dagger:
        assert info["empty"] >= 1                                     # the case is named for a range without columns
    if N <= 9:
        assert info["units"] == 1                                     # one wave, one partial trip
    inputs = _inputs(oracle, Kt, ncols, f32)
    out = []
    for i, j in enumerate((0, 1, 0)):
        U, it, alpha, mu, LF = inputs[j]
        eng.set_items(ot, U)
        s, p, n = eng.sample_side(me, ot, it, alpha, mu, LF)
        items = eng.get_items(me)
        assert items.shape == (ncols, Kt)
        assert not items[:col_from].any() and not items[col_to:].any()     # columns outside the slice stay zero
        if i == 0 or (i == 1 and N < 50000):                          # (launch 3 is launch 1 byte for byte: below)
            _check_sums(form, "N=%d launch %d" % (N, i), items[col_from:col_to], s, p, n)
        out.append((items, s.copy(), p.copy(), n))
    after = eng.stat_info(me)
    assert after["alone_passes"] == 3 and after["rider_passes"] == 0
    assert not np.array_equal(out[1][1], out[0][1])                   # B is another launch
    assert np.array_equal(out[2][0], out[0][0])                       # bit for bit
    assert out[2][1].tobytes() == out[0][1].tobytes() and out[2][2].tobytes() == out[0][2].tobytes() and out[2][3] == out[0][3]
    eng.side_destroy(me); eng.side_destroy(ot)


# ----------------------------------------------------------------------------------------------------------------------
# a. stateless sums
WAVE_NS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 97, 129, 768, 769, 3840, 3841]
WAVE_DAGGER = {769, 20000}
# (id, num_latent, dtype, BPMF_HIP_PF)
WAVE_FORMS = [("k_colstats<8>", 8, None), ("k_colstats<16>", 16, None), ("k_colstats<32>", 32, None), ("k_colstats<64>", 64, None),
              ("k_colstats<64> PF=0", 64, 0), ("k_colstats<16> padded 10", 10, None), ("k_colstats<32> padded 20", 20, None),
              ("k_colstats<64> padded 50", 50, None)]
WAVE_CASES = [pytest.param(f, N, id="%s-N%d" % (f[0].replace(" ", "-"), N)) for f in WAVE_FORMS for N in WAVE_NS] + \
             [pytest.param(f, N, id="%s-N%d" % (f[0], N)) for f in WAVE_FORMS[:3] for N in (19999, 20000)]


@pytest.mark.parametrize("form,N", WAVE_CASES)
def test_wave_form(oracle, hip_engine_factory, monkeypatch, form, N):
    tag, Kt, pf = form
    _stateless(oracle, hip_engine_factory(Kt), monkeypatch, tag, N, "waves", N in WAVE_DAGGER, pf=pf)


TILE_NS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 3841]
TILE_DAGGER = {2049, 3841}
TILE_FORMS = [("k_colstats_f32<128,double>", 128, "f64"), ("k_colstats_f32<128,float>", 128, "f32"),
              ("k_colstats_f32<128,double> padded 100", 100, "f64"), ("k_colstats_f32<128,float> padded 100", 100, "f32")]


@pytest.mark.parametrize("form,N", [pytest.param(f, N, id="%s-N%d" % (f[0].replace(" ", "-"), N)) for f in TILE_FORMS for N in TILE_NS])
def test_tile_form(oracle, hip_engine_factory, monkeypatch, form, N):
    tag, Kt, dtype = form
    _stateless(oracle, hip_engine_factory(Kt, dtype), monkeypatch, tag, N, "tiles", N in TILE_DAGGER)


@pytest.mark.parametrize("Kt,N", [(8, 100000), (8, 100001), (8, 100003), (32, 100001), (32, 100003), (64, 100001)])
def test_workgroup_form_and_the_last_count_below_it(oracle, hip_engine_factory, monkeypatch, Kt, N):
    big = N > 100000
    _stateless(oracle, hip_engine_factory(Kt), monkeypatch, "k_colstats_wg<%d>" % Kt if big else "k_colstats<%d>" % Kt, N,
               "workgroups" if big else "waves", big)


@pytest.mark.parametrize("Kt", [16, 64, 128])
@pytest.mark.parametrize("lo,hi", [(3, 767), (5, 6)], ids=["3-to-N-2", "one-column"])
def test_slice(oracle, hip_engine_factory, monkeypatch, Kt, lo, hi):
    """col_from / col_to of a 769-column side: c0 is no multiple of 4, the sums are over the local columns only."""
    _stateless(oracle, hip_engine_factory(Kt), monkeypatch, "slice K=%d" % Kt, hi - lo, "tiles" if Kt == 128 else "waves", False,
               ncols=769, col_from=lo, col_to=hi)


def test_slice_in_the_workgroup_form(oracle, hip_engine_factory, monkeypatch):
    """(100 001, 200 003) of a 200 005-column side at K = 8: k_colstats_wg with c0 != 0."""
    _stateless(oracle, hip_engine_factory(8), monkeypatch, "slice k_colstats_wg<8>", 100002, "workgroups", True,
               ncols=200005, col_from=100001, col_to=200003)


# ----------------------------------------------------------------------------------------------------------------------
# b. riders against the stand-alone pass, stateful path
def _stateful_run(eng, Na, Nb, weighted):
    """Three iterations of (a, b) through sys_sample.  A side's state is read only after the partner's next launch has been
    enqueued (its sums were then formed by riders, when there are riders) -- but for b's last pass, read straight away: no launch to
    ride in.  Returns [(side name, iteration, norm, cov, local factors)] and the two stat_infos."""
    Ma = _matrix(Na, Nb, 100 + Na)
    Mb = _transpose(Ma, Nb)
    a = eng.side_create(Na, Nb, *Ma, _mean(Ma))
    b = eng.side_create(Nb, Na, *Mb, _mean(Ma))
    if weighted:
        rng = np.random.default_rng(5)
        w = rng.uniform(0.5, 2.0, size=len(Ma[2]))
        col = np.repeat(np.arange(Na), np.diff(Ma[0]))
        eng.set_weights(a, w)
        eng.set_weights(b, w[np.lexsort((col, Ma[1]))])               # the same cells in the transpose's order
    reads = []

    def read(name, side):
        it, norm, cov = eng.sys_state(side)[:3]
        reads.append((name, it, norm, np.array(cov), eng.get_items(side).copy()))

    for i in range(3):
        eng.sys_sample(a, b, 2.0)
        if i >= 1:
            read("b", b)                                              # b's pass of iteration i - 1: carried by a's launch
        eng.sys_sample(b, a, 2.0)
        if i == 2:
            read("b", b)                                              # nothing will carry this one: a kernel of its own
        read("a", a)                                                  # carried by b's launch
    names = (eng.kernel_name(a), eng.kernel_name(b))
    infos = (eng.stat_info(a), eng.stat_info(b))
    eng.side_destroy(a); eng.side_destroy(b)
    return reads, infos, names


def _stateful(eng, monkeypatch, form, Na, Nb, switch, weighted=False, riders=True):
    runs = {}
    for on in (1, 0):
        _env(monkeypatch, pf=0 if _kdev(eng.K) == 64 else None, **{switch: on})
        runs[on] = _stateful_run(eng, Na, Nb, weighted)
    (ra, ia, names), (rb, ib, _) = runs[1], runs[0]
    print("colstats %-28s (%d, %d) %s | %s  riders on: %s  off: %s" % (form, Na, Nb, names[0], names[1], ia, ib))
    assert len(ra) == len(rb) == 6
    for (name, it, norm, cov, X), (name0, it0, norm0, cov0, X0) in zip(ra, rb):
        assert (name, it) == (name0, it0)
        assert norm == norm0 and cov.tobytes() == cov0.tobytes() and np.array_equal(X, X0)    # byte-identical between the settings
        ref = R.sums(X)
        N = X.shape[0]
        c_ref, B = R.cov(ref)
        rc = float((np.abs(np.asarray(cov, R.LD) - c_ref) / B).max())
        rn = float(abs(R.LD(norm) - ref["n"]) / R.bounds(ref)[2])
        _note(form, "(%d, %d) side %s iteration %d: cov, -, norm" % (Na, Nb, name, it), (rc, 0.0, rn))
        assert rc <= 1.0 and rn <= 1.0
        assert np.array_equal(cov, cov.T) and np.count_nonzero(X) == X.size      # (every column was sampled: not sums of zeros)
    for info in ia + ib:
        assert info["rider_passes"] + info["alone_passes"] == 3       # one pass per half-iteration, whoever carried it
    assert all(info["rider_passes"] == 0 for info in ib)
    if riders:
        assert ia[0]["rider_passes"] > 0 and ia[1]["rider_passes"] > 0
        assert ia[1]["alone_passes"] >= 1                             # b's last pass had no launch to ride in
    else:
        assert all(info["rider_passes"] == 0 for info in ia)


PAIRS = [(769, 33), (5, 161), (3841, 770), (2, 9)]
STATEFUL = [(Kt, False) for Kt in (8, 16, 32, 64, 20, 50)] + [(Kt, True) for Kt in (8, 16, 32, 64)]


@pytest.mark.parametrize("Na,Nb", PAIRS)
@pytest.mark.parametrize("Kt,weighted", STATEFUL, ids=["K%d%s" % (k, "-weighted" if w else "") for k, w in STATEFUL])
def test_riders_equal_the_stand_alone_pass(hip_engine_factory, monkeypatch, Kt, weighted, Na, Nb):
    """colstats_body at the head of k_sample1 / k_sample1w / k_sample1s<64> / k_sample1sw<64> against k_colstats."""
    _stateful(hip_engine_factory(Kt), monkeypatch, "riders K=%d%s" % (Kt, " weighted" if weighted else ""), Na, Nb, "fused", weighted)


@pytest.mark.parametrize("Na,Nb", [(2049, 65), (5, 64)])
@pytest.mark.parametrize("Kt", [128, 100])
def test_f32_riders_equal_the_stand_alone_pass(hip_engine_factory, monkeypatch, Kt, Na, Nb):
    """colstats_f32_rider inside k_sample_wg2<128, 2, float> against k_colstats_f32 + k_colstats_f32_final."""
    _stateful(hip_engine_factory(Kt, "f32"), monkeypatch, "f32 riders K=%d" % Kt, Na, Nb, "f32_riders")


def test_k128_fp64_has_no_rider_form(hip_engine_factory, monkeypatch):
    _stateful(hip_engine_factory(128), monkeypatch, "K=128 fp64 stateful", 2049, 65, "f32_riders", riders=False)
