"""The -o posterior outputs -- k_aggr_add / k_aggr_finalize (U-mu.ddm, U-Lambda.ddm) and every form of k_predict (Pavg.sdm,
Pm2.sdm) -- against references written here in numpy longdouble (independent of the oracle's fp64 code).

  1. Aggregation.  S sample matrices go in with set_items, aggr_add follows each, aggr_finalize(S) returns mu and Lambda.  The
     reference is the longdouble mean and two-pass centred covariance; Lambda_ref is numpy's inverse of it refined by two
     Newton-Schulz steps in longdouble.  mu: rtol 1e-13.  Lambda: per column err = max|L - L_ref| / max|L_ref|, and the device's
     err may be at most 8 x the err of the plain fp64 restatement of the device's formula on the same inputs (sums in sample
     order, (prod - sum sum^T / n) / (n - 1), np.linalg.inv): the cancellation of the one-pass formula and the condition number
     are in the bar, not in a constant.  K = 8 .. 128, the padded sizes (device leading dimension != K), fp32 factors, S = K + 72
     (condition number of a few hundred) and S = K + 1 (up to 1e6), a col_from / col_to slice, a side that aggregates a second
     time after _finalize freed its buffers, every sequence twice bit for bit.  The inputs make the elimination interchange
     rows: interchanges() restates the kernel's pivot rule and every case asserts at least one per column.
  2. nsamples <= K.  A covariance of n samples has rank n - 1 at most: every Lambda entry is NaN (the kernel used to run the
     elimination on the rounding residue of the pivots and return finite entries of 1e15 .. 1e17), mu is still sum / n, and
     `bpmf -o` says so on stderr.
  3. k_predict<K, 256>, k_predict<K, 64> (BPMF_HIP_PREDICT_WG=64), k_predict_f32<128> and k_predict<128, 256, float> (fp32 with a
     twin) over the call sequence n = 0, 0, 1, 2, 5 with the factors changed between calls, at 0 .. 65 537 test entries (one
     entry, a tail block, one block more than the final tree has threads), with a twin, on a slice, every case twice from fresh
     test matrices bit for bit.  Bars of test_predict_matches_oracle: se / se_avg 1e-9 relative, Pavg rtol 1e-12, Pm2 rtol
     1e-10 + atol 1e-12, count exact.

The sums.  The error of Lambda is the rounding of prod, amplified by the condition number; the elimination adds little.  The
factor 8 stands between two eliminations OF THE SAME MATRIX, so the restatement has to round its sums as the device does:
k_aggr_add's `l += x_i x_j` is one fused multiply-add (the library is built with -ffp-contract=on), and fma() below is that
operation in numpy, exact (checked against the C library's fma in test_the_restatement_fuses_like_the_c_library).  With a
plain `p += x * x'` in the restatement -- two roundings, another realisation of the same noise -- the per-column ratio is a
quotient of two independent errors: over the 24 columns of one case the restatement's own err / cond spreads over a factor
of 30 .. 170, and the first run on an MI355X gave ratios of 13.4 (K = 8, S = 80), 11.4 (8, 9), 97.8 (32, 33), 9.0 (10, 11),
8.6 (20, 21), 10.8 (100, 101), 12.4 (re-use, 20, 21) in the column where the restatement was lucky.  That is not the kernel:
the CPU gives the same figures with no device involved (numpy's own inverse of the fused sums against the unfused
restatement: 11.6 at (8, 80), 11.4 at (8, 9), 88.9 at (32, 33), 11.1 at (100, 101), 11.4 at the re-use's (20, 21), in the same
columns), and the fp32 cases, whose products are exact in fp64 so that fused and unfused sums agree, sat at 1.06 .. 1.10 all
along.  Bar, reference and formula are unchanged.

Observed on an MI355X, worst over all cases (Lambda: device err / restatement err per column, bar 8; mu: relative, bar 1e-13;
row interchanges per column of the inputs, from interchanges()):
  K              8        16       32       64       128      10       20       50       100      128 fp32
  Lambda ratio   1.84     2.19     1.20     2.35     2.04     1.58     2.44     2.62     1.15     1.10
  mu             6.3e-16  8.1e-16  9.8e-16  1.1e-15  1.5e-15  7.2e-16  8.2e-16  1.2e-15  1.2e-15  8.8e-17
  interchanges   2 .. 7   6 .. 11  13 .. 18 25 .. 36 56 .. 69 4 .. 6   7 .. 14  21 .. 28 44 .. 53 56 .. 65
  (Lambda err itself: 2e-12 .. 1e-11 at S = K + 72, up to 4.6e-4 at K = 128, S = 129 in fp64 and 8.9e-4 in fp32, where the
  restatement has 4.7e-4 and 8.8e-4.)  Slices and second aggregations equal the whole / fresh side bit for bit.
  form                       se / se_avg   Pavg      Pm2 (absolute; share of rtol 1e-10 + atol 1e-12)
  k_predict<K, 256>          9.6e-16       1.3e-13   3.6e-16; 1.9e-4
  k_predict<K, 64>           9.6e-16       1.1e-14   2.4e-16; 1.7e-4
  k_predict_f32<128>         5.4e-16       5.7e-15   3.7e-16; 1.8e-4
  k_predict<128, 256, float> 5.4e-16       6.5e-15   3.7e-16; 1.8e-4     (owner and twin)
  Every repeated run, the 64- against the 256-thread form, the twin against the users' side alone, fp32 with against without a
  twin and the slice against the whole side: bit for bit.
86 cases.  At the first run 8 of the 85 there were then failed -- six whole-side Lambda cases and two re-use cases, every
one the unfused restatement of "The sums" above, a defect of this file; after it none.  The kernels' defect is the one of
part 2 (found by reading, confirmed by the cases of test_too_few_samples_give_nan); one more was found by reading on the way to
nnz = 0:
dev_upload copied one element from an EMPTY host array (an over-read of the caller's memory at an empty test or rating
matrix), and now copies none.
That the net holds was checked once with a library carrying two mutations: k_aggr_finalize without the column interchanges at
its end failed every one of the 26 cases that check a Lambda (20 whole sides, 3 slices, 3 re-uses; ratios of 8e8 and more)
and no mu check; k_predict's final loop without its stride (a thread adds its own block's partial only) failed exactly the 5
cases with more blocks than threads -- 65 537 entries at 256 threads, 4 097 entries at 64 threads at K = 8, 32, 128 and the
64-thread twin -- each at its se bar, and no other.  (Starting that loop at w = 0 for every thread was not tried: it
multiplies every sum by the number of threads and fails everything.)
"""
import os
import subprocess

import numpy as np
import pytest

from bpmf_amd import io as bio
from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

LD = np.longdouble
BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
_CACHE = {}


def _same_bytes(a, b):
    """bit for bit, NaN included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _empty_side(eng, ncols, nrows, mean=0.0, col_from=0, col_to=None):
    nloc = (ncols if col_to is None else col_to) - col_from
    return eng.side_create(ncols, nrows, np.zeros(nloc + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), mean, col_from=col_from, col_to=col_to)


# ----------------------------------------------------------------------------------------------------------------------
# 1. aggregation
AG_NCOLS, AG_NROWS = 24, 30
LAMBDA_FACTOR = 8.0                                                   # device err <= 8 x the fp64 restatement's err
MU_RTOL = 1e-13


def aggr_samples(K, S, seed, f32=False):
    """X [S, ncols, K]: column c is a mix of a scaled normal vector and its mirror image, so that the largest entry of the
    covariance's k-th column under elimination is not on the diagonal (the kernel has to interchange rows)."""
    key = ("X", K, S, seed, f32)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        sc = np.linspace(0.2, 1.5, K)
        X = np.empty((S, AG_NCOLS, K))
        for c in range(AG_NCOLS):
            Z = rng.standard_normal((S, K))
            X[:, c, :] = 0.7 + 0.3 * (Z * sc + 0.8 * Z[:, ::-1] * sc[::-1])
        if f32:
            X = X.astype(np.float32).astype(np.float64)               # the references see the factors the device sees
        X.setflags(write=False)
        _CACHE[key] = X
    return _CACHE[key]


def lambda_reference(X):
    """longdouble: (mu [n, K], Lambda [n, K, K]) of the samples X [S, n, K] -- mean, two-pass centred covariance, numpy's fp64
    inverse refined by two Newton-Schulz steps Y <- Y (2 I - C Y)."""
    Xl = np.asarray(X).astype(LD)
    S, n, K = Xl.shape
    mu = Xl.sum(0) / LD(S)
    D = Xl - mu
    lam = np.empty((n, K, K), LD)
    I2 = 2 * np.eye(K, dtype=LD)
    for c in range(n):
        C = D[:, c].T @ D[:, c] / LD(S - 1)
        Y = np.linalg.inv(C.astype(np.float64)).astype(LD)
        for _ in range(2):
            Y = Y @ (I2 - C @ Y)
        lam[c] = Y
    return mu, lam


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """(p, e) with p + e = a b exactly (Dekker; 2^27 + 1 splits a double into two halves of 26 bits)"""
    p = a * b
    t = 134217729.0 * a; ah = t - (t - a); al = a - ah
    t = 134217729.0 * b; bh = t - (t - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """a b + c with ONE rounding, in numpy (Boldo & Melquiond, "Emulation of a FMA and correctly rounded sums", 2008): the exact
    product as two doubles, c added to the high one, the two low parts added with rounding to odd (the TwoSum result moved to
    its odd neighbour on the side of the remainder when it is inexact and even), the high part last."""
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    vh, vl = _two_sum(tl, ul)
    bits = np.ascontiguousarray(vh).view(np.uint64)
    adjust = (vl != 0) & ((bits & np.uint64(1)) == 0)
    away = (vl > 0) == (vh > 0)                                       # the remainder points away from zero: the next pattern up
    bits = np.where(adjust, np.where(away, bits + np.uint64(1), bits - np.uint64(1)), bits)
    return th + bits.view(np.float64)


def lambda_restatement(X):
    """(cov, Lambda) [n, K, K] in plain fp64 by the device's formula AND its roundings: sum and prod in sample order, prod with
    the fused multiply-add k_aggr_add compiles to (-ffp-contract=on), the one-pass covariance (prod - sum sum^T / n) / (n - 1),
    np.linalg.inv.  The two eliminations then start from the same matrix, which is what the factor between them assumes; see
    "The sums" in the module docstring for what an unfused sum does to the bar."""
    X = np.asarray(X, np.float64)
    S, n, K = X.shape
    iu, ju = np.triu_indices(K)                                       # (x_i x_j = x_j x_i bit for bit: the upper triangle, mirrored)
    s = np.zeros((n, K)); pu = np.zeros((n, len(iu)))
    exact = np.array_equal(X, X.astype(np.float32))                   # products of fp32 numbers are exact: nothing to fuse
    for x in X:
        s += x
        pu = pu + x[:, iu] * x[:, ju] if exact else fma(x[:, iu], x[:, ju], pu)
    p = np.empty((n, K, K))
    p[:, iu, ju] = pu; p[:, ju, iu] = pu
    cov = (p - s[:, :, None] * s[:, None, :] / S) / (S - 1)
    return cov, np.linalg.inv(cov)


def lambda_err(L, Lref):
    """per column: max|L - L_ref| / max|L_ref|"""
    d = np.abs(np.asarray(L).astype(LD) - Lref).reshape(len(Lref), -1).max(1)
    return (d / np.abs(Lref).reshape(len(Lref), -1).max(1)).astype(np.float64)


def interchanges(C):
    """Row interchanges of k_aggr_finalize's elimination of one covariance: in-place Gauss-Jordan, the pivot of step k is the
    largest |A(r, k)|, r >= k, the lowest r among equals."""
    A = np.array(C, np.float64)
    n = 0
    for k in range(len(A)):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]; n += 1
        d = A[k, k]
        A[k] /= d; A[k, k] = 1.0 / d
        f = A[:, k].copy(); f[k] = 0.0
        A -= np.outer(f, A[k])
        A[:, k] = -f * A[k, k]; A[k, k] = 1.0 / d
    return n


def _aggr_refs(K, S, seed, f32=False):
    """(X, mu_ref, Lambda_ref, err of the restatement per column, interchanges per column): once per input set, never written"""
    key = ("ref", K, S, seed, f32)
    if key not in _CACHE:
        X = aggr_samples(K, S, seed, f32)
        if S > K:
            mu, lam = lambda_reference(X)
            cov, rest = lambda_restatement(X)
            err = lambda_err(rest, lam)
            swaps = np.array([interchanges(c) for c in cov])
        else:                                                         # (no K x K covariance to invert: the mean alone)
            mu, lam, err, swaps = X.astype(LD).sum(0) / LD(S), None, None, None
        for a in (mu, lam, err, swaps):
            if a is not None:
                a.setflags(write=False)
        _CACHE[key] = (X, mu, lam, err, swaps)
    return _CACHE[key]


def _aggregate(eng, side, X):
    for x in X:
        eng.set_items(side, x)
        eng.aggr_add(side)
    return eng.aggr_finalize(side, len(X))


def _lam3(lam, K):
    """[n, K*K] (column-major K x K per column, the layout of U-Lambda.ddm) -> [n, K, K]"""
    return lam.reshape(len(lam), K, K).transpose(0, 2, 1)


def _check_mu(tag, mu, mu_ref):
    rel = float((np.abs(mu.astype(LD) - mu_ref) / np.abs(mu_ref)).max())
    print("posterior-outputs %s: mu rel err %.3e (bar %.0e)" % (tag, rel, MU_RTOL))
    assert np.all(np.isfinite(mu)) and rel <= MU_RTOL, rel


def _check_aggr(tag, K, mu, lam, refs, cols=slice(None)):
    X, mu_ref, lam_ref, err_rest, swaps = refs
    assert mu.shape == mu_ref[cols].shape and lam.shape == (len(mu), K * K)
    assert swaps[cols].min() >= 1, swaps                              # (a condition on the inputs)
    _check_mu(tag, mu, mu_ref[cols])
    err = lambda_err(_lam3(lam, K), lam_ref[cols])
    ratio = err / err_rest[cols]
    print("posterior-outputs %s: Lambda err device %.3e restatement %.3e, worst ratio %.3f (bar %.0f), interchanges %d .. %d"
          % (tag, err.max(), err_rest[cols].max(), ratio.max(), LAMBDA_FACTOR, swaps[cols].min(), swaps[cols].max()))
    assert np.all(np.isfinite(lam))
    assert np.all(err <= LAMBDA_FACTOR * err_rest[cols]), (ratio.max(), int(np.argmax(ratio)))


def test_the_restatement_fuses_like_the_c_library():
    """fma() above against the C library's fma on operands of the aggregation's kind and on products that cancel against c."""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    rng = np.random.default_rng(3)
    a = 0.7 + 0.5 * rng.standard_normal(20000); b = 0.7 + 0.5 * rng.standard_normal(20000)
    c = np.concatenate([rng.uniform(0, 200, 10000), -(a[10000:] * b[10000:]) * (1 + rng.integers(-4, 5, 10000) * 2.0 ** -52)])
    want = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert _same_bytes(fma(a, b, c), want)
    assert (want != a * b + c).sum() > 1000                           # (the operands do tell one rounding from two)


AGGR_K = [(K, "f64") for K in (8, 16, 32, 64, 128, 10, 20, 50, 100)] + [(128, "f32")]
AGGR_CASES = [pytest.param(K, dt, extra, id="K%d-%s-S=K+%d" % (K, dt, extra)) for K, dt in AGGR_K for extra in (72, 1)]


@pytest.mark.parametrize("K,dtype,extra", AGGR_CASES)
def test_aggregation_against_longdouble(hip_engine_factory, K, dtype, extra):
    """mu and Lambda of S = K + extra samples on a whole side; the sequence a second time on a fresh side, bit for bit."""
    S, f32 = K + extra, dtype == "f32"
    refs = _aggr_refs(K, S, 100 + K, f32)
    eng = hip_engine_factory(K, dtype)
    out = []
    for _ in range(2):
        side = _empty_side(eng, AG_NCOLS, AG_NROWS)
        out.append(_aggregate(eng, side, refs[0]))
        eng.side_destroy(side)
    _check_aggr("aggr K=%d %s S=%d" % (K, dtype, S), K, out[0][0], out[0][1], refs)
    assert _same_bytes(out[0][0], out[1][0]) and _same_bytes(out[0][1], out[1][1])


@pytest.mark.parametrize("K", [32, 50, 128])
def test_aggregation_of_a_slice(hip_engine_factory, K):
    """A side that owns the columns [5, 19) of 24: 14 columns come back, and they are columns 5 .. 18 of the whole side's result
    bit for bit (k_aggr_add reads the factors from column col_from on)."""
    lo, hi = 5, 19
    refs = _aggr_refs(K, K + 72, 100 + K)
    eng = hip_engine_factory(K)
    whole = _empty_side(eng, AG_NCOLS, AG_NROWS)
    part = _empty_side(eng, AG_NCOLS, AG_NROWS, col_from=lo, col_to=hi)
    mu_w, lam_w = _aggregate(eng, whole, refs[0])
    mu_p, lam_p = _aggregate(eng, part, refs[0])
    eng.side_destroy(whole); eng.side_destroy(part)
    assert mu_p.shape == (hi - lo, K) and lam_p.shape == (hi - lo, K * K)
    _check_aggr("aggr slice K=%d" % K, K, mu_p, lam_p, refs, slice(lo, hi))
    assert _same_bytes(mu_p, mu_w[lo:hi]) and _same_bytes(lam_p, lam_w[lo:hi])


@pytest.mark.parametrize("K", [8, 20, 128])
def test_aggregation_a_second_time_on_the_same_side(hip_engine_factory, K):
    """_finalize frees the buffers: set A (S = K + 72), finalize, then set B (S = K + 1, other samples) on the SAME side gives B's
    result alone -- the bars for B, and the bytes of a fresh side that saw only B."""
    refs_a, refs_b = _aggr_refs(K, K + 72, 100 + K), _aggr_refs(K, K + 1, 900 + K)
    eng = hip_engine_factory(K)
    side = _empty_side(eng, AG_NCOLS, AG_NROWS)
    mu_a, lam_a = _aggregate(eng, side, refs_a[0])
    mu_b, lam_b = _aggregate(eng, side, refs_b[0])
    fresh = _empty_side(eng, AG_NCOLS, AG_NROWS)
    mu_f, lam_f = _aggregate(eng, fresh, refs_b[0])
    eng.side_destroy(side); eng.side_destroy(fresh)
    _check_aggr("aggr re-use K=%d, set A" % K, K, mu_a, lam_a, refs_a)
    _check_aggr("aggr re-use K=%d, set B" % K, K, mu_b, lam_b, refs_b)
    assert _same_bytes(mu_b, mu_f) and _same_bytes(lam_b, lam_f)


def test_finalize_without_aggregation_raises(hip_engine_factory):
    import bpmf_amd
    eng = hip_engine_factory(8)
    side = _empty_side(eng, AG_NCOLS, AG_NROWS)
    with pytest.raises(bpmf_amd.BpmfHipError) as e:
        eng.aggr_finalize(side, 3)
    assert "nothing was aggregated" in str(e.value)
    eng.aggr_add(side)                                                # ... and once more after a finalize
    eng.aggr_finalize(side, 1)
    with pytest.raises(bpmf_amd.BpmfHipError):
        eng.aggr_finalize(side, 1)
    eng.side_destroy(side)


# ----------------------------------------------------------------------------------------------------------------------
# 2. nsamples <= K: NaN, not the inverse of rounding residue
@pytest.mark.parametrize("K,S", [(8, 1), (8, 2), (8, 8), (20, 20), (128, 15), (8, 9), (128, 129)],
                         ids=lambda v: str(v))
def test_too_few_samples_give_nan(hip_engine_factory, K, S):
    """S <= K: every entry of every Lambda is NaN, mu meets its bar.  S = K + 1: every entry is finite."""
    X, mu_ref, lam_ref, err_rest, swaps = _aggr_refs(K, S, 100 + K if S > K else 500 + K)
    eng = hip_engine_factory(K)
    side = _empty_side(eng, AG_NCOLS, AG_NROWS)
    mu, lam = _aggregate(eng, side, X)
    eng.side_destroy(side)
    _check_mu("too few samples K=%d S=%d" % (K, S), mu, mu_ref)
    if S <= K:
        assert np.all(np.isnan(lam)), "%d finite entries, max %.3e" % (np.isfinite(lam).sum(), np.nanmax(np.abs(lam)))
    else:
        assert np.all(np.isfinite(lam))


def _bpmf(args, cwd):
    data = ["-n", os.path.join(util.GOLDEN, "tiny-train.mtx"), "-p", os.path.join(util.GOLDEN, "tiny-test.mtx")]
    return subprocess.run([BPMF] + args + data, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_cli_says_when_the_kept_samples_are_too_few(tmp_path):
    """bpmf -d 32 -i 6 -b 2 -o: four samples of a 32-vector.  Exit 0, one line on stderr, Lambda all NaN, mu finite."""
    (tmp_path / "o").mkdir()
    r = _bpmf(["-d", "32", "-i", "6", "-b", "2", "-o", "o/"], tmp_path)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stderr.splitlines() if "Lambda.ddm" in l]
    assert len(lines) == 1 and "NaN" in lines[0] and "do not determine a 32 x 32 covariance" in lines[0], r.stderr
    assert "Lambda.ddm" not in r.stdout and "Final Avg RMSE:" in r.stdout
    for side in "UV":
        lam = bio.read_dense(tmp_path / "o" / ("%s-Lambda.ddm" % side)); mu = bio.read_dense(tmp_path / "o" / ("%s-mu.ddm" % side))
        assert lam.shape[0] == 32 * 32 and np.all(np.isnan(lam))
        assert mu.shape[0] == 32 and np.all(np.isfinite(mu))


def test_cli_is_silent_when_the_kept_samples_suffice(tmp_path):
    """bpmf -d 8 -i 12 -b 2 -o: ten samples of an 8-vector, no such line, finite Lambda."""
    (tmp_path / "o").mkdir()
    r = _bpmf(["-d", "8", "-i", "12", "-b", "2", "-o", "o/"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "Lambda.ddm" not in r.stderr and "NaN" not in r.stderr and "Lambda.ddm" not in r.stdout, r.stderr
    assert np.all(np.isfinite(bio.read_dense(tmp_path / "o" / "U-Lambda.ddm")))


# ----------------------------------------------------------------------------------------------------------------------
# 3. k_predict
PN = 300                                                              # both sides have 300 columns
MEAN_M, MEAN_U = 3.6, 3.1                                             # the two sides' means differ: a twin must add its own
NS = (0, 0, 1, 2, 5)
SE_RTOL, PAVG_RTOL, PM2_RTOL, PM2_ATOL = 1e-9, 1e-12, 1e-10, 1e-12


def predict_matrix(nnz):
    """nnz distinct cells of the 300 x 300 matrix in CSC order, non-integer values: ((colptr, rowidx, vals), column per entry)"""
    key = ("T", nnz)
    if key not in _CACHE:
        rng = np.random.default_rng(7000 + nnz)
        cell = np.sort(rng.choice(PN * PN, size=nnz, replace=False))
        col, row = (cell // PN).astype(np.int64), (cell % PN).astype(np.int32)
        vals = rng.normal(3.5, 1.1, size=nnz)
        colptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=PN))]).astype(np.int64)
        for a in (colptr, row, vals, col):
            a.setflags(write=False)
        _CACHE[key] = ((colptr, row, vals), col)
    return _CACHE[key]


def transpose_matrix(T, col):
    """The same entries by column of the other side: ((colptr, rowidx, vals), order) with entry p = entry order[p] of T."""
    colptr, row, vals = T
    order = np.lexsort((col, row))
    tp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=PN))]).astype(np.int64)
    return (tp, col[order].astype(np.int32), vals[order]), order


def predict_factors(K, f32=False):
    """(V of the movies, U of the users) for each of the five calls: U stays, V moves by 0.01 N(0, 1) between calls"""
    key = ("F", K, f32)
    if key not in _CACHE:
        rng = np.random.default_rng(50 + K)
        rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
        U = rnd(0.3 * rng.standard_normal((PN, K))); V = rnd(0.3 * rng.standard_normal((PN, K)))
        out = []
        for _ in NS:
            out.append((V, U))
            V = rnd(V + 0.01 * rng.standard_normal(V.shape))
        for v, u in out:
            v.setflags(write=False); u.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def predict_reference(vals, col, row, factors, mean):
    """Per call (se, se_avg, Pavg, Pm2) in longdouble: pred = items[col] . other[row] + mean, then the reference's running mean
    as k_predict states it -- n = 0 overwrites avg and zeroes m2, otherwise avg += delta / n (n, not n + 1) and
    m2 += delta * (pred - avg)."""
    v = vals.astype(LD)
    avg = v.copy(); m2 = v.copy()
    out = []
    for (V, U), n in zip(factors, NS):
        pred = (V[col].astype(LD) * U[row].astype(LD)).sum(1) + LD(mean)
        if n == 0:
            avg = pred.copy(); m2 = np.zeros_like(pred)
        else:
            delta = pred - avg
            avg = avg + delta / LD(n)
            m2 = m2 + delta * (pred - avg)
        out.append((((v - pred) ** 2).sum(), ((v - avg) ** 2).sum(), avg.copy(), m2.copy()))
    return out


def _predict_refs(K, nnz, f32=False):
    key = ("P", K, nnz, f32)
    if key not in _CACHE:
        T, col = predict_matrix(nnz)
        _CACHE[key] = predict_reference(T[2], col, T[1], predict_factors(K, f32), MEAN_M)
    return _CACHE[key]


def _wg(monkeypatch, wg):
    if wg == 64:
        monkeypatch.setenv("BPMF_HIP_PREDICT_WG", "64")               # (read by test_create)
    else:
        monkeypatch.delenv("BPMF_HIP_PREDICT_WG", raising=False)


def _sides(eng, col_from=0, col_to=None):
    return _empty_side(eng, PN, PN, MEAN_M, col_from, col_to), _empty_side(eng, PN, PN, MEAN_U)


def _run_predict(eng, movies, users, T, factors, twin=None):
    """A fresh test matrix on the movies (and a fresh twin on the users) through the five calls: per call
    (se, se_avg, count, Pavg, Pm2) and the same of the twin."""
    t = eng.test_create(movies, *T)
    tw = None
    if twin is not None:
        tw = eng.test_create(users, *twin)
        eng.test_set_twin(t, tw)
    out, out_tw = [], []
    for (V, U), n in zip(factors, NS):
        eng.set_items(movies, V); eng.set_items(users, U)
        out.append(eng.predict(t, movies, users, n) + eng.test_get(t))
        if tw is not None:
            out_tw.append(eng.predict_finish(tw) + eng.test_get(tw))
    if tw is not None:
        eng.test_destroy(tw)
    eng.test_destroy(t)
    return out, out_tw


def _rel(a, ref):
    return float(abs(LD(a) - ref) / ref)


def _check_predict(tag, got, ref, nnz):
    """every figure, then the bars"""
    worst = [0.0, 0.0, 0.0, 0.0]
    for se, sea, cnt, pavg, pm2 in got:
        assert cnt == nnz and pavg.shape == (nnz,) and pm2.shape == (nnz,)
    if nnz == 0:
        assert all((se, sea, cnt) == (0.0, 0.0, 0) for se, sea, cnt, _, _ in got)
        return
    for (se, sea, cnt, pavg, pm2), (se_r, sea_r, pavg_r, pm2_r) in zip(got, ref):
        d2 = np.abs(pm2.astype(LD) - pm2_r)
        worst = [max(worst[0], _rel(se, se_r), _rel(sea, sea_r)), max(worst[1], float((np.abs(pavg.astype(LD) - pavg_r) / np.abs(pavg_r)).max())),
                 max(worst[2], float(d2.max())), max(worst[3], float((d2 / (PM2_ATOL + PM2_RTOL * np.abs(pm2_r))).max()))]
    print("posterior-outputs %s: se %.3e (bar %.0e)  Pavg %.3e (bar %.0e)  Pm2 abs %.3e, %.3e of its bar" % (tag, worst[0], SE_RTOL, worst[1], PAVG_RTOL, worst[2], worst[3]))
    for (se, sea, cnt, pavg, pm2), (se_r, sea_r, pavg_r, pm2_r) in zip(got, ref):
        assert _rel(se, se_r) < SE_RTOL and _rel(sea, sea_r) < SE_RTOL
        assert np.allclose(pavg, pavg_r.astype(np.float64), rtol=PAVG_RTOL, atol=0.0)
        assert np.allclose(pm2, pm2_r.astype(np.float64), rtol=PM2_RTOL, atol=PM2_ATOL)
    assert np.all(got[0][4] == 0.0) and np.all(got[1][4] == 0.0)      # n = 0 zeroes m2 (it was created as a copy of the values)


def _same_runs(a, b, sums=True):
    """two runs of the five calls: entries bit for bit, and the sums too"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert _same_bytes(x[3], y[3]) and _same_bytes(x[4], y[4])
        if sums:
            assert x[:3] == y[:3], (x[:3], y[:3])


NNZ_ALL = [0, 1, 63, 64, 65, 255, 256, 257, 4097, 65537]
NNZ_FEW = [1, 65, 257, 4097]
PREDICT_CASES = [pytest.param(32, n, id="K32-nnz%d" % n) for n in NNZ_ALL] + \
                [pytest.param(K, n, id="K%d-nnz%d" % (K, n)) for K in (8, 64, 128, 20, 100) for n in NNZ_FEW]


@pytest.mark.parametrize("K,nnz", PREDICT_CASES)
def test_predict_fp64_against_longdouble(hip_engine_factory, monkeypatch, K, nnz):
    """k_predict<K, 256>: 65 537 entries are 257 blocks, one more than the final tree has threads; 0 entries give (0, 0, 0)."""
    _wg(monkeypatch, 256)
    eng = hip_engine_factory(K)
    T, col = predict_matrix(nnz)
    movies, users = _sides(eng)
    a, _ = _run_predict(eng, movies, users, T, predict_factors(K))
    b, _ = _run_predict(eng, movies, users, T, predict_factors(K))
    eng.side_destroy(movies); eng.side_destroy(users)
    _check_predict("k_predict<%d,256> nnz=%d" % (K, nnz), a, _predict_refs(K, nnz) if nnz else None, nnz)
    _same_runs(a, b)


@pytest.mark.parametrize("nnz", [1, 63, 65, 4097])
@pytest.mark.parametrize("K", [8, 32, 128])
def test_predict_single_wave_workgroups(hip_engine_factory, monkeypatch, K, nnz):
    """BPMF_HIP_PREDICT_WG=64 (k_predict<K, 64>): 4 097 entries are 65 blocks, one more than its final tree has threads.  The
    entries equal those of the 256-thread form bit for bit; the sums (other blocks, another tree) meet the bar."""
    eng = hip_engine_factory(K)
    T, col = predict_matrix(nnz)
    movies, users = _sides(eng)
    _wg(monkeypatch, 64)
    a, _ = _run_predict(eng, movies, users, T, predict_factors(K))
    b, _ = _run_predict(eng, movies, users, T, predict_factors(K))
    _wg(monkeypatch, 256)
    c, _ = _run_predict(eng, movies, users, T, predict_factors(K))
    eng.side_destroy(movies); eng.side_destroy(users)
    _check_predict("k_predict<%d,64> nnz=%d" % (K, nnz), a, _predict_refs(K, nnz), nnz)
    _same_runs(a, b)
    _same_runs(a, c, sums=False)


@pytest.mark.parametrize("nnz", [1, 257, 4097])
def test_predict_fp32_with_and_without_a_twin(hip_engine_factory, monkeypatch, nnz):
    """fp32 factors at K = 128 (rounded once; the products of two fp32 numbers are exact in fp64, so the fp64 bars hold):
    k_predict_f32<128> without a twin, k_predict<128, 256, float> with one, the same entries bit for bit; the twin's copy
    against the reference with the users' mean, in the transposed order."""
    K = 128
    _wg(monkeypatch, 256)
    eng = hip_engine_factory(K, "f32")
    T, col = predict_matrix(nnz)
    Tt, order = transpose_matrix(T, col)
    F = predict_factors(K, True)
    movies, users = _sides(eng)
    a, _ = _run_predict(eng, movies, users, T, F)
    b, _ = _run_predict(eng, movies, users, T, F)
    c, ctw = _run_predict(eng, movies, users, T, F, twin=Tt)
    d, dtw = _run_predict(eng, movies, users, T, F, twin=Tt)
    eng.side_destroy(movies); eng.side_destroy(users)
    ref = _predict_refs(K, nnz, True)
    _check_predict("k_predict_f32<128> nnz=%d" % nnz, a, ref, nnz)
    _check_predict("k_predict<128,256,float> nnz=%d" % nnz, c, ref, nnz)
    _check_predict("k_predict<128,256,float> twin nnz=%d" % nnz, ctw, predict_reference(T[2][order], col[order], T[1][order], F, MEAN_U), nnz)
    _same_runs(a, b); _same_runs(c, d); _same_runs(ctw, dtw)
    _same_runs(a, c, sums=False)


@pytest.mark.parametrize("wg", [256, 64])
def test_predict_twin_equals_the_other_side_evaluated_alone(hip_engine_factory, monkeypatch, wg):
    """K = 32: users.predict(movies) as a twin of movies.predict(users) (one kernel writes both copies) against a test matrix
    created on the users and evaluated by itself -- entries bit for bit (the same products in the same order, the users' mean),
    sums to the bar -- and against the longdouble reference."""
    K, nnz = 32, 4097
    _wg(monkeypatch, wg)
    eng = hip_engine_factory(K)
    T, col = predict_matrix(nnz)
    Tt, order = transpose_matrix(T, col)
    F = predict_factors(K)
    movies, users = _sides(eng)
    a, atw = _run_predict(eng, movies, users, T, F, twin=Tt)
    b, btw = _run_predict(eng, movies, users, T, F, twin=Tt)
    solo, _ = _run_predict(eng, users, movies, Tt, [(u, v) for v, u in F])
    plain, _ = _run_predict(eng, movies, users, T, F)
    eng.side_destroy(movies); eng.side_destroy(users)
    ref_tw = predict_reference(T[2][order], col[order], T[1][order], F, MEAN_U)
    _check_predict("k_predict<32,%d> with a twin nnz=%d" % (wg, nnz), a, _predict_refs(K, nnz), nnz)
    _check_predict("k_predict<32,%d> the twin nnz=%d" % (wg, nnz), atw, ref_tw, nnz)
    _check_predict("k_predict<32,%d> users alone nnz=%d" % (wg, nnz), solo, ref_tw, nnz)
    _same_runs(a, b); _same_runs(atw, btw)
    _same_runs(atw, solo, sums=False)
    _same_runs(a, plain)                                              # the owner's copy does not notice the twin
    for x, y in zip(atw, solo):
        assert abs(x[0] - y[0]) < SE_RTOL * y[0] and abs(x[1] - y[1]) < SE_RTOL * y[1] and x[2] == y[2]


@pytest.mark.parametrize("K", [32, 20])
def test_predict_on_a_slice(hip_engine_factory, monkeypatch, K):
    """The movies created as the columns [40, 260) of 300 with the test entries of those columns only: sums to the bar, entries
    equal the corresponding ones of the whole side's run bit for bit."""
    lo, hi, nnz = 40, 260, 4097
    _wg(monkeypatch, 256)
    eng = hip_engine_factory(K)
    T, col = predict_matrix(nnz)
    F = predict_factors(K)
    mine = (col >= lo) & (col < hi)
    Ts = (T[0][lo:hi + 1] - T[0][lo], T[1][mine], T[2][mine])
    assert 0 < Ts[0][-1] == mine.sum() < nnz
    movies, users = _sides(eng)
    whole, _ = _run_predict(eng, movies, users, T, F)
    eng.side_destroy(movies)
    part_side = _empty_side(eng, PN, PN, MEAN_M, lo, hi)
    a, _ = _run_predict(eng, part_side, users, Ts, F)
    b, _ = _run_predict(eng, part_side, users, Ts, F)
    eng.side_destroy(part_side); eng.side_destroy(users)
    ref = predict_reference(Ts[2], col[mine], Ts[1], F, MEAN_M)
    _check_predict("k_predict<%d,256> slice nnz=%d" % (K, int(mine.sum())), a, ref, int(mine.sum()))
    _same_runs(a, b)
    for x, y in zip(a, whole):
        assert _same_bytes(x[3], y[3][mine]) and _same_bytes(x[4], y[4][mine])
