"""PSIS-LOO (include/bpmf_hip.h): the rule restated in numpy, once per floating-point type.

psis(L, dtype) runs the rule on the traces L [n, S] of log densities in `dtype`: np.float64 restates the device's order of operations
(positions of the sorted order lane-strided over 64 lanes, then the butterfly; the terms of a k_j in increasing i) with numpy's exp,
log, log1p and expm1 in place of the device's; np.longdouble is the same rule 11 bits wider, which the tests take as the truth.  The
difference of the two is the rounding level of the rule, and the bar the device is held to is a multiple of it.

Positions: a_0 <= .. <= a_{S-1} are the l_s in increasing order, so position i holds the (i + 1)-th largest importance ratio, rho_i =
a_0 - a_i.  The issue's r_(S-M-1+j) is rho_{M-j}."""
import math

import numpy as np

TINY_K = 1e-30
MAX_SAMPLES = 4096


def tail_length(S):
    """M = min(floor(S / 5), ceil(3 sqrt S)), in integers."""
    r = math.isqrt(9 * S)
    if r * r < 9 * S:
        r += 1
    return min(S // 5, r)


def wave_sum(A):
    """Sum over the last axis in the device's order: lane l adds positions l, l + 64, .. in increasing order from 0, then the 64 lanes
    add pairwise (l, l + 32), (l, l + 16), .. (l, l + 1)."""
    n = A.shape[-1]
    pad = (-n) % 64
    if pad:
        A = np.concatenate([A, np.zeros(A.shape[:-1] + (pad,), A.dtype)], axis=-1)
    A = A.reshape(A.shape[:-1] + (-1, 64))
    v = np.zeros(A.shape[:-2] + (64,), A.dtype)
    for r in range(A.shape[-2]):
        v = v + A[..., r, :]
    w = 32
    while w >= 1:
        v = v[..., :w] + v[..., w:2 * w]
        w //= 2
    return v[..., 0]


def gpd_fit(x, dtype=np.float64):
    """(k, sigma, khat, ok) of the generalised Pareto fit of Zhang & Stephens 2009 to the excesses x [n, M], increasing along the last
    axis: k is the fitted shape, khat = (k M + 5) / (M + 10) the one with the weak prior; ok is False where the rule does not fit
    (x_M = x_1, x* = 0, or a value that is not finite)."""
    x = np.asarray(x, dtype)
    n, M = x.shape
    dM = dtype(M)
    m = 30 + math.isqrt(M)
    with np.errstate(all="ignore"):
        xM, x1, xs = x[:, M - 1], x[:, 0], x[:, int(0.25 * M + 0.5) - 1]
        ok = ~(xM == x1) & ~(xs == 0)
        j = np.arange(1, m + 1).astype(dtype)
        theta = (dtype(1) / xM)[:, None] + (dtype(1) - np.sqrt(dtype(m) / (j - dtype(0.5))))[None, :] / (dtype(3) * xs)[:, None]
        acc = np.zeros((n, m), dtype)
        for i in range(M):
            acc = acc + np.log1p(-theta * x[:, i:i + 1])
        kj = acc / dM
        L = dM * ((np.log(-theta / kj) - kj) - dtype(1))
        ok &= np.isfinite(L).all(axis=1)
        Lmax = np.where(np.isfinite(L), L, -np.inf).max(axis=1)
        e = np.exp(L - Lmax[:, None])
        w = e / wave_sum(e)[:, None]                                      # (lanes m .. 63 add zeros; M > 1156 needs more than a wave)
        th = wave_sum(w * theta)
        k = wave_sum(np.log1p(-th[:, None] * x)) / dM
        sigma = -k / th
        khat = (k * dM + dtype(5)) / (dM + dtype(10))
        ok &= np.isfinite(th) & np.isfinite(k) & np.isfinite(sigma) & np.isfinite(khat)
    return k, sigma, khat, ok


def logsumexp_sorted(V):
    with np.errstate(all="ignore"):
        mx = V.max(axis=1)
        return mx + np.log(wave_sum(np.exp(V - mx[:, None])))


def psis(L, dtype=np.float64):
    """dict(elpd_loo, khat, lpd), [n] each in `dtype`, of the traces L [n, S]; a trace holding a value that is not finite gives NaN."""
    L = np.atleast_2d(np.asarray(L))                                     # (longdouble traces keep their bits in the longdouble form)
    L = L.astype(np.longdouble if dtype is np.longdouble and L.dtype == np.longdouble else np.float64)
    n, S = L.shape
    assert 1 <= S <= MAX_SAMPLES
    bad = ~np.isfinite(L).all(axis=1)
    a = np.sort(np.where(bad[:, None], 0.0, L), axis=1).astype(dtype)
    M = tail_length(S)
    rho = a[:, :1] - a
    lw = rho.copy()
    khat = np.full(n, np.inf, dtype)
    if M >= 5:
        with np.errstate(all="ignore"):
            ec = np.exp(rho[:, M])
            x = np.exp(rho[:, M - 1::-1][:, :M]) - ec[:, None]          # x_j at column j - 1: position M - j
            _, sigma, kh, ok = gpd_fit(x, dtype)
            j = np.arange(1, M + 1).astype(dtype)
            t = -np.log1p(-((j - dtype(0.5)) / dtype(M)))
            q = np.where((np.abs(kh) < TINY_K)[:, None], sigma[:, None] * t[None, :],
                         sigma[:, None] * np.expm1(kh[:, None] * t[None, :]) / kh[:, None])
            sm = np.minimum(np.log(q + ec[:, None]), dtype(0))             # column j - 1
            lw[:, :M] = np.where(ok[:, None], sm[:, ::-1], rho[:, :M])
            khat = np.where(ok, kh, dtype(np.inf))
    elpd = logsumexp_sorted(lw + a) - logsumexp_sorted(lw)
    lpd = logsumexp_sorted(a) - np.log(dtype(S))
    nan = dtype(np.nan)
    return dict(elpd_loo=np.where(bad, nan, elpd), khat=np.where(bad, nan, khat), lpd=np.where(bad, nan, lpd))


def rule_error(L, Ltrue=None):
    """(fp64 result, longdouble result, dict of the largest absolute differences over the traces) of psis on L; Ltrue: the same traces
    in longdouble where they were computed there (else L itself).  An infinite khat must agree exactly and counts as no difference."""
    f, g = psis(L, np.float64), psis(L if Ltrue is None else Ltrue, np.longdouble)
    err = {}
    for key in ("elpd_loo", "khat", "lpd"):
        x, y = f[key].astype(np.longdouble), g[key]
        fin = np.isfinite(y)
        assert np.array_equal(fin, np.isfinite(x)) and np.array_equal(x[~fin & ~np.isnan(y)], y[~fin & ~np.isnan(y)]), key
        err[key] = float(np.abs(x[fin] - y[fin]).max()) if fin.any() else 0.0
    return f, g, err


BAR_FACTOR = 16                                  # what the project holds its Cholesky comparisons to


def held_to_reference(got, L, Ltrue=None, tag=""):
    """The device's dict(elpd_loo, khat, lpd) of the traces L against the longdouble form: per figure at most BAR_FACTOR x the largest
    error of the fp64 form over these traces; khat infinite or NaN exactly where the reference's is.  Returns the shares of the bars used."""
    f, g, err = rule_error(L, Ltrue)
    used = {}
    for key in ("elpd_loo", "khat", "lpd"):
        x, y = np.asarray(got[key], np.float64), g[key]
        assert x.shape == y.shape, (tag, key)
        fin = np.isfinite(y)
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(np.isposinf(x), np.isposinf(y)) and not np.isneginf(x).any(), (tag, key)
        e = float(np.abs(x[fin].astype(np.longdouble) - y[fin]).max()) if fin.any() else 0.0
        bar = BAR_FACTOR * err[key]
        assert e <= bar, (tag, key, e, bar)
        used[key] = e / bar if bar > 0 else 0.0
    return used, g, err


def loo_summary_ref(elpd, khat, lpd, S):
    elpd = np.asarray(elpd, np.float64); khat = np.asarray(khat, np.float64); lpd = np.asarray(lpd, np.float64)
    n = len(elpd)
    s = float(elpd.sum())
    se = math.sqrt(n * elpd.var(ddof=1)) if n > 1 else 0.0
    thr = min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else float("-inf")
    return dict(n=n, elpd_loo=s, se=se, p_loo=float((lpd - elpd).sum()), looic=-2.0 * s, threshold=thr)
