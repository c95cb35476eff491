"""The estimator of the multi-chain convergence diagnostics (bpmf_amd/csrc/kernels_diag_mc.h), restated for the
tests: in numpy longdouble (the reference; the normal scores from mpmath at 40 digits) and in fp64 with the device's order of additions
and scipy's fp64 erfcinv in the device's formula (what fp64 can be held to).

A trace is C * S values, chain-major: chain c is x[c S : (c + 1) S], chronological inside; 1 <= C <= 64, S >= 8, C S <= 4096.
    n = S // 2; half-chain 2c = x_c[0:n], half-chain 2c + 1 = x_c[S - n:S]  (an odd S drops the middle draw); M = 2C, N = M n
    est(y), y [M, n]:
        per half-chain: m_h = mean (of a half whose values are all equal: that value), d = y - m_h
        c(t) = (1 / N) sum_h sum_{i=0}^{n-1-t} d_{h,i} d_{h,i+t};  W = c(0) n / (n - 1);  Bv = sum (m_h - mean m)^2 / (M - 1)
        var+ = c(0) + Bv;  rhat = sqrt(var+ / W);  rho_t = 1 - (W - c(t)) / var+
        P_0 = 1 + rho_1;  for k = 1, 2, .. while 2k + 1 <= n - 3:  p = rho_2k + rho_2k+1;  stop unless p > 0;  P_k = min(p, P_k-1)
        tau = max(-1 + 2 sum_k P_k, 1 / log10 N);  ess = N / tau;  W not > 0: both NaN
      -- with C = 1 this is the estimator of tests/diag_ref.py
    z(y): r = average rank of y among the N (1-based), a = min(r, N + 1 - r), z = -+ sqrt 2 erfcinv((2a - 0.75) / (N + 0.25)),
        negative for r < (N + 1) / 2, 0 at r = (N + 1) / 2
    rhat = max(est(z(x)).rhat, est(z(|x - med|)).rhat), med = mean of the two middle order statistics; NaN if either is
    ess_bulk = est(z(x)).ess
    ess_tail = min over p in {0.05, 0.95} of est(1[x <= x_(floor((N - 1) p) + 1)]).ess (1-based order statistic); NaN if either is
    a value that is not finite anywhere among the C S: NaN for all three
"""
import numpy as np

from tests import diag_ref as dr

ld = np.longdouble
MAX_CHAINS, MIN_SAMPLES, MAX_VALUES = 64, 8, 4096
NAN3 = (float("nan"),) * 3


def half_chains(x, C, S):
    """[M, n]: the half-chains of the chain-major trace x, in the order 2c, 2c + 1"""
    x = np.asarray(x).reshape(C, S)
    n = S // 2
    return np.stack([x[:, :n], x[:, S - n:]], axis=1).reshape(2 * C, n)


def _group_sum(v, G):
    """the device's sum of a half-chain: lane j of G adds i = j, j + G, .. ascending, then a butterfly over the G lanes"""
    pad = (-len(v)) % G
    part = _rows_sum(np.concatenate([v, np.zeros(pad)]).reshape(-1, G))
    w = G // 2
    while w >= 1:
        part = part[:w] + part[w:2 * w]
        w //= 2
    return part[0]


def _rows_sum(rows):
    """sequential sum of the rows of a [r, lanes] array, row 0 first"""
    acc = np.zeros(rows.shape[1])
    for r in rows:
        acc = acc + r
    return acc


def _lane_sum_fast(v):
    """diag_ref._lane_sum, its loop over the rows kept but nothing else in Python"""
    pad = (-len(v)) % 64
    part = _rows_sum(np.concatenate([v, np.zeros(pad)]).reshape(-1, 64))
    w = 32
    while w >= 1:
        part = part[:w] + part[w:2 * w]
        w //= 2
    return part[0]


def est(Y, f64=False):
    """(rhat, ess) of the half-chains Y [M, n]: in longdouble, or in fp64 in the device's order of additions"""
    real = np.float64 if f64 else ld
    Y = np.asarray(Y, real)
    M, n = Y.shape
    N = M * n
    nan = (float("nan"), float("nan"))
    dn, dN, dM = real(n), real(N), real(M)
    with np.errstate(all="ignore"):
        if f64:
            G = 4
            while G < n and G < 64:
                G *= 2
            m = np.array([h[0] if (h == h[0]).all() else np.float64(_group_sum(h, G)) / dn for h in Y])
            mbar = np.float64(_lane_sum_fast(m)) / dM
            Bv = np.float64(_lane_sum_fast((m - mbar) * (m - mbar))) / (dM - real(1))
        else:
            m = np.array([h[0] if (h == h[0]).all() else h.sum() / dn for h in Y], ld)
            mbar = m.sum() / dM
            Bv = ((m - mbar) ** 2).sum() / (dM - real(1))
        D = Y - m[:, None]

        def lag(t):
            if f64:
                prod = np.zeros((M, n))
                prod[:, :n - t] = D[:, :n - t] * D[:, t:]
                return np.float64(_lane_sum_fast(prod.reshape(-1))) / dN
            return (D[:, :n - t] * D[:, t:]).sum() / dN
        c0 = lag(0)
        W = c0 * dn / (dn - real(1))
        varp = c0 + Bv
        if not W > 0:
            return nan
        rhat = np.sqrt(varp / W)

        def rho(t):
            return real(1) - (W - lag(t)) / varp
        P = real(1) + rho(1)
        acc = P
        k = 1
        while 2 * k + 1 <= n - 3:
            p = rho(2 * k) + rho(2 * k + 1)
            if not p > 0:
                break
            P = min(p, P)
            acc = acc + P
            k += 1
        tau = real(-1) + real(2) * acc
        floor = real(1) / np.log10(dN)
        tau = floor if tau < floor else tau
        return float(rhat), float(dN / tau)


def ranks2(y):
    """twice the average rank (1-based) of every value of y among all of them: values below + values not above + 1"""
    s = np.sort(y, axis=None)
    return np.searchsorted(s, y, "left") + np.searchsorted(s, y, "right") + 1


_Z_LD = {}


def _z_ld(a2, N):
    """sqrt 2 erfcinv((a2 - 0.75) / (N + 0.25)) as a longdouble, from mpmath at 40 digits"""
    key = (int(a2), int(N))
    if key not in _Z_LD:
        import mpmath
        with mpmath.workdps(40):
            arg = mpmath.mpf(4 * key[0] - 3) / mpmath.mpf(4 * key[1] + 1)
            z = mpmath.sqrt(2) * mpmath.erfinv(1 - arg)
            _Z_LD[key] = ld(mpmath.nstr(z, 30))
    return _Z_LD[key]


def zscores(y, f64=False):
    """the normal scores of the ranks of y (any shape), in y's shape"""
    y = np.asarray(y)
    N = y.size
    r2 = ranks2(y)
    a2 = np.minimum(r2, 2 * N + 2 - r2)
    if f64:
        from scipy.special import erfcinv
        z = np.float64(1.41421356237309504880) * erfcinv((a2.astype(np.float64) - 0.75) / (np.float64(N) + 0.25))
    else:
        z = np.array([_z_ld(a, N) for a in a2.reshape(-1)], ld).reshape(a2.shape)
    return np.where(r2 < N + 1, -z, np.where(r2 > N + 1, z, 0 * z))


def tail_cuts(kept):
    """the order statistics x_(floor((N - 1) p) + 1), p = 0.05 and 0.95, of the kept values"""
    s = np.sort(np.asarray(kept), axis=None)
    N = len(s)
    return s[(N - 1) * 5 // 100], s[(N - 1) * 95 // 100]


def parts(x, C, S, f64=False):
    """dict of the four est results of one trace: bulk, folded, tail_lo, tail_hi -> (rhat, ess); None for a value that is not finite"""
    real = np.float64 if f64 else ld
    x = np.asarray(x, np.float64).reshape(-1)       # the median and the folded keys in fp64 in both forms: ranks are not continuous in them
    assert len(x) == C * S and 1 <= C <= MAX_CHAINS and S >= MIN_SAMPLES and C * S <= MAX_VALUES
    if not np.isfinite(x).all():
        return None
    H = half_chains(x, C, S)
    N = H.size
    s = np.sort(H, axis=None)
    with np.errstate(all="ignore"):
        med = np.float64(0.5) * (s[N // 2 - 1] + s[N // 2])
        lo, hi = tail_cuts(H)
        return dict(bulk=est(zscores(H, f64), f64), folded=est(zscores(np.abs(H - med), f64), f64),
                    tail_lo=est((H <= lo).astype(real), f64), tail_hi=est((H <= hi).astype(real), f64))


def diag_mc(x, C, S, f64=False):
    """(rhat, ess_bulk, ess_tail) of one chain-major trace"""
    p = parts(x, C, S, f64)
    if p is None:
        return NAN3
    rb, rf = p["bulk"][0], p["folded"][0]
    tl, th = p["tail_lo"][1], p["tail_hi"][1]
    rhat = float("nan") if (np.isnan(rb) or np.isnan(rf)) else max(rb, rf)
    tail = float("nan") if (np.isnan(tl) or np.isnan(th)) else min(tl, th)
    return rhat, p["bulk"][1], tail


def diag_mc_f64(x, C, S):
    return diag_mc(x, C, S, True)


def diag_mc_many(X, C, S, f64=False):
    """(rhat [n], ess_bulk [n], ess_tail [n]) of the rows of X [n, C S]"""
    out = np.array([diag_mc(x, C, S, f64) for x in X], np.float64).reshape(-1, 3)
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()


def chains_ar1(rng, m, C, S, rho):
    """m traces [m, C S] of C independent stationary AR(1) chains of S draws"""
    return dr.ar1(rng, m * C, S, rho).reshape(m, C * S)
