"""The estimator of the convergence diagnostics (bpmf_amd/csrc/kernels_diag.h), restated for the tests: in numpy
longdouble (the reference) and in fp64 with the device's order of additions (what fp64 can be held to).

For one trace x_0 .. x_{S-1} in chronological order, S >= 8 -- the split-chain estimator of Vehtari et al. (2021) without rank
normalisation:
    n = S // 2;  A = x[0:n], B = x[S-n:S]  (an odd S drops the middle sample)
    per half h: m_h = mean (of a half whose values are all equal: that value), d = x - m_h,
                c_h(t) = (1/n) sum_{i=0}^{n-1-t} d_i d_{i+t};  c(t) = (c_A(t) + c_B(t)) / 2
    W = c(0) n / (n - 1);  Bv = (m_A - m_B)^2 / 2;  var+ = c(0) + Bv;  rhat = sqrt(var+ / W)
    rho_0 = 1, rho_t = 1 - (W - c(t)) / var+
    P_0 = rho_0 + rho_1;  for k = 1, 2, .. while 2k + 1 <= n - 3:  p = rho_2k + rho_2k+1;  stop unless p > 0;  P_k = min(p, P_k-1)
    tau = max(-1 + 2 sum_k P_k, 1 / log10(2n));  ess = 2n / tau
W not > 0 (a constant trace, a value that is not finite): rhat = ess = NaN.
"""
import numpy as np

ld = np.longdouble
MIN_SAMPLES, MAX_SAMPLES = 8, 4096


def _estimate(n, mA, mB, lag, real):
    """(rhat, ess) from the means of the halves and lag(t) -> c(t), every quantity of type `real`"""
    nan = (float("nan"), float("nan"))
    dn = real(n)
    with np.errstate(all="ignore"):
        c0 = lag(0)
        W = c0 * dn / (dn - real(1))
        dm = mA - mB
        varp = c0 + real(0.5) * (dm * dm)
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
        floor = real(1) / np.log10(real(2) * dn)
        tau = floor if tau < floor else tau
        return float(rhat), float(real(2) * dn / tau)


def diag(x):
    """(rhat, ess) of one trace in longdouble"""
    x = np.asarray(x, ld)
    S = len(x)
    assert S >= MIN_SAMPLES
    n = S // 2
    halves = (x[:n], x[S - n:])
    with np.errstate(all="ignore"):
        m = [h[0] if (h == h[0]).all() else h.sum() / ld(n) for h in halves]
        dA, dB = (h - mh for h, mh in zip(halves, m))

        def lag(t):
            return ld(0.5) * (np.dot(dA[:n - t], dA[t:]) / ld(n) + np.dot(dB[:n - t], dB[t:]) / ld(n))
        return _estimate(n, m[0], m[1], lag, ld)


def _lane_sum(v):
    """the device's sum of the values v_0, v_1, ..: lane l adds i = l, l + 64, .. ascending, then a butterfly over the 64 lanes"""
    pad = (-len(v)) % 64
    lanes = np.concatenate([v, np.zeros(pad)]).reshape(-1, 64)
    part = np.zeros(64)
    for row in lanes:                                # ascending in i; adding the pad zeros changes no bit
        part = part + row
    w = 32
    while w >= 1:
        part = part[:w] + part[w:2 * w]
        w //= 2
    return part[0]


def diag_f64(x):
    """(rhat, ess) of one trace in fp64, in the device's order of additions (separate multiply and add where the device fuses them)"""
    x = np.asarray(x, np.float64)
    S = len(x)
    assert S >= MIN_SAMPLES
    n = S // 2
    halves = (x[:n], x[S - n:])
    with np.errstate(all="ignore"):
        m = [h[0] if (h == h[0]).all() else np.float64(_lane_sum(h)) / np.float64(n) for h in halves]
        dA, dB = (h - mh for h, mh in zip(halves, m))

        def lag(t):
            return np.float64(0.5) * (_lane_sum(dA[:n - t] * dA[t:]) / np.float64(n) + _lane_sum(dB[:n - t] * dB[t:]) / np.float64(n))
        return _estimate(n, m[0], m[1], lag, np.float64)


def diag_many(X, fn=diag):
    """(rhat [n], ess [n]) of the rows of X"""
    out = np.array([fn(x) for x in X], np.float64).reshape(-1, 2)
    return out[:, 0].copy(), out[:, 1].copy()


def ar1(rng, n, S, rho, scale=1.0):
    """n stationary AR(1) traces of S samples with lag-one correlation rho and unit marginal variance, times scale"""
    e = rng.standard_normal((n, S))
    x = np.empty((n, S))
    x[:, 0] = e[:, 0]
    s = np.sqrt(1.0 - rho * rho)
    for t in range(1, S):
        x[:, t] = rho * x[:, t - 1] + s * e[:, t]
    return scale * x


def relative_error(got, want):
    """max |got - want| / |want| over the entries; NaN must meet NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN in different places"
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))) if ok.any() else 0.0
