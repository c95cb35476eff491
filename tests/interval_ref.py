"""The posterior predictive mixture of a cell, its probability integral transform and its quantiles (DESIGN.md section 31;
bpmf_amd/csrc/kernels_interval.h), restated for the tests: in numpy longdouble (the reference) and, as `rule_f64`, the device's own
root-finding rule in plain fp64 Python (what the rule can be held to without a GPU).

For a trace d_0 .. d_{S-1} (d_s = u_s . v_s, without the mean rating) and r_s = sqrt(alpha_s w):
    F(x) = (1/S) sum_s Phi((x - d_s) r_s)      f(x) = (1/S) sum_s r_s phi((x - d_s) r_s)
    pit = F(y - mean)                          q(tau) = mean + F^-1(tau)
"""
import math

import numpy as np

from tests import score_ref as sr

LD = np.longdouble
EPS = 2.0 ** -53


# ---- Phi in longdouble, to an absolute error of a few 1e-20 ---------------------------------------------------------------------------------

def Phi_ld(t):
    """Phi(t), longdouble.  |t| < 3: 1/2 + phi(t) (t + t^3 / 3 + t^5 / 15 + ..), 90 terms of one sign (the last below 1e-30 of the
    first); from 3 on the continued fraction of the upper tail (score_ref._upper_tail_terms, 64 terms: below 1e-20 relative).  The
    absolute error is a few longdouble ulp of 1/2 everywhere, which is what a residual F(q) - tau needs."""
    t = np.asarray(t, LD)
    out = np.empty(t.shape, LD)
    a = np.abs(t)
    far = a >= 3
    if far.any():
        with np.errstate(under="ignore"):
            tail = np.exp(sr._upper_tail_terms(a[far], 64))
        out[far] = np.where(t[far] > 0, LD(1) - tail, tail)
    near = ~far
    if near.any():
        x = t[near]
        term, tot = x.copy(), x.copy()
        for k in range(1, 90):
            term = term * x * x / LD(2 * k + 1)
            tot = tot + term
        out[near] = LD(0.5) + np.exp(-LD(0.5) * x * x) / np.sqrt(LD(2) * sr.PI_LD) * tot
    return out


def rates(alpha, w, S):
    """r [n, S] = sqrt(alpha_s w_i), longdouble; alpha one number or [S], w None or [n]"""
    al = np.broadcast_to(np.asarray(alpha, LD).reshape(-1), (S,)) if np.ndim(alpha) else np.full(S, LD(alpha))
    w = np.ones(1, LD) if w is None else np.asarray(w, LD)
    return np.sqrt(al[None, :] * w[:, None])


def mixture(x, D, r):
    """(F, f) [n], longdouble, of the mixtures around the traces D [n, S] with the rates r [n or 1, S], at x [n]"""
    D = np.asarray(D, LD); x = np.asarray(x, LD)
    t = (x[:, None] - D) * r
    with np.errstate(under="ignore"):
        F = Phi_ld(t).mean(axis=1)
        f = (r * np.exp(-LD(0.5) * t * t)).mean(axis=1) / np.sqrt(LD(2) * sr.PI_LD)
    return F, f


def pit(D, alpha, y, w=None, mean=0.0):
    D = np.asarray(D, LD)
    return mixture(np.asarray(y, LD) - LD(mean), D, rates(alpha, w, D.shape[1]))[0]


def quantile(D, alpha, tau, w=None, mean=0.0):
    """F^-1(tau) + mean [n], longdouble, by bisection down to longdouble resolution"""
    D = np.asarray(D, LD)
    r = rates(alpha, w, D.shape[1])
    reach = LD(8) / r.min(axis=1)                                # |Phi^-1(tau)| < 3.1 for tau in [0.001, 0.999]
    lo, hi = D.min(axis=1) - reach, D.max(axis=1) + reach
    for _ in range(90):
        mid = lo + (hi - lo) / 2
        below = mixture(mid, D, r)[0] < LD(tau)
        lo = np.where(below, mid, lo); hi = np.where(below, hi, mid)
    return lo + (hi - lo) / 2 + LD(mean)


# ---- what the device is held to ------------------------------------------------------------------------------------------------------------

def ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)))


def residual_bound(S, f, ulps):
    """(S / 64 + 32) 2^-53 + 4 f ulps: the lane sums, the butterfly and an erfc of up to 16 ulp; then the rounding of the argument"""
    return (S / 64.0 + 32.0) * EPS + 4.0 * np.asarray(f, np.float64) * ulps


def quantile_residual(D, alpha, tau, q, w=None, mean=0.0):
    """(|F_ld(q) - tau|, its bound) [n] for the device's roots q [n] (with the mean added)"""
    D = np.asarray(D, LD)
    F, f = mixture(np.asarray(q, LD) - LD(mean), D, rates(alpha, w, D.shape[1]))
    return np.abs(F - LD(tau)).astype(np.float64), residual_bound(D.shape[1], f, ulp(q))


def pit_residual(D, alpha, y, got, w=None, mean=0.0):
    """(|F_ld(y) - pit|, its bound) [n] for the device's pits"""
    D = np.asarray(D, LD)
    F, f = mixture(np.asarray(y, LD) - LD(mean), D, rates(alpha, w, D.shape[1]))
    pmax = np.abs(np.asarray(D, np.float64) + mean).max(axis=1)
    return np.abs(F - np.asarray(got, LD)).astype(np.float64), residual_bound(D.shape[1], f, ulp(y) + ulp(pmax))


# ---- the device's rule in fp64 -------------------------------------------------------------------------------------------------------------

def normal_quantile(p):
    """Phi^-1(p) as the host computes it for the bracket (capi_internal.h)"""
    upper = p > 0.5
    q = 1.0 - p if upper else p
    x = 0.0
    for _ in range(200):
        f = 0.5 * math.erfc(-x * 0.70710678118654752440) - q
        d = math.exp(-0.5 * x * x) * 0.3989422804014326779
        step = max(-1.0, min(1.0, f / d))
        x -= step
        if abs(step) <= 1e-16 * (1.0 + abs(x)):
            break
    return -x if upper else x


def rule_f64(d, r, taus, cap=128):
    """(roots, evaluations) of one trace d [S] with the rates r [S] by the rule of k_trace_quantiles, fp64 (sums in numpy's order, not
    the lanes'): the bracket of the component quantiles with the previous root as its lower end, the moment-matched start, Newton
    steps kept inside the bracket, bisection when a step leaves it, f is not > 0 or the bracket has not halved in two steps; the stop
    at h = 0, a step of at most 2 ulp, a bracket without a double inside, or `cap` evaluations."""
    from scipy.special import erfc
    d = np.asarray(d, np.float64); r = np.asarray(r, np.float64)
    S = len(d)
    m = d.sum() / S
    sd = math.sqrt(((d - m) ** 2 + 1.0 / (r * r)).sum() / S)
    roots, evals, prev = [], [], -math.inf
    for tau in taus:
        z = normal_quantile(tau)
        upper = tau > 0.5
        tail, sgn = (1.0 - tau, -1.0) if upper else (tau, 1.0)
        c = d + z / r
        lo, hi = max(c.min(), prev), c.max()
        hi = max(hi, lo)
        x = z * sd + m
        x = lo if not x >= lo else hi if not x <= hi else x
        w1 = w2 = math.inf
        root, n = x, 0
        if hi > lo:
            for _ in range(cap):
                n += 1
                t = (x - d) * r
                with np.errstate(under="ignore"):
                    P = (0.5 * erfc(-sgn * t * 0.70710678118654752440)).sum() / S
                    f = (r * np.exp(-0.5 * t * t)).sum() * 0.39894228040143267794 / S
                h = tail - P if upper else P - tail
                if h == 0.0:
                    root = x
                    break
                if h < 0.0:
                    lo = x
                else:
                    hi = x
                width = hi - lo
                mid = lo + 0.5 * width
                root = mid
                if not (lo < mid < hi):
                    break
                xn = x - h / f if f > 0.0 else math.nan
                if not (f > 0.0 and lo < xn < hi and width <= 0.5 * w2):
                    xn = mid
                w2, w1 = w1, width
                if not abs(xn - x) > 2.0 ** -52 * abs(x):
                    root = xn
                    break
                x = xn
        prev = root
        roots.append(root); evals.append(n)
    return np.array(roots), evals


# ---- crafted traces ------------------------------------------------------------------------------------------------------------------------

TAUS = (0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 0.999)


def families(rng, n, S):
    """name -> dict(D [n, S], alpha (a number or [S]), w (None or [n])): the trace families of the root finder's tests"""
    g = lambda: rng.standard_normal((n, S))
    modes = np.where(np.arange(S) % 2 == 0, -25.0, 25.0)[None, :] + 0.0 * g()      # two equal modes 50 sigma apart (S = 1: one)
    return dict(unimodal=dict(D=0.3 + 0.7 * g(), alpha=2.0, w=None),
                bimodal=dict(D=modes, alpha=1.0, w=None),
                equal=dict(D=np.repeat(rng.standard_normal((n, 1)), S, axis=1), alpha=1.5, w=None),
                offset=dict(D=1e6 + g(), alpha=1.0, w=None),
                alphas=dict(D=g(), alpha=10.0 ** rng.uniform(-1.5, 1.5, S), w=None),
                weights=dict(D=g(), alpha=1.0, w=10.0 ** rng.uniform(-3.0, 3.0, n)))
