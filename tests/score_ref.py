"""The log pointwise predictive density and its WAIC correction (bpmf_amd/csrc/kernels_score.h), restated for the
tests: in numpy longdouble (the reference) and in plain fp64 numpy (what fp64 can be held to), and the planted experiment.

For a cell i = (row, col) with the value y_i, over the S kept samples, p_s = mean + u_s(row) . v_s(col) and l_s = log p(y_i | sample s):
    lpd_i = log((1/S) sum_s exp l_s)      pw_i = sum_s (l_s - lbar)^2 / (S - 1)  [0 for S = 1]      elpd_i = lpd_i - pw_i
    gaussian              l_s = (1/2) log(alpha_s w_i / 2 pi) - (1/2) alpha_s w_i (y_i - p_s)^2
    gaussian, flag +-1    l_s = log Phi(flag sqrt(alpha_s) (p_s - y_i))
    student               l_s = lgamma((nu+1)/2) - lgamma(nu/2) + (1/2) log(alpha_s / (nu pi)) - ((nu+1)/2) log1p(alpha_s (y_i - p_s)^2 / nu)
    probit                l_s = log Phi(p_s) for y_i > 0, log Phi(-p_s) otherwise
"""
import math

import numpy as np

LD = np.longdouble
PI_LD = LD(4) * np.arctan(LD(1))


# ---- log Phi in longdouble --------------------------------------------------------------------------------------------------------------

def _log_upper_tail_ld(a):
    """log(1 - Phi(a)) for a >= 1, longdouble: the continued fraction of the Mills ratio, 1 - Phi(a) = phi(a) / (a + 1 / (a + 2 / (a +
    3 / ...))), evaluated bottom-up with a fixed number of terms.  Its error after n terms falls like exp(-2 a sqrt(n)): 560 terms
    for a in [1, 1.5), 250 in [1.5, 3), 64 from 3 on leave less than 1e-20 (tests/test_score_host.py holds it to scipy and to the
    700-term value)."""
    a = np.asarray(a, LD)
    out = np.empty(a.shape, LD)
    for lo, hi, n in ((1.0, 1.5, 560), (1.5, 3.0, 250), (3.0, np.inf, 64)):
        sel = (a >= lo) & (a < hi) if np.isfinite(hi) else (a >= lo)
        if sel.any():
            out[sel] = _upper_tail_terms(a[sel], n)
    return out


def _upper_tail_terms(a, n):
    t = a.copy()
    for k in range(n, 0, -1):
        t = a + LD(k) / t
    return -LD(0.5) * a * a - LD(0.5) * np.log(LD(2) * PI_LD) - np.log(t)


def _phi_centre_ld(x):
    """Phi(x) for |x| < 1, longdouble: 1/2 + phi(x) (x + x^3 / 3 + x^5 / 15 + ...), terms of one sign."""
    x = np.asarray(x, LD)
    term, tot = x.copy(), x.copy()
    for k in range(1, 60):
        term = term * x * x / LD(2 * k + 1)
        tot = tot + term
    return LD(0.5) + np.exp(-LD(0.5) * x * x) / np.sqrt(LD(2) * PI_LD) * tot


def log_phi_ld(x):
    """log Phi(x) in longdouble, finite and accurate to a few longdouble ulp for every finite x."""
    x = np.asarray(x, LD)
    out = np.empty(x.shape, LD)
    lo, hi = x <= -1, x >= 1
    mid = ~(lo | hi)
    if lo.any():
        out[lo] = _log_upper_tail_ld(-x[lo])
    if hi.any():
        out[hi] = np.log1p(-np.exp(_log_upper_tail_ld(x[hi])))
    if mid.any():
        out[mid] = np.log(_phi_centre_ld(x[mid]))
    return out


def log_phi_f64(x):
    """log Phi(x) as the kernel forms it (score_log_phi), fp64: log(erfcx(-x / sqrt 2) / 2) - x^2 / 2 left of -1, else
    log1p(-erfc(x / sqrt 2) / 2)."""
    from scipy.special import erfc, erfcx
    x = np.asarray(x, np.float64)
    t = x * 0.70710678118654752440
    with np.errstate(all="ignore"):
        return np.where(x < -1.0, np.log(0.5 * erfcx(-t)) - 0.5 * (x * x), np.log1p(-0.5 * erfc(t)))


def _lgamma_ld(x):
    """lgamma(x) for x > 0 in longdouble: the argument is shifted up to >= 16 (one logarithm of the product of the steps), then
    Stirling's series to B_16, whose first dropped term is below 1e-21 there."""
    x = LD(x)
    prod = LD(1)
    while x < 16:
        prod *= x
        x = x + LD(1)
    shift = np.log(prod)
    b = [LD(1) / 12, -LD(1) / 360, LD(1) / 1260, -LD(1) / 1680, LD(1) / 1188, -LD(691) / 360360, LD(1) / 156, -LD(3617) / 122400]
    s, xi, x2 = LD(0), LD(1) / x, LD(1) / (x * x)
    for c in b:
        s += c * xi
        xi *= x2
    return (x - LD(0.5)) * np.log(x) - x + LD(0.5) * np.log(LD(2) * PI_LD) + s - shift


# ---- the log densities and the two figures ------------------------------------------------------------------------------------------------

def _per_sample(U, V, mean, rows, cols, y, w, flag, kind, nu, alpha, T, log_phi, lgamma, extra=None):
    """l [n, S] in the type T.  U [nusers, S, K], V [nmovies, S, K] (engine.samples_get); alpha: a number or S values; extra [n, S]:
    added to the dot products (the bias terms of a pair of sides that carries them)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    U, V = np.asarray(U, T), np.asarray(V, T)
    S = U.shape[1]
    d = np.einsum("nsk,nsk->ns", U[rows], V[cols])
    p = T(mean) + (d if extra is None else d + np.asarray(extra, T))
    y = np.asarray(y, T)[:, None]
    al = np.broadcast_to(np.asarray(alpha, T).reshape(-1), (S,))[None, :]
    pi = PI_LD if T is LD else T(math.pi)
    if kind == "probit":
        sign = np.where(y > 0, T(1), T(-1))
        return log_phi(sign * p)
    if kind == "student":
        nu = T(nu)
        c = lgamma((nu + 1) / 2) - lgamma(nu / 2)
        e = y - p
        return c + T(0.5) * np.log(al / (nu * pi)) - (nu + 1) / 2 * np.log1p(al * (e * e) / nu)
    if kind != "gaussian":
        raise ValueError(kind)
    wv = np.ones_like(y) if w is None else np.asarray(w, T)[:, None]
    e = y - p
    l = T(0.5) * np.log(al * wv / (2 * pi)) - T(0.5) * (al * wv) * (e * e)
    if flag is not None:
        f = np.asarray(flag, np.int64)
        cen = f != 0
        if cen.any():
            x = np.asarray(f[cen], T)[:, None] * np.sqrt(al) * (p[cen] - y[cen])
            l[cen] = log_phi(x)
    return l


def _figures(l, T):
    """(lpd [n], pw [n]) of l [n, S]: the maximum is taken out of the sum of exponentials; two-pass variance."""
    S = l.shape[1]
    mx = l.max(axis=1, keepdims=True)
    lpd = mx[:, 0] + np.log(np.exp(l - mx).sum(axis=1)) - np.log(T(S))
    if S > 1:
        d = l - l.mean(axis=1, keepdims=True)
        pw = (d * d).sum(axis=1) / T(S - 1)
    else:
        pw = np.zeros(l.shape[0], T)
    return lpd, pw


def logdens(U, V, mean, rows, cols, y, w=None, flag=None, kind="gaussian", nu=None, alpha=1.0, extra=None):
    """(lpd, pw), [n] each, numpy longdouble: the reference."""
    l = _per_sample(U, V, mean, rows, cols, y, w, flag, kind, nu, alpha, LD, log_phi_ld, _lgamma_ld, extra)
    return _figures(l, LD)


def logdens_f64(U, V, mean, rows, cols, y, w=None, flag=None, kind="gaussian", nu=None, alpha=1.0, extra=None):
    """The same formulas in plain fp64 numpy: the yardstick for the rounding error."""
    l = _per_sample(U, V, mean, rows, cols, y, w, flag, kind, nu, alpha, np.float64, log_phi_f64, lambda x: np.float64(math.lgamma(float(x))),
                    extra)
    return _figures(l, np.float64)


def relative_error(got, want):
    """max over the cells of |got - want| / max(1, |want|), in longdouble; 0 for an empty list."""
    got, want = np.asarray(got, LD), np.asarray(want, LD)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / np.maximum(LD(1), np.abs(want))))


BAR_FACTOR = 8.0


def bar(f64, want, S):
    """What the device is held to: 8 x the error the fp64 restatement makes against the longdouble reference on the same input, and
    at least S 2^-52 (cells where the fp64 restatement happens to be exact)."""
    return max(BAR_FACTOR * relative_error(f64, want), S * 2.0 ** -52)


# ---- the planted experiment ----------------------------------------------------------------------------------------------------------------

def restate_chain_samples(oracle, K, M, Mt, nu, nsims, burnin, alpha):
    """robust_ref.restate_chain (the chain of gibbs(..., robust=nu), nu = None: the plain Gaussian chain) which keeps what a sample
    ring keeps: (U [nusers, S, K], V [nmovies, S, K]) of the post-burn-in iterations."""
    import robust_ref
    import util
    import weights_ref
    nm, nusers = len(M[0]) - 1, len(Mt[0]) - 1
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    U, V = np.zeros((nusers, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    keepU, keepV = [], []
    for it in range(nsims):
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        if nu is not None:
            sw, _ = robust_ref.weights(M, V, U, it, robust_ref.TAG_MOVIES, alpha, nu, mean_m)
            s, prod, _ = weights_ref.sample_side_weighted(oracle, K, M, sw * sw, mean_m, alpha, U, V, it, mu, LF)
        else:
            s, prod, _ = oracle.sample_side(K, M, mean_m, alpha, U, V, it, mu, LF, nthreads=robust_ref.NT)
        cov_m = oracle.cov(K, nm, s, prod)
        mu, LU, LF = oracle.hyper_sample(K, nusers, cov_u, it)
        if nu is not None:
            sw, _ = robust_ref.weights(Mt, U, V, it, robust_ref.TAG_USERS, alpha, nu, mean_u)
            s, prod, _ = weights_ref.sample_side_weighted(oracle, K, Mt, sw * sw, mean_u, alpha, V, U, it, mu, LF)
        else:
            s, prod, _ = oracle.sample_side(K, Mt, mean_u, alpha, V, U, it, mu, LF, nthreads=robust_ref.NT)
        cov_u = oracle.cov(K, nusers, s, prod)
        if it >= burnin:
            keepU.append(U.copy()); keepV.append(V.copy())
    return np.stack(keepU, axis=1), np.stack(keepV, axis=1), mean_m


def cells_of(A):
    """(rows, cols) of the CSC triple A, in its order"""
    return np.asarray(A[1], np.int64), np.repeat(np.arange(len(A[0]) - 1), np.diff(np.asarray(A[0], np.int64)))


def summary(lpd, pw):
    """bpmf_amd.score_summary's sums, restated"""
    lpd, pw = np.asarray(lpd, np.float64), np.asarray(pw, np.float64)
    n = len(lpd)
    e = lpd - pw
    return dict(n=n, lpd_sum=float(lpd.sum()), p_waic=float(pw.sum()), elpd=float(e.sum()), se=math.sqrt(n * e.var(ddof=1)),
                se_lpd=math.sqrt(n * lpd.var(ddof=1)))


def compare(a, b):
    """(difference of the sums, its paired standard error) of two per-cell arrays over the same cells"""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(d.sum()), math.sqrt(len(d) * d.var(ddof=1))


def planted_measure(oracle):
    """robust_ref.PLANTED (5 % of the training cells shifted by +-10, clean test cells) through the restated CPU chains of the
    Student-t model (nu = 4) and of the Gaussian model at the same alpha: dict(test=(lpd difference student - gaussian, its paired
    standard error), train=(elpd difference, its paired standard error), and the four sums)."""
    import robust_ref
    P = robust_ref.PLANTED
    d = robust_ref.planted_data(**P)
    tr, tc = cells_of(d["T"])
    mr, mc = cells_of(d["M"])
    out = {}
    per = {}
    for name, nu in (("student", P["nu"]), ("gaussian", None)):
        U, V, mean = restate_chain_samples(oracle, P["K"], d["M"], d["Mt"], nu, P["nsims"], P["burnin"], P["alpha"])
        kind = "student" if nu is not None else "gaussian"
        t_lpd, t_pw = logdens_f64(U, V, mean, tr, tc, d["T"][2], kind=kind, nu=nu, alpha=P["alpha"])
        m_lpd, m_pw = logdens_f64(U, V, mean, mr, mc, d["M"][2], kind=kind, nu=nu, alpha=P["alpha"])
        per[name] = (t_lpd, m_lpd - m_pw)
        out[name] = dict(test_lpd=float(t_lpd.sum()), train_elpd=float((m_lpd - m_pw).sum()), p_waic=float(m_pw.sum()))
    out["test"] = compare(per["student"][0], per["gaussian"][0])
    out["train"] = compare(per["student"][1], per["gaussian"][1])
    return out


# What the restated CPU chains give (tests/test_score_host.py re-measures them):
#   python -c "import sys; sys.path.insert(0, 'tests'); import score_ref as R; from oracle.oracle import Oracle; print(R.planted_measure(Oracle()))"
#   test cells (6000, clean):    lpd  student 1070.48, gaussian -406290.34: difference 407360.82, paired se 45756.32 (8.9 se)
#   training cells (24000):      elpd student -21373.36 (p_waic 3216.10), gaussian -1946415.32 (p_waic 1544361.85): difference
#                                1925041.96, paired se 80708.61 (23.9 se)
# The Gaussian model at alpha = 16 pays (1/2) 16 10^2 = 800 nats for every planted cell, and its factors, bent towards the planted
# values, miss the clean test cells.
PLANTED_MEASURED = dict(test=(407360.821231392, 45756.316508970885), train=(1925041.9587133676, 80708.61222012217),
                        student=dict(test_lpd=1070.4773023407674, train_elpd=-21373.3563631894, p_waic=3216.099907588806),
                        gaussian=dict(test_lpd=-406290.34392905125, train_elpd=-1946415.315076557, p_waic=1544361.8493551114))
PLANTED_MARGIN_SE = 2.0            # the Student-t model must lead by more than this many paired standard errors, on both sets of cells
