"""CPU restatement of the ordinal probit likelihood, formula for formula: the interval mass and its logarithm,
the one-block inversion draw of the latent scores, the Metropolis-Hastings step of the cutpoints, and the chain.

numpy / scipy for the arithmetic (erfc, erfcinv); the Philox4x32-10 blocks come from tests/probit_ref.py.  The chain
(`restate_chain`) composes these with the oracle's pieces the way probit_ref.restate_chain does: oracle.hyper_sample,
oracle.sample_side fed the latent scores as `vals` with mean 0 and alpha 1, oracle.cov, oracle.predict.
"""
import math

import numpy as np
from scipy.special import erfc, erfcinv, ndtri

from tests import util
from tests.probit_ref import NT, canonical53, dots, philox4x32_10

TAG_MOVIES, TAG_USERS = 11, 12
TAIL = 37.0
RSQRT2 = 0.70710678118654752440
SQRT2 = 1.41421356237309504880
HALF_LOG_2PI = 0.91893853320467274178
TINY = 2.2250738585072014e-308
MAX_ATTEMPTS = 64
TARGET = 0.35


def counter(it):
    return 0x40000000 + int(it)


def table(cut):
    """-inf, g_1 .. g_{C-1}, +inf"""
    return np.concatenate(([-math.inf], np.asarray(cut, np.float64), [math.inf]))


def _reflect(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    with np.errstate(invalid="ignore"):
        refl = a + b < 0.0
    return np.where(refl, -b, a), np.where(refl, -a, b), refl


def log_tail(a):
    r = 1.0 / (a * a)
    s = r * (r * (r * (r * 105.0 - 15.0) + 3.0) - 1.0) + 1.0
    return -0.5 * a * a - np.log(a) - HALF_LOG_2PI + np.log(s)


def logmass(a, b):
    """log[Phi(b) - Phi(a)], a < b"""
    a, b, _ = _reflect(a, b)
    with np.errstate(all="ignore"):
        tail = a > TAIL
        at = np.where(tail, a, 40.0)
        la = log_tail(at)
        bt = np.where(tail & np.isfinite(b), b, 41.0)
        lt = np.where(np.isfinite(b), la + np.log1p(-np.exp(log_tail(bt) - la)), la)
        lc = np.log(0.5 * (erfc(a * RSQRT2) - erfc(b * RSQRT2)))
    return np.where(tail, lt, lc)


def mass(a, b):
    """Phi(b) - Phi(a), a < b"""
    a, b, _ = _reflect(a, b)
    with np.errstate(all="ignore"):
        return np.where(a > TAIL, np.exp(logmass(a, b)), 0.5 * (erfc(a * RSQRT2) - erfc(b * RSQRT2)))


def truncated(p, it, tag, a, b, full=False):
    """t ~ N(0, 1) | a < t <= b for the rating positions p at iteration `it` on the streams `tag`: one Philox block per rating.
    full: also (u, which form each draw took: 0 = erfcinv, 1 = erfcinv through the other tail, 2 = exponential tail)."""
    p = np.asarray(p, np.int64)
    plo = (p & 0xFFFFFFFF).astype(np.uint64)
    phi = (p >> 32).astype(np.uint64)
    w0, w1, _, _ = philox4x32_10(plo, phi, it, 0, 42, tag)
    u = canonical53(w1, w0)
    a, b, refl = _reflect(a, b)
    with np.errstate(all="ignore"):
        tail = a > TAIL
        span = -np.expm1(-a * (b - a))
        t_tail = a - np.log1p(-u * span) / np.where(tail, a, 1.0)
        v = (1.0 - u) * erfc(a * RSQRT2) + u * erfc(b * RSQRT2)
        v2 = (1.0 - u) * erfc(-a * RSQRT2) + u * erfc(-b * RSQRT2)
        t_c = SQRT2 * erfcinv(np.maximum(v, TINY))
        t_o = -SQRT2 * erfcinv(np.maximum(v2, TINY))
    other = ~tail & (v > 1.0)
    t = np.where(tail, t_tail, np.where(other, t_o, t_c))
    t = np.minimum(np.maximum(t, a), b)
    t = np.where(refl, -t, t)
    if full:
        return t, u, np.where(tail, 2, np.where(other, 1, 0))
    return t


def level_index(vals, levels):
    levels = np.asarray(levels, np.float64)
    idx = np.searchsorted(levels, vals)
    assert np.all(idx < len(levels)) and np.all(levels[idx] == vals), "a value is not a level"
    return idx


def latent_from(m, lev, it, tag, cut):
    g = table(cut)
    lo, hi = g[lev], g[lev + 1]
    z = m + truncated(np.arange(len(m)), it, tag, lo - m, hi - m)
    return np.minimum(np.maximum(z, lo), hi)


def latent(A, X, Y, it, tag, levels, cut):
    """The latent scores of the side with ratings A and factors X (before its update) against the factors Y, iteration `it`."""
    return latent_from(dots(A, X, Y), level_index(A[2], levels), it, tag, cut)


def loglik_from(m, lev, cut):
    g = table(cut)
    return float(np.sum(logmass(g[lev] - m, g[lev + 1] - m).astype(np.longdouble)))


def probs_from(m, cut):
    """[n, C]: the probability of every level"""
    g = table(cut)
    return np.stack([mass(g[c] - m, g[c + 1] - m) for c in range(len(g) - 1)], axis=1) if len(m) else np.zeros((0, len(g) - 1))


def default_cutpoints(vals, levels):
    cnt = np.bincount(level_index(vals, levels), minlength=len(levels)).astype(np.float64)
    add = 0.5 if cnt.min() == 0 else 0.0
    cum = np.cumsum(cnt + add)[:-1] / (len(vals) + add * len(levels))
    return ndtri(cum)


def propose(cut, step, it):
    """The proposal of the cutpoint step at iteration `it`.  Returns (g', attempts per cutpoint, bound margin): the closest a
    candidate of any attempt came to one of its bounds."""
    g = table(cut)
    C = len(g) - 1
    gp = g.copy()
    attempts, margin = [], math.inf
    for k in range(1, C):
        lo, hi = gp[k - 1], g[k + 1]
        x, n_used = g[k], MAX_ATTEMPTS
        for n in range(MAX_ATTEMPTS):
            w0, w1, w2, w3 = (np.atleast_1d(w) for w in philox4x32_10(counter(it), k, 0, n, 42, 0))
            u1 = 1.0 - float(canonical53(w3, w2)[0])
            u2 = float(canonical53(w1, w0)[0])
            rho, ang = math.sqrt(-2.0 * math.log(u1)), 2.0 * math.pi * u2
            x1, x2 = g[k] + step * (rho * math.cos(ang)), g[k] + step * (rho * math.sin(ang))
            ok1 = lo < x1 < hi
            cands = [x1] if ok1 else [x1, x2]
            margin = min([margin] + [abs(c - e) for c in cands for e in (lo, hi) if math.isfinite(e)])
            if ok1:
                x, n_used = x1, n + 1
                break
            if lo < x2 < hi:
                x, n_used = x2, n + 1
                break
        gp[k] = x
        attempts.append(n_used)
    return gp[1:-1].copy(), attempts, margin


def accept(cut, prop, step, it, ll_cur, ll_prop):
    """(accepted, margin): margin = |ln u - log ratio|"""
    g, gp = table(cut), table(prop)
    corr = 0.0
    for k in range(1, len(g) - 1):
        corr += float(logmass((gp[k - 1] - g[k]) / step, (g[k + 1] - g[k]) / step)) - float(logmass((g[k - 1] - gp[k]) / step, (gp[k + 1] - gp[k]) / step))
    _, _, w2, w3 = (np.atleast_1d(w) for w in philox4x32_10(counter(it), 0, 0, 0, 42, 0))
    u = 1.0 - float(canonical53(w3, w2)[0])
    ratio = (ll_prop - ll_cur) + corr
    return (math.log(u) < ratio), abs(math.log(u) - ratio)


def cut_step(cut, step, it, m, lev):
    """One step at iteration `it` given the scores m and levels of the movies' ratings: (new cutpoints, accepted, accept margin,
    bound margin, (l(g), l(g')))"""
    prop, _, bmargin = propose(cut, step, it)
    l0, l1 = loglik_from(m, lev, cut), loglik_from(m, lev, prop)
    acc, amargin = accept(cut, prop, step, it, l0, l1)
    return (prop if acc else np.asarray(cut, np.float64).copy()), acc, amargin, bmargin, (l0, l1)


def adapt(step, acc, it):
    return math.exp(math.log(step) + ((1.0 if acc else 0.0) - TARGET) / math.sqrt(it + 1))


# ---- the inputs of the GPU kernel tests (tests/test_gpu_ordinal.py), shared with the margin checks of tests/test_ordinal_host.py --------

KERNEL_CASES = [(8, "f64"), (10, "f64"), (32, "f64"), (64, "f64"), (128, "f64"), (128, "f32")]
KERNEL_NNZ = [0, 1, 255, 256, 257, 4097]
KERNEL_ITER = 3
LEVEL_SETS = {2: ([0.0, 1.0], [0.3]),
              5: ([1.0, 2.0, 3.0, 4.0, 5.0], [-1.5, -1.0, 0.5, 2.5]),
              16: (list(range(16)), list(np.linspace(-2.6, 2.5, 15)))}


def kernel_matrix(nnz, C, seed=7, absent=None):
    """(M, Mt, nu, nm): 37 movies x 211 users with nnz ratings at distinct random cells; movies 0, 5 and 36 and users 0, 3, 100 and 210 have no
    ratings; the values are levels of LEVEL_SETS[C], `absent` (a level index) never among them."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed + nnz + 1000 * C)
    nu, nm = 211, 37
    cols_ok = np.setdiff1d(np.arange(nm), [0, 5, 36])
    rows_ok = np.setdiff1d(np.arange(nu), [0, 3, 100, 210])
    cells = rng.permutation(len(rows_ok) * len(cols_ok))[:nnz]
    r, c = rows_ok[cells // len(cols_ok)], cols_ok[cells % len(cols_ok)]
    levels = np.asarray(LEVEL_SETS[C][0], np.float64)
    pick = np.setdiff1d(np.arange(C), [] if absent is None else [absent])
    v = levels[rng.choice(pick, nnz)]
    m = sp.coo_matrix((v + 100.0, (r, c)), shape=(nu, nm)).tocsc()     # (explicit zeros must survive: a level may be 0)
    A, At = util.csc_arrays(m), util.csc_arrays(m.T)
    return (A[0], A[1], A[2] - 100.0), (At[0], At[1], At[2] - 100.0), nu, nm


def kernel_factors(K, dtype, nu, nm):
    """Random factors scaled so that u . v has standard deviation 1.5; fp32: the values the device stores."""
    rng = np.random.default_rng(2000 + K)
    sigma = (2.25 / K) ** 0.25
    V = rng.standard_normal((nm, K)) * sigma
    U = rng.standard_normal((nu, K)) * sigma
    if dtype == "f32":
        V, U = V.astype(np.float32).astype(np.float64), U.astype(np.float32).astype(np.float64)
    return U, V


GIVEN_STEP = dict(nsims=5, burnin=3, step=0.03)       # the chain of test_given_step_disables_the_adaptation, on the CHAIN data
FAR_SCALE = 6.0                                        # kernel_factors times this: u . v has standard deviation 54, |m| beyond 37 + |g|
CHAIN = dict(nusers=120, nmovies=60, nobs=2400, ntest=300, rank=3, seed=77, K=8, nsims=8, burnin=4)


def planted(nusers, nmovies, nobs, ntest, rank, seed, cut=(-1.5, -1.0, 0.5, 2.5), levels=(1.0, 2.0, 3.0, 4.0, 5.0), **_):
    """Levels of u . v + eps against the planted cutpoints, eps ~ N(0, 1), at nobs + ntest distinct random cells; u, v ~ N(0, I_rank).
    Returns (M, Mt, T, Tt, nusers, nmovies)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    n = nobs + ntest
    pos = rng.permutation(nusers * nmovies)[:n]
    r, c = pos // nmovies, pos % nmovies
    Ut = rng.standard_normal((nusers, rank))
    Vt = rng.standard_normal((nmovies, rank))
    score = np.einsum("ij,ij->i", Ut[r], Vt[c]) + rng.standard_normal(n)
    val = np.asarray(levels, np.float64)[np.searchsorted(np.asarray(cut), score)]

    def csc(sel):
        m = sp.coo_matrix((val[sel] + 100.0, (r[sel], c[sel])), shape=(nusers, nmovies)).tocsc()
        A, At = util.csc_arrays(m), util.csc_arrays(m.T)
        return (A[0], A[1], A[2] - 100.0), (At[0], At[1], At[2] - 100.0)
    M, Mt = csc(np.arange(n) < nobs)
    T, Tt = csc(np.arange(n) >= nobs)
    return M, Mt, T, Tt, nusers, nmovies


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def restate_chain(oracle, K, M, Mt, T, nsims, burnin, levels, cutpoints=None, step=None):
    """gibbs(..., ordinal=levels) from oracle pieces.  Per iteration: (from iteration 1 on, sampled cutpoints) the cutpoint step at
    the newest factors of both sides; per side the latent scores from the factors the side holds and the other side's newest,
    hyper draw at counter it, oracle.sample_side with vals = z, mean 0, alpha 1, cov.  After both sides of a post-burn-in iteration
    the level probabilities of the test entries are added up."""
    levels = np.asarray(levels, np.float64)
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    U, V = np.zeros((nu, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    have_t = T is not None and len(T[2]) > 0
    Pavg, Pm2 = (T[2].copy(), T[2].copy()) if have_t else (None, None)
    psum, nadd = None, 0
    sampled = cutpoints is None
    cut = default_cutpoints(M[2], levels) if sampled else np.asarray(cutpoints, np.float64)
    s = step if step is not None else 1.0 / math.sqrt(len(M[2]))
    lev_m = level_index(M[2], levels)
    out = dict(rmse=[], rmse_avg=[], cutpoints=[], accepted=[], step=[], accept_margin=math.inf, bound_margin=math.inf, loglik=[])
    for it in range(nsims):
        acc = False
        out["step"].append(s)
        if sampled and it > 0:
            cut, acc, am, bm, ll = cut_step(cut, s, it, dots(M, V, U), lev_m)
            out["accept_margin"] = min(out["accept_margin"], am); out["bound_margin"] = min(out["bound_margin"], bm)
            out["loglik"].append(ll)
            if step is None and it < burnin:
                s = adapt(s, acc, it)
        out["accepted"].append(acc); out["cutpoints"].append(np.array(cut))
        z = latent(M, V, U, it, TAG_MOVIES, levels, cut)
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        sm, prod, _ = oracle.sample_side(K, (M[0], M[1], z), 0.0, 1.0, U, V, it, mu, LF, nthreads=NT)
        cov_m = oracle.cov(K, nm, sm, prod)
        z = latent(Mt, U, V, it, TAG_USERS, levels, cut)
        mu, LU, LF = oracle.hyper_sample(K, nu, cov_u, it)
        sm, prod, _ = oracle.sample_side(K, (Mt[0], Mt[1], z), 0.0, 1.0, V, U, it, mu, LF, nthreads=NT)
        cov_u = oracle.cov(K, nu, sm, prod)
        if have_t:
            if it >= burnin:
                pr = probs_from(dots(T, V, U), cut)
                psum = pr if psum is None else psum + pr
                nadd += 1
            se, se_avg, nump = oracle.predict(K, T, V, U, 0.0, 0 if it < burnin else it - burnin, Pavg, Pm2, nthreads=NT)
            out["rmse"].append(math.sqrt(se / nump)); out["rmse_avg"].append(math.sqrt(se_avg / nump))
    out["U"], out["V"] = U, V
    out["cutpoints"] = np.array(out["cutpoints"]).reshape(nsims, len(levels) - 1)
    if have_t and nadd:
        out["cat_prob"] = psum / nadd
        out["expected"] = out["cat_prob"] @ levels
        true = level_index(T[2], levels)
        with np.errstate(divide="ignore"):
            out["logp"] = float(np.mean(np.log(out["cat_prob"][np.arange(len(true)), true])))
    return out
