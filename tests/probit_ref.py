"""CPU restatement of the probit latent step, decision for decision, and the inputs the GPU tests run it on.

numpy for the arithmetic; the Philox4x32-10 blocks come from a vectorised numpy restatement of the generator that
tests/test_probit_host.py checks against oracle.philox.  The chain (`restate_chain`) composes it with the oracle's pieces the way
restate() in tests/test_gpu_noise.py composes the adaptive chain: oracle.hyper_sample, oracle.sample_side fed the latent scores as
`vals` with mean 0 and alpha 1, oracle.cov, oracle.predict.
"""
import math
import os

import numpy as np

from tests import util

NT = max(1, min(os.cpu_count() or 1, 16))
MAX_ATTEMPTS = 64
TAG_MOVIES, TAG_USERS = 1, 2

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds over arrays of counters (uint64 arithmetic on 32-bit words); returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) & _MASK for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(_M0) * c0
        p1 = np.uint64(_M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(_W0)) & _MASK
        k1 = (k1 + np.uint64(_W1)) & _MASK
    return c0, c1, c2, c3


def canonical53(w_first, w_second):
    """libstdc++ generate_canonical<double, 53> fed two 32-bit words (the first is the low half), clamped below 1."""
    s = w_first.astype(np.float64) + w_second.astype(np.float64) * 4294967296.0
    return np.minimum(s * 2.0 ** -64, 1.0 - 2.0 ** -53)


def truncated_draw(p, it, tag, m, s):
    """z_p ~ N(m_p, 1) truncated to the half line of the sign s_p, for the rating positions p at iteration `it` on the streams
    `tag`.  Returns (z, attempts, margin, branch_margin): margin is the closest any accept / reject comparison came to its
    threshold, branch_margin the smallest nonzero |a| (the choice between the two proposals is a comparison of a with 0)."""
    p = np.asarray(p, np.int64)
    m = np.asarray(m, np.float64)
    s = np.asarray(s, np.float64)
    a = -(s * m)
    plo = (p & 0xFFFFFFFF).astype(np.uint64)
    phi = (p >> 32).astype(np.uint64)
    tail = a > 0.0
    lam = 0.5 * (a + np.sqrt(a * a + 4.0))
    d = np.full(len(p), -1.0)
    attempts = np.zeros(len(p), np.int64)
    margin = math.inf
    active = np.arange(len(p))
    for n in range(MAX_ATTEMPTS):
        if len(active) == 0:
            break
        w0, w1, w2, w3 = philox4x32_10(plo[active], phi[active], it, n, 42, tag)
        u1 = 1.0 - canonical53(w3, w2)
        u2 = canonical53(w1, w0)
        lg = np.log(u1)
        aa, tl = a[active], tail[active]
        # a > 0: Robert's exponential proposal
        with np.errstate(over="ignore", invalid="ignore"):
            t = aa - lg / lam[active]
            e = t - lam[active]
            bound = np.exp(-0.5 * (e * e))
            acc_tail = tl & (u2 <= bound)
            # a <= 0: Box-Muller, first the cosine branch, then the sine branch
            rho = np.sqrt(-2.0 * lg)
            t1 = rho * np.cos(2.0 * math.pi * u2)
            t2 = rho * np.sin(2.0 * math.pi * u2)
        acc1 = ~tl & (t1 > aa)
        acc2 = ~tl & ~acc1 & (t2 > aa)
        dist = np.where(tl, np.abs(u2 - bound), np.where(acc1, np.abs(t1 - aa), np.minimum(np.abs(t1 - aa), np.abs(t2 - aa))))
        margin = min(margin, float(dist.min()))
        out = np.where(acc_tail, t - aa, np.where(acc1, t1 - aa, t2 - aa))
        done = acc_tail | acc1 | acc2
        d[active[done]] = out[done]
        attempts[active] += 1
        active = active[~done]
    assert len(active) == 0, "the attempt cap was reached"
    nz = np.abs(a[a != 0.0])
    return s * d, attempts, margin, (float(nz.min()) if len(nz) else math.inf)


def labels(vals, threshold):
    return np.where(np.asarray(vals) > threshold, 1.0, -1.0)


def dots(A, X, Y):
    """m_p = X[c] . Y[r] for every rating p of the CSC matrix A (column c = row of X, row r = row of Y)"""
    colptr, rowidx, _ = A
    cols = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))
    return np.einsum("ij,ij->i", X[cols], Y[rowidx])


def latent(A, X, Y, it, tag, threshold, full=False):
    """The latent scores of the side with ratings A and factors X (before its update) against the factors Y, iteration `it`."""
    m = dots(A, X, Y)
    z, att, margin, bmargin = truncated_draw(np.arange(len(A[2])), it, tag, m, labels(A[2], threshold))
    return (z, m, att, margin, bmargin) if full else z


def phi(m):
    from scipy.special import erfc
    return 0.5 * erfc(-np.asarray(m) / math.sqrt(2.0))


def auc_pairs(score, label):
    """AUC by counting pairs, O(P x N): (#(pos > neg) + #(pos == neg) / 2) / (P N) as an exact fraction (numerator x 2, denominator)."""
    pos, neg = np.asarray(score)[np.asarray(label) > 0], np.asarray(score)[np.asarray(label) <= 0]
    gt = int((pos[:, None] > neg[None, :]).sum())
    eq = int((pos[:, None] == neg[None, :]).sum())
    return 2 * gt + eq, 2 * len(pos) * len(neg)


def auc_ranks(score, label):
    from scipy.stats import rankdata
    label = np.asarray(label) > 0
    P, N = int(label.sum()), int((~label).sum())
    if P == 0 or N == 0:
        return float("nan")
    r = rankdata(score)
    return (float(r[label].sum()) - P * (P + 1) / 2) / (P * N)


# ---- the inputs of the GPU latent tests (tests/test_gpu_probit.py), shared with the margin check of tests/test_probit_host.py --------

LATENT_CASES = [(8, "f64"), (10, "f64"), (16, "f64"), (32, "f64"), (64, "f64"), (100, "f64"), (128, "f64"), (128, "f32")]
LATENT_THRESHOLD = 3.0            # ratings 1 .. 5: 4 and 5 are positives
LATENT_ITER = 5


def skewed(seed=11):
    """(M, Mt, nu, nm): 600 movies x 60 000 users, movie 0 rated by 50 000 users, movies 1 .. 9 and 590 .. 599 unrated, every user
    1 or 2 ratings apart from movie 0 (the shape tests/test_gpu_noise.py uses for the same column search), ratings 1 .. 5."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    nu, nm = 60000, 600
    rows = [rng.choice(nu, 50000, replace=False)]
    cols = [np.zeros(50000, np.int64)]
    per = rng.integers(1, 3, nu)
    r = np.repeat(np.arange(nu), per)
    rows.append(r)
    cols.append(rng.integers(10, 590, len(r)))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    m = sp.coo_matrix((rng.integers(1, 6, len(rows)).astype(np.float64), (rows, cols)), shape=(nu, nm)).tocsc()
    m.data[:] = np.minimum(m.data, 5.0)
    M = util.csc_arrays(m)
    return M, util.csc_arrays(m.T), nu, nm


def latent_factors(K, dtype, nu, nm):
    """Random factors scaled so that u . v has standard deviation 2 (it spans about +-6); fp32: the values the device stores."""
    rng = np.random.default_rng(1000 + K)
    sigma = (4.0 / K) ** 0.25
    V = rng.standard_normal((nm, K)) * sigma
    U = rng.standard_normal((nu, K)) * sigma
    if dtype == "f32":
        V, U = V.astype(np.float32).astype(np.float64), U.astype(np.float32).astype(np.float64)
    return U, V


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def restate_chain(oracle, K, M, Mt, T, nsims, burnin, threshold=0.5):
    """gibbs(..., probit=True) from oracle pieces.  Per iteration and side: latent scores from the factors the side holds and the
    other side's newest, hyper draw at counter it, oracle.sample_side with vals = z, mean 0, alpha 1, cov.  After both sides of a
    post-burn-in iteration Phi(v . u) of the test entries is added up."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    U, V = np.zeros((nu, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    have_t = T is not None and len(T[2]) > 0
    Pavg, Pm2 = (T[2].copy(), T[2].copy()) if have_t else (None, None)
    psum, nadd = (np.zeros(len(T[2])) if have_t else np.zeros(0)), 0
    out = dict(rmse=[], rmse_avg=[], margin=math.inf)
    for it in range(nsims):
        z, _, _, mg, _ = latent(M, V, U, it, TAG_MOVIES, threshold, full=True)
        out["margin"] = min(out["margin"], mg)
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        s, prod, _ = oracle.sample_side(K, (M[0], M[1], z), 0.0, 1.0, U, V, it, mu, LF, nthreads=NT)
        cov_m = oracle.cov(K, nm, s, prod)
        z, _, _, mg, _ = latent(Mt, U, V, it, TAG_USERS, threshold, full=True)
        out["margin"] = min(out["margin"], mg)
        mu, LU, LF = oracle.hyper_sample(K, nu, cov_u, it)
        s, prod, _ = oracle.sample_side(K, (Mt[0], Mt[1], z), 0.0, 1.0, V, U, it, mu, LF, nthreads=NT)
        cov_u = oracle.cov(K, nu, s, prod)
        if have_t:
            if it >= burnin:
                psum += phi(dots(T, V, U))
                nadd += 1
            se, se_avg, nump = oracle.predict(K, T, V, U, 0.0, 0 if it < burnin else it - burnin, Pavg, Pm2, nthreads=NT)
            out["rmse"].append(math.sqrt(se / nump)); out["rmse_avg"].append(math.sqrt(se_avg / nump))
    out["U"], out["V"] = U, V
    if have_t and nadd:
        out["prob"] = psum / nadd
        lab = (T[2] > threshold).astype(np.float64)
        out["auc"] = auc_ranks(out["prob"], lab)
        out["brier"] = float(np.mean((out["prob"] - lab) ** 2))
    return out


# ---- the recovery experiment --------------------------------------------------------------------------------------------------------

# (1 000 x 500: 400 ratings per movie and 200 per user.  The chain starts from zero factors, a saddle of the bilinear model, and
#  leaves it within ~15 iterations at this density; at 4 000 x 2 000 it needs ~100, and over hundreds of iterations the rounding
#  differences between two implementations grow past any parity bound.)
RECOVERY = dict(nusers=1000, nmovies=500, ntrain=200_000, ntest=20_000, rank=4, seed=2025, K=8, nsims=40, burnin=20)


def recovery_data(nusers, nmovies, ntrain, ntest, rank, seed, **_):
    """Labels 1 if u . v + eps > 0 else 0, eps ~ N(0, 1), at ntrain + ntest distinct random positions; u, v ~ N(0, I_rank).
    Returns (M, Mt, T, Tt, nusers, nmovies, ceiling): ceiling = the AUC of the true Phi(u . v) on the test pairs."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    n = ntrain + ntest
    pos = rng.permutation(nusers * nmovies)[:n]
    r, c = pos // nmovies, pos % nmovies
    Ut = rng.standard_normal((nusers, rank))
    Vt = rng.standard_normal((nmovies, rank))
    score = np.einsum("ij,ij->i", Ut[r], Vt[c])
    lab = (score + rng.standard_normal(n) > 0).astype(np.float64)
    # (explicit zeros must survive the sparse containers: store label + 1 and take it off again)
    def csc(sel):
        m = sp.coo_matrix((lab[sel] + 1.0, (r[sel], c[sel])), shape=(nusers, nmovies)).tocsc()
        A = util.csc_arrays(m); At = util.csc_arrays(m.T)
        return (A[0], A[1], A[2] - 1.0), (At[0], At[1], At[2] - 1.0)
    tr, te = np.arange(n) < ntrain, np.arange(n) >= ntrain
    M, Mt = csc(tr)
    T, Tt = csc(te)
    ceiling = auc_ranks(score[te], lab[te])
    return M, Mt, T, Tt, nusers, nmovies, ceiling
