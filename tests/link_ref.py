"""CPU restatement of the side-information model and the inputs the GPU tests run it on.

The six steps of a half-iteration are composed from oracle pieces the way tests/probit_ref.py::restate_chain composes the probit
chain: oracle.hyper_sample (the extended draw through the identity tests/test_link_host.py pins), oracle.sample_side fed the
residual ratings as `vals`, oracle.cov, oracle.predict; numpy / LAPACK for G, its inverse and factor and the dense products.  The
normals Z of the link draw come from a numpy restatement of libstdc++'s polar method on the keyed Philox stream (key word 1 =
tag), which tests/test_link_host.py checks against oracle.randn (tag 0, bit for bit) and oracle.philox (the keyed block).

The conditional of beta is the one the model defines: beta | U, mu, Lambda regresses U - 1 mu^T (the factors themselves, not the
residual factors U - F beta_old) on F.
"""
import math
import os

import numpy as np

from tests import util
from tests.probit_ref import philox4x32_10, canonical53, dots

NT = max(1, min(os.cpu_count() or 1, 16))
TAG_MOVIES, TAG_USERS = 3, 4


# ---- the keyed normal stream ---------------------------------------------------------------------------------------------------------

def randn_tag(counter, tag, n):
    """n calls of `std::normal_distribution<>()(rng)` on the stream `counter` with key (42, tag): every call starts a fresh
    distribution object, so it runs polar attempts until one is accepted and returns y * mult of that attempt (the saved x * mult
    is dropped).  Attempt a consumes block a: x from the words (w3, w2), y from (w1, w0)."""
    out = np.empty(0)
    a0 = 0
    while len(out) < n:
        na = 2 * (n - len(out)) + 64
        w0, w1, w2, w3 = philox4x32_10(counter, 0, 0, np.arange(a0, a0 + na), 42, tag)
        x = 2.0 * canonical53(w3, w2) - 1.0
        y = 2.0 * canonical53(w1, w0) - 1.0
        r2 = x * x + y * y
        ok = ~((r2 > 1.0) | (r2 == 0.0))
        r2 = r2[ok]
        lg = np.array([math.log(v) for v in r2])                       # (libm's log, as libstdc++ calls it: numpy's vector log may differ in the last bit)
        out = np.concatenate([out, y[ok] * np.sqrt(-2.0 * lg / r2)])
        a0 += na
    return out[:n]


# ---- one side --------------------------------------------------------------------------------------------------------------------------

class Link:
    """The one-time quantities of a side with features F [N, D]: G = F^T F + lambda I, G^-1, L_G^-T (G = L_G L_G^T)."""

    def __init__(self, F, lam):
        self.F = np.ascontiguousarray(F, np.float64)
        self.lam = float(lam)
        self.D = self.F.shape[1]
        self.G = self.F.T @ self.F + self.lam * np.eye(self.D)
        self.cond = float(np.linalg.cond(self.G))
        self.Ginv = np.linalg.inv(self.G)
        self.LinvT = np.linalg.inv(np.linalg.cholesky(self.G)).T


def hyper_ex(oracle, K, N, cov, scatter, dof, it):
    """The extended draw from the oracle's plain one: N + dof points of covariance (N cov + S) / (N + dof) have the same posterior
    scale and degrees of freedom; kappa_c stays 2 + N, which rescales mu."""
    if scatter is None:
        return oracle.hyper_sample(K, N, cov, it)
    mu, LU, LF = oracle.hyper_sample(K, N + dof, (N * cov + scatter) / (N + dof), it)
    return mu * math.sqrt((2.0 + N + dof) / (2.0 + N)), LU, LF


def residuals(A, M, Y):
    """r_p - m_c . y_r over the ratings of the CSC matrix A (column c = row of M, row r = row of Y)"""
    return A[2] - dots(A, M, Y)


def half_iteration(oracle, K, A, mean, alpha, st, Y, it, tag, link=None):
    """One half-iteration of the side with ratings A against the factors Y.  st: dict(U, cov[, beta, M]), updated in place."""
    N = len(A[0]) - 1
    if link is None:
        mu, LU, LF = oracle.hyper_sample(K, N, st["cov"], it)
        s, prod, _ = oracle.sample_side(K, A, mean, alpha, Y, st["U"], it, mu, LF, nthreads=NT)
        st["cov"] = oracle.cov(K, N, s, prod)
        st["mu"], st["LU"] = mu, LU
        return
    D = link.D
    mu, LU, LF = hyper_ex(oracle, K, N, st["cov"], link.lam * (st["beta"].T @ st["beta"]), D, it)
    P = link.F.T @ (st["U"] - mu)
    Z = randn_tag(it, tag, D * K).reshape(D, K)
    E = np.linalg.solve(np.triu(LU), Z.T).T                          # E = Z R^-T, Lambda = R^T R
    st["beta"] = link.Ginv @ P + link.LinvT @ E
    st["M"] = link.F @ st["beta"]
    vals = residuals(A, st["M"], Y)
    Ut = np.zeros((N, K))
    s, prod, _ = oracle.sample_side(K, (A[0], A[1], vals), mean, alpha, Y, Ut, it, mu, LF, nthreads=NT)
    st["cov"] = oracle.cov(K, N, s, prod)
    st["Ut"] = Ut
    st["U"] = Ut + st["M"]
    st["mu"], st["LU"] = mu, LU


def new_state(N, K, D=None):
    st = dict(U=np.zeros((N, K)), cov=np.zeros((K, K)))
    if D is not None:
        st["beta"] = np.zeros((D, K)); st["M"] = np.zeros((N, K))
    return st


def restate_chain(oracle, K, M, Mt, T, nsims, burnin, row_features=None, col_features=None, lam=5.0, alpha=2.0, predictions=False):
    """gibbs(..., row_features=, col_features=) from oracle pieces.  Returns the traces, the factors, the posterior means of beta
    and (predictions=True) the posterior-mean prediction of every test entry."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    lm = Link(col_features, lam) if col_features is not None else None
    lu = Link(row_features, lam) if row_features is not None else None
    sm = new_state(nm, K, lm.D if lm else None)
    su = new_state(nu, K, lu.D if lu else None)
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    have_t = T is not None and len(T[2]) > 0
    Pavg, Pm2 = (T[2].copy(), T[2].copy()) if have_t else (None, None)
    out = dict(rmse=[], rmse_avg=[], norm_u=[], norm_m=[])
    bsum_m = np.zeros_like(sm["beta"]) if lm else None
    bsum_u = np.zeros_like(su["beta"]) if lu else None
    psum, nkept = (np.zeros(len(T[2])) if have_t else None), 0
    for it in range(nsims):
        half_iteration(oracle, K, M, mean_m, alpha, sm, su["U"], it, TAG_MOVIES, lm)
        half_iteration(oracle, K, Mt, mean_u, alpha, su, sm["U"], it, TAG_USERS, lu)
        if it >= burnin:
            nkept += 1
            if lm:
                bsum_m += sm["beta"]
            if lu:
                bsum_u += su["beta"]
            if have_t:
                psum += mean_m + dots(T, sm["U"], su["U"])
        out["norm_m"].append(math.sqrt(float((sm["U"] ** 2).sum()))); out["norm_u"].append(math.sqrt(float((su["U"] ** 2).sum())))
        if have_t:
            se, se_avg, nump = oracle.predict(K, T, sm["U"], su["U"], mean_m, 0 if it < burnin else it - burnin, Pavg, Pm2, nthreads=NT)
            out["rmse"].append(math.sqrt(se / nump)); out["rmse_avg"].append(math.sqrt(se_avg / nump))
    if have_t and nsims > 0:                                         # movies.predict(users) once more with the same iter (c++/bpmf.cpp:242)
        se, se_avg, nump = oracle.predict(K, T, sm["U"], su["U"], mean_m, 0 if nsims - 1 < burnin else nsims - 1 - burnin, Pavg, Pm2, nthreads=NT)
        out["final_rmse_avg"] = math.sqrt(se_avg / nump)
    out["U"], out["V"] = su["U"], sm["U"]
    out["beta_rows"] = bsum_u / nkept if lu and nkept else None
    out["beta_cols"] = bsum_m / nkept if lm and nkept else None
    out["cond"] = max(l.cond for l in (lm, lu) if l is not None) if (lm or lu) else 1.0
    if predictions and have_t and nkept:
        out["pred"] = psum / nkept
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def features(n, D, seed):
    """[n, D] i.i.d. N(0, 1)"""
    return np.random.default_rng(seed).standard_normal((n, D))


# the planted experiment: user features explain the users' factors; the last `cold` users have every rating held out
PLANTED = dict(nusers=600, nmovies=300, rank=4, D=16, per_user=12, alpha=4.0, held_out=0.3, cold=100, noise=0.2, seed=31,
               K=8, lam=5.0, nsims=60, burnin=30)


def planted_data(nusers, nmovies, rank, D, per_user, alpha, held_out, cold, noise, seed, **_):
    """(M, Mt, T, Tt, F, cold_mask): ratings r = u . v + eps, eps ~ N(0, 1 / alpha), u = B^T f + noise N(0, I), B ~ N(0, 1 / D),
    v ~ N(0, I_rank); per_user ratings per user at distinct random movies.  Test set: held_out of the ratings of the warm users and
    ALL ratings of the last `cold` users.  cold_mask marks the test entries (order of T) of cold users."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((nusers, D))
    B = rng.standard_normal((D, rank)) / math.sqrt(D)
    U = F @ B + noise * rng.standard_normal((nusers, rank))
    V = rng.standard_normal((nmovies, rank))
    rows = np.repeat(np.arange(nusers), per_user)
    cols = np.concatenate([rng.choice(nmovies, per_user, replace=False) for _ in range(nusers)])
    r = np.einsum("ij,ij->i", U[rows], V[cols]) + rng.standard_normal(len(rows)) / math.sqrt(alpha)
    test = (rng.random(len(rows)) < held_out) | (rows >= nusers - cold)

    def csc(sel):
        m = sp.coo_matrix((r[sel], (rows[sel], cols[sel])), shape=(nusers, nmovies)).tocsc()
        return util.csc_arrays(m), util.csc_arrays(m.T.tocsc())
    (M, Mt), (T, Tt) = csc(~test), csc(test)
    cold_mask = T[1] >= nusers - cold                                  # T is CSC by movie: its row indices are users
    return M, Mt, T, Tt, F, cold_mask


def split_rmse(pred, T, cold_mask):
    """(warm, cold) RMSE of the predictions of every test entry"""
    e2 = (np.asarray(pred) - T[2]) ** 2
    return math.sqrt(float(e2[~cold_mask].mean())), math.sqrt(float(e2[cold_mask].mean()))
