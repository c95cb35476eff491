"""CPU restatement of side information with a SPARSE feature matrix and the inputs its tests run on.

Only the link draw differs from tests/link_ref.py: the noise matrices come from row streams (row i of a matrix with key word t is the
first K normals of the polar method on Philox4x32-10(counter = {i low, i high, it, attempt}, key = {42, t})), and beta solves
(F^T F + lambda I) beta = F^T (U - 1 mu^T + Z1 R^-T) + sqrt(lambda) Z2 R^-T by K conjugate-gradient solves in lockstep with the
device's freeze rule (a column is active in an iteration iff |r_k|^2 > tol^2 |rhs_k|^2 at its start; only active columns move).
`solver="exact"` replaces CG by numpy.linalg.solve on the dense G: the yardstick of what CG at a tolerance costs a chain.
"""
import math

import numpy as np
import scipy.sparse as sp

from tests import link_ref as ref
from tests import util
from tests.probit_ref import philox4x32_10, canonical53, dots

NT = ref.NT
TAG_MOVIES, TAG_USERS = ref.TAG_MOVIES, ref.TAG_USERS
KEY_Z1, KEY_Z2 = 0x10000, 0x20000


# ---- the row streams -------------------------------------------------------------------------------------------------------------------

def randn_rows(nrows, K, it, key, row0=0, details=False):
    """[nrows, K]: row i holds the first K accepted polar attempts of the stream (row0 + i, it) with key word `key`.  Attempt a
    consumes block a: x from the words (w3, w2), y from (w1, w0); the normal is y * sqrt(-2 log(r2) / r2).
    details=True: also the accept mask [nrows, attempts] of the attempts looked at and the closest any r2 came to 1."""
    rows = np.arange(row0, row0 + nrows, dtype=np.int64)
    lo, hi = (rows & 0xFFFFFFFF)[:, None], (rows >> 32)[:, None]
    out = np.zeros((nrows, K))
    filled = np.zeros(nrows, np.int64)
    a0, masks, margin = 0, [], math.inf
    while nrows and filled.min() < K:
        na = 2 * K + 32
        w0, w1, w2, w3 = philox4x32_10(lo, hi, it, np.arange(a0, a0 + na)[None, :], 42, key)
        x = 2.0 * canonical53(w3, w2) - 1.0
        y = 2.0 * canonical53(w1, w0) - 1.0
        r2 = x * x + y * y
        ok = ~((r2 > 1.0) | (r2 == 0.0))
        rank = np.cumsum(ok, axis=1) - 1 + filled[:, None]
        take = ok & (rank < K)
        ri, ai = np.nonzero(take)
        rr = r2[ri, ai]
        lg = np.fromiter(map(math.log, rr), np.float64, len(rr))       # (libm's log, as tests/link_ref.py::randn_tag)
        out[ri, rank[ri, ai]] = y[ri, ai] * np.sqrt(-2.0 * lg / rr)
        filled = np.minimum(filled + ok.sum(axis=1), K)
        masks.append(ok)
        margin = min(margin, float(np.abs(r2 - 1.0).min()))
        a0 += na
    if details:
        return out, (np.concatenate(masks, axis=1) if masks else np.zeros((0, 0), bool)), margin
    return out


# ---- K conjugate-gradient solves in lockstep -------------------------------------------------------------------------------------------

def cg_lockstep(F, Ft, lam, RHS, tol, max_iter):
    """(X, iterations per column, an active column was left at max_iter): (F^T F + lam I) X = RHS from X = 0."""
    RHS = np.asarray(RHS, np.float64)
    n = RHS.shape[1]
    x = np.zeros_like(RHS)
    r = RHS.copy()
    p = r.copy()
    bb = (r * r).sum(axis=0)
    rr = bb.copy()
    tol2 = tol * tol
    active = rr > tol2 * bb
    iters = np.zeros(n, np.int64)
    j = 0
    while j < max_iter and active.any():
        a = np.nonzero(active)[0]
        q = Ft @ (F @ p[:, a]) + lam * p[:, a]
        alpha = rr[a] / (p[:, a] * q).sum(axis=0)
        x[:, a] += alpha * p[:, a]
        r[:, a] -= alpha * q
        rn = (r[:, a] * r[:, a]).sum(axis=0)
        beta = rn / rr[a]
        rr[a] = rn
        iters[a] += 1
        still = rn > tol2 * bb[a]
        p[:, a[still]] = r[:, a[still]] + beta[still] * p[:, a[still]]
        active[a] = still
        j += 1
    return x, iters, bool(active.any())


# ---- one side --------------------------------------------------------------------------------------------------------------------------

class SparseLink:
    """A side with sparse features F [N, D] (scipy.sparse): F by rows and by columns; the dense G only on request."""

    def __init__(self, F, lam, tol=1e-6, max_iter=1000, solver="cg"):
        self.F = sp.csr_matrix(F, dtype=np.float64)
        self.F.sum_duplicates()
        self.Ft = self.F.T.tocsr()
        self.lam, self.tol, self.max_iter, self.solver = float(lam), float(tol), int(max_iter), solver
        self.D = self.F.shape[1]
        self._G = None
        self.iters = []                                                # CG iterations of every draw
        self.hit = False

    @property
    def G(self):
        if self._G is None:
            self._G = (self.Ft @ self.F).toarray() + self.lam * np.eye(self.D)
        return self._G

    @property
    def cond(self):
        return float(np.linalg.cond(self.G))

    def solve(self, RHS):
        if self.solver == "exact":
            self.iters.append(0)
            return np.linalg.solve(self.G, RHS)
        x, iters, hit = cg_lockstep(self.F, self.Ft, self.lam, RHS, self.tol, self.max_iter)
        self.iters.append(int(iters.max()) if len(iters) else 0)
        self.hit = self.hit or hit
        return x


def rhs(link, U, mu, LU, it, tag):
    """RHS = F^T (U - 1 mu^T + Z1 R^-T) + sqrt(lambda) Z2 R^-T, Lambda = R^T R, R = LU (upper)"""
    N, K = U.shape
    RinvT = np.linalg.inv(np.triu(LU)).T
    X = (U - mu) + randn_rows(N, K, it, tag + KEY_Z1) @ RinvT
    return link.Ft @ X + math.sqrt(link.lam) * (randn_rows(link.D, K, it, tag + KEY_Z2) @ RinvT)


def draw_beta(link, U, mu, LU, it, tag):
    return link.solve(rhs(link, U, mu, LU, it, tag))


def half_iteration(oracle, K, A, mean, alpha, st, Y, it, tag, link=None):
    """tests/link_ref.py::half_iteration with step 2' / 3' for a SparseLink (anything else goes to the dense restatement)."""
    if not isinstance(link, SparseLink):
        return ref.half_iteration(oracle, K, A, mean, alpha, st, Y, it, tag, link)
    N = len(A[0]) - 1
    mu, LU, LF = ref.hyper_ex(oracle, K, N, st["cov"], link.lam * (st["beta"].T @ st["beta"]), link.D, it)
    st["beta"] = draw_beta(link, st["U"], mu, LU, it, tag)
    st["M"] = link.F @ st["beta"]
    vals = ref.residuals(A, st["M"], Y)
    Ut = np.zeros((N, K))
    s, prod, _ = oracle.sample_side(K, (A[0], A[1], vals), mean, alpha, Y, Ut, it, mu, LF, nthreads=NT)
    st["cov"] = oracle.cov(K, N, s, prod)
    st["Ut"] = Ut
    st["U"] = Ut + st["M"]
    st["mu"], st["LU"] = mu, LU


def restate_chain(oracle, K, M, Mt, T, nsims, burnin, row_features=None, col_features=None, lam=5.0, alpha=2.0, predictions=False,
                  tol=1e-6, max_iter=1000, solver="cg"):
    """gibbs(..., row_features=, col_features=) with scipy.sparse features, from oracle pieces (the loop of tests/link_ref.py)."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    lm = SparseLink(col_features, lam, tol, max_iter, solver) if col_features is not None else None
    lu = SparseLink(row_features, lam, tol, max_iter, solver) if row_features is not None else None
    sm = ref.new_state(nm, K, lm.D if lm else None)
    su = ref.new_state(nu, K, lu.D if lu else None)
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
    if have_t and nsims > 0:
        se, se_avg, nump = oracle.predict(K, T, sm["U"], su["U"], mean_m, 0 if nsims - 1 < burnin else nsims - 1 - burnin, Pavg, Pm2, nthreads=NT)
        out["final_rmse_avg"] = math.sqrt(se_avg / nump)
    out["U"], out["V"] = su["U"], sm["U"]
    out["beta_rows"] = bsum_u / nkept if lu and nkept else None
    out["beta_cols"] = bsum_m / nkept if lm and nkept else None
    out["cg_iters"] = dict(movies=lm.iters if lm else None, users=lu.iters if lu else None)
    out["hit_max_iter"] = any(l.hit for l in (lm, lu) if l is not None)
    if predictions and have_t and nkept:
        out["pred"] = psum / nkept
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

def skewed_bits(n, D, per_row, seed):
    """[n, D] binary CSR: column d is on with probability proportional to 1 / (d + 1), scaled to per_row bits per row on average
    and capped at 1 (the first columns are then on in every row)."""
    rng = np.random.default_rng(seed)
    w = 1.0 / (np.arange(D) + 1.0)
    scale = per_row / w.sum()
    for _ in range(200):                                               # capping lowers the mean: rescale the uncapped part
        prob = np.minimum(1.0, scale * w)
        scale *= per_row / prob.sum()
    prob = np.minimum(1.0, scale * w)
    cols = [np.nonzero(rng.random(n) < prob[d])[0] for d in range(D)]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    Fc = sp.csc_matrix((np.ones(indptr[-1]), np.concatenate(cols), indptr), shape=(n, D))
    return Fc.tocsr()


def random_sparse(n, D, density, seed, binary=False):
    """[n, D] CSR with i.i.d. N(0, 1) (or 1) entries at uniformly random places"""
    rng = np.random.default_rng(seed)
    F = sp.random(n, D, density=density, format="csr", random_state=rng, data_rvs=(lambda k: np.ones(k)) if binary else rng.standard_normal)
    F.sum_duplicates()
    F.sort_indices()
    return F


# the planted experiment with sparse features: D = 2048 binary user features, which the dense path refuses
PLANTED = dict(nusers=3000, nmovies=300, rank=4, D=2048, bits=32, per_user=12, alpha=4.0, held_out=0.3, cold=500, noise=0.2, seed=31,
               K=8, lam=5.0, nsims=60, burnin=30, tol=1e-6)


def planted_data(nusers, nmovies, rank, D, bits, per_user, alpha, held_out, cold, noise, seed, **_):
    """(M, Mt, T, Tt, F, cold_mask) as tests/link_ref.py::planted_data, with F = skewed_bits and true U = F B + noise N(0, I),
    B ~ N(0, 1 / bits)."""
    rng = np.random.default_rng(seed)
    F = skewed_bits(nusers, D, bits, seed + 1)
    B = rng.standard_normal((D, rank)) / math.sqrt(bits)
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
    cold_mask = T[1] >= nusers - cold
    return M, Mt, T, Tt, F, cold_mask


split_rmse = ref.split_rmse
