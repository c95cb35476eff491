"""CPU restatement of the prediction of rows unseen in training, in numpy longdouble, with the error bounds
the GPU tests judge the device by, and the planted experiment without its cold users in the matrix.

A side with features draws u ~ N(mu_s + beta_s^T f, Lambda_s^-1) in kept sample s.  For a new entity with features f and a column
c of the other side with factors v_s(c):
    e_s = mu_s + beta_s^T f          p_s = mean_rating + e_s . v_s(c)          mean = (1/S) sum_s p_s
    var = sum_s (p_s - mean)^2 / (S - 1)  [0 for S = 1]  +  w[c],   w[c] = (1/S) sum_s v_s(c)^T Lambda_s^-1 v_s(c)
std = sqrt(var) does not include the observation noise 1 / alpha.

The case worked by hand (test_newrows_host.py checks this module against it): 6 new rows x 5 columns, S = 2, K = 2, D = 2,
mean_rating = 3.
    F = (1,0) (0,1) (1,1) (2,0) (0,2) (0,0)                         one row (f1, f2) per new entity
    sample 1: mu = (0, 0), beta = I,   v(c) = (c, 1), Lambda = I          e_1 = (f1, f2)          p_1 - 3 = f1 c + f2
    sample 2: mu = (1, 0), beta = 2 I, v(c) = (1, c), Lambda = diag(2, 4) e_2 = (1 + 2 f1, 2 f2)  p_2 - 3 = 1 + 2 f1 + 2 f2 c
    mean = 3 + (f1 c + f2 + 1 + 2 f1 + 2 f2 c) / 2
    between the samples (S = 2): (p_1 - p_2)^2 / 2
    v^T Lambda^-1 v: sample 1: c^2 + 1, sample 2: 1 / 2 + c^2 / 4, so w[c] = (5 c^2 / 4 + 3 / 2) / 2 = 5 c^2 / 8 + 3 / 4
    e.g. row (1, 1), column 2: p_1 = 3 + 3 = 6, p_2 = 3 + 7 = 10, mean = 8, between = 16 / 2 = 8, w = 5 / 2 + 3 / 4 = 3.25,
    var = 11.25.  Every number is a small dyadic rational: the restatement must return them exactly.
"""
import math

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


# ---- the hand-worked case -------------------------------------------------------------------------------------------------------------

def hand_case():
    """inputs and the closed forms of the docstring: dict(F, betas, mus, Vs, Lambdas, mean_rating, mean, var, w, E)"""
    F = np.array([[1, 0], [0, 1], [1, 1], [2, 0], [0, 2], [0, 0]], float)
    c = np.arange(5.0)
    betas = [np.eye(2), 2.0 * np.eye(2)]
    mus = [np.zeros(2), np.array([1.0, 0.0])]
    Vs = [np.stack([c, np.ones(5)], 1), np.stack([np.ones(5), c], 1)]
    Lambdas = [np.eye(2), np.diag([2.0, 4.0])]
    f1, f2 = F[:, :1], F[:, 1:]
    p1 = f1 * c + f2
    p2 = 1.0 + 2.0 * f1 + 2.0 * f2 * c
    w = 5.0 * c * c / 8.0 + 0.75
    E = np.stack([F, np.stack([1.0 + 2.0 * F[:, 0], 2.0 * F[:, 1]], 1)])
    return dict(F=F, betas=betas, mus=mus, Vs=Vs, Lambdas=Lambdas, mean_rating=3.0, mean=3.0 + (p1 + p2) / 2.0,
                var=(p1 - p2) ** 2 / 2.0 + w, w=w, E=E)


# ---- the stages -----------------------------------------------------------------------------------------------------------------------

def project(F, beta, mu):
    """E = 1 mu^T + F beta in longdouble, and the magnitude |mu_k| + sum_d |F_id beta_dk| the bound of the projection is stated in.
    F: dense ndarray or scipy.sparse."""
    Fd = np.asarray(F.todense() if hasattr(F, "todense") else F, LD)
    b = np.asarray(beta, LD)
    return np.asarray(mu, LD) + Fd @ b, np.abs(np.asarray(mu, LD)) + np.abs(Fd) @ np.abs(b)


def project_bound(D, mag):
    return 2.0 * (D + 2) * U53 * mag


def cholesky_ld(A):
    """lower factor of a symmetric positive definite matrix, longdouble"""
    A = np.asarray(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def quadform(V, Lam):
    """v^T Lambda^-1 v for every row v of V, longdouble: Lambda = L L^T, |L^-1 v|^2 by forward substitution"""
    L = cholesky_ld(Lam)
    B = np.asarray(V, LD).T.copy()
    n = L.shape[0]
    for i in range(n):
        B[i] = (B[i] - L[i, :i] @ B[:i]) / L[i, i]
    return (B * B).sum(0)


def w_of(Vs, Lambdas):
    """w[c] = (1/S) sum_s v_s(c)^T Lambda_s^-1 v_s(c)"""
    return sum(quadform(V, L) for V, L in zip(Vs, Lambdas)) / LD(len(Vs))


def predict(Es, Vs, mean_rating, w=None):
    """Es [S, nq, K], Vs [S, nc, K] -> dict(mean, var) in longdouble and what the bounds need: absdot = (1/S) sum_s sum_k |e v|,
    absmax = max_s sum_k |e v|, dev1 = sum_s |p_s - mean|, dev2 = sum_s (p_s - mean)^2"""
    Es, Vs = np.asarray(Es, LD), np.asarray(Vs, LD)
    S = Es.shape[0]
    P = np.einsum("sqk,sck->sqc", Es, Vs)
    A = np.einsum("sqk,sck->sqc", np.abs(Es), np.abs(Vs))
    m = P.sum(0) / LD(S)
    dev = P - m
    between = (dev * dev).sum(0) / LD(S - 1) if S > 1 else np.zeros_like(m)
    var = between + (0 if w is None else np.asarray(w, LD))
    return dict(mean=LD(mean_rating) + m, var=var, between=between, absdot=A.sum(0) / LD(S), absmax=A.max(0), dev1=np.abs(dev).sum(0),
                dev2=(dev * dev).sum(0), absdev=np.abs(dev), S=S)


def mean_bound(ref, Kp, mean_rating):
    """the forward bound of a dot product of S Kp + 3 terms in any order"""
    return 2.0 * (ref["S"] * Kp + 3) * U53 * (abs(mean_rating) + ref["absdot"])


def var_bound(ref, Kp):
    """first-order perturbation of a two-pass variance; the factor 4 covers second-order terms and a one-pass scheme's constant"""
    S = ref["S"]
    if S == 1:
        return np.zeros_like(ref["var"])
    e_p = (Kp + 2) * U53 * ref["absmax"]
    return 4.0 * (4.0 * e_p * ref["dev1"] + (S + 3) * U53 * ref["dev2"]) / (S - 1) + 4.0 * U53 * ref["var"]


def predict_naive(Es, Vs, mean_rating):
    """(mean, var) from sum p and sum p^2 in fp64: what a kernel must NOT do (it cancels when |p_s| >> spread)"""
    Es, Vs = np.asarray(Es, np.float64), np.asarray(Vs, np.float64)
    S = Es.shape[0]
    s1 = np.zeros((Es.shape[1], Vs.shape[1])); s2 = np.zeros_like(s1)
    for s in range(S):
        p = Es[s] @ Vs[s].T
        s1 += p; s2 += p * p
    var = (s2 - s1 * s1 / S) / (S - 1) if S > 1 else np.zeros_like(s1)
    return mean_rating + s1 / S, var


def topn_of(mean, n):
    """the n best columns of every row of `mean` by (mean descending, id ascending); -1 beyond the columns"""
    nq, nc = mean.shape
    idx = np.full((nq, n), -1, np.int32)
    for i in range(nq):
        order = np.lexsort((np.arange(nc), -mean[i]))[:n]
        idx[i, :len(order)] = order
    return idx


# ---- the chain ------------------------------------------------------------------------------------------------------------------------

def restate_newrows(oracle, K, M, Mt, nsims, burnin, row_features, new_row_features, lam=5.0, alpha=2.0, tol=1e-6):
    """gibbs(..., row_features=, new_row_features=) from the pieces of tests/link_ref.py: the chain of link_ref.restate_chain, and per
    kept iteration the users' (mu, Lambda, beta) of that iteration and the movies' factors after it.  scipy.sparse features take the
    link draw of tests/link_sparse_ref.py (K conjugate-gradient solves in lockstep at `tol`).  Returns dict(mean, std) as
    res["new_rows"] (float64), and the per-sample state."""
    from tests import link_ref as ref
    from tests import util
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    if hasattr(row_features, "tocsr"):
        from tests import link_sparse_ref as ref_sparse
        lu = ref_sparse.SparseLink(row_features, lam, tol)
        ref = ref_sparse                                                      # (its half_iteration hands a side without a link on)
    else:
        lu = ref.Link(np.asarray(row_features, np.float64), lam)
    from tests.link_ref import new_state
    sm = new_state(nm, K)
    su = new_state(nu, K, lu.D)
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    Es, Vs, Lams, state = [], [], [], []
    for it in range(nsims):
        ref.half_iteration(oracle, K, M, mean_m, alpha, sm, su["U"], it, ref.TAG_MOVIES, None)
        ref.half_iteration(oracle, K, Mt, mean_u, alpha, su, sm["U"], it, ref.TAG_USERS, lu)
        if it >= burnin:
            R = np.triu(su["LU"])
            Es.append(project(new_row_features, su["beta"], su["mu"])[0]); Vs.append(sm["U"].copy()); Lams.append(R.T @ R)
            state.append(dict(mu=su["mu"].copy(), beta=su["beta"].copy(), LU=R, V=sm["U"].copy()))
    w = w_of(Vs, Lams)
    out = predict(np.stack(Es), np.stack(Vs), mean_m, w)
    return dict(mean=np.asarray(out["mean"], np.float64), std=np.sqrt(np.asarray(out["var"], np.float64)), state=state, mean_rating=mean_m,
                U=su["U"], V=sm["U"], good=out, w=w, kappa=max(float(np.linalg.cond(L)) for L in Lams))


def chain_bounds(want, Fnew, D, Kp):
    """(mean bound, var bound) of a device chain against restate_newrows' result `want`: the bounds of the three stages combined to
    first order -- the block kernel's (mean_bound, var_bound), the projection's error 2 (D + 2) u (|mu| + |F| |beta|) carried into
    every p_s through |v_s|, and the relative error 8 Kp u kappa_2(Lambda) of w."""
    good, S = want["good"], want["good"]["S"]
    dp = []
    for st in want["state"]:
        mag = project(Fnew, st["beta"], st["mu"])[1]
        dp.append(project_bound(D, mag) @ np.abs(np.asarray(st["V"], LD)).T)
    dp = np.stack(dp)
    mb = mean_bound(good, Kp, want["mean_rating"]) + dp.sum(0) / LD(S)
    vb = var_bound(good, Kp) + 8.0 * Kp * U53 * want["kappa"] * np.asarray(want["w"], LD)
    if S > 1:
        vb = vb + 4.0 * (good["absdev"] * dp).sum(0) / LD(S - 1)              # 2 |p_s - mean| (dp_s + the mean's share), doubled
    return mb, vb


def planted_split(P):
    """link_ref.PLANTED with its cold users taken out of the matrix: dict(Mw, Mtw, Tw, Ttw: training and test matrices of the warm
    users only; F_warm, F_cold; cells = (cold user, 0-based among the new rows; movie; rating) of the cold users' held-out ratings;
    full: the in-matrix data of link_ref.planted_data)."""
    from tests import link_ref as ref
    import scipy.sparse as sp
    from tests import util
    M, Mt, T, Tt, F, cold = ref.planted_data(**P)
    nu, nm, nc = P["nusers"], P["nmovies"], P["cold"]
    nw = nu - nc
    A = sp.csc_matrix((M[2], M[1], M[0]), shape=(nu, nm))
    assert A[nw:].nnz == 0                                             # the cold users rated nothing in training
    Aw = A[:nw].tocsc()
    Mw, Mtw = util.csc_arrays(Aw), util.csc_arrays(Aw.T.tocsc())
    tcol = np.repeat(np.arange(nm), np.diff(T[0]))
    cells = (T[1][cold] - nw, tcol[cold], T[2][cold])
    Tw = sp.csc_matrix((T[2], T[1], T[0]), shape=(nu, nm))[:nw].tocsc()            # the test entries of the warm users
    return dict(full=(M, Mt, T, Tt, F, cold), Mw=Mw, Mtw=Mtw, Tw=util.csc_arrays(Tw), Ttw=util.csc_arrays(Tw.T.tocsc()), F_warm=F[:nw],
                F_cold=F[nw:], cells=cells, nw=nw)


def coverage(r, mean, std, alpha):
    """the share of cells with |r - mean| <= 2 sqrt(std^2 + 1 / alpha)"""
    return float(np.mean(np.abs(r - mean) <= 2.0 * np.sqrt(std * std + 1.0 / alpha)))


def rmse(r, mean):
    return math.sqrt(float(np.mean((r - mean) ** 2)))
