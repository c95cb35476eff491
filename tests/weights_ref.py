"""CPU reference of per-rating precision weights and the inputs the GPU tests run it on.

The conditional of column j under r_ij ~ N(mean + u_i . v_j, 1 / (alpha w_ij)) is
    Lambda* = Lambda + alpha sum_i w_ij u_i u_i^T,   b = Lambda mu + alpha sum_i w_ij (r_ij - mean) u_i,
and sum w u u^T = sum (sqrt(w) u)(sqrt(w) u)^T: the unchanged oracle draws from it exactly when it is fed one private, pre-scaled
row per rating -- rowidx = arange(nnz), other = sqrt(w)[:, None] * Y[rowidx], vals = sqrt(w) (r - mean), mean_rating = 0
(`sample_side_weighted`).  With all weights 1 that is the plain call bit for bit.  The chain (`restate_chain`) composes it with the
oracle's other pieces in the shape of censor_ref.restate_chain.
"""
import math

import numpy as np

from tests import probit_ref
from tests import util

NT = probit_ref.NT


def weights_of(A, W):
    """The per-rating weights of the CSC triple A from the CSC triple W (a listed cell takes its value, every other cell 1), cell by
    cell through a dictionary -- the plain statement bpmf_amd.rating_weights is checked against."""
    colptr, rowidx, _ = A
    at = {}
    for c in range(len(colptr) - 1):
        for p in range(int(colptr[c]), int(colptr[c + 1])):
            at[(int(rowidx[p]), c)] = p
    w = np.ones(len(rowidx), np.float64)
    wcp, wri, wv = W
    for c in range(len(wcp) - 1):
        for q in range(int(wcp[c]), int(wcp[c + 1])):
            w[at[(int(wri[q]), c)]] = wv[q]
    return w


def transpose(W, nrows):
    """CSC triple of the transpose of a weight matrix (its values are > 0: nothing sums to an explicit zero)"""
    import scipy.sparse as sp
    ncols = len(W[0]) - 1
    return util.csc_arrays(sp.csc_matrix((np.asarray(W[2], np.float64), W[1], W[0]), shape=(nrows, ncols)).T)


def expanded(A, w, mean, other):
    """(csc, other) of the expanded-rows construction: one private row sqrt(w) Y[r] per rating, the value sqrt(w) (r - mean)."""
    colptr, rowidx, vals = A
    sw = np.sqrt(np.asarray(w, np.float64))
    nnz = len(rowidx)
    rows = np.ascontiguousarray(sw[:, None] * other[rowidx]) if nnz else np.zeros((1, other.shape[1]))
    return (colptr, np.arange(nnz, dtype=np.int32), sw * (np.asarray(vals, np.float64) - mean)), rows


def sample_side_weighted(oracle, K, A, w, mean, alpha, other, items, it, mu, LF):
    """oracle.sample_side for the ratings A with the weights w: `items` is updated in place, returns (sum, prod, norm)."""
    csc, rows = expanded(A, w, mean, other)
    return oracle.sample_side(K, csc, 0.0, alpha, rows, items, it, mu, LF, nthreads=NT)


# ---- the edge side --------------------------------------------------------------------------------------------------------------------

EDGE_COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)


def edge_side(seed=17, nrows=300):
    """(A, nrows, w): columns of 0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129 and 257 ratings 1 .. 5 over 300 rows -- the
    counts on both sides of the group and index-block boundaries of the sampler forms (4, 16, 64) -- and a seeded weight
    Gamma(2, 0.5) per rating (every sqrt(w) rounds)."""
    rng = np.random.default_rng(seed)
    counts = np.array(EDGE_COUNTS)
    colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rowidx = np.concatenate([np.sort(rng.choice(nrows, size=c, replace=False)) for c in counts]).astype(np.int32)
    vals = rng.integers(1, 6, len(rowidx)).astype(np.float64)
    return (colptr, rowidx, vals), nrows, rng.gamma(2.0, 0.5, len(rowidx))


def seeded_weights(nnz, seed):
    """Gamma(2, 0.5) per rating"""
    return np.random.default_rng(seed).gamma(2.0, 0.5, nnz)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------

def restate_chain(oracle, K, M, Mt, T, W, nsims, burnin, alpha):
    """gibbs(..., weights=W) from oracle pieces.  Per iteration and side: hyper draw at counter it, sample_side_weighted with the
    side's own mean rating and alpha, cov.  W = None: the plain chain.  out["pred"]: the mean over the post-burn-in samples of
    mean + v . u per test entry."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    if W is not None:
        wm, wu = weights_of(M, W), weights_of(Mt, transpose(W, nu))
    U, V = np.zeros((nu, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    have_t = T is not None and len(T[2]) > 0
    Pavg, Pm2 = (T[2].copy(), T[2].copy()) if have_t else (None, None)
    psum, nadd = (np.zeros(len(T[2])) if have_t else np.zeros(0)), 0
    out = dict(rmse=[], rmse_avg=[])
    for it in range(nsims):
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        if W is not None:
            s, prod, _ = sample_side_weighted(oracle, K, M, wm, mean_m, alpha, U, V, it, mu, LF)
        else:
            s, prod, _ = oracle.sample_side(K, M, mean_m, alpha, U, V, it, mu, LF, nthreads=NT)
        cov_m = oracle.cov(K, nm, s, prod)
        mu, LU, LF = oracle.hyper_sample(K, nu, cov_u, it)
        if W is not None:
            s, prod, _ = sample_side_weighted(oracle, K, Mt, wu, mean_u, alpha, V, U, it, mu, LF)
        else:
            s, prod, _ = oracle.sample_side(K, Mt, mean_u, alpha, V, U, it, mu, LF, nthreads=NT)
        cov_u = oracle.cov(K, nu, s, prod)
        if have_t:
            if it >= burnin:
                psum += mean_m + probit_ref.dots(T, V, U)
                nadd += 1
            se, se_avg, nump = oracle.predict(K, T, V, U, mean_m, 0 if it < burnin else it - burnin, Pavg, Pm2, nthreads=NT)
            out["rmse"].append(math.sqrt(se / nump)); out["rmse_avg"].append(math.sqrt(se_avg / nump))
    if have_t and nsims > 0:                                         # movies.predict(users, true) once more (c++/bpmf.cpp:242)
        it = nsims - 1
        se, se_avg, nump = oracle.predict(K, T, V, U, mean_m, 0 if it < burnin else it - burnin, Pavg, Pm2, nthreads=NT)
        out["final_rmse_avg"] = math.sqrt(se_avg / nump)
    out["U"], out["V"] = U, V
    if have_t and nadd:
        out["pred"] = psum / nadd
    if W is not None:
        out["weights"] = (int((wm != 1.0).sum()), float(wm.min()), float(wm.max()))
    return out


def ml100k_weights(M, seed=23, frac=0.3):
    """The weight matrix of the chain tests: a seeded 30 % of the training cells, each with a weight of 0.25, 4 or 0.37."""
    colptr, rowidx, vals = M
    rng = np.random.default_rng(seed)
    keep = rng.random(len(vals)) < frac
    val = rng.choice(np.array([0.25, 4.0, 0.37]), size=len(vals))
    cols = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))[keep]
    wcp = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=len(colptr) - 1))]).astype(np.int64)
    return wcp, np.ascontiguousarray(rowidx[keep], np.int32), np.ascontiguousarray(val[keep], np.float64)


# ---- the planted heteroscedastic experiment -------------------------------------------------------------------------------------------

PLANTED = dict(nusers=600, nmovies=300, rank=4, per_user=40, ntest=6000, sd_noisy=2.0, sd_clean=0.25, alpha=16.0, w_noisy=1.0 / 64.0,
               seed=2029, K=8, nsims=60, burnin=30)


def planted_data(nusers, nmovies, rank, per_user, ntest, sd_noisy, sd_clean, w_noisy, seed, **_):
    """y = u . v + eps, u, v ~ N(0, I_rank): per_user training cells per user, a seeded half of them with noise sd sd_noisy, the others
    sd_clean; ntest noise-free held-out cells elsewhere.  Returns dict(M, Mt: the training matrix; W: the weight matrix (w_noisy at
    the noisy cells); Md, Mdt: the training matrix without the noisy cells; T, Tt: the test cells; mean_var: the mean noise variance)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    Ut, Vt = rng.standard_normal((nusers, rank)), rng.standard_normal((nmovies, rank))
    tr_c = np.concatenate([rng.choice(nmovies, size=per_user, replace=False) for _ in range(nusers)])
    tr_r = np.repeat(np.arange(nusers), per_user)
    taken = set((tr_r * nmovies + tr_c).tolist())
    te = []
    while len(te) < ntest:
        k = int(rng.integers(0, nusers * nmovies))
        if k not in taken:
            taken.add(k); te.append(k)
    te = np.array(te)
    te_r, te_c = te // nmovies, te % nmovies
    noisy = rng.random(len(tr_r)) < 0.5
    sd = np.where(noisy, sd_noisy, sd_clean)
    y_tr = np.einsum("ij,ij->i", Ut[tr_r], Vt[tr_c]) + sd * rng.standard_normal(len(tr_r))
    y_te = np.einsum("ij,ij->i", Ut[te_r], Vt[te_c])

    def csc(r, c, v):                                                # (+ 100: no value is an explicit zero for the containers)
        m = sp.coo_matrix((v + 100.0, (r, c)), shape=(nusers, nmovies)).tocsc()
        A, At = util.csc_arrays(m), util.csc_arrays(m.T)
        return (A[0], A[1], A[2] - 100.0), (At[0], At[1], At[2] - 100.0)
    M, Mt = csc(tr_r, tr_c, y_tr)
    Md, Mdt = csc(tr_r[~noisy], tr_c[~noisy], y_tr[~noisy])
    T, Tt = csc(te_r, te_c, y_te)
    Wm = util.csc_arrays(sp.coo_matrix((np.full(int(noisy.sum()), w_noisy), (tr_r[noisy], tr_c[noisy])), shape=(nusers, nmovies)))
    return dict(M=M, Mt=Mt, W=Wm, Md=Md, Mdt=Mdt, T=T, Tt=Tt, nnoisy=int(noisy.sum()), mean_var=float(np.mean(sd ** 2)))


def planted_rmse(pred, truth):
    return float(np.sqrt(np.mean((np.asarray(pred) - np.asarray(truth)) ** 2)))


# Measured with the restated CPU chains (tests/test_gpu_weights.py::test_planted_weights_are_honoured prints the first two again):
#   python -c "from tests import weights_ref as R; from oracle.oracle import Oracle; print(R.planted_measure(Oracle()))"
# test RMSE of (a) the weights honoured, (b) the weights ignored at alpha = 16, (c) the weights ignored at alpha = 1 / mean variance
# (the best single alpha), (d) the noisy cells dropped
PLANTED_MEASURED = (0.16851064279049544, 1.3976078703740435, 0.6112329159084524, 0.17138268078178603)
# (a) beats (c) by 0.443; the tests ask for half of that margin
PLANTED_HALF_MARGIN = 0.5 * (PLANTED_MEASURED[2] - PLANTED_MEASURED[0])


def planted_measure(oracle):
    P = PLANTED
    d = planted_data(**P)
    out = []
    for M, Mt, W, alpha in ((d["M"], d["Mt"], d["W"], P["alpha"]), (d["M"], d["Mt"], None, P["alpha"]),
                            (d["M"], d["Mt"], None, 1.0 / d["mean_var"]), (d["Md"], d["Mdt"], None, P["alpha"])):
        r = restate_chain(oracle, P["K"], M, Mt, d["T"], W, P["nsims"], P["burnin"], alpha)
        out.append(planted_rmse(r["pred"], d["T"][2]))
    return tuple(out)
