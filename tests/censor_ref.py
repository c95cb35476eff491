"""CPU restatement of the latent step of censored ratings and the inputs the GPU tests run it on.

numpy only.  The truncated-normal draw is the one of tests/probit_ref.py (imported, not restated twice): the censored draw feeds it
m' = -sqrt(alpha) e, so that the a it forms, -(s m'), is the a of the kernel, s (sqrt(alpha) e).  The chain (`restate_chain`) composes
the latent step with the oracle's pieces in the shape of probit_ref.restate_chain: oracle.hyper_sample, oracle.sample_side fed the
latent values as `vals` with the side's own mean rating and the caller's alpha, oracle.cov, oracle.predict.
"""
import math

import numpy as np

from tests import probit_ref
from tests import util

NT = probit_ref.NT
TAG_MOVIES, TAG_USERS = 5, 6


def flags_of(A, C):
    """The per-rating flags of the CSC triple A from the CSC triple C (entry > 0: +1, entry < 0: -1), cell by cell through a
    dictionary -- the plain statement bpmf_amd.censor_flags is checked against."""
    colptr, rowidx, _ = A
    at = {}
    for c in range(len(colptr) - 1):
        for p in range(int(colptr[c]), int(colptr[c + 1])):
            at[(int(rowidx[p]), c)] = p
    flags = np.zeros(len(rowidx), np.int8)
    ccp, cri, cv = C
    for c in range(len(ccp) - 1):
        for q in range(int(ccp[c]), int(ccp[c + 1])):
            flags[at[(int(cri[q]), c)]] = 1 if cv[q] > 0 else -1
    return flags


def transpose(C, nrows):
    """CSC triple of the transpose (through scipy, which the tests have anyway)"""
    import scipy.sparse as sp
    ncols = len(C[0]) - 1
    m = sp.csc_matrix((np.asarray(C[2], np.float64) + 4.0, C[1], C[0]), shape=(nrows, ncols))    # (+ 4: nothing sums to an explicit zero)
    t = util.csc_arrays(m.T)
    return t[0], t[1], t[2] - 4.0


def censored_dots(A, pos, X, Y):
    """m_p = X[c] . Y[r] for the rating positions `pos` of the CSC matrix A (column c = row of X, row r = row of Y)"""
    colptr, rowidx, _ = A
    cols = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))[pos]
    return np.einsum("ij,ij->i", X[cols], Y[rowidx[pos]])


def latent(A, flags, X, Y, it, tag, alpha, mean, full=False):
    """The array the sampler of the side with ratings A, flags, factors X (before its update) reads at iteration `it` against the
    factors Y: the ratings, with z_p = b_p + s (d / sqrt(alpha)) at every censored position.  The four operations of the draw:
        e = (b - mean) - m;  a = s (sqrt(alpha) e);  d = t - a, t ~ N(0, 1) | t > a;  z = b + s (d (1 / sqrt(alpha)))"""
    vals = np.asarray(A[2], np.float64)
    flags = np.asarray(flags)
    pos = np.flatnonzero(flags).astype(np.int64)
    s = flags[pos].astype(np.float64)
    b = vals[pos]
    m = censored_dots(A, pos, X, Y)
    sa = math.sqrt(float(alpha))
    isa = 1.0 / sa
    e = (b - mean) - m
    sd, attempts, margin, bmargin = probit_ref.truncated_draw(pos, it, tag, -(sa * e), s)      # sd = s d, d > 0
    d = s * sd
    z = vals.copy()
    z[pos] = b + s * (d * isa)
    return (z, pos, m, attempts, margin, bmargin) if full else z


def seeded_flags(nnz, seed, right=0.15, left=0.10):
    """about 15 % +1 and about 10 % -1"""
    u = np.random.default_rng(seed).random(nnz)
    return np.where(u < right, 1, np.where(u < right + left, -1, 0)).astype(np.int8)


# ---- the inputs of the GPU latent test (tests/test_gpu_censored.py), shared with the margin check of tests/test_censor_host.py ------

LATENT_ALPHAS = (0.5, 2.0, 3.0)
LATENT_ITER = 5
LATENT_FLAG_SEEDS = (301, 302)        # movies' orientation, users' orientation


def latent_inputs():
    """[(A, nrows, side, tag, flags)] for both orientations of probit_ref.skewed(); side 0: X = V, Y = U; side 1: X = U, Y = V"""
    M, Mt, nu, nm = probit_ref.skewed()
    return [(M, nu, 0, TAG_MOVIES, seeded_flags(len(M[2]), LATENT_FLAG_SEEDS[0])),
            (Mt, nm, 1, TAG_USERS, seeded_flags(len(Mt[2]), LATENT_FLAG_SEEDS[1]))], nu, nm


# ---- list-length edges --------------------------------------------------------------------------------------------------------------

def edge_side(seed=7, ncols=33, nrows=64):
    """33 columns with 0 .. 40 ratings (both ends present), ratings 1 .. 5"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 41, ncols)
    counts[3], counts[4], counts[0], counts[-1] = 0, 40, 7, 5        # (the first and the last column are not empty)
    colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rowidx = np.concatenate([np.sort(rng.choice(nrows, size=c, replace=False)) for c in counts]).astype(np.int32)
    return (colptr, rowidx, rng.integers(1, 6, len(rowidx)).astype(np.float64)), nrows


EDGE_COUNTS = (0, 1, 255, 256, 257, "nnz")
EDGE_SIGNS = ("right", "left", "mixed")


def edge_flags(A, count, signs, seed=11):
    """`count` censored positions: always the first and the last position of the CSC (count >= 2) and every rating of column 4
    (count >= 255), the rest seeded."""
    colptr = A[0]
    nnz = int(colptr[-1])
    n = nnz if count == "nnz" else int(count)
    rng = np.random.default_rng(seed + n)
    must = []
    if n >= 1:
        must.append(0)
    if n >= 2:
        must.append(nnz - 1)
    if n >= 255:
        must += list(range(int(colptr[4]), int(colptr[5])))
    must = np.unique(must)
    rest = np.setdiff1d(np.arange(nnz), must)
    pos = np.concatenate([must, rng.choice(rest, size=n - len(must), replace=False)]).astype(np.int64)
    flags = np.zeros(nnz, np.int8)
    if signs == "right":
        flags[pos] = 1
    elif signs == "left":
        flags[pos] = -1
    else:
        flags[pos] = np.where(rng.random(len(pos)) < 0.5, 1, -1)
    assert int(np.count_nonzero(flags)) == n
    return flags


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def restate_chain(oracle, K, M, Mt, T, C, nsims, burnin, alpha, nusers=None):
    """gibbs(..., censored=C) from oracle pieces.  Per iteration and side: the latent values from the factors the side holds and
    the other side's newest, hyper draw at counter it, oracle.sample_side with vals = z, the side's own mean rating and alpha, cov.
    C = None: the plain chain.  out["pred"]: the mean over the post-burn-in samples of mean + v . u per test entry."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    if C is not None:
        fm, fu = flags_of(M, C), flags_of(Mt, transpose(C, nu))
    U, V = np.zeros((nu, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    have_t = T is not None and len(T[2]) > 0
    Pavg, Pm2 = (T[2].copy(), T[2].copy()) if have_t else (None, None)
    psum, nadd = (np.zeros(len(T[2])) if have_t else np.zeros(0)), 0
    out = dict(rmse=[], rmse_avg=[], margin=math.inf)
    for it in range(nsims):
        zm = M[2]
        if C is not None:
            zm, _, _, _, mg, bmg = latent(M, fm, V, U, it, TAG_MOVIES, alpha, mean_m, full=True)
            out["margin"] = min(out["margin"], mg, bmg)
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        s, prod, _ = oracle.sample_side(K, (M[0], M[1], zm), mean_m, alpha, U, V, it, mu, LF, nthreads=NT)
        cov_m = oracle.cov(K, nm, s, prod)
        zu = Mt[2]
        if C is not None:
            zu, _, _, _, mg, bmg = latent(Mt, fu, U, V, it, TAG_USERS, alpha, mean_u, full=True)
            out["margin"] = min(out["margin"], mg, bmg)
        mu, LU, LF = oracle.hyper_sample(K, nu, cov_u, it)
        s, prod, _ = oracle.sample_side(K, (Mt[0], Mt[1], zu), mean_u, alpha, V, U, it, mu, LF, nthreads=NT)
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
    if C is not None:
        out["censored"] = (int((fm > 0).sum()), int((fm < 0).sum()))
    return out


def ml100k_censoring(M, seed=19, frac=0.2):
    """The censoring matrix of the chain tests: `frac` of the training cells drawn by a seeded rule; of those, the ratings <= 2
    are lower bounds (+1), the ratings >= 4 upper bounds (-1), the recorded bound is the rating itself (a 3 stays exact)."""
    colptr, rowidx, vals = M
    pick = np.random.default_rng(seed).random(len(vals)) < frac
    val = np.where(vals <= 2, 1.0, np.where(vals >= 4, -1.0, 0.0))
    keep = pick & (val != 0.0)
    cols = np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))[keep]
    ccp = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=len(colptr) - 1))]).astype(np.int64)
    return ccp, np.ascontiguousarray(rowidx[keep], np.int32), np.ascontiguousarray(val[keep], np.float64)


# ---- the planted experiment ---------------------------------------------------------------------------------------------------------

PLANTED = dict(nusers=600, nmovies=300, rank=4, per_user=40, ntest=6000, noise_var=0.25, alpha=4.0, quantile=70.0, seed=2027, K=8,
               nsims=60, burnin=30)


def planted_data(nusers, nmovies, rank, per_user, ntest, noise_var, quantile, seed, **_):
    """y = u . v + eps, eps ~ N(0, noise_var), u, v ~ N(0, I_rank): per_user training cells per user, ntest held-out cells elsewhere.
    Every training cell whose value exceeds the `quantile`-th percentile q of the training values is recorded as q with flag +1.
    Returns dict(M, Mt: the recorded training matrix; C: the censoring matrix; Md, Mdt: the training matrix without the censored
    cells; T, Tt: the test cells with their true values; q; above: the test cells whose true value is above q)."""
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
    sd = math.sqrt(noise_var)
    y_tr = np.einsum("ij,ij->i", Ut[tr_r], Vt[tr_c]) + sd * rng.standard_normal(len(tr_r))
    y_te = np.einsum("ij,ij->i", Ut[te_r], Vt[te_c]) + sd * rng.standard_normal(len(te_r))
    q = float(np.percentile(y_tr, quantile))
    cens = y_tr > q
    rec = np.where(cens, q, y_tr)

    def csc(r, c, v):                                                # (+ 100: no recorded value is an explicit zero for the containers)
        m = sp.coo_matrix((v + 100.0, (r, c)), shape=(nusers, nmovies)).tocsc()
        A, At = util.csc_arrays(m), util.csc_arrays(m.T)
        return (A[0], A[1], A[2] - 100.0), (At[0], At[1], At[2] - 100.0)
    M, Mt = csc(tr_r, tr_c, rec)
    Md, Mdt = csc(tr_r[~cens], tr_c[~cens], rec[~cens])
    T, Tt = csc(te_r, te_c, y_te)
    Cm = util.csc_arrays(sp.coo_matrix((np.ones(int(cens.sum())), (tr_r[cens], tr_c[cens])), shape=(nusers, nmovies)))
    return dict(M=M, Mt=Mt, C=Cm, Md=Md, Mdt=Mdt, T=T, Tt=Tt, q=q, above=T[2] > q, ncens=int(cens.sum()))


def planted_scores(pred, truth, above):
    """(RMSE on the test cells whose true value is above q, RMSE on all test cells)"""
    err = np.asarray(pred) - np.asarray(truth)
    return float(np.sqrt(np.mean(err[above] ** 2))), float(np.sqrt(np.mean(err ** 2)))


# Measured with the restated CPU chains (tests/test_gpu_censored.py::test_planted_bounds_are_honoured prints them again):
#   python -c "from tests import censor_ref as R; from oracle.oracle import Oracle; print(R.planted_measure(Oracle()))"
# (RMSE above q, RMSE on all test cells) of (a) the flags honoured, (b) the bounds taken as measurements, (c) the censored cells dropped
PLANTED_MEASURED = ((0.8178094421856322, 0.6577015149546273), (1.7018270935501427, 1.1086728011364877),
                    (1.4404012480645327, 0.978338647556144))
# (a) beats (b) on the cells above q by 0.884; the test asks for half of that (the noise floor sqrt(1 / alpha) is 0.5)
PLANTED_HALF_MARGIN = 0.5 * (PLANTED_MEASURED[1][0] - PLANTED_MEASURED[0][0])


def planted_measure(oracle):
    P = PLANTED
    d = planted_data(**P)
    out = []
    for M, Mt, C in ((d["M"], d["Mt"], d["C"]), (d["M"], d["Mt"], None), (d["Md"], d["Mdt"], None)):
        r = restate_chain(oracle, P["K"], M, Mt, d["T"], C, P["nsims"], P["burnin"], P["alpha"])
        out.append(planted_scores(r["pred"], d["T"][2], d["above"]))
    return out
