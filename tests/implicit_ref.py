"""CPU reference of the implicit-feedback model and of the held-out ranks, and the inputs the tests run on.

Under the implicit model every cell (i, j) of the matrix is observed with precision alpha w_ij: a cell the matrix does not store as
r = 0 with w = w0, a stored one with its value and a confidence w_ij > w0; the mean rating is 0.  `sample_side_dense` says exactly
that to the weighted reference (weights_ref.sample_side_weighted): it hands it the DENSE matrix, every cell of a column an explicit
weighted rating.  It never forms G = sum u u^T, so it is independent of the reformulation the device runs (prior precision Lambda +
alpha w0 G, rows scaled by sqrt(w - w0), values w r / sqrt(w - w0)), which `sample_side_reformulated` restates on the CPU.
"""
import math

import numpy as np

from tests import probit_ref
from tests import util
from tests import weights_ref

NT = probit_ref.NT


def dense_side(A, w, w0, nrows):
    """(csc, weights) of the dense matrix behind the ratings A with the confidences w: every cell of every column, the value 0 and the
    weight w0 where A stores nothing."""
    colptr, rowidx, vals = A
    ncols = len(colptr) - 1
    V = np.zeros((ncols, nrows))
    Wd = np.full((ncols, nrows), float(w0))
    cols = np.repeat(np.arange(ncols), np.diff(colptr))
    V[cols, rowidx] = vals
    Wd[cols, rowidx] = w
    dcp = (np.arange(ncols + 1, dtype=np.int64) * nrows)
    dri = np.tile(np.arange(nrows, dtype=np.int32), ncols)
    return (dcp, dri, V.ravel()), Wd.ravel()


def sample_side_dense(oracle, K, A, w, w0, alpha, other, items, it, mu, LF):
    """One half-iteration of an implicit side through the dense matrix: `items` is updated in place, returns (sum, prod, norm)."""
    csc, wd = dense_side(A, w, w0, other.shape[0])
    return weights_ref.sample_side_weighted(oracle, K, csc, wd, 0.0, alpha, other, items, it, mu, LF)


def sample_side_reformulated(oracle, K, A, w, w0, alpha, other, items, it, mu, LF):
    """The same half-iteration the way the device runs it: the stored ratings only, rows scaled by sqrt(w - w0), values w r /
    sqrt(w - w0), under the prior precision LF + alpha w0 G with the right-hand side LF mu.  The oracle takes (mu, LF) and forms
    LF mu itself, so it is given mu' = (LF + alpha w0 G)^-1 LF mu."""
    colptr, rowidx, vals = A
    G = other.T @ other
    LF2 = LF + alpha * w0 * G
    mu2 = np.linalg.solve(LF2, LF @ mu)
    sw = np.sqrt(np.asarray(w) - w0)
    nnz = len(rowidx)
    rows = np.ascontiguousarray(sw[:, None] * other[rowidx]) if nnz else np.zeros((1, other.shape[1]))
    csc = (colptr, np.arange(nnz, dtype=np.int32), np.asarray(w) * np.asarray(vals, np.float64) / sw)
    return oracle.sample_side(K, csc, 0.0, alpha, rows, items, it, mu2, LF2, nthreads=NT)


def edge_implicit(w0=0.3, seed=41):
    """(A, nrows, w) of the half-iteration tests: weights_ref.edge_side()'s pattern (columns of 0 .. 257 ratings, 300 rows) with every
    value 1 and the confidences w = w0 + 0.05 + Gamma(2, 0.5)."""
    A, nrows, _ = weights_ref.edge_side()
    w = w0 + 0.05 + np.random.default_rng(seed).gamma(2.0, 0.5, len(A[1]))
    return (A[0], A[1], np.ones(len(A[1]))), nrows, w


# ---- the chain ------------------------------------------------------------------------------------------------------------------------

def restate_chain(oracle, K, M, Mt, T, W, w0, nsims, burnin, alpha, keep=False):
    """gibbs(..., implicit=w0, weights=W) from oracle pieces, with the dense reference.  Per iteration and side: hyper draw at counter
    it, sample_side_dense with mean rating 0, cov.  out["pred"]: the mean over the post-burn-in samples of v . u per test entry;
    keep=True: out["samples"] = [(U, V)] of the post-burn-in iterations."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    if W is not None:
        wm, wu = weights_ref.weights_of(M, W), weights_ref.weights_of(Mt, weights_ref.transpose(W, nu))
    else:
        wm, wu = np.ones(len(M[2])), np.ones(len(Mt[2]))
    U, V = np.zeros((nu, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    have_t = T is not None and len(T[2]) > 0
    Pavg, Pm2 = (T[2].copy(), T[2].copy()) if have_t else (None, None)
    psum, nadd = (np.zeros(len(T[2])) if have_t else np.zeros(0)), 0
    out = dict(rmse=[], rmse_avg=[], samples=[])
    for it in range(nsims):
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        s, prod, _ = sample_side_dense(oracle, K, M, wm, w0, alpha, U, V, it, mu, LF)
        cov_m = oracle.cov(K, nm, s, prod)
        mu, LU, LF = oracle.hyper_sample(K, nu, cov_u, it)
        s, prod, _ = sample_side_dense(oracle, K, Mt, wu, w0, alpha, V, U, it, mu, LF)
        cov_u = oracle.cov(K, nu, s, prod)
        if keep and it >= burnin:
            out["samples"].append((U.copy(), V.copy()))
        if have_t:
            if it >= burnin:
                psum += probit_ref.dots(T, V, U)
                nadd += 1
            se, se_avg, nump = oracle.predict(K, T, V, U, 0.0, 0 if it < burnin else it - burnin, Pavg, Pm2, nthreads=NT)
            out["rmse"].append(math.sqrt(se / nump)); out["rmse_avg"].append(math.sqrt(se_avg / nump))
    if have_t and nsims > 0:
        it = nsims - 1
        se, se_avg, nump = oracle.predict(K, T, V, U, 0.0, 0 if it < burnin else it - burnin, Pavg, Pm2, nthreads=NT)
        out["final_rmse_avg"] = math.sqrt(se_avg / nump)
    out["U"], out["V"] = U, V
    if have_t and nadd:
        out["pred"] = psum / nadd
    return out


def small_ones(nusers=60, nmovies=40, density=0.08, ntest=40, seed=5):
    """The 60 x 40 matrix of the chain and CLI tests: about 8 % ones; ntest further cells as the test matrix, half of them ones (held
    out of the training matrix) and half zeros.  -> M, Mt, T, Tt, nusers, nmovies"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    one = rng.random((nusers, nmovies)) < density
    r, c = np.nonzero(one)
    pick = rng.permutation(len(r))[:ntest // 2]
    held = np.zeros(len(r), bool); held[pick] = True
    zr, zc = np.nonzero(~one)
    zp = rng.permutation(len(zr))[:ntest - ntest // 2]

    def csc(rr, cc, vv):                                             # (+ 100: an explicit zero stays stored)
        m = sp.coo_matrix((vv + 100.0, (rr, cc)), shape=(nusers, nmovies)).tocsc()
        A, At = util.csc_arrays(m), util.csc_arrays(m.T)
        return (A[0], A[1], A[2] - 100.0), (At[0], At[1], At[2] - 100.0)
    M, Mt = csc(r[~held], c[~held], np.ones(int((~held).sum())))
    T, Tt = csc(np.concatenate([r[held], zr[zp]]), np.concatenate([c[held], zc[zp]]),
                np.concatenate([np.ones(int(held.sum())), np.zeros(len(zp))]))
    return M, Mt, T, Tt, nusers, nmovies


# ---- ranks, stated plainly --------------------------------------------------------------------------------------------------------------

def better(sa, ia, sb, ib):
    """topn's order: the higher score first, then the lower candidate"""
    return sa > sb or (sa == sb and ia < ib)


def plain_ranks(score, rated, tptr, tcand, exclude_rated=True):
    """(rank, ncand) from the dense score matrix [nq, nc] by the definition, cell by cell.  rated: per query the set of rated
    candidates; query q holds out tcand[tptr[q] : tptr[q + 1]]."""
    nq, nc = score.shape
    rank = np.zeros(len(tcand), np.int32)
    ncand = np.zeros(nq, np.int32)
    for q in range(nq):
        cands = [c for c in range(nc) if not (exclude_rated and c in rated[q])]
        ncand[q] = len(cands)
        for p in range(int(tptr[q]), int(tptr[q + 1])):
            c = int(tcand[p])
            rank[p] = 1 + sum(1 for c2 in cands if c2 != c and better(score[q, c2], c2, score[q, c], c))
    return rank, ncand


def rated_sets(At, nq):
    """per query (a column of the CSC triple At) the set of its rated candidates"""
    return [set(int(r) for r in At[1][int(At[0][q]):int(At[0][q + 1])]) for q in range(nq)]


def mean_scores(samples, mean_rating=0.0):
    """mean_rating + (1/S) sum_s U_s V_s^T, [nusers, nmovies]"""
    return mean_rating + sum(U @ V.T for U, V in samples) / len(samples)


# ---- the planted experiment -------------------------------------------------------------------------------------------------------------

PLANTED = dict(nusers=200, nmovies=120, rank=4, seed=2031, scale=1.6, shift=2.6, holdout=0.2, K=8, w0=0.3, alpha=2.0, nsims=30, burnin=10, n=10)


# Measured with the restated CPU chains (tests/test_implicit_host.py re-measures the third and checks the order of all three):
#   python -c "from tests import implicit_ref as R; from oracle.oracle import Oracle; print(R.planted_measure(Oracle()))"
# (recall@10, MPR) of (a) the implicit chain, (b) the plain chain on the ones only, (c) the popularity ranking
PLANTED_MEASURED = ((0.42485770402437073, 0.21734338644088794), (0.10292007375340707, 0.5070653897579115), (0.16597122013788682, 0.4147987808103668))


def planted(nusers, nmovies, rank, seed, scale, shift, holdout, **_):
    """A planted preference u . v (u, v ~ N(0, I_rank)); cell (i, j) is observed -- a one -- with the probability sigmoid(scale u . v -
    shift), which rises with the preference.  A seeded `holdout` share of the ones is held out as the test matrix.
    -> dict(M, Mt: the training ones; T, Tt: the held-out ones; pref: the planted preferences)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    Ut, Vt = rng.standard_normal((nusers, rank)), rng.standard_normal((nmovies, rank))
    pref = Ut @ Vt.T
    one = rng.random((nusers, nmovies)) < 1.0 / (1.0 + np.exp(-(scale * pref - shift)))
    r, c = np.nonzero(one)
    held = rng.random(len(r)) < holdout

    def csc(rr, cc):
        m = sp.coo_matrix((np.ones(len(rr)), (rr, cc)), shape=(nusers, nmovies)).tocsc()
        return util.csc_arrays(m), util.csc_arrays(m.T)
    M, Mt = csc(r[~held], c[~held])
    T, Tt = csc(r[held], c[held])
    return dict(M=M, Mt=Mt, T=T, Tt=Tt, pref=pref)


def score_arm(score, d, n):
    """(recall@n, MPR) of a dense score matrix [nusers, nmovies] on the planted data: the held-out ones of every user ranked among the
    movies the user has no training one for."""
    from bpmf_amd import held_out_lists, rank_metrics
    nu = score.shape[0]
    tptr, tcand, _ = held_out_lists(d["T"], nu, "rows")
    rank, ncand = plain_ranks(score, rated_sets(d["Mt"], nu), tptr, tcand)
    m = rank_metrics(rank, tptr, ncand, n)
    return m["recall"], m["mpr"]


def popularity_scores(d):
    """every user scores a movie by its number of training ones"""
    counts = np.diff(d["M"][0]).astype(np.float64)
    return np.tile(counts, (len(d["Mt"][0]) - 1, 1))


def planted_measure(oracle, P=PLANTED):
    """((recall@n, MPR) of the implicit chain, of the plain chain on the ones only, of the popularity ranking), restated on the CPU"""
    d = planted(**P)
    a = restate_chain(oracle, P["K"], d["M"], d["Mt"], d["T"], None, P["w0"], P["nsims"], P["burnin"], P["alpha"], keep=True)
    b = plain_chain_samples(oracle, P["K"], d["M"], d["Mt"], P["nsims"], P["burnin"], P["alpha"])
    return (score_arm(mean_scores(a["samples"]), d, P["n"]), score_arm(mean_scores(b), d, P["n"]), score_arm(popularity_scores(d), d, P["n"]))


def plain_chain_samples(oracle, K, M, Mt, nsims, burnin, alpha):
    """the post-burn-in samples [(U, V)] of the plain Gaussian chain on the stored ratings (for a matrix of ones: mean rating 1)"""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    U, V = np.zeros((nu, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    out = []
    for it in range(nsims):
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        s, prod, _ = oracle.sample_side(K, M, mean_m, alpha, U, V, it, mu, LF, nthreads=NT)
        cov_m = oracle.cov(K, nm, s, prod)
        mu, LU, LF = oracle.hyper_sample(K, nu, cov_u, it)
        s, prod, _ = oracle.sample_side(K, Mt, mean_u, alpha, V, U, it, mu, LF, nthreads=NT)
        cov_u = oracle.cov(K, nu, s, prod)
        if it >= burnin:
            out.append((U.copy(), V.copy()))
    return out


def count_ranks(score, rated, tptr, tcand, exclude_rated=True):
    """plain_ranks with the inner count over the candidates as one numpy expression per held-out entry (the GPU tests' reference at
    the larger shapes; tests/test_implicit_host.py holds it against plain_ranks)"""
    nq, nc = score.shape
    ids = np.arange(nc)
    rank = np.zeros(len(tcand), np.int32)
    ncand = np.zeros(nq, np.int32)
    for q in range(nq):
        ok = np.ones(nc, bool)
        if exclude_rated and rated[q]:
            ok[sorted(rated[q])] = False
        ncand[q] = int(ok.sum())
        s = score[q]
        for p in range(int(tptr[q]), int(tptr[q + 1])):
            c = int(tcand[p])
            first = (s > s[c]) | ((s == s[c]) & (ids < c))
            rank[p] = 1 + int((first & ok & (ids != c)).sum())
    return rank, ncand
