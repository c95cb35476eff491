"""CPU restatement of the fold-in and the inputs the tests run it on.

For a new row i with ratings {(j, r_ij)} and kept sample s -- v_js from the candidate side, (alpha_s, mu_s, Lambda_s) of the side the
row belongs to --

    Lambda* = Lambda_s + alpha_s sum_j v_js v_js^T,   b = Lambda_s mu_s + alpha_s sum_j (r_ij - mean) v_js
    Lambda* = L L^T,   u_is = L^-T (L^-1 b + z)

numpy / LAPACK for the factorisation and the solves.  The normals z are Box-Muller on the keyed Philox blocks: block n of (i, s) has
the counter (i lo, i hi, s, n) and the key (42, tag); u1 = 1 - canonical53(w3, w2), u2 = canonical53(w1, w0), rho = sqrt(-2 ln u1),
component 2 n = rho cos(2 pi u2), component 2 n + 1 = rho sin(2 pi u2).  Philox and canonical53 are those of tests/probit_ref.py,
which tests/test_probit_host.py checks against the oracle.
"""
import math

import numpy as np
import scipy.sparse as sp

from tests.probit_ref import philox4x32_10, canonical53

TAG_ROWS, TAG_COLS = 7, 8            # gibbs / bpmf: new users, new movies


def uniforms(n_rows, S, K, tag, row0=0):
    """(u1, u2), [n_rows, S, ceil(K / 2)] each: the two uniforms of every Philox block the rows row0 .. row0 + n_rows - 1 draw"""
    nb = (K + 1) // 2
    i = (np.arange(n_rows, dtype=np.int64) + row0)[:, None, None]
    s = np.arange(S, dtype=np.int64)[None, :, None]
    n = np.arange(nb, dtype=np.int64)[None, None, :]
    i, s, n = np.broadcast_arrays(i, s, n)
    w0, w1, w2, w3 = philox4x32_10(i & 0xFFFFFFFF, i >> 32, s, n, 42, tag)
    return 1.0 - canonical53(w3, w2), canonical53(w1, w0)


def normals(n_rows, S, K, tag, row0=0):
    """z [n_rows, S, K]"""
    u1, u2 = uniforms(n_rows, S, K, tag, row0)
    rho = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(u1.shape[:2] + (2 * u1.shape[2],))
    z[:, :, 0::2] = rho * np.cos(2.0 * math.pi * u2)
    z[:, :, 1::2] = rho * np.sin(2.0 * math.pi * u2)
    return z[:, :, :K]


def fold_in(R, Vs, alphas, mus, Lams, mean, tag=None, want_cond=False):
    """u [n_new, S, K] for the new rows R (scipy.sparse [n_new, ncols]; stored zeros are ratings) against the kept samples Vs
    [S, ncols, K] with the hyper-parameters alphas [S], mus [S, K], Lams [S, K, K].  tag None: z = 0, the conditional mean.
    want_cond: also the largest 2-norm condition number of a Lambda* (NaN entries for an indefinite one are skipped)."""
    R = sp.csr_matrix(R)
    n, S, K = R.shape[0], len(Vs), Vs[0].shape[1]
    z = normals(n, S, K, tag) if tag is not None else np.zeros((n, S, K))
    out = np.empty((n, S, K))
    worst = 0.0
    for i in range(n):
        cols = R.indices[R.indptr[i]:R.indptr[i + 1]]
        order = np.argsort(cols, kind="stable")
        cols = cols[order]
        r = R.data[R.indptr[i]:R.indptr[i + 1]][order] - mean
        for s in range(S):
            V = Vs[s][cols]
            A = Lams[s] + alphas[s] * (V.T @ V)
            b = Lams[s] @ mus[s] + alphas[s] * (V.T @ r)
            L = np.linalg.cholesky(A)
            y = np.linalg.solve(L, b) + z[i, s]
            out[i, s] = np.linalg.solve(L.T, y)
            if want_cond:
                worst = max(worst, float(np.linalg.cond(A)))
    return (out, worst) if want_cond else out


def predict(E, Vs, mean):
    """(mean, std) [n_new, ncols] of p_s = mean + u_is . v_cs over the samples (std with S - 1; 0 for S = 1)"""
    P = mean + np.einsum("isk,sck->sic", E, Vs)
    return P.mean(axis=0), (P.std(axis=0, ddof=1) if len(Vs) > 1 else np.zeros(P.shape[1:]))


def topn_of(mean, n, exclude=None):
    """[nq, n] ids by (mean descending, id ascending), -1 past the candidates; exclude: per query the ids left out"""
    nq, nc = mean.shape
    out = np.full((nq, n), -1, np.int64)
    for q in range(nq):
        m = mean[q].copy()
        ids = np.arange(nc)
        if exclude is not None and len(exclude[q]):
            keep = np.ones(nc, bool); keep[exclude[q]] = False
            ids, m = ids[keep], m[keep]
        order = np.lexsort((ids, -m))[:n]
        out[q, :len(order)] = ids[order]
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

NCOLS = 300


def edge_counts(K, chunk):
    """the ratings per row one batch covers: nothing, one, around K, around the kernel's chunk, several chunks + 1, every column"""
    return [0, 1, K - 1, K, K + 1, chunk - 1, chunk, chunk + 1, 257, NCOLS]


def rows_with_counts(counts, ncols, seed):
    """scipy.sparse CSR [len(counts), ncols]: row i rates counts[i] distinct random columns with values in 1 .. 5 (halves)"""
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for c in counts:
        cols = np.sort(rng.choice(ncols, c, replace=False))
        indices.extend(cols.tolist()); data.extend((rng.integers(2, 11, c) * 0.5).tolist())
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data, float), np.array(indices, np.int32), np.array(indptr, np.int64)), shape=(len(counts), ncols))


def hypers(K, S, seed):
    """(alphas [S] -- a different one per sample --, mus [S, K], Lams [S, K, K] = A^T A / K + I)"""
    rng = np.random.default_rng(seed)
    alphas = 1.5 + 0.75 * np.arange(S)
    mus = 0.3 * rng.standard_normal((S, K))
    A = rng.standard_normal((S, K, K))
    Lams = np.einsum("ski,skj->sij", A, A) / K + np.eye(K)
    return alphas, mus, Lams


def factors(K, S, ncols, seed):
    """[S, ncols, K] i.i.d. N(0, 1 / 4): |v|^2 ~ K / 4, so a row with many ratings has a Gram well above its prior"""
    return 0.5 * np.random.default_rng(seed).standard_normal((S, ncols, K))


# ---- the planted experiment ------------------------------------------------------------------------------------------------------------

PLANTED = dict(nusers=600, nmovies=300, rank=4, per_user=24, given=12, alpha=4.0, held=100, seed=41, K=8, nsims=60, burnin=30)


def planted_data(nusers, nmovies, rank, per_user, given, alpha, held, seed, **_):
    """link_ref.planted_data's shape without features: r = u . v + eps, eps ~ N(0, 1 / alpha), u, v ~ N(0, I_rank),
    per_user ratings per user at distinct random movies.  The last `held` users are held out of the matrix: `given` of their
    ratings are what they arrive with, the rest are the held-out cells they are scored on.  Returns dict(rows, cols, r: every
    rating; given_mask, score_mask over them; nusers, nmovies, held)."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((nusers, rank))
    V = rng.standard_normal((nmovies, rank))
    rows = np.repeat(np.arange(nusers), per_user)
    cols = np.concatenate([rng.choice(nmovies, per_user, replace=False) for _ in range(nusers)])
    r = np.einsum("ij,ij->i", U[rows], V[cols]) + rng.standard_normal(len(rows)) / math.sqrt(alpha)
    new = rows >= nusers - held
    first = np.tile(np.arange(per_user) < given, nusers)
    return dict(rows=rows, cols=cols, r=r, given_mask=new & first, score_mask=new & ~first, warm_mask=~new, nusers=nusers, nmovies=nmovies, held=held)


def planted_matrices(d, with_new):
    """(M, Mt, nu) of the training matrix: the warm users alone, or (with_new) also the held-out users' given ratings as rows"""
    from tests import util
    sel = d["warm_mask"] | (d["given_mask"] if with_new else False)
    nu = d["nusers"] if with_new else d["nusers"] - d["held"]
    m = sp.coo_matrix((d["r"][sel], (d["rows"][sel], d["cols"][sel])), shape=(nu, d["nmovies"])).tocsc()
    return util.csc_arrays(m), util.csc_arrays(m.T.tocsc()), nu


def planted_new_rows(d):
    """scipy.sparse CSR [held, nmovies]: what the held-out users arrive with"""
    sel = d["given_mask"]
    return sp.csr_matrix((d["r"][sel], (d["rows"][sel] - (d["nusers"] - d["held"]), d["cols"][sel])), shape=(d["held"], d["nmovies"]))


def planted_cells(d):
    """(row among the held-out users, movie, rating) of the cells they are scored on"""
    sel = d["score_mask"]
    return d["rows"][sel] - (d["nusers"] - d["held"]), d["cols"][sel], d["r"][sel]


def rmse(r, pred):
    return float(np.sqrt(np.mean((np.asarray(pred) - np.asarray(r)) ** 2)))


def cpu_chain(oracle, K, M, Mt, nsims, burnin, alpha):
    """The plain chain from oracle pieces (link_ref.half_iteration without features), keeping per post-burn-in iteration the factors
    of both sides and the users' hyper-parameters: dict(Vs [S, nm, K], Us [S, nu, K], mus, Lams, mean)"""
    from tests import link_ref, util
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    sm, su = link_ref.new_state(nm, K), link_ref.new_state(nu, K)
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    Vs, Us, mus, Lams = [], [], [], []
    for it in range(nsims):
        link_ref.half_iteration(oracle, K, M, mean_m, alpha, sm, su["U"], it, 0)
        link_ref.half_iteration(oracle, K, Mt, mean_u, alpha, su, sm["U"], it, 0)
        if it >= burnin:
            Vs.append(sm["U"].copy()); Us.append(su["U"].copy()); mus.append(su["mu"].copy())
            Lams.append(su["LU"].T @ su["LU"])                      # Lambda = R^T R, R = LambdaU (upper)
    return dict(Vs=np.stack(Vs), Us=np.stack(Us), mus=np.stack(mus), Lams=np.stack(Lams), mean=mean_m)


def planted_measure(oracle):
    """(fold-in, the same users in the matrix, the mean predictor): RMSE at the held-out users' held-out cells"""
    P = PLANTED
    d = planted_data(**P)
    i, c, r = planted_cells(d)
    M, Mt, _ = planted_matrices(d, False)
    ch = cpu_chain(oracle, P["K"], M, Mt, P["nsims"], P["burnin"], P["alpha"])
    E = fold_in(planted_new_rows(d), ch["Vs"], np.full(len(ch["Vs"]), P["alpha"]), ch["mus"], ch["Lams"], ch["mean"], TAG_ROWS)
    folded = predict(E, ch["Vs"], ch["mean"])[0][i, c]
    M2, Mt2, _ = planted_matrices(d, True)
    ch2 = cpu_chain(oracle, P["K"], M2, Mt2, P["nsims"], P["burnin"], P["alpha"])
    base = d["nusers"] - d["held"]
    inside = ch2["mean"] + np.mean(np.einsum("snk,snk->sn", ch2["Us"][:, base + i], ch2["Vs"][:, c]), axis=0)
    return rmse(r, folded), rmse(r, inside), rmse(r, np.full(len(r), ch["mean"]))


# Measured with the restated CPU chains (tests/test_foldin_host.py::test_planted_fold_in_beats_the_mean_predictor prints them again):
#   python -c "from tests import foldin_ref as R; from oracle.oracle import Oracle; print(R.planted_measure(Oracle()))"
# RMSE at the 1 200 held-out cells of the 100 held-out users: by fold-in | with the users in the matrix | by the mean predictor
PLANTED_MEASURED = (0.6973206287420437, 0.6914425846744452, 2.051592827616552)
# fold-in beats the mean predictor by 1.354; the tests ask for half of that (the noise floor sqrt(1 / alpha) is 0.5)
PLANTED_HALF_MARGIN = 0.5 * (PLANTED_MEASURED[2] - PLANTED_MEASURED[0])
