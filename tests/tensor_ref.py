"""CPU reference of the sparse tensor factorisation (Bayesian CP of order 3) and the inputs the tests run it on.

    r(i, j, t) ~ N(mean + sum_k a_ik b_jk c_tk, 1 / alpha),   a Normal-Wishart prior per mode.

The conditional of one factor row of a mode is the column update of the matrix model with the other side's row replaced by the
Hadamard product of the two other modes' rows.  So the unchanged oracle draws from it when it is fed one private row per entry: the
expanded-rows call of tests/weights_ref.py with all weights 1 (`sample_mode`).  `restate_chain` composes it with the oracle's
hyper-parameter draw, cov and predict; `plain_row` states one row's conditional again from the definition, with explicit loops and
numpy.linalg.  One oracle thread everywhere: the chain is then bit-reproducible.
"""
import math

import numpy as np

from tests import weights_ref

NT = 1


def others(m):
    """the two other modes of mode m, ascending"""
    return [k for k in range(3) if k != m]


def mode_order(idx, m):
    """positions -> entries: the entries sorted stably by their index in mode m (ties in input order)"""
    return np.argsort(np.asarray(idx)[:, m], kind="stable")


def mode_colptr(idx, dims, m):
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(idx)[:, m], minlength=dims[m]))]).astype(np.int64)


def khatri_rao(factors, idx, m, order=None):
    """[nnz, K]: per entry in the order of mode m the Hadamard product of its rows in the two other modes (one multiply each)"""
    a, b = others(m)
    o = mode_order(idx, m) if order is None else order
    idx = np.asarray(idx)
    return factors[a][idx[o, a]] * factors[b][idx[o, b]]


def sample_mode(oracle, K, idx, vals, dims, mean, alpha, factors, m, it, mu, LF):
    """One half-iteration of mode m on the unchanged oracle: factors[m] is updated in place; returns (sum, prod, norm)."""
    o = mode_order(idx, m)
    nnz = len(o)
    A = (mode_colptr(idx, dims, m), np.arange(nnz, dtype=np.int32), np.asarray(vals, np.float64)[o])
    P = np.ascontiguousarray(khatri_rao(factors, idx, m, o)) if nnz else np.zeros((1, K))
    csc, rows = weights_ref.expanded(A, np.ones(nnz), mean, P)
    return oracle.sample_side(K, csc, 0.0, alpha, rows, factors[m], it, mu, LF, nthreads=NT)


def plain_row(oracle, K, idx, vals, mean, alpha, factors, m, c, it, mu, LF):
    """The draw of row c of mode m from the tensor definition: Lambda* and b by explicit loops over the entries (input order),
    numpy.linalg for the factorisation and the solves, the normals from the oracle's stream of the column."""
    a, b = others(m)
    Ls = np.array(LF, np.float64, copy=True)
    rhs = np.asarray(LF, np.float64) @ np.asarray(mu, np.float64)
    for e in range(len(vals)):
        if idx[e][m] != c:
            continue
        p = np.array([factors[a][idx[e][a]][k] * factors[b][idx[e][b]][k] for k in range(K)])
        for i in range(K):
            for j in range(K):
                Ls[i, j] += alpha * p[i] * p[j]
            rhs[i] += alpha * (vals[e] - mean) * p[i]
    L = np.linalg.cholesky(Ls)
    z = oracle.randn((c + 1) * K * (it + 1), K)
    return np.linalg.solve(L.T, np.linalg.solve(L, rhs) + z)


def tcsc(tidx, tvals, dims):
    """the test entries as the matrix oracle.predict reads: one column per index of the last mode, entry p of that order in row p"""
    o = mode_order(tidx, 2)
    return (mode_colptr(tidx, dims, 2), np.arange(len(o), dtype=np.int32), np.asarray(tvals, np.float64)[o]), o


def restate_chain(oracle, K, idx, vals, dims, tidx, tvals, nsims, burnin, alpha):
    """tensor_gibbs from oracle pieces: per iteration and mode (last mode first) the hyper draw at counter it, sample_mode, cov; then
    predict over the test entries' Khatri-Rao rows of modes 0 and 1 against mode 2."""
    idx = np.asarray(idx); vals = np.asarray(vals, np.float64)
    mean = float(vals.mean()) if len(vals) else 0.0
    F = [np.zeros((d, K)) for d in dims]
    cov = [np.zeros((K, K)) for _ in range(3)]
    have_t = tidx is not None and len(tvals) > 0
    out = dict(rmse=[], rmse_avg=[], norms=np.zeros((nsims, 3)), mean_rating=mean)
    if have_t:
        T, o = tcsc(tidx, tvals, dims)
        Pavg, Pm2 = T[2].copy(), T[2].copy()
        psum, nadd = np.zeros(len(o)), 0
    for it in range(nsims):
        for m in (2, 1, 0):
            mu, LU, LF = oracle.hyper_sample(K, dims[m], cov[m], it)
            s, prod, nrm = sample_mode(oracle, K, idx, vals, dims, mean, alpha, F, m, it, mu, LF)
            cov[m] = oracle.cov(K, dims[m], s, prod)
            out["norms"][it, m] = nrm
        if have_t:
            Q = np.ascontiguousarray(khatri_rao(F, tidx, 2, o))
            if it >= burnin:
                psum += mean + np.einsum("ij,ij->i", Q, F[2][np.asarray(tidx)[o, 2]])
                nadd += 1
            se, se_avg, nump = oracle.predict(K, T, F[2], Q, mean, 0 if it < burnin else it - burnin, Pavg, Pm2, nthreads=NT)
            out["rmse"].append(math.sqrt(se / nump)); out["rmse_avg"].append(math.sqrt(se_avg / nump))
    out["factors"] = F
    if have_t:
        inv = np.empty(len(o), np.int64); inv[o] = np.arange(len(o))
        out["pavg"], out["pm2"] = Pavg[inv], Pm2[inv]
        out["final_rmse_avg"] = out["rmse_avg"][-1] if nsims else float("nan")
        if nadd:
            out["pred"] = (psum / nadd)[inv]
    return out


def matrix_chain(oracle, K, rows, cols, vals, nrows, ncols, trows, tcols, tvals, nsims, burnin, alpha):
    """The matrix model on (rows, cols, vals) through the same pieces (columns first, then rows): the posterior-mean prediction per
    test entry, in the order given.  The unfolded and collapsed arms of the planted experiment."""
    from oracle.oracle import csc_from_coo, transpose_csc
    M = csc_from_coo(rows, cols, vals, nrows, ncols)
    Mt = transpose_csc(M, nrows)
    mean = float(np.sum(M[2])) / len(M[2])
    U, V = np.zeros((nrows, K)), np.zeros((ncols, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    psum, nadd = np.zeros(len(tvals)), 0
    for it in range(nsims):
        mu, LU, LF = oracle.hyper_sample(K, ncols, cov_m, it)
        s, prod, _ = oracle.sample_side(K, M, mean, alpha, U, V, it, mu, LF, nthreads=NT)
        cov_m = oracle.cov(K, ncols, s, prod)
        mu, LU, LF = oracle.hyper_sample(K, nrows, cov_u, it)
        s, prod, _ = oracle.sample_side(K, Mt, mean, alpha, V, U, it, mu, LF, nthreads=NT)
        cov_u = oracle.cov(K, nrows, s, prod)
        if it >= burnin:
            psum += mean + np.einsum("ij,ij->i", U[trows], V[tcols])
            nadd += 1
    return psum / nadd


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------

EDGE_DIMS = (12, 40, 9)
EDGE_COUNTS = (1, 15, 16, 17, 63, 64, 65)


def edge_tensor(seed=5):
    """(idx, vals, dims) over 12 x 40 x 9: in every mode the last index has no entry; indices 0 .. 6 of mode 1 have 1, 15, 16, 17, 63,
    64 and 65 entries; index 0 of mode 0 has every cell (0, j, t), 7 <= j < 39, t < 8, and one of each of those seven: 263 entries,
    which BPMF_HIP_CHUNK=16 cuts into chunks; a seeded 15 % of the remaining cells.  Values 1 .. 5, entries in a seeded order."""
    rng = np.random.default_rng(seed)
    I, J, T = EDGE_DIMS[0] - 1, EDGE_DIMS[1] - 1, EDGE_DIMS[2] - 1
    cells = []
    for j, c in enumerate(EDGE_COUNTS):
        pool = [(i, t) for i in range(I) for t in range(T) if (i, t) != (0, 0)]
        pick = rng.choice(len(pool), size=c - 1, replace=False)
        cells += [(0, j, 0)] + [(pool[q][0], j, pool[q][1]) for q in pick]
    for j in range(len(EDGE_COUNTS), J):
        for t in range(T):
            cells.append((0, j, t))
        for i in range(1, I):
            for t in range(T):
                if rng.random() < 0.15:
                    cells.append((i, j, t))
    idx = np.array(cells, np.int32)[rng.permutation(len(cells))]
    vals = rng.integers(1, 6, len(idx)).astype(np.float64)
    return idx, vals, EDGE_DIMS


def factors(K, dims, seed):
    rng = np.random.default_rng(seed)
    sigma = (2.0 / K) ** 0.25
    return [sigma * rng.standard_normal((d, K)) for d in dims]


def planted(dims, rank, frac, sd, seed, test_frac=0.2):
    """A planted rank-`rank` tensor: a seeded fraction `frac` of the cells observed with noise sd, a fifth of them held out.
    Returns (idx, vals, tidx, tvals)."""
    rng = np.random.default_rng(seed)
    F = [rng.standard_normal((d, rank)) for d in dims]
    ncell = dims[0] * dims[1] * dims[2]
    pick = rng.choice(ncell, size=int(round(frac * ncell)), replace=False)
    idx = np.stack(np.unravel_index(pick, dims), axis=1).astype(np.int32)
    y = np.einsum("ik,ik,ik->i", F[0][idx[:, 0]], F[1][idx[:, 1]], F[2][idx[:, 2]]) + sd * rng.standard_normal(len(idx))
    nt = int(round(test_frac * len(idx)))
    return idx[nt:], y[nt:], idx[:nt], y[:nt]


# The planted experiment of tests/test_tensor_host.py: posterior-mean test RMSE of (tensor chain, unfolded users x (movie, time)
# matrix, collapsed matrix with the third index ignored, mean predictor), measured with the chains above:
#   python -c "from tests import tensor_ref as R; from oracle.oracle import Oracle; print(R.planted_measure(Oracle()))"
PLANTED = dict(dims=(60, 40, 8), rank=4, frac=0.25, sd=0.3, seed=2031, K=8, nsims=60, burnin=20, alpha=2.0)


def rmse(pred, truth):
    return float(np.sqrt(np.mean((np.asarray(pred) - np.asarray(truth)) ** 2)))


def planted_measure(oracle, **over):
    P = dict(PLANTED, **over)
    dims = P["dims"]
    idx, vals, tidx, tvals = planted(dims, P["rank"], P["frac"], P["sd"], P["seed"])
    K, nsims, burnin, alpha = P["K"], P["nsims"], P["burnin"], P["alpha"]
    tensor = rmse(restate_chain(oracle, K, idx, vals, dims, tidx, tvals, nsims, burnin, alpha)["pred"], tvals)
    # unfolded: users x (movie, time), every pair a column of its own
    unfolded = rmse(matrix_chain(oracle, K, idx[:, 0], idx[:, 1] * dims[2] + idx[:, 2], vals, dims[0], dims[1] * dims[2],
                                 tidx[:, 0], tidx[:, 1] * dims[2] + tidx[:, 2], tvals, nsims, burnin, alpha), tvals)
    # collapsed: the third index dropped; cells that then coincide are averaged
    key = idx[:, 0].astype(np.int64) * dims[1] + idx[:, 1]
    uk, inv = np.unique(key, return_inverse=True)
    cv = np.bincount(inv, weights=vals) / np.bincount(inv)
    collapsed = rmse(matrix_chain(oracle, K, uk // dims[1], uk % dims[1], cv, dims[0], dims[1], tidx[:, 0], tidx[:, 1], tvals,
                                  nsims, burnin, alpha), tvals)
    return tensor, unfolded, collapsed, rmse(np.full(len(tvals), vals.mean()), tvals)
