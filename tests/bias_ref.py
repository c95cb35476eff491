"""CPU restatement of the bias step and the inputs the GPU tests run it on.

numpy only.  The Philox4x32-10 blocks and canonical53 are those of tests/probit_ref.py (imported, not restated twice).  `step` is the
conditional of a side's biases in longdouble -- every term of S_a, the quotient, the normal -- together with the sums of magnitudes
the derived bar of tests/test_gpu_bias.py needs; `values` is what the side's samplers read, in the kernel's order of operations.  The
chain (`restate_chain`) composes the step in double with the oracle's pieces in the shape of censor_ref.restate_chain:
oracle.hyper_sample, oracle.sample_side fed z as `vals` with the side's own mean rating, oracle.cov; the evaluation is restated
here (the oracle's adds no biases).
"""
import json
import math
import os

import numpy as np

from tests import censor_ref
from tests import probit_ref
from tests import util

NT = probit_ref.NT
TAG_MOVIES, TAG_USERS = 13, 14
PIECE = 256                       # consecutive ratings of a column per piece (kernels_bias.h: kBiasPiece)
LD = np.longdouble
EPS = 2.0 ** -53


def columns(A):
    return np.repeat(np.arange(len(A[0]) - 1), np.diff(A[0]))


def normals(cols, it, tag, dtype=LD):
    """xi_a = sqrt(-2 ln u1) cos(2 pi u2) from the Philox block (a lo, a hi, it, 0; 42, tag), u1 = 1 - canonical53(w3, w2),
    u2 = canonical53(w1, w0): the normal of robust_ref.gamma_draw.  u1 and u2 are exact in double; the rest is evaluated in `dtype`."""
    a = np.asarray(cols, np.int64)
    w0, w1, w2, w3 = probit_ref.philox4x32_10((a & 0xFFFFFFFF).astype(np.uint64), (a >> 32).astype(np.uint64), it, 0, 42, tag)
    u1 = (1.0 - probit_ref.canonical53(w3, w2)).astype(dtype)
    u2 = probit_ref.canonical53(w1, w0).astype(dtype)
    two_pi = dtype(2) * (np.arctan(dtype(1)) * dtype(4))
    return np.sqrt(dtype(-2) * np.log(u1)) * np.cos(two_pi * u2)


def step(A, X, Y, c, it, tag, alpha, lam, mean, dtype=LD):
    """The biases of the side with ratings A and factors X (before its update) at iteration `it` against the factors Y and the
    biases c of the other side.  Returns dict(b, mean_part, noise_part, M, n): b = mean_part + noise_part per column in `dtype`,
    M_a the sum of the magnitudes of every term of S_a (|r - mean|, |c[row]| and every |x_k y_k| of every rating)."""
    colptr, rowidx, vals = A
    ncols = len(colptr) - 1
    cols = columns(A)
    Xl, Yl = np.asarray(X, dtype)[cols], np.asarray(Y, dtype)[rowidx]
    d = np.asarray(vals, dtype) - dtype(mean)
    cr = np.asarray(c, dtype)[rowidx]
    prods = Xl * Yl
    e = (d - cr) - prods.sum(axis=1)
    mag = np.abs(d) + np.abs(cr) + np.abs(prods).sum(axis=1)
    S, M = np.zeros(ncols, dtype), np.zeros(ncols, dtype)
    np.add.at(S, cols, e)
    np.add.at(M, cols, mag)
    n = np.diff(colptr)
    prec = dtype(lam) + dtype(alpha) * n.astype(dtype)
    mean_part = dtype(alpha) * S / prec
    noise_part = normals(np.arange(ncols), it, tag, dtype) / np.sqrt(prec)
    return dict(b=mean_part + noise_part, mean_part=mean_part, noise_part=noise_part, M=M, n=n)


def lambda_draw(b, it, tag, a0, b0, dtype=LD):
    """lambda ~ Gamma(a0 + N / 2, rate b0 + sum b^2 / 2) as k_bias_lambda draws it: g ~ Gamma(a, 1) from robust_ref.gamma_draw
    (Marsaglia-Tsang, decision for decision) on the Philox blocks of the position -1 (both counter words all ones), lambda = g / rate.
    Returns (lambda, attempts, margin of the closest decision)."""
    from tests import robust_ref
    b = np.asarray(b, dtype)
    g, attempts, margin = robust_ref.gamma_draw(np.array([-1], np.int64), it, tag, a0 + 0.5 * len(b))
    rate = dtype(b0) + dtype(0.5) * (b * b).sum()
    return dtype(g[0]) / rate, int(attempts[0]), margin


def bar(r, kt, alpha, lam):
    """The bound on |b_dev - b_ref| per column: 2 alpha (n + kt + 8) eps M / (lambda + alpha n) + 8 eps (|mean part| + |noise part|)"""
    n = r["n"].astype(np.float64)
    return (2.0 * alpha * (n + kt + 8) * EPS * r["M"].astype(np.float64) / (lam + alpha * n)
            + 8.0 * EPS * (np.abs(r["mean_part"]) + np.abs(r["noise_part"])).astype(np.float64))


def values(A, b, c):
    """z_p = (r_p - b[col p]) - c[row p] in double, in that order"""
    t = np.asarray(A[2], np.float64) - np.asarray(b, np.float64)[columns(A)]
    return t - np.asarray(c, np.float64)[A[1]]


def dots(T, X, Y):
    return np.einsum("ij,ij->i", X[columns(T)], Y[T[1]])


# ---- the inputs of the GPU step tests ---------------------------------------------------------------------------------------------------

LIGHT = 16                        # ratings up to which a column has no piece (kernels_bias.h: kBiasLight)
EDGE_COUNTS = (0, 1, LIGHT, LIGHT + 1, 63, 64, 65, 255, 256, 257, 3 * PIECE + 1)
EDGE_ROWS = 800


def edge_side(seed=7):
    """(A, nrows): the 33 columns of censor_ref.edge_side (0 .. 40 ratings, rows below 64) and behind them one column each of 0, 1, 16,
    17, 63, 64, 65, 255, 256, 257 and 3 x piece + 1 ratings over 800 rows: the last column without a piece and the first with one,
    every piece boundary, and a column of four pieces."""
    (cp, ri, v), _ = censor_ref.edge_side(seed)
    rng = np.random.default_rng(seed + 1)
    extra = [np.sort(rng.choice(EDGE_ROWS, size=n, replace=False)).astype(np.int32) for n in EDGE_COUNTS]
    colptr = np.concatenate([cp, cp[-1] + np.cumsum([len(x) for x in extra])]).astype(np.int64)
    rowidx = np.concatenate([ri] + extra).astype(np.int32)
    vals = np.concatenate([v, rng.integers(1, 6, len(rowidx) - len(v)).astype(np.float64)])
    return (colptr, rowidx, vals), EDGE_ROWS


def factors(K, ncols, nrows, seed=0):
    """Random factors scaled so that x . y has standard deviation 1"""
    rng = np.random.default_rng(2800 + K + seed)
    sigma = (1.0 / K) ** 0.25
    return rng.standard_normal((ncols, K)) * sigma, rng.standard_normal((nrows, K)) * sigma


# ---- the chain ------------------------------------------------------------------------------------------------------------------------

def predict(T, V, U, bm, bu, mean, n, Pavg, Pm2):
    """k_predict_bias: pred = ((v . u + mean) + b_movie) + b_user, the running mean / M2 of Sys::predict (n, not n + 1)"""
    pred = ((dots(T, V, U) + mean) + bm[columns(T)]) + bu[T[1]]
    se = float(np.sum((T[2] - pred) ** 2))
    if n == 0:
        Pavg[:] = pred
        Pm2[:] = 0.0
    else:
        delta = pred - Pavg
        Pavg += delta / n
        Pm2 += delta * (pred - Pavg)
    return se, float(np.sum((T[2] - Pavg) ** 2)), len(T[2]), pred


def restate_chain(oracle, K, M, Mt, T, lam, nsims, burnin, alpha, prior=None):
    """gibbs(..., bias=lam) from oracle pieces.  Per iteration and side: the bias step in double from the factors the side holds, the
    other side's newest factors and biases; hyper draw at counter it; oracle.sample_side with vals = z; cov.  lam = None: the plain
    chain.  prior = (A0, B0): either side's lambda is redrawn from its own biases ahead of every step but its first (out["lam_m"],
    out["lam_u"]: the precision every iteration's step ran with).  out["pred"]: the mean over the post-burn-in samples of the prediction per test entry."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    U, V = np.zeros((nu, K)), np.zeros((nm, K))
    bm, bu = np.zeros(nm), np.zeros(nu)
    bm_sum, bu_sum = np.zeros(nm), np.zeros(nu)
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    Pavg, Pm2 = T[2].copy(), T[2].copy()
    psum, nadd = np.zeros(len(T[2])), 0
    out = dict(rmse=[], rmse_avg=[], lam_m=[], lam_u=[], margin=math.inf)
    lam_m = lam_u = lam
    for it in range(nsims):
        zm = M[2]
        if lam is not None:
            if prior is not None and it > 0:
                lam_m, _, mg = lambda_draw(bm, it, TAG_MOVIES, prior[0], prior[1], np.float64)
                out["margin"] = min(out["margin"], mg)
            out["lam_m"].append(float(lam_m))
            bm = step(M, V, U, bu, it, TAG_MOVIES, alpha, lam_m, mean_m, np.float64)["b"]
            zm = values(M, bm, bu)
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        s, prod, _ = oracle.sample_side(K, (M[0], M[1], zm), mean_m, alpha, U, V, it, mu, LF, nthreads=NT)
        cov_m = oracle.cov(K, nm, s, prod)
        zu = Mt[2]
        if lam is not None:
            if prior is not None and it > 0:
                lam_u, _, mg = lambda_draw(bu, it, TAG_USERS, prior[0], prior[1], np.float64)
                out["margin"] = min(out["margin"], mg)
            out["lam_u"].append(float(lam_u))
            bu = step(Mt, U, V, bm, it, TAG_USERS, alpha, lam_u, mean_u, np.float64)["b"]
            zu = values(Mt, bu, bm)
        mu, LU, LF = oracle.hyper_sample(K, nu, cov_u, it)
        s, prod, _ = oracle.sample_side(K, (Mt[0], Mt[1], zu), mean_u, alpha, V, U, it, mu, LF, nthreads=NT)
        cov_u = oracle.cov(K, nu, s, prod)
        if it >= burnin:
            bm_sum += bm; bu_sum += bu
        se, se_avg, nump, pred = predict(T, V, U, bm, bu, mean_m, 0 if it < burnin else it - burnin, Pavg, Pm2)
        if it >= burnin:
            psum += pred; nadd += 1
        out["rmse"].append(math.sqrt(se / nump)); out["rmse_avg"].append(math.sqrt(se_avg / nump))
    if nsims > 0:                                                    # movies.predict(users, true) once more (c++/bpmf.cpp:242)
        it = nsims - 1
        se, se_avg, nump, _ = predict(T, V, U, bm, bu, mean_m, 0 if it < burnin else it - burnin, Pavg, Pm2)
        out["final_rmse_avg"] = math.sqrt(se_avg / nump)
    out["U"], out["V"], out["bm"], out["bu"] = U, V, bm, bu
    kept = max(nsims - burnin, 0)
    out["bm_mean"], out["bu_mean"] = (bm_sum / kept, bu_sum / kept) if kept else (bm_sum, bu_sum)
    if nadd:
        out["pred"] = psum / nadd
    return out


# ---- the planted experiment -------------------------------------------------------------------------------------------------------------

PLANTED = dict(nusers=600, nmovies=300, rank=4, per_user=8, ntest=6000, alpha=4.0, spread=1.0, seed=2028, K=8, nsims=60, burnin=30, lam=1.0)
PLANTED_FILE = os.path.join(util.GOLDEN, "bias_planted.json")


def planted_data(nusers, nmovies, rank, per_user, ntest, alpha, spread, seed, **_):
    """y = b_u + c_m + u . v + eps: u, v ~ N(0, I_rank / sqrt(rank)), b, c ~ N(0, spread^2), eps ~ N(0, 1 / alpha); per_user training
    cells per user, ntest held-out cells elsewhere.  Returns (M, Mt, T, Tt)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    Ut, Vt = rng.standard_normal((nusers, rank)) / rank ** 0.25, rng.standard_normal((nmovies, rank)) / rank ** 0.25
    bu, bm = spread * rng.standard_normal(nusers), spread * rng.standard_normal(nmovies)
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
    sd = 1.0 / math.sqrt(alpha)

    def cells(r, c):
        return bu[r] + bm[c] + np.einsum("ij,ij->i", Ut[r], Vt[c]) + sd * rng.standard_normal(len(r))

    def csc(r, c, v):                                                # (+ 100: no value is an explicit zero for the containers)
        m = sp.coo_matrix((v + 100.0, (r, c)), shape=(nusers, nmovies)).tocsc()
        A, At = util.csc_arrays(m), util.csc_arrays(m.T)
        return (A[0], A[1], A[2] - 100.0), (At[0], At[1], At[2] - 100.0)
    M, Mt = csc(tr_r, tr_c, cells(tr_r, tr_c))
    T, Tt = csc(te_r, te_c, cells(te_r, te_c))
    return M, Mt, T, Tt


def planted_measure(oracle):
    """(test RMSE of the chain with biases, test RMSE of the plain chain): the final average RMSE of the restated chains, the figure
    gibbs returns as res["final_rmse_avg"]"""
    P = PLANTED
    M, Mt, T, Tt = planted_data(**P)
    out = []
    for lam in (P["lam"], None):
        r = restate_chain(oracle, P["K"], M, Mt, T, lam, P["nsims"], P["burnin"], P["alpha"])
        out.append(float(r["final_rmse_avg"]))
    return tuple(out)


def planted_recorded():
    with open(PLANTED_FILE) as f:
        return json.load(f)


if __name__ == "__main__":                                           # python -m tests.bias_ref: measures and prints the record
    from oracle.oracle import Oracle
    with_bias, plain = planted_measure(Oracle())
    print(json.dumps(dict(spread=PLANTED["spread"], rmse_bias=with_bias, rmse_plain=plain), indent=1))
