"""CPU restatement of the weight step of Student-t noise, decision for decision, and the inputs the GPU tests
run it on.

numpy only.  The Philox4x32-10 blocks and canonical53 are those of tests/probit_ref.py (imported, not restated twice).  Nothing below
fuses a product with a sum: numpy rounds every operation on its own, and kernels_robust.h is compiled to do the same.  The chain
(`restate_chain`) is weights_ref.restate_chain with the weights of every half-iteration freshly drawn: weights_ref.
sample_side_weighted on the unchanged oracle.
"""
import math

import numpy as np

from tests import probit_ref
from tests import util
from tests import weights_ref

NT = probit_ref.NT
MAX_ATTEMPTS = 64
TAG_MOVIES, TAG_USERS = 9, 10
MARGIN = 1e-9                      # the project's bar on a decision (tests/test_censor_host.py)


def gamma_draw(p, it, tag, a):
    """g_p ~ Gamma(a, 1), a >= 1, for the rating positions p at iteration `it` on the streams `tag`: Marsaglia-Tsang without the
    squeeze test.  Returns (g, attempts, margin): margin is the closest any `v <= 0` or `ln u < bound` comparison came to its
    threshold."""
    p = np.asarray(p, np.int64)
    plo = (p & 0xFFFFFFFF).astype(np.uint64)
    phi = (p >> 32).astype(np.uint64)
    dd = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * dd)
    g = np.full(len(p), -1.0)
    attempts = np.zeros(len(p), np.int64)
    margin = math.inf
    active = np.arange(len(p))
    for n in range(MAX_ATTEMPTS):
        if len(active) == 0:
            break
        w0, w1, w2, w3 = probit_ref.philox4x32_10(plo[active], phi[active], it, 2 * n, 42, tag)
        u1 = 1.0 - probit_ref.canonical53(w3, w2)
        u2 = probit_ref.canonical53(w1, w0)
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)
        t = 1.0 + c * x
        v = (t * t) * t
        pos = v > 0.0
        w0, w1, _, _ = probit_ref.philox4x32_10(plo[active], phi[active], it, 2 * n + 1, 42, tag)
        u = 1.0 - probit_ref.canonical53(w1, w0)
        with np.errstate(invalid="ignore", divide="ignore"):
            bound = ((0.5 * (x * x) + dd) - dd * v) + dd * np.log(np.where(pos, v, 1.0))
            lu = np.log(u)
        acc = pos & (lu < bound)
        dist = np.where(pos, np.minimum(np.abs(v), np.abs(lu - bound)), np.abs(v))
        margin = min(margin, float(dist.min()))
        g[active[acc]] = (dd * v)[acc]
        attempts[active] += 1
        active = active[~acc]
    assert len(active) == 0, "the attempt cap was reached"
    return g, attempts, margin


def weights(A, X, Y, it, tag, alpha, nu, mean, full=False):
    """(sw, zw) the sampler of the side with ratings A and factors X (before its update) reads at iteration `it` against the factors
    Y:  d = r - mean;  e = d - m;  q = sqrt(alpha) e;  b = (nu + q q) / 2;  w = g / b, g ~ Gamma((nu + 1) / 2, 1);  sw = sqrt(w);
    zw = sw d.  full=True: also m, the attempts per rating and the margin of gamma_draw."""
    vals = np.asarray(A[2], np.float64)
    m = probit_ref.dots(A, X, Y)
    d = vals - mean
    e = d - m
    q = math.sqrt(float(alpha)) * e
    b = 0.5 * (nu + q * q)
    g, attempts, margin = gamma_draw(np.arange(len(vals)), it, tag, 0.5 * (nu + 1.0))
    sw = np.sqrt(g / b)
    zw = sw * d
    return (sw, zw, m, attempts, margin) if full else (sw, zw)


# ---- the inputs of the GPU weight test (tests/test_gpu_robust.py), shared with the margin check of tests/test_robust_host.py ---------

KS = (8, 10, 32, 64, 100, 128)
NUS = (1.0, 4.0, 30.0)
ALPHAS = (0.5, 2.0, 3.0)
ITER = 5
SMALL_NNZ = (0, 1, 255, 256, 257)
CHAIN = dict(nsims=8, burnin=3, alpha=1.5, nu=4.0)        # the ml-100k chains
CLI = dict(nsims=6, burnin=2, alpha=3.0, nu=4.0, K=8)     # `bpmf --robust 4` on data/tiny


def edge_side():
    """(A, nrows): the edge side of weights_ref -- 300 rows, columns of 0 .. 257 ratings: tiles of 256 ratings end inside columns and,
    with the empty column at the front, the first tile starts behind a column boundary."""
    A, nrows, _ = weights_ref.edge_side()
    return A, nrows


def small_side(nnz, nrows=300, seed=29):
    """(A, nrows): 5 columns that share nnz ratings 1 .. 5 -- the first and the last empty, 128 ratings each in the second and third,
    the rest in the fourth: an empty side, a single rating, and one tile of 256 less one, full, plus one (whose second tile starts on
    a column boundary)."""
    rng = np.random.default_rng(seed + nnz)
    c1 = min(nnz, 128)
    c2 = min(nnz - c1, 128)
    counts = np.array([0, c1, c2, nnz - c1 - c2, 0], np.int64)
    colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rowidx = (np.concatenate([np.sort(rng.choice(nrows, size=int(c), replace=False)) for c in counts]).astype(np.int32)
              if nnz else np.zeros(0, np.int32))
    return (colptr, rowidx, rng.integers(1, 6, nnz).astype(np.float64)), nrows


def factors(K, ncols, nrows, seed=0):
    """Random factors scaled so that x . y has standard deviation 1 (residuals of ratings 1 .. 5 around their mean span a few units)"""
    rng = np.random.default_rng(2000 + K + seed)
    sigma = (1.0 / K) ** 0.25
    return rng.standard_normal((ncols, K)) * sigma, rng.standard_normal((nrows, K)) * sigma


# ---- the chain ------------------------------------------------------------------------------------------------------------------------

def restate_chain(oracle, K, M, Mt, T, nu, nsims, burnin, alpha):
    """gibbs(..., robust=nu) from oracle pieces.  Per iteration and side: the weights from the factors the side holds and the other
    side's newest, hyper draw at counter it, weights_ref.sample_side_weighted with the side's own mean rating and alpha, cov.
    nu = None: the plain Gaussian chain.  out["pred"]: the mean over the post-burn-in samples of mean + v . u per test entry;
    out["weight_mean"]: the mean over them of the movies' weights (M's CSC order); out["margin"]: the smallest of gamma_draw."""
    nm, nusers = len(M[0]) - 1, len(Mt[0]) - 1
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    U, V = np.zeros((nusers, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    have_t = T is not None and len(T[2]) > 0
    Pavg, Pm2 = (T[2].copy(), T[2].copy()) if have_t else (None, None)
    psum, nadd = (np.zeros(len(T[2])) if have_t else np.zeros(0)), 0
    wsum, nkept = np.zeros(len(M[2])), 0
    out = dict(rmse=[], rmse_avg=[], margin=math.inf)
    for it in range(nsims):
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        if nu is not None:
            sw, _, _, _, mg = weights(M, V, U, it, TAG_MOVIES, alpha, nu, mean_m, full=True)
            out["margin"] = min(out["margin"], mg)
            wm = sw * sw
            s, prod, _ = weights_ref.sample_side_weighted(oracle, K, M, wm, mean_m, alpha, U, V, it, mu, LF)
        else:
            s, prod, _ = oracle.sample_side(K, M, mean_m, alpha, U, V, it, mu, LF, nthreads=NT)
        cov_m = oracle.cov(K, nm, s, prod)
        mu, LU, LF = oracle.hyper_sample(K, nusers, cov_u, it)
        if nu is not None:
            sw, _, _, _, mg = weights(Mt, U, V, it, TAG_USERS, alpha, nu, mean_u, full=True)
            out["margin"] = min(out["margin"], mg)
            s, prod, _ = weights_ref.sample_side_weighted(oracle, K, Mt, sw * sw, mean_u, alpha, V, U, it, mu, LF)
        else:
            s, prod, _ = oracle.sample_side(K, Mt, mean_u, alpha, V, U, it, mu, LF, nthreads=NT)
        cov_u = oracle.cov(K, nusers, s, prod)
        if it >= burnin and nu is not None:
            wsum += wm
            nkept += 1
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
    if nu is not None:
        out["weight_mean"] = wsum / nkept if nkept else wsum
        out["kept"] = nkept
    return out


# ---- the planted outliers -------------------------------------------------------------------------------------------------------------

# weights_ref.PLANTED's matrix (600 x 300, rank 4, 40 training cells per user, seed 2029) with noise sd 0.25 everywhere; a seeded 5 % of
# the training cells is replaced by the truth u . v + 10 or - 10.  alpha = 16 = 1 / 0.25^2 is the precision of the clean cells.
PLANTED = dict(weights_ref.PLANTED, sd_noisy=0.25, sd_clean=0.25, alpha=16.0, nu=4.0, frac=0.05, shift=10.0, outlier_seed=2031)


def planted_data(nusers, nmovies, rank, per_user, ntest, sd_clean, seed, frac, shift, outlier_seed, **_):
    """The generator of weights_ref.planted_data, draw for draw (the same cells, factors and noise), then the outliers.  Returns
    dict(M, Mt: the training matrix; T, Tt: the noise-free test cells; planted: True at the outlier cells, M's CSC order;
    mean_var: the mean noise variance of the training cells, outliers included)."""
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
    rng.random(len(tr_r))                                            # (weights_ref draws its noisy / clean split here)
    truth = np.einsum("ij,ij->i", Ut[tr_r], Vt[tr_c])
    y_tr = truth + sd_clean * rng.standard_normal(len(tr_r))
    y_te = np.einsum("ij,ij->i", Ut[te_r], Vt[te_c])
    orng = np.random.default_rng(outlier_seed)
    out = orng.random(len(tr_r)) < frac
    sign = np.where(orng.random(len(tr_r)) < 0.5, 1.0, -1.0)
    y_tr = np.where(out, truth + sign * shift, y_tr)

    def csc(r, c, v):                                                # (+ 100: no value is an explicit zero for the containers)
        m = sp.coo_matrix((v + 100.0, (r, c)), shape=(nusers, nmovies)).tocsc()
        A, At = util.csc_arrays(m), util.csc_arrays(m.T)
        return (A[0], A[1], A[2] - 100.0), (At[0], At[1], At[2] - 100.0)
    M, Mt = csc(tr_r, tr_c, y_tr)
    T, Tt = csc(te_r, te_c, y_te)
    flag = util.csc_arrays(sp.coo_matrix((out.astype(np.float64) + 1.0, (tr_r, tr_c)), shape=(nusers, nmovies)).tocsc())[2] > 1.5
    mean_var = float(np.mean(np.where(out, shift * shift, sd_clean * sd_clean)))
    return dict(M=M, Mt=Mt, T=T, Tt=Tt, planted=flag, nplanted=int(out.sum()), mean_var=mean_var)


def planted_auc(weight_mean, planted):
    """The AUC with which a SMALL posterior-mean weight identifies the planted cells"""
    return probit_ref.auc_ranks(-np.asarray(weight_mean), np.asarray(planted, np.float64))


# Measured with the restated CPU chains (tests/test_gpu_robust.py::test_planted_outliers prints the GPU's figures beside them):
#   python -c "from tests import robust_ref as R; from oracle.oracle import Oracle; print(R.planted_measure(Oracle()))"
# test RMSE of (a) Student-t noise with nu = 4 at alpha = 16, (b) Gaussian noise at alpha = 16, (c) Gaussian noise at alpha = 1 / mean
# noise variance (the best single alpha); then the AUC of (a)'s weight_mean against the planted cells
PLANTED_MEASURED = (0.12007900533217565, 4.102471177735007, 0.9837007412030032)
PLANTED_AUC = 1.0                  # (every planted cell has a smaller weight_mean than every other cell: +-10 against a noise sd of 0.25)
# (a) beats (c) by 0.864; the test asks for half of that margin
PLANTED_HALF_MARGIN = 0.5 * (PLANTED_MEASURED[2] - PLANTED_MEASURED[0])


def planted_measure(oracle):
    P = PLANTED
    d = planted_data(**P)
    out, auc = [], None
    for nu, alpha in ((P["nu"], P["alpha"]), (None, P["alpha"]), (None, 1.0 / d["mean_var"])):
        r = restate_chain(oracle, P["K"], d["M"], d["Mt"], d["T"], nu, P["nsims"], P["burnin"], alpha)
        out.append(weights_ref.planted_rmse(r["pred"], d["T"][2]))
        if nu is not None:
            auc = planted_auc(r["weight_mean"], d["planted"])
    return tuple(out), auc
