"""Ill-conditioned inputs for the column samplers, and a dtype-generic restatement of the oracle's column update (plain numpy).

sample_columns(dtype, ...) restates sample_col of oracle/bpmf_oracle.c:358-412 for all columns of a side at once, entirely in
`dtype` (np.longdouble: the reference of tests/test_gpu_conditioning.py; np.float64: pinned to oracle.sample_side by
tests/test_cond_host.py; np.float32: the project's reference for the fp32 form, Gram summed in fp32 too):

    rr = LF mu + sum_r u_r ((r - mean) alpha)            MM = LF + alpha sum_r u_r u_r^T      (ratings in ascending row order)
    L L^T = MM  (every element: a_ij - l_i0 l_j0 - l_i1 l_j1 - ..., in that order, then / l_jj: chol_lower's own sequence)
    L y = rr,  y += z,  L^T x = y                        z = oracle.randn(((idx + 1) K (it + 1)) mod 2^32, K), K = num_latent

It is vectorised over the columns: one numpy step per rating position, per pivot and per solve row, never per element.

The input families (all seeds fixed, LambdaF symmetrised exactly, num_latent the true K):

    P(kappa)         LambdaF = Q diag(lambda) Q^T, Q from the QR of a Gaussian matrix, lambda_i = 4 kappa^(-i/(K-1));
                     U = 0.3 N(0,1), mu = 0.3 N(0,1), alpha = 2
    D(s, eps, alpha) LambdaF of P(10); row r of U = s (v + eps g_r) with ONE Gaussian v: a heavy column's Gram is nearly rank
                     one and much larger than the prior
    S(k, kappa)      P(kappa) with LambdaF and alpha both times 4^k: the posterior mean is unchanged, the noise scales by 2^-k

In fp32 U, mu and LambdaF are rounded to fp32 first and LambdaF is symmetrised again (the project's fp32 convention: the
references see the inputs the device sees).
"""
import numpy as np

IT = 3

# (id, family tuple)
FP64_CASES = [("P1e3", ("P", 1e3)), ("P1e6", ("P", 1e6)), ("P1e9", ("P", 1e9)),
              ("D-3-1e-1-100", ("D", 3.0, 1e-1, 100.0)), ("D-3-1e-3-100", ("D", 3.0, 1e-3, 100.0)),
              ("S-20", ("S", -20, 1e3)), ("S+20", ("S", 20, 1e3))]
FP32_CASES = [("P1e1", ("P", 1e1)), ("P1e2", ("P", 1e2)), ("P1e3", ("P", 1e3)), ("P1e4", ("P", 1e4)),
              ("D-0.3-0.1-2", ("D", 0.3, 0.1, 2.0)), ("D-1-0.1-8", ("D", 1.0, 0.1, 8.0)),
              ("S-20", ("S", -20, 1e2)), ("S+20", ("S", 20, 1e2))]
SINGULAR = ("P1e18", ("P", 1e18))
KAPPA_MAX = 1e12                                                      # kappa_2(Lambda*) of every column of every fp64 case
EPS = {np.float32: float(np.finfo(np.float32).eps), np.float64: float(np.finfo(np.float64).eps)}

_ORACLE = []
_CACHE = {}


def cases(f32):
    return FP32_CASES if f32 else FP64_CASES


def is_D(case):
    return case[1][0] == "D"


def _oracle():
    if not _ORACLE:
        from oracle.oracle import Oracle
        _ORACLE.append(Oracle())
    return _ORACLE[0]


def _prior(K, kappa, seed):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((K, K)))[0]
    lam = 4.0 * kappa ** (-np.arange(K) / (K - 1.0))
    LF = (Q * lam) @ Q.T
    return 0.5 * (LF + LF.T)


def inputs(case, K, nrows, f32=False):
    """(U [nrows, K], it, alpha, mu, LambdaF) of a case, as _launch of tests/test_gpu_schedule_edges.py takes them.  Cached,
    read-only."""
    key = ("in", case[0], case[1], K, nrows, f32)
    if key in _CACHE:
        return _CACHE[key]
    fam = case[1]
    rng = np.random.default_rng([K, nrows, 20261])
    g = rng.standard_normal((nrows, K))
    mu = 0.3 * rng.standard_normal(K)
    v = rng.standard_normal(K)
    if fam[0] == "P":
        U, alpha, LF = 0.3 * g, 2.0, _prior(K, fam[1], 7 * K + 1)
    elif fam[0] == "D":
        s, eps, alpha = fam[1:]
        U, LF = s * (v[None, :] + eps * g), _prior(K, 10.0, 7 * K + 1)
    else:
        k, kappa = fam[1:]
        U, alpha, LF = 0.3 * g, 2.0 * 4.0 ** k, _prior(K, kappa, 7 * K + 1) * 4.0 ** k       # exact: powers of two
    if f32:
        U = U.astype(np.float32).astype(np.float64)
        mu = mu.astype(np.float32).astype(np.float64)
        LF = LF.astype(np.float32).astype(np.float64)
        LF = 0.5 * (LF + LF.T)                                        # (exact: rounding kept the symmetry, the mean of a pair is the pair)
        assert np.array_equal(LF, LF.astype(np.float32))
    assert np.array_equal(LF, LF.T)
    for a in (U, mu, LF):
        a.setflags(write=False)
    _CACHE[key] = (U, IT, float(alpha), mu, LF)
    return _CACHE[key]


def sample_columns(dtype, K, csc, mean, alpha, U, mu, LF, it, oracle=None):
    """All columns of a side in `dtype`: returns (x [ncols, K] as dtype, ok [ncols] -- every pivot > 0).  x of a column whose
    factorisation failed is NaN."""
    oracle = oracle or _oracle()
    T = np.dtype(dtype).type
    colptr, rowidx, vals = csc
    ncols = len(colptr) - 1
    counts = np.diff(colptr)
    Ud = np.asarray(U).astype(dtype)
    LFd = np.asarray(LF).astype(dtype)
    mud = np.asarray(mu).astype(dtype)
    alpha_d, mean_d = T(alpha), T(mean)
    vals_d = np.asarray(vals).astype(dtype)

    lmu = np.zeros(K, dtype)
    for j in range(K):                                                # s += LF[i, j] mu[j], ascending j
        lmu = lmu + LFd[:, j] * mud[j]
    rr = np.tile(lmu, (ncols, 1))
    G = np.zeros((ncols, K, K), dtype)
    for t in range(int(counts.max()) if ncols else 0):               # the t-th rating of every column that has one
        cols = np.nonzero(counts > t)[0]
        p = colptr[cols] + t
        u = Ud[rowidx[p]]
        w = (vals_d[p] - mean_d) * alpha_d
        G[cols] += u[:, :, None] * u[:, None, :]
        rr[cols] += u * w[:, None]
    A = LFd[None, :, :] + alpha_d * G

    ok = np.ones(ncols, bool)
    L = np.zeros((ncols, K, K), dtype)
    with np.errstate(all="ignore"):
        for j in range(K):                                            # right-looking: element (i, j) has had l_ik l_jk, k < j, taken off
            d = A[:, j, j]
            ok &= d > 0
            d = np.sqrt(np.where(d > 0, d, T(1)))
            L[:, j, j] = d
            l = A[:, j + 1:, j] / d[:, None]
            L[:, j + 1:, j] = l
            A[:, j + 1:, j + 1:] -= l[:, :, None] * l[:, None, :]
        y = rr
        for j in range(K):                                            # L y = rr
            y[:, j] = y[:, j] / L[:, j, j]
            y[:, j + 1:] -= L[:, j + 1:, j] * y[:, j][:, None]
        z = np.empty((ncols, K))
        for c in range(ncols):
            z[c] = oracle.randn(((c + 1) * K * (it + 1)) % (1 << 32), K)
        y = y + z.astype(dtype)
        for j in range(K - 1, -1, -1):                                # L^T x = y
            y[:, j] = y[:, j] / L[:, j, j]
            y[:, :j] -= L[:, j, :j] * y[:, j][:, None]
    y[~ok] = np.nan
    return y, ok


def posterior_precisions(K, csc, alpha, U, LF):
    """Lambda* = LF + alpha sum u u^T of every column, in fp64 (for the condition numbers only)."""
    colptr, rowidx, _ = csc
    out = np.empty((len(colptr) - 1, K, K))
    for c in range(len(colptr) - 1):
        u = U[rowidx[colptr[c]:colptr[c + 1]]]
        out[c] = LF + alpha * (u.T @ u)
    return out


def col_err(x, x_ld):
    """e(c) = max_k |x(c,k) - x_ld(c,k)| / max_k |x_ld(c,k)|, in longdouble."""
    x_ld = np.asarray(x_ld, np.longdouble)
    d = np.abs(np.asarray(x).astype(np.longdouble) - x_ld).max(axis=1)
    return (d / np.abs(x_ld).max(axis=1)).astype(np.float64)


def references(key, K, csc, mean, nrows, case, f32=False, oracle=None):
    """For one (matrix, K, case, dtype): the inputs, x_ld (longdouble restatement on the inputs the device sees) and e_ref(c) of
    the project's reference for that dtype -- oracle.sample_side in fp64, the restatement at np.float32 in fp32 -- with its
    success flags.  Computed once per key, shared, never written."""
    key = ("ref", key, K, case[0], case[1], f32)
    if key in _CACHE:
        return _CACHE[key]
    oracle = oracle or _oracle()
    inp = inputs(case, K, nrows, f32)
    U, it, alpha, mu, LF = inp
    ncols = len(csc[0]) - 1
    x_ld, ok_ld = sample_columns(np.longdouble, K, csc, mean, alpha, U, mu, LF, it, oracle)
    if f32:
        x_ref, ok_ref = sample_columns(np.float32, K, csc, mean, alpha, U, mu, LF, it, oracle)
    else:
        x_ref = np.zeros((ncols, K))
        try:
            oracle.sample_side(K, csc, mean, alpha, U, x_ref, it, mu, LF)
            ok_ref = np.ones(ncols, bool)
        except RuntimeError:                                          # (reports one column; which others failed is not known)
            ok_ref = np.zeros(ncols, bool)
    with np.errstate(all="ignore"):
        e_ref = col_err(x_ref, x_ld) if ok_ld.all() else np.full(ncols, np.nan)
    for a in (x_ld, e_ref, ok_ld, ok_ref):
        a.setflags(write=False)
    _CACHE[key] = dict(inputs=inp, x_ld=x_ld, ok_ld=ok_ld, ok_ref=ok_ref, e_ref=e_ref, x_ref=x_ref)
    return _CACHE[key]
