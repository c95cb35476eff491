"""CPU restatement of side information with a SAMPLED link precision lambda_beta.

The chain is the one of tests/link_ref.py (dense F) / tests/link_sparse_ref.py (sparse F) with one more step at the START of a side's
half-iteration `it`, skipped at the side's first:

    t = |beta R^T|_F^2  (beta of the side's previous half-iteration, Lambda = R^T R the one it was drawn under)
    lambda_beta = g / (B0 + t / 2),   g = oracle.gamma_stream(BPMF_LINK_LAMBDA_COUNTER(it, tag), [A0 + D K / 2])[0][0]

and everything after it -- the scatter lambda_beta beta^T beta, G(lambda_beta), the sparse operator and sqrt(lambda_beta) -- uses the
new value.  G(lambda) goes through numpy / LAPACK every half-iteration.
"""
import math

import numpy as np

from tests import link_ref as ref
from tests import link_sparse_ref as sref
from tests import util
from tests.probit_ref import dots

NT = ref.NT
TAG_MOVIES, TAG_USERS = ref.TAG_MOVIES, ref.TAG_USERS
DEFAULT_PRIOR = (5e-4, 5e-4)


def counter(it, tag):
    """BPMF_LINK_LAMBDA_COUNTER(it, tag) of include/bpmf_hip.h"""
    return (0x80000000 + 16 * it + (tag & 15)) & 0xFFFFFFFF


def trace(beta, LU):
    """tr(Lambda beta^T beta) = |beta R^T|_F^2, Lambda = R^T R, R = LU (upper)"""
    return float(((beta @ np.triu(LU).T) ** 2).sum())


def draw_lambda(oracle, a0, b0, t, D, K, it, tag):
    g = oracle.gamma_stream(counter(it, tag), [a0 + D * K / 2.0])[0][0]
    return float(g / (b0 + t / 2.0))


class DenseLink:
    """tests/link_ref.py::Link with a lambda that moves: F^T F once, G(lambda), G^-1 and L_G^-T per set_lambda."""

    def __init__(self, F, lam):
        self.F = np.ascontiguousarray(F, np.float64)
        self.D = self.F.shape[1]
        self.FtF = self.F.T @ self.F
        self.cond = 0.0
        self.set_lambda(lam)

    def set_lambda(self, lam):
        self.lam = float(lam)
        self.G = self.FtF + self.lam * np.eye(self.D)
        self.cond = max(self.cond, float(np.linalg.cond(self.G)))
        self.Ginv = np.linalg.inv(self.G)
        self.LinvT = np.linalg.inv(np.linalg.cholesky(self.G)).T


class SparseLink(sref.SparseLink):
    def set_lambda(self, lam):
        self.lam = float(lam)
        self._G = None


def make_link(F, lam, tol=1e-6, max_iter=1000):
    if F is None:
        return None
    if hasattr(F, "tocsr"):
        return SparseLink(F, lam, tol, max_iter)
    return DenseLink(F, lam)


def half_iteration(oracle, K, A, mean, alpha, st, Y, it, tag, link=None, prior=None):
    """One half-iteration with the draw of lambda_beta in front.  st["lambda"]: the value this half-iteration used."""
    if link is not None and prior is not None and "LU" in st:            # (no "LU": the side's first half-iteration, no draw)
        t = trace(st["beta"], st["LU"])
        link.set_lambda(draw_lambda(oracle, prior[0], prior[1], t, link.D, K, it, tag))
        st["trace"] = t
    if link is not None:
        st["lambda"] = link.lam
    sref.half_iteration(oracle, K, A, mean, alpha, st, Y, it, tag, link)


def restate_chain(oracle, K, M, Mt, T, nsims, burnin, row_features=None, col_features=None, lam=5.0, alpha=2.0, predictions=False,
                  prior=None, tol=1e-6, max_iter=1000):
    """gibbs(..., lambda_beta_prior=prior) from oracle pieces (the loop of tests/link_ref.py::restate_chain).  Also returns
    lambda_rows / lambda_cols: the value each half-iteration used (None for a side without features)."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    lm, lu = make_link(col_features, lam, tol, max_iter), make_link(row_features, lam, tol, max_iter)
    sm = ref.new_state(nm, K, lm.D if lm else None)
    su = ref.new_state(nu, K, lu.D if lu else None)
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    have_t = T is not None and len(T[2]) > 0
    Pavg, Pm2 = (T[2].copy(), T[2].copy()) if have_t else (None, None)
    out = dict(rmse=[], rmse_avg=[], norm_u=[], norm_m=[], lambda_rows=[] if lu else None, lambda_cols=[] if lm else None)
    bsum_m = np.zeros_like(sm["beta"]) if lm else None
    bsum_u = np.zeros_like(su["beta"]) if lu else None
    psum, nkept = (np.zeros(len(T[2])) if have_t else None), 0
    for it in range(nsims):
        half_iteration(oracle, K, M, mean_m, alpha, sm, su["U"], it, TAG_MOVIES, lm, prior)
        half_iteration(oracle, K, Mt, mean_u, alpha, su, sm["U"], it, TAG_USERS, lu, prior)
        if lm:
            out["lambda_cols"].append(sm["lambda"])
        if lu:
            out["lambda_rows"].append(su["lambda"])
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
    dense = [l for l in (lm, lu) if isinstance(l, DenseLink)]
    out["cond"] = max(l.cond for l in dense) if dense else 1.0
    if predictions and have_t and nkept:
        out["pred"] = psum / nkept
    return out


# the planted experiment of tests/link_ref.py, run long enough for a sampled lambda_beta to come down from its early values
PLANTED = dict(ref.PLANTED, nsims=120, burnin=60)
_planted_cache = {}


def planted_runs(oracle, keys=("fixed500", "fixed5", "sampled")):
    """The restated chains of the planted experiment, each computed once per process and shared: fixed lambda_beta = 500, fixed 5,
    and sampled from a start of 500 with the default prior.  dict(data=(M, Mt, T, Tt, F, cold), fixed500=, fixed5=, sampled=)."""
    P = PLANTED
    if "data" not in _planted_cache:
        _planted_cache["data"] = ref.planted_data(**P)
    M, Mt, T, Tt, F, cold = _planted_cache["data"]
    settings = dict(fixed500=dict(lam=500.0), fixed5=dict(lam=5.0), sampled=dict(lam=500.0, prior=DEFAULT_PRIOR))
    for key in keys:
        if key not in _planted_cache:
            _planted_cache[key] = restate_chain(oracle, P["K"], M, Mt, T, P["nsims"], P["burnin"], alpha=P["alpha"], predictions=True,
                                                row_features=F, **settings[key])
    return _planted_cache
