"""CPU reference of the stateful loop with a prior variant on, and the priors the GPU tests set.

oracle.gibbs is one C call and takes neither per-column propagated priors (-m / -l, c++/sample.cpp:157-174,272-277) nor the
diagonal-only precision (BPMF_NO_COVARIANCE, :300-304).  `gibbs` restates its loop (oracle/bpmf_oracle.c: bpmf_oracle_gibbs)
from the pieces the oracle exports -- hyper_sample at counter it, sample_side(prop_lambda= / no_covariance=) with the side's own
mean rating, cov, predict with n = it - burnin, the users' evaluation that nothing reads left out, the trailing extra predict --
in the shape of weights_ref.restate_chain.  With no variant it is oracle.gibbs (tests/test_variants_host.py).
"""
import math
import os

import numpy as np

from tests import util

NT = max(1, min(os.cpu_count() or 1, 16))

_PROP = {}


def prop_priors(ncols, K, seed):
    """[ncols, K, K]: one SPD matrix B B^T + 2 I, B = 0.2 N(0, 1), per column -- those of test_propagated_posterior_priors.
    Symmetric, so the column-major layout of *-Lambda.ddm and the oracle's transposed one are the same bytes.  Computed once per
    key, shared, never written."""
    key = (ncols, K, seed)
    if key not in _PROP:
        B = np.random.default_rng(seed).standard_normal((ncols, K, K)) * 0.2
        P = np.einsum("nij,nkj->nik", B, B) + 2.0 * np.eye(K)[None]
        P = np.ascontiguousarray(0.5 * (P + P.transpose(0, 2, 1)))    # (symmetric to the last bit)
        P.setflags(write=False)
        _PROP[key] = P
    return _PROP[key]


def gibbs(oracle, K, M, Mt, T, Tt, nsims, burnin, alpha=2.0, prop_m=None, prop_u=None, no_covariance=False, nthreads=NT):
    """oracle.gibbs(K, M, Mt, T, Tt, alpha, nsims, burnin) with per-column priors on the movies (prop_m [nmovies, K, K]) and / or
    the users (prop_u [nusers, K, K]), or with the diagonal-only precision on both sides.  Returns the keys oracle.gibbs returns
    (secs: zeros)."""
    nm, nu = len(M[0]) - 1, len(Mt[0]) - 1
    mean_m, mean_u = util.mean_rating(M), util.mean_rating(Mt)
    U, V = np.zeros((nu, K)), np.zeros((nm, K))
    cov_m, cov_u = np.zeros((K, K)), np.zeros((K, K))
    nnzt = int(T[0][-1])
    Pavg, Pm2 = np.array(T[2], np.float64), np.array(T[2], np.float64)     # Pm2 = Pavg = T (c++/sample.cpp:123,134)
    rmse, rmse_avg, norm_u, norm_m = [], [], [], []
    kw_m = dict(prop_lambda=prop_m, no_covariance=no_covariance, nthreads=nthreads)
    kw_u = dict(prop_lambda=prop_u, no_covariance=no_covariance, nthreads=nthreads)
    nump, final = 0, 0.0
    for it in range(nsims):
        mu, LU, LF = oracle.hyper_sample(K, nm, cov_m, it)
        s, prod, nrm_m = oracle.sample_side(K, M, mean_m, alpha, U, V, it, mu, LF, **kw_m)
        cov_m = oracle.cov(K, nm, s, prod)
        mu, LU, LF = oracle.hyper_sample(K, nu, cov_u, it)
        s, prod, nrm_u = oracle.sample_side(K, Mt, mean_u, alpha, V, U, it, mu, LF, **kw_u)
        cov_u = oracle.cov(K, nu, s, prod)
        n = 0 if it < burnin else it - burnin
        se, se_avg, nump = oracle.predict(K, T, V, U, mean_m, n, Pavg, Pm2, nthreads=nthreads)
        rmse.append(math.sqrt(se / nump)); rmse_avg.append(math.sqrt(se_avg / nump))
        norm_u.append(math.sqrt(nrm_u)); norm_m.append(math.sqrt(nrm_m))
        final = rmse_avg[-1]
    if nsims > 0:                                                    # movies.predict(users, true) once more (c++/bpmf.cpp:242)
        it = nsims - 1
        se, se_avg, nump = oracle.predict(K, T, V, U, mean_m, 0 if it < burnin else it - burnin, Pavg, Pm2, nthreads=nthreads)
        final = math.sqrt(se_avg / nump)
    return dict(U=U, V=V, Pavg=Pavg[:nnzt], Pm2=Pm2[:nnzt], rmse=np.array(rmse), rmse_avg=np.array(rmse_avg),
                norm_u=np.array(norm_u), norm_m=np.array(norm_m), secs=np.zeros(nsims), final_rmse_avg=float(final),
                num_predict=int(nump))
