"""Sparse tensor factorisation (Bayesian CP of order 3): the Gibbs loop over the engine's tensor entry points."""
import math

import numpy as np

from . import engine as _engine


def tensor_gibbs(engine, idx, vals, dims, test_idx=None, test_vals=None, nsims=20, burnin=5, alpha=2.0, keep_samples=False):
    """r(i, j, t) ~ N(mean + sum_k a_ik b_jk c_tk, 1 / alpha) with a Normal-Wishart prior per mode.

    idx [nnz, 3] (0-based) / vals [nnz]: the training entries; dims: the three sizes; test_idx / test_vals: held-out entries.
    Per iteration `it`, for each mode, last mode first (the matrix loop samples the movies before the users): the hyper-parameters
    of the mode at counter `it` from its cov, engine.tensor_sample, cov from the sums; then the test evaluation with n = 0 during
    burn-in and it - burnin after it.  The mean rating is the mean of the training values.

    Returns dict(factors: three [dims[m], K] arrays, rmse, rmse_avg: one per iteration, norms [nsims, 3], pavg, pm2: per test entry
    in the order given, mean_rating, final_rmse_avg); keep_samples=True adds samples: per iteration the three factor arrays.
    fp64 engines, one GPU."""
    if getattr(engine, "dtype", "f64") == "f32":
        raise ValueError("tensor_gibbs needs an fp64 engine")
    K = engine.K
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3:
        raise ValueError("tensor_gibbs: tensors of order 3 only (dims must hold three sizes)")
    vals = np.ascontiguousarray(vals, np.float64)
    mean = float(vals.mean()) if len(vals) else 0.0
    have_t = test_idx is not None and len(test_vals) > 0
    T = engine.tensor_create(idx, vals, dims, mean)
    try:
        tt = engine.tensor_test(T, test_idx, test_vals) if have_t else None
        cov = [np.zeros((K, K)) for _ in range(3)]
        res = dict(rmse=[], rmse_avg=[], norms=np.zeros((nsims, 3)), mean_rating=mean, samples=[] if keep_samples else None)
        for it in range(nsims):
            for m in (2, 1, 0):
                mu, _, LF = _engine.hyper_sample(K, dims[m], cov[m], it)
                s, prod, nrm = engine.tensor_sample(T, m, it, alpha, mu, LF)
                cov[m] = _engine.cov_from_sums(K, dims[m], s, prod)
                res["norms"][it, m] = nrm
            if have_t:
                se, se_avg, cnt = engine.tensor_predict(tt, 0 if it < burnin else it - burnin)
                res["rmse"].append(math.sqrt(se / cnt)); res["rmse_avg"].append(math.sqrt(se_avg / cnt))
            if keep_samples:
                res["samples"].append([engine.get_items(sd) for sd in T.sides])
        res["factors"] = [engine.get_items(sd) for sd in T.sides]
        if have_t:
            res["pavg"], res["pm2"] = engine.tensor_test_get(tt)
            res["final_rmse_avg"] = res["rmse_avg"][-1] if nsims > 0 else float("nan")
        else:
            res["pavg"] = res["pm2"] = None
            res["final_rmse_avg"] = float("nan")
        if not keep_samples:
            del res["samples"]
        return res
    finally:
        engine.tensor_destroy(T)
