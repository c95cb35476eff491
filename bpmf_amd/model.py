"""Saved models: the kept samples of a run as a directory, written after training and loaded into another
process that serves top-N lists, ranked evaluation, blocks, fold-in and single cells without a chain.

Format version 1 (written and read by the library: include/bpmf_io.h) -- everything in the numbering of the input:
    model.txt        key value lines: bpmf_model 1, num_latent, rows, cols, samples, mean_rating, alpha, likelihood gaussian|probit,
                     probit_threshold, dtype, hyper 0|1
    U-samples.ddm    (S K) x rows,  V-samples.ddm  (S K) x cols: column c = sample 0's K values, then sample 1's, ...
    U-hyper.ddm      (1 + K + K^2) x S, and V-hyper.ddm, with hyper 1: column s = alpha_s, mu_s, Lambda_s (column-major)
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .io import BpmfIoError


def write_model(path, model):
    """Writes the dict `model` as a model directory: num_latent, rows, cols, samples, mean_rating, alpha, probit (bool),
    probit_threshold, dtype ("f64" | "f32"), U [rows, S, K], V [cols, S, K] and, for hyper 1, U_hyper = (alpha [S], mu [S, K],
    Lambda [S, K, K]) and V_hyper; U_hyper = V_hyper = None writes hyper 0."""
    lib = _lib.load_library()
    K, S, rows, cols = int(model["num_latent"]), int(model["samples"]), int(model["rows"]), int(model["cols"])
    U = np.ascontiguousarray(model["U"], np.float64); V = np.ascontiguousarray(model["V"], np.float64)
    if U.shape != (rows, S, K) or V.shape != (cols, S, K):
        raise ValueError("write_model: U must be [%d, %d, %d] and V [%d, %d, %d]" % (rows, S, K, cols, S, K))
    hyp = []
    for key in ("U_hyper", "V_hyper"):
        h = model.get(key)
        if h is None:
            hyp.append(None)
            continue
        alpha, mu, lam = (np.asarray(a, np.float64) for a in h)
        if alpha.shape != (S,) or mu.shape != (S, K) or lam.shape != (S, K, K):
            raise ValueError("write_model: %s must be (alpha [%d], mu [%d, %d], Lambda [%d, %d, %d])" % (key, S, S, K, S, K, K))
        # one column per sample: alpha, mu, Lambda column-major
        hyp.append(np.ascontiguousarray(np.concatenate([alpha[:, None], mu, np.transpose(lam, (0, 2, 1)).reshape(S, K * K)], axis=1)))
    if (hyp[0] is None) != (hyp[1] is None):
        raise ValueError("write_model: U_hyper and V_hyper are given together or not at all")
    rc = lib.bpmf_io_write_model(str(path).encode(), K, rows, cols, S, float(model["mean_rating"]), float(model["alpha"]),
                                 1 if model.get("probit") else 0, float(model.get("probit_threshold", 0.0)),
                                 1 if model.get("dtype", "f64") == "f32" else 0, U.ctypes.data, V.ctypes.data,
                                 hyp[0].ctypes.data if hyp[0] is not None else None, hyp[1].ctypes.data if hyp[1] is not None else None)
    if rc:
        raise BpmfIoError(lib.bpmf_io_last_error().decode("utf-8", "replace"))


def read_model(path):
    """The dict write_model takes, from a model directory.  Refused with BpmfIoError in one line that names the file and the reason: an
    unknown version, a missing file, a row count that is not S K, unequal S between the files, a value that is not finite."""
    lib = _lib.load_library()
    ints = np.zeros(7, np.int64); reals = np.zeros(3)
    ptr = [_lib.c_f64p() for _ in range(4)]
    rc = lib.bpmf_io_read_model(str(path).encode(), ints.ctypes.data, reals.ctypes.data, *[C.byref(p) for p in ptr])
    if rc:
        raise BpmfIoError(lib.bpmf_io_last_error().decode("utf-8", "replace"))
    K, rows, cols, S, probit, f32, hyper = (int(v) for v in ints)
    try:
        U = np.ctypeslib.as_array(ptr[0], shape=(rows, S, K)).copy()
        V = np.ctypeslib.as_array(ptr[1], shape=(cols, S, K)).copy()
        hyp = [None, None]
        if hyper:
            for i in (0, 1):
                h = np.ctypeslib.as_array(ptr[2 + i], shape=(S, 1 + K + K * K)).copy()
                hyp[i] = (h[:, 0].copy(), h[:, 1:1 + K].copy(), np.ascontiguousarray(np.transpose(h[:, 1 + K:].reshape(S, K, K), (0, 2, 1))))
    finally:
        for p in ptr:
            if p:
                lib.bpmf_io_free(p)
    return dict(num_latent=K, rows=rows, cols=cols, samples=S, mean_rating=float(reals[0]), alpha=float(reals[1]), probit=bool(probit),
                probit_threshold=float(reals[2]), dtype="f32" if f32 else "f64", U=U, V=V, U_hyper=hyp[0], V_hyper=hyp[1])


def save_model(res, path):
    """Writes the kept samples of the run `res` = gibbs(...) as a model directory.  The run must have kept the sample rings of both
    sides (save_model=, topn=, foldin= or rank_eval=); the hyper-parameters are stored when both sides kept theirs (save_model= of a
    Gaussian run, foldin=True without features).  The engine of the run must still be open."""
    write_model(path, _run_model("save_model", res))


def _run_model(who, res):
    """the dict write_model takes, read back from the rings of the run `res`"""
    if not isinstance(res, dict) or "users" not in res or "movies" not in res:
        raise ValueError("%s needs the result of gibbs(...)" % who)
    users, movies = res["users"], res["movies"]
    info = res.get("model_info")
    if info is None:
        raise ValueError("%s: the result carries no model_info (it comes from gibbs or load_model)" % who)
    if not info.get("plain", True):
        raise ValueError("%s: %s" % (who, info["why"]))
    engine = users.engine
    S = engine.samples_count(users.side)
    if S < 1 or engine.samples_count(movies.side) != S:
        raise ValueError("%s: the run kept no samples of both sides (gibbs(save_model=DIR), or topn / foldin / rank_eval)" % who)
    hyper = engine.hyper_count(users.side) == S and engine.hyper_count(movies.side) == S
    return dict(num_latent=engine.K, rows=users.num(), cols=movies.num(), samples=S, mean_rating=movies.mean_rating,
                alpha=info["alpha"], probit=info["probit"], probit_threshold=info["probit_threshold"],
                dtype=getattr(engine, "dtype", "f64"), U=engine.samples_get(users.side), V=engine.samples_get(movies.side),
                U_hyper=engine.hyper_get(users.side) if hyper else None, V_hyper=engine.hyper_get(movies.side) if hyper else None)


def pool_models(models):
    """One model from the chains `models`: each the dict of read_model, or a run gibbs(...) that kept its
    rings.  U, V and the hyper arrays are concatenated along the sample axis in the order given, "samples" counts them all and
    "chains" says how many chains they are -- everything that reads rings serves the pool as it serves one chain, and
    bpmf_amd.diagnose takes the multi-chain estimator.  ValueError: chains that differ in shape, num_latent, likelihood, mean rating,
    dtype, samples or presence of the hyper-parameters; two chains whose first kept sample of U is byte-identical (the same chain
    twice: gibbs(chain=) or bpmf --chain was forgotten)."""
    ms = [_run_model("pool_models", m) if not isinstance(m, dict) or "users" in m else m for m in models]   # (a run has "users" and "movies")
    if not ms:
        raise ValueError("pool_models: no chain given")
    first = ms[0]
    for c, m in enumerate(ms[1:], 1):
        for key, what in (("rows", "shape"), ("cols", "shape"), ("num_latent", "num_latent"), ("probit", "likelihood"),
                          ("probit_threshold", "likelihood"), ("mean_rating", "mean rating"), ("dtype", "dtype"), ("samples", "samples")):
            if m[key] != first[key]:
                raise ValueError("pool_models: chain %d differs from chain 0 in %s (%s: %r, not %r)" % (c, what, key, m[key], first[key]))
        if (m["U_hyper"] is None) != (first["U_hyper"] is None) or (m["V_hyper"] is None) != (first["V_hyper"] is None):
            raise ValueError("pool_models: chain %d differs from chain 0 in the presence of the hyper-parameters" % c)
    heads = [np.ascontiguousarray(m["U"][:, 0, :], np.float64).tobytes() for m in ms]
    for c in range(1, len(ms)):
        if heads[c] in heads[:c]:
            raise ValueError("pool_models: chain %d has the first kept sample of chain %d, byte for byte: the same chain twice "
                             "(gibbs(chain=c) / bpmf --chain c makes them differ)" % (c, heads[:c].index(heads[c])))
    out = dict(first)
    out["U"] = np.concatenate([np.asarray(m["U"], np.float64) for m in ms], axis=1)
    out["V"] = np.concatenate([np.asarray(m["V"], np.float64) for m in ms], axis=1)
    for key in ("U_hyper", "V_hyper"):
        out[key] = None if first[key] is None else tuple(np.concatenate([np.asarray(m[key][j], np.float64) for m in ms], axis=0) for j in range(3))
    out["samples"] = first["samples"] * len(ms)
    out["chains"] = len(ms)
    return out


def load_model(engine, path, M=None):
    """Loads a model directory -- or, given a list of directories, the pool of those chains (pool_models, in list order; the dict
    then has "chains") -- into `engine` (its num_latent must be the model's) and returns a dict with "users", "movies" and
    "foldin" like gibbs's result: bpmf_amd.fold_in, engine.topn, topn_scored, rank_eval, predict_block and bpmf_amd.predict_cells
    work on it unchanged, with res["movies"].mean_rating as the mean rating.  M: the training matrix as gibbs takes it (CSC, one
    column per movie), whose cells the rankings exclude; None: no cell is excluded.  No chain runs."""
    if isinstance(path, (list, tuple)):
        return _load(engine, pool_models([read_model(p) for p in path]), M)
    return _load(engine, read_model(path), M)


def _load(engine, m, M=None):
    """load_model of the dict `m` of read_model / pool_models"""
    from scipy import sparse as sp
    from .sys import Sys
    if engine.K != m["num_latent"]:
        raise ValueError("load_model: the engine has num_latent %d, the model %d" % (engine.K, m["num_latent"]))
    rows, cols, S = m["rows"], m["cols"], m["samples"]
    if M is None:
        M = (np.zeros(cols + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    M = (np.ascontiguousarray(M[0], np.int64), np.ascontiguousarray(M[1], np.int32), np.ascontiguousarray(M[2], np.float64))
    if len(M[0]) != cols + 1 or (len(M[1]) and int(M[1].max()) >= rows):
        raise ValueError("load_model: the training matrix does not have the model's shape %d x %d" % (rows, cols))
    A = sp.csc_matrix((M[2], M[1], M[0]), shape=(rows, cols))
    At = A.T.tocsc(); At.sort_indices()
    Mt = (At.indptr.astype(np.int64), At.indices.astype(np.int32), At.data.astype(np.float64))
    movies = Sys("movs", engine, M, cols, rows, mean_rating=m["mean_rating"])
    users = Sys("users", engine, Mt, rows, cols, mean_rating=m["mean_rating"])
    for sd, key in ((users, "U"), (movies, "V")):
        engine.samples_reserve(sd.side, S)
        engine.samples_set(sd.side, m[key])
    foldin = m["U_hyper"] is not None and not m["probit"]
    if foldin:
        for sd, key in ((users, "U_hyper"), (movies, "V_hyper")):
            alpha, mu, lam = m[key]
            engine.hyper_reserve(sd.side, S)
            for s in range(S):
                engine.hyper_add(sd.side, alpha[s], mu[s], lam[s])
    info = dict(alpha=m["alpha"], probit=m["probit"], probit_threshold=m["probit_threshold"], plain=True, dtype=m["dtype"], samples=S,
                nu=None, alpha_samples=[float(a) for a in m["U_hyper"][0]] if foldin else None)   # (score_cells: the format stores no nu)
    res = dict(users=users, movies=movies, foldin=foldin, model_info=info)
    if "chains" in m:
        res["chains"] = int(m["chains"])
    return res


def run_chains(engine, M, Mt, T, nusers, nmovies, chains=4, **gibbs_kwargs):
    """Runs gibbs(chain=c, keep_rings=True, **gibbs_kwargs) for c = 0 .. chains - 1 one after the other on `engine` and returns the
    pool (pool_models, loaded as load_model loads it: "users", "movies", "foldin", "model_info", "chains") with "per_chain": per
    chain dict(chain, rmse, rmse_avg, final_rmse, final_rmse_avg).  What goes with chain= goes here (gibbs's docstring); every chain
    needs nsims > burnin.  The sides of the single chains are destroyed once their samples are read back."""
    from .sys import gibbs
    chains = int(chains)
    if not 1 <= chains <= 64:
        raise ValueError("run_chains: chains must be 1 .. 64, not %r" % (chains,))
    for key in ("chain", "keep_rings"):
        if key in gibbs_kwargs:
            raise ValueError("run_chains sets %s itself" % key)
    models, per_chain = [], []
    for c in range(chains):
        r = gibbs(engine, M, Mt, T, nusers, nmovies, chain=c, keep_rings=True, **gibbs_kwargs)
        models.append(_run_model("run_chains", r))
        per_chain.append(dict(chain=c, rmse=list(r["rmse"]), rmse_avg=list(r["rmse_avg"]), final_rmse=r.get("final_rmse"),
                              final_rmse_avg=r.get("final_rmse_avg")))
        engine.side_destroy(r["users"].side); engine.side_destroy(r["movies"].side)
    pool = _load(engine, pool_models(models), M)
    pool["chains"] = chains
    pool["per_chain"] = per_chain
    return pool


def predict_cells(res, rows, cols, threshold=None):
    """Predictions for the cells (rows[i], cols[i]) -- user, movie, 0-based -- from the kept samples of `res` (gibbs with the rings kept,
    or load_model): dict(mean, std), [n] each, std without the observation noise 1 / alpha.  threshold=t adds "prob", the posterior
    probability that a rating exceeds t with sigma = 1 / sqrt(alpha); a probit model always has it, with t = 0 unless given and
    sigma = 1 (the probability of a positive label)."""
    users, movies = res["users"], res["movies"]
    info = res.get("model_info") or {}
    probit = bool(info.get("probit"))
    if threshold is None and probit:
        threshold = 0.0
    if threshold is not None:
        if not math.isfinite(float(threshold)):
            raise ValueError("predict_cells: the threshold must be finite")
        alpha = float(info.get("alpha", float("nan")))
        if not probit and not (alpha > 0 and math.isfinite(alpha)):
            raise ValueError("predict_cells: the threshold needs the alpha of the run (sigma = 1 / sqrt(alpha))")
        sigma = 1.0 if probit else 1.0 / math.sqrt(alpha)
        mean, std, prob = users.engine.predict_cells(users.side, movies.side, movies.mean_rating, rows, cols, float(threshold), sigma)
        return dict(mean=mean, std=std, prob=prob)
    mean, std = users.engine.predict_cells(users.side, movies.side, movies.mean_rating, rows, cols)
    return dict(mean=mean, std=std)


def diag_summary(d):
    """What one line says of the per-cell diagnostics `d` = dict(std, rhat, ess) (engine.diag_cells, res["diag"]): n (cells), n_nan
    (cells whose rhat or ess is NaN: a constant trace), samples (d["samples"] if given, else None), ess_min, ess_median,
    rhat_median, rhat_max, rhat_above (the share of cells with rhat > 1.01) and mcse_over_std_median, the median of
    mcse / std = 1 / sqrt(ess) with mcse = std / sqrt(ess) the Monte-Carlo standard error of the mean.  NaNs are left out and
    counted; without a cell left every figure is NaN.
    The dict of the multi-chain estimator (rhat, ess_bulk, ess_tail: engine.diag_cells_mc, diagnose of a pool or with rank=True;
    DESIGN.md section 33) gives the same keys with ess = ess_bulk and rhat the rank-normalised one, and adds chains, ess_bulk_min,
    ess_bulk_median, ess_tail_min, ess_tail_median; a cell with a NaN in any of the three is left out and counted."""
    mc = "ess_bulk" in d
    rhat = np.asarray(d["rhat"], np.float64); ess = np.asarray(d["ess_bulk" if mc else "ess"], np.float64)
    ok = ~(np.isnan(rhat) | np.isnan(ess))
    if mc:
        tail = np.asarray(d["ess_tail"], np.float64)
        ok &= ~np.isnan(tail)
    r, e = rhat[ok], ess[ok]
    nan = float("nan")
    have = len(r) > 0
    s = dict(n=int(len(rhat)), n_nan=int(len(rhat) - len(r)), samples=d.get("samples"),
             ess_min=float(e.min()) if have else nan, ess_median=float(np.median(e)) if have else nan,
             rhat_median=float(np.median(r)) if have else nan, rhat_max=float(r.max()) if have else nan,
             rhat_above=float(np.mean(r > 1.01)) if have else nan,
             mcse_over_std_median=float(np.median(1.0 / np.sqrt(e))) if have else nan)
    if mc:
        t = tail[ok]
        s.update(chains=d.get("chains"), ess_bulk_min=s["ess_min"], ess_bulk_median=s["ess_median"],
                 ess_tail_min=float(t.min()) if have else nan, ess_tail_median=float(np.median(t)) if have else nan)
    return s


def diagnose(res, rows, cols, rank=None):
    """Convergence diagnostics of the predictions of the cells (rows[i], cols[i]) -- user, movie, 0-based -- over the kept samples of
    `res` (gibbs with the rings kept, or load_model; 8 .. 4096 samples): dict(rows, cols, mean, std, rhat, ess, mcse, samples, summary)
    with mean and std as predict_cells gives them, rhat and ess the split-Rhat and the effective sample size of the cell's trace
    (DESIGN.md section 29), mcse = std / sqrt(ess) and summary = diag_summary of it.
    A pool of chains (res["chains"] > 1: run_chains, load_model of a list) or rank=True takes the rank-normalised multi-chain
    estimator (one chain: C = 1) instead: dict(rows, cols, mean, std, rhat, ess_bulk, ess_tail, mcse, chains,
    samples, summary) with mcse = std / sqrt(ess_bulk); every chain needs 8 samples or more, all of them 4096 at most."""
    users, movies = res["users"], res["movies"]
    rows = np.ascontiguousarray(rows, np.int32); cols = np.ascontiguousarray(cols, np.int32)
    chains = int(res.get("chains", 1))
    if chains > 1 or rank:
        d = users.engine.diag_cells_mc(users.side, movies.side, movies.mean_rating, rows, cols, chains)
        d.update(rows=rows, cols=cols, chains=chains, samples=users.engine.samples_count(users.side))
        with np.errstate(invalid="ignore", divide="ignore"):
            d["mcse"] = d["std"] / np.sqrt(d["ess_bulk"])
        d["summary"] = diag_summary(d)
        return d
    d = users.engine.diag_cells(users.side, movies.side, movies.mean_rating, rows, cols)
    d.update(rows=rows, cols=cols, samples=users.engine.samples_count(users.side))
    with np.errstate(invalid="ignore", divide="ignore"):
        d["mcse"] = d["std"] / np.sqrt(d["ess"])
    d["summary"] = diag_summary(d)
    return d


def _sum_se(x):
    """(sum, sqrt(n var)) of the per-cell values x, var with n - 1 in the denominator (0 for fewer than two cells)."""
    x = np.asarray(x, np.float64)
    n = len(x)
    return float(x.sum()), float(math.sqrt(n * x.var(ddof=1))) if n > 1 else 0.0


def score_summary(d):
    """What one line says of the per-cell scores `d` = dict(lpd, pwaic) (engine.score_cells, bpmf_amd.score_cells): n (cells), lpd_sum
    and lpd_mean (the log score: sum and mean of lpd_i), p_waic = sum pwaic_i (the effective number of parameters), elpd = sum (lpd_i -
    pwaic_i), waic = -2 elpd, se = sqrt(n var_i elpd_i) and se_lpd = sqrt(n var_i lpd_i) (the standard errors of the two sums; var
    with n - 1), pwaic_above = the share of cells with pwaic_i > 0.4 (where the WAIC correction is known to be unreliable: reported,
    not asserted), samples (d["samples"] if given, else None).  Without a cell the sums are 0 and lpd_mean, pwaic_above are NaN."""
    lpd = np.asarray(d["lpd"], np.float64); pw = np.asarray(d["pwaic"], np.float64)
    n = len(lpd)
    lpd_sum, se_lpd = _sum_se(lpd)
    elpd, se = _sum_se(lpd - pw)
    nan = float("nan")
    return dict(n=int(n), samples=d.get("samples"), lpd_sum=lpd_sum, lpd_mean=lpd_sum / n if n else nan, p_waic=float(pw.sum()), elpd=elpd,
                waic=-2.0 * elpd, se=se, se_lpd=se_lpd, pwaic_above=float(np.mean(pw > 0.4)) if n else nan)


def score_compare(a, b):
    """Two models scored on the same cells, `a` and `b` = dict(lpd, pwaic) in the same order: dict(n, elpd_diff, elpd_se, lpd_diff,
    lpd_se) with the differences a - b of the sums and their paired standard errors sqrt(n var_i(a_i - b_i)).  A positive
    difference of more than a few standard errors says that `a` predicts these cells better.  PSIS-LOO results compare the same way:
    `a` and `b` = dict(elpd_loo, lpd) (bpmf_amd.loo_cells), or the two per-cell elpd_loo arrays themselves, which give dict(n,
    elpd_diff, elpd_se) alone."""
    def per_cell(d):
        if not isinstance(d, dict):
            return np.asarray(d, np.float64), None
        lpd = np.asarray(d["lpd"], np.float64) if d.get("lpd") is not None else None
        if "pwaic" in d:
            return lpd - np.asarray(d["pwaic"], np.float64), lpd
        return np.asarray(d["elpd_loo"], np.float64), lpd
    (ea, la), (eb, lb) = per_cell(a), per_cell(b)
    if ea.shape != eb.shape or ea.ndim != 1 or (la is None) != (lb is None):
        raise ValueError("score_compare: the two results must cover the same cells")
    elpd_diff, elpd_se = _sum_se(ea - eb)
    if la is None:
        return dict(n=int(len(ea)), elpd_diff=elpd_diff, elpd_se=elpd_se)
    lpd_diff, lpd_se = _sum_se(la - lb)
    return dict(n=int(len(la)), elpd_diff=elpd_diff, elpd_se=elpd_se, lpd_diff=lpd_diff, lpd_se=lpd_se)


def _likelihood(who, res, values, weights, flags):
    """(S, y, alpha, kind, nu) of the likelihood `res` ran with, for the observed values: what score_cells and loo_cells hand to the engine."""
    info = res.get("model_info")
    if info is None:
        raise ValueError("%s: the result carries no model_info (it comes from gibbs or load_model)" % who)
    if not info.get("scored", True):
        raise ValueError("%s: ordinal and implicit runs are not scored" % who)
    S = res["users"].engine.samples_count(res["users"].side)
    y = np.ascontiguousarray(values, np.float64)
    alpha = info.get("alpha_samples")
    if alpha is None:
        alpha = float(info.get("alpha", float("nan")))
    elif len(alpha) != S:
        raise ValueError("%s: model_info has %d values of alpha for %d kept samples" % (who, len(alpha), S))
    nu = info.get("nu")
    if info.get("probit"):
        kind, nu, alpha = "probit", 0.0, 1.0
        y = np.where(y > float(info.get("probit_threshold", 0.0)), 1.0, -1.0)
    elif nu is not None:
        kind = "student"
    else:
        kind, nu = "gaussian", 0.0
    if kind != "gaussian" and (weights is not None or flags is not None):
        raise ValueError("%s: weights and flags go with the Gaussian likelihood alone, this run is %s" % (who, kind))
    return S, y, alpha, kind, nu


def score_cells(res, rows, cols, values, weights=None, flags=None):
    """The log pointwise predictive density of the observed cells (rows[i], cols[i]) -- user, movie, 0-based -- with the values
    values[i], over the kept samples of `res` (gibbs with the rings kept, or load_model):
    dict(rows, cols, lpd, pwaic, elpd, mean, std, samples, summary).  lpd_i = log mean_s p(y_i | sample s), pwaic_i = var_s log p(y_i |
    sample s), elpd_i = lpd_i - pwaic_i; over held-out cells sum lpd_i is the log score, over training cells sum elpd_i is WAIC's
    estimate of it; mean and std are predict_cells's; summary = score_summary of it.  The likelihood comes from
    res["model_info"]: probit (values > probit_threshold is a positive label), Student-t with nu degrees of freedom after robust=nu
    (the marginal density: the drawn weights are integrated out), else Gaussian; alpha is the precision every kept sample ran with
    (model_info["alpha_samples"], one per sample, else model_info["alpha"]).  weights: per-cell precision weights as weights= of
    gibbs gave them to the training cells; flags: int8, +-1 for a censored value (the value is then a bound, as censored= of gibbs);
    both Gaussian only, None for held-out cells."""
    users, movies = res["users"], res["movies"]
    S, y, alpha, kind, nu = _likelihood("score_cells", res, values, weights, flags)
    engine = users.engine
    rows = np.ascontiguousarray(rows, np.int32); cols = np.ascontiguousarray(cols, np.int32)
    d = engine.score_cells(users.side, movies.side, movies.mean_rating, rows, cols, y, alpha, kind, nu, weights, flags)
    d.update(rows=rows, cols=cols, samples=S, kind=kind, elpd=d["lpd"] - d["pwaic"])
    d["summary"] = score_summary(d)
    return d


def loo_summary(d):
    """What one line says of the per-cell PSIS-LOO results `d` = dict(elpd_loo, khat, lpd) (engine.loo_cells, bpmf_amd.loo_cells):
    n (cells), elpd_loo (the sum) and se = sqrt(n var_i elpd_loo_i) (var with n - 1), p_loo = sum (lpd_i - elpd_loo_i) (the effective
    number of parameters), looic = -2 elpd_loo, samples (d["samples"] if given, else None), khat_counts = the cells with khat <= 0.5,
    in (0.5, 0.7], in (0.7, 1], > 1 and finite, and infinite (nothing was smoothed: fewer than 25 samples, or a constant tail), as a
    dict(good, ok, bad, very_bad, inf), khat_threshold = min(1 - 1 / log10 S, 0.7) (Vehtari et al. 2024; NaN without samples) and
    khat_above = the share of cells whose khat exceeds it (infinite ones included), khat_above_07 the share above 0.7.  Cells whose
    khat is NaN (a trace that was not finite) are counted as n_nan and fall in no class.  Without a cell the sums are 0 and the
    shares NaN."""
    elpd = np.asarray(d["elpd_loo"], np.float64); khat = np.asarray(d["khat"], np.float64); lpd = np.asarray(d["lpd"], np.float64)
    n = len(elpd)
    S = d.get("samples")
    nan = float("nan")
    s, se = _sum_se(elpd)
    thr = nan if S is None else (min(1.0 - 1.0 / math.log10(S), 0.7) if S > 1 else -math.inf)
    fin = np.isfinite(khat)
    counts = dict(good=int(np.sum(khat <= 0.5)), ok=int(np.sum((khat > 0.5) & (khat <= 0.7))), bad=int(np.sum((khat > 0.7) & (khat <= 1.0))),
                  very_bad=int(np.sum(fin & (khat > 1.0))), inf=int(np.sum(np.isposinf(khat))))
    return dict(n=int(n), samples=S, elpd_loo=s, se=se, p_loo=float((lpd - elpd).sum()), looic=-2.0 * s, khat_counts=counts,
                n_nan=int(np.sum(np.isnan(khat))), khat_threshold=thr, khat_above=float(np.mean(khat > thr)) if n and S is not None else nan,
                khat_above_07=float(np.mean(khat > 0.7)) if n else nan)


def loo_cells(res, rows, cols, values, weights=None, flags=None):
    """PSIS-LOO of the observed cells (rows[i], cols[i]) -- user, movie, 0-based -- with the values values[i], over the kept samples of
    `res` (gibbs with the rings kept, or load_model; 1 .. 4096 samples): dict(rows, cols, elpd_loo, khat, lpd,
    p_loo, mean, std, samples, kind, summary).  Over the training cells elpd_loo_i estimates the log predictive density cell i would get
    from a model fitted without it, by Pareto-smoothed importance sampling of the per-sample log densities; khat_i is the shape of the
    generalised Pareto distribution fitted to the tail of its importance ratios and says whether the estimate can be trusted (<= 0.7;
    +inf where nothing was smoothed); lpd is score_cells's, p_loo_i = lpd_i - elpd_loo_i; mean and std are predict_cells's; summary =
    loo_summary of it.  The likelihood, weights and flags are those of score_cells."""
    users, movies = res["users"], res["movies"]
    S, y, alpha, kind, nu = _likelihood("loo_cells", res, values, weights, flags)
    engine = users.engine
    rows = np.ascontiguousarray(rows, np.int32); cols = np.ascontiguousarray(cols, np.int32)
    d = engine.loo_cells(users.side, movies.side, movies.mean_rating, rows, cols, y, alpha, kind, nu, weights, flags)
    d.update(rows=rows, cols=cols, samples=S, kind=kind, p_loo=d["lpd"] - d["elpd_loo"])
    d["summary"] = loo_summary(d)
    return d


def interval_taus(levels):
    """(levels, taus, lo_at, hi_at): the 1 .. 4 distinct levels in [0.01, 0.998] as floats, the strictly increasing quantile orders
    (1 - l) / 2 and (1 + l) / 2 of their central intervals, and per level the places of its two ends among them."""
    levels = [float(l) for l in np.atleast_1d(np.asarray(levels, np.float64))]
    if not 1 <= len(levels) <= 4:
        raise ValueError("intervals: 1 .. 4 levels, not %d" % len(levels))
    for l in levels:
        if not (0.01 <= l <= 0.998):
            raise ValueError("intervals: the level %r is outside [0.01, 0.998]" % (l,))
    if len(set(levels)) != len(levels):
        raise ValueError("intervals: the levels must differ")
    taus = sorted([(1.0 - l) / 2.0 for l in levels] + [(1.0 + l) / 2.0 for l in levels])
    lo_at = [taus.index((1.0 - l) / 2.0) for l in levels]
    hi_at = [taus.index((1.0 + l) / 2.0) for l in levels]
    return levels, np.asarray(taus, np.float64), lo_at, hi_at


def calibration_summary(pit, levels, lo=None, hi=None):
    """How well central predictive intervals cover held-out values, from their probability integral transforms pit [n] alone (a value
    lies inside the central interval of level l exactly when |pit - 1/2| <= l / 2): dict(n, levels, coverage, se, width, hist, ks) with
    per level the share of values inside and its binomial standard error sqrt(l (1 - l) / n) under perfect calibration, the mean width
    hi - lo of the intervals (lo, hi [n, levels]; NaN without them), the ten-bin histogram of the pits (counts; uniform when calibrated:
    a hump in the middle says the intervals are too wide, a U that they are too narrow) and the Kolmogorov distance
    sup_u |ecdf(pit)(u) - u|.  Pits that are NaN are left out and counted as n_nan."""
    pit = np.asarray(pit, np.float64).ravel()
    ok = ~np.isnan(pit)
    p = np.sort(pit[ok])
    n = len(p)
    levels = [float(l) for l in np.atleast_1d(np.asarray(levels, np.float64))]
    nan = float("nan")
    cover = [float(np.mean(np.abs(p - 0.5) <= 0.5 * l)) if n else nan for l in levels]
    se = [math.sqrt(l * (1.0 - l) / n) if n else nan for l in levels]
    if lo is not None and hi is not None and n:
        wd = (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)).reshape(len(pit), len(levels))[ok]
        width = [float(wd[:, k].mean()) for k in range(len(levels))]
    else:
        width = [nan] * len(levels)
    hist = np.bincount(np.minimum((p * 10.0).astype(np.int64), 9), minlength=10).astype(np.int64) if n else np.zeros(10, np.int64)
    if n:
        i = np.arange(n, dtype=np.float64)
        ks = float(max(((i + 1.0) / n - p).max(), (p - i / n).max()))
    else:
        ks = nan
    return dict(n=int(n), n_nan=int(len(pit) - n), levels=levels, coverage=cover, se=se, width=width, hist=hist, ks=ks)


def predict_intervals(res, rows, cols, levels=(0.9,), values=None, weights=None):
    """Central predictive intervals of the cells (rows[i], cols[i]) -- user, movie, 0-based -- from the kept samples of `res` (gibbs with
    the rings kept, or load_model; 1 .. 4096 samples): dict(rows, cols, mean, std, levels, lo, hi, pit, samples,
    summary).  The posterior predictive of a cell is the mixture over the samples of N(p_s, 1 / (alpha_s w)); lo and hi [n, levels] are
    its quantiles at (1 - l) / 2 and (1 + l) / 2 for each of the 1 .. 4 levels in [0.01, 0.998]; mean and std are predict_cells's.
    values: observed values of the cells; then pit [n] is their probability integral transform and summary = calibration_summary of
    it (else both None).  weights: per-cell precision weights (None: 1, what held-out cells have).  alpha is the precision every
    kept sample ran with (model_info["alpha_samples"], one per sample, else model_info["alpha"]).  Gaussian likelihoods only: probit,
    ordinal, implicit and Student-t (robust=) runs are refused."""
    users, movies = res["users"], res["movies"]
    info = res.get("model_info")
    if info is None:
        raise ValueError("predict_intervals: the result carries no model_info (it comes from gibbs or load_model)")
    if info.get("probit") or not info.get("scored", True):
        raise ValueError("predict_intervals: probit, ordinal and implicit runs have no Gaussian predictive")
    if info.get("nu") is not None:
        raise ValueError("predict_intervals: not after robust= (a mixture of Student-t distributions needs an incomplete beta function on the device: out of scope)")
    levels, taus, lo_at, hi_at = interval_taus(levels)
    engine = users.engine
    S = engine.samples_count(users.side)
    rows = np.ascontiguousarray(rows, np.int32); cols = np.ascontiguousarray(cols, np.int32)
    alpha = info.get("alpha_samples")
    if alpha is None:
        alpha = float(info.get("alpha", float("nan")))
    elif len(alpha) != S:
        raise ValueError("predict_intervals: model_info has %d values of alpha for %d kept samples" % (len(alpha), S))
    d = engine.interval_cells(users.side, movies.side, movies.mean_rating, rows, cols, alpha, taus, y=values, w=weights)
    quant = d.pop("quant")
    d.update(rows=rows, cols=cols, levels=levels, lo=np.ascontiguousarray(quant[:, lo_at]), hi=np.ascontiguousarray(quant[:, hi_at]), samples=S)
    d["summary"] = calibration_summary(d["pit"], levels, d["lo"], d["hi"]) if values is not None else None
    return d
