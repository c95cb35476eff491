"""Host-side mirror of the reference's `struct Sys` / `HyperParams` (c++/bpmf.h:78-239).

Same names, same argument meaning, same quirks, so that the
parity tests read like the reference: `movies.sample(users); users.sample(movies);
movies.predict(users)`.  All column work happens in the engine (HipEngine ->
libbpmf_hip.so); this file only sequences the calls the way `Sys::sample(Sys&)`
(c++/sample.cpp:341-385) and `main` (c++/bpmf.cpp:180-253) do.
"""
import math
import os as _os
import sys as _sys
import time

import numpy as np

from . import engine as _engine
from .censor import censor_flags, transpose_csc
from .weights import rating_weights
from .rank import held_out_lists, rank_metrics


class HyperParams:
    """c++/bpmf.h:78-104: fixed prior b0=2, df=K, mu0=0, WI=I; sampled mu, LambdaU, LambdaF."""

    def __init__(self, K):
        self.K = K
        self.b0 = 2
        self.df = K
        self.mu0 = np.zeros(K)
        self.WI = np.eye(K)
        self.mu = np.zeros(K)
        self.LambdaF = np.zeros((K, K))
        self.LambdaU = np.zeros((K, K))
        self.LambdaL = np.zeros((K, K))

    def sample(self, N, sum_, cov, counter):
        """std::tie(mu, LambdaU) = CondNormalWishart(N, cov, sum / N, mu0, b0, WI, df) after
        rng_set_pos(counter) (c++/sample.cpp:349-350)."""
        um = None if not np.any(sum_) else np.asarray(sum_) / N
        self.mu, self.LambdaU, self.LambdaF = _engine.hyper_sample(self.K, N, cov, counter, um)
        self.LambdaL = self.LambdaU.T


class Sys:
    """One factor ("movs" or "users").  M is CSC with one column per item of this
    side; rows index the other side.  `dom` = (col_from, col_to) is the column
    range this rank samples (Sys::from()/to(), c++/bpmf.h:170-172) and M / T are
    the slices of exactly those columns; `num` is the global number of columns."""

    # static members of the reference (c++/sample.cpp:26-34)
    alpha = 2.0
    burnin = 5
    nsims = 20
    procid = 0
    nprocs = 1

    def __init__(self, name, engine, M, num, nrows, T=None, dom=None, mean_rating=None, comm=None):
        self.name = name
        self.engine = engine
        self.K = engine.K
        self.iter = -1                                    # c++/sample.cpp:113
        self.key_offset = 0                               # gibbs(chain=c): c * 2^20, added where the host keys random numbers by iter
        self._num = int(num)
        self.nrows = int(nrows)
        self.dom = (0, self._num) if dom is None else (int(dom[0]), int(dom[1]))
        self.comm = comm
        colptr, rowidx, vals = M
        self.local_nnz = int(colptr[-1])
        on_device = hasattr(rowidx, "data_ptr")           # torch tensors on the GPU (a matrix generated there): adopted, not copied
        if mean_rating is None:                           # Sys::init, c++/sample.cpp:183 (single rank)
            mean_rating = float(vals.sum()) / max(self.local_nnz, 1)
        self.mean_rating = float(mean_rating)
        if on_device:
            self.side = engine.side_create_dev(self._num, self.nrows, colptr, rowidx.data_ptr(), vals.data_ptr(), self.mean_rating,
                                               self.dom[0], self.dom[1], keep=(rowidx, vals))
        else:
            self.side = engine.side_create(self._num, self.nrows, colptr, rowidx, vals, self.mean_rating,
                                           self.dom[0], self.dom[1])
        self.test = None
        self.T_nnz = 0
        if T is not None:
            self.test = engine.test_create(self.side, *T)
            self.T_nnz = int(T[0][-1])
        self.hp = HyperParams(self.K)
        self.sum = np.zeros(self.K)                       # never updated: SURVEY Q1 (c++/sample.cpp:187,379)
        self.cov = np.zeros((self.K, self.K))
        self.norm = 0.0
        self.rmse = float("nan")
        self.rmse_avg = float("nan")
        self.num_predict = 0
        self.sample_ms = 0.0

    def refresh(self):
        """Pulls norm / cov / hp back from the library after sys_sample calls."""
        if getattr(self, "_stale", False):
            it, self.norm, self.cov, self.hp.mu, self.hp.LambdaF, self.hp.LambdaU = self.engine.sys_state(self.side)
            assert it == self.iter
            self._stale = False

    # -- accessors with the reference's names ---------------------------------
    def num(self):
        return self._num

    def from_(self):
        return self.dom[0]

    def to(self):
        return self.dom[1]

    def items(self):
        """K x num() factor matrix as an [num, K] array (row = one column of the reference's items())."""
        return self.engine.get_items(self.side)

    # -- Sys::sample(Sys&), c++/sample.cpp:341-385 ------------------------------
    def sample(self, other):
        if getattr(self, "implicit", False):
            # an implicit model: BOTH sides take the blocking half-iteration that forms G
            self.engine.implicit_sample(self.side, other.side, Sys.alpha)
            self.iter += 1
            self._stale = True
            return
        if getattr(self, "linked", False):
            # a model with side information: BOTH sides take the blocking half-iteration
            self.engine.link_sample(self.side, other.side, Sys.alpha)
            self.iter += 1
            self._stale = True
            return
        if (self.comm is None or getattr(self.comm, "native", False)) and hasattr(self.engine, "sys_sample"):
            # NO_COMM: the whole of Sys::sample(Sys&) (iter++, hyper draw, column loop, cov) runs
            # behind one C-ABI call, which also overlaps the host draws with the kernels
            self.engine.sys_sample(self.side, other.side, Sys.alpha)
            self.iter += 1
            self._stale = True
            return
        self.iter += 1
        self.hp.sample(self.num(), self.sum, self.cov, self.iter + self.key_offset)          # :349-350
        t0 = time.perf_counter()
        s, prod, norm = self.engine.sample_side(self.side, other.side, self.iter + self.key_offset, Sys.alpha, self.hp.mu, self.hp.LambdaF)
        if self.comm is not None:
            # exchange the fresh columns (send_item / bcast of the MPI back-ends) and
            # all-reduce sum | prod | norm, then form cov once from the global sums
            self.comm.exchange_items(self)
            red = self.comm.allreduce(np.concatenate([np.asarray(prod, order="F").ravel(order="F"), s, [norm]]))
            K = self.K
            prod = red[:K * K].reshape((K, K), order="F"); s = red[K * K:K * K + K]; norm = float(red[-1])
        self.sample_ms = (time.perf_counter() - t0) * 1e3
        self.norm = norm                                                     # :381
        N = self.num()
        self.cov = _engine.cov_from_sums(self.K, N, s, prod)                 # :383-384
        self.last_sum = s

    # -- Sys::predict, c++/sample.cpp:48-96 -------------------------------------
    def predict(self, other, all=False):
        n = 0 if self.iter < Sys.burnin else self.iter - Sys.burnin          # :50
        if self.test is None:
            return
        if getattr(self, "_twin_of", None) is not None:                    # evaluated with its owner: only the sums are collected here
            self.predict_finish()
            return
        se, se_avg, nump = self.engine.predict(self.test, self.side, other.side, n)
        if self.comm is not None and not getattr(self.comm, "native", False) and all:
            red = self.comm.allreduce(np.array([se, se_avg, float(nump)]))
            se, se_avg, nump = float(red[0]), float(red[1]), int(round(red[2]))
        self.num_predict = nump
        self.rmse = math.sqrt(se / nump) if nump else float("nan")
        self.rmse_avg = math.sqrt(se_avg / nump) if nump else float("nan")

    def set_twin(self, other):
        """`other.predict(self)` of the reference's loop (c++/bpmf.cpp:190) rides with every self.predict(other): `other`
        must hold the transposed test entries (its own T).  Its sums: other.predict_finish() after self's."""
        self.engine.test_set_twin(self.test, other.test)
        self._twin = other
        other._twin_of = self

    def predict_launch(self, other):
        """First half of predict(): enqueue the evaluation behind the samplers.  The caller may start
        the next half-iteration before predict_finish() (software pipelining of main()'s loop)."""
        n = 0 if self.iter < Sys.burnin else self.iter - Sys.burnin
        if self.test is not None:
            self.engine.predict_launch(self.test, self.side, other.side, n)

    def predict_finish(self):
        if self.test is None:
            return
        se, se_avg, nump = self.engine.predict_finish(self.test)
        self.num_predict = nump
        self.rmse = math.sqrt(se / nump) if nump else float("nan")
        self.rmse_avg = math.sqrt(se_avg / nump) if nump else float("nan")

    # -- Sys::print, c++/sample.cpp:101-107 --------------------------------------
    def format_line(self, items_per_sec, ratings_per_sec, norm_u, norm_m):
        phase = "Burnin" if self.iter < Sys.burnin else "Sampling"
        return "%d: %s iteration %d:\t RMSE: %3.4f\tavg RMSE: %3.4f\tFU(%6.2f)\tFM(%6.2f)\titems/sec: %6.2f\tratings/sec: %6.2fM\n" % (
            Sys.procid, phase, self.iter, self.rmse, self.rmse_avg, norm_u, norm_m, items_per_sec, ratings_per_sec / 1e6)


CHAIN_STRIDE, CHAIN_MAX = 1 << 20, 63


def _check_chain(engine, chain, nsims, features, ordinal, bias, bias_prior, implicit):
    """gibbs(chain=): the chain as an int, or the ValueError of what it does not go together with (before the device is used)"""
    if isinstance(chain, bool) or not isinstance(chain, (int, np.integer)) or not 0 <= int(chain) <= CHAIN_MAX:
        raise ValueError("chain must be an integer 0 .. %d, not %r" % (CHAIN_MAX, chain))
    chain = int(chain)
    if chain == 0:
        return 0
    for on, what in ((features, "features"), (ordinal is not None and ordinal is not False, "ordinal"),
                     ((bias is not None and bias is not False) or bias_prior is not None, "bias"), (implicit is not None, "implicit"),
                     (getattr(engine, "comm_nranks", lambda: 1)() > 1, "a communicator"),
                     (_os.environ.get("BPMF_REDUCE", "0") not in ("", "0"), "BPMF_REDUCE")):
        if on:
            raise ValueError("chain=%d does not go together with %s (only chain 0 runs with it)" % (chain, what))
    if nsims > CHAIN_STRIDE:
        raise ValueError("chain=%d needs nsims <= %d: the chains' random streams are %d half-iterations apart (nsims = %d)"
                         % (chain, CHAIN_STRIDE, CHAIN_STRIDE, nsims))
    return chain


def gibbs(engine, M, Mt, T, nusers, nmovies, nsims=20, burnin=5, alpha=None, out=None, keep_samples=False, Tt=None, pipelined=False,
          topn=None, noise="fixed", alpha_prior=(1.0, 1.0), alpha_max=None, probit=False, threshold=0.5,
          row_features=None, col_features=None, lambda_beta=5.0, link_tol=1e-6, link_max_iter=1000, lambda_beta_prior=None, censored=None,
          new_row_features=None, new_col_features=None, topn_score=None, foldin=False, weights=None, robust=None,
          ordinal=None, cutpoints=None, ordinal_step=None, implicit=None, rank_eval=None, rank_by="rows", rank_threshold=None, save_model=None,
          similar=None, similar_by="cols", similar_kind="cosine", similar_kappa=0.0, similar_min_ratings=0, bias=None, bias_prior=None, diagnose=None, score=False, intervals=None, loo=False, chain=0, keep_rings=False):
    """The loop of main() (c++/bpmf.cpp:131-253) in NO_COMM mode.  M / T: CSC
    with one column per movie (rows = users); Mt its transpose.  Returns a dict
    with the per-iteration trace; `out` (a file object) receives the reference's
    stdout lines.

    pipelined=True: the same iterations the way the `bpmf` executable (bpmf_main.cpp) and bench.py's timed
    region run them -- the line of iteration i - 1 (RMSE sums, norms) is collected after iteration i has been
    enqueued, the evaluation of i - 1 runs beside the samplers of i (which write the other copy of the factors).
    Same chain, same numbers; `secs` is then the time between two collected lines.

    topn=N: every post-burn-in sample of both sides is kept on the device (nsims - burnin slots each) and res["topn"] holds
    engine.topn(users, movies, ...) after the loop -- (idx, mean, std), [nusers, N] each: the N unrated movies of every user
    with the highest posterior-mean prediction.

    topn_score=("ucb", kappa) | ("prob", t) | ("ei", t), with topn=N: the lists are ranked by an acquisition score of the kept
    samples instead of their mean -- mean + kappa std (kappa < 0: a lower bound), the posterior probability
    that a rating exceeds t, or the expected excess over t, with the observation noise sigma = 1 / sqrt(alpha) of the run (1 under
    probit=True, where t is on the latent-score scale and 0 the natural value).  res["topn"] is then engine.topn_scored's
    (idx, score, mean, std).  "prob" and "ei" are refused with noise="adaptive" (alpha is not one number).  res["new_rows_topn"]
    / res["new_cols_topn"] stay the 3-tuples ranked by the mean (see new_row_features below).  None (the default): nothing changes.

    noise="adaptive": the noise precision is sampled too.  Iteration 0 runs with `alpha`; after iteration i (both sides
    sampled) the sum of squared training residuals SSE_i is reduced on the device (engine.train_sse over the movies' ratings)
    and iteration i + 1 runs with alpha = g / (b0 + SSE_i / 2), g ~ Gamma(a0 + n / 2, 1) (engine.noise_sample, alpha_prior =
    (a0, b0) = shape / rate of the Gamma prior), capped at alpha_max.  The pipelined loop then waits once per iteration for
    SSE_i before it enqueues iteration i + 1.  res["alpha"]: the alpha each iteration ran with, res["train_rmse"]:
    sqrt(SSE_i / n).  noise="fixed" (the default) is the reference's constant alpha.

    alpha: the noise precision (None: the reference's default 2, or 1 with probit=True).

    probit=True: the ratings are labels (positive if > threshold) under the probit likelihood: both sides
    are created with mean rating 0 and turned into probit sides (engine.set_probit, tags 1 = movies, 2 = users), alpha is 1, and
    every post-burn-in sample adds Phi(u . v) to the running sums of the test entries (engine.probit_add, enqueue only: the
    pipelined loop does not drain).  res["prob"]: the posterior-mean probability of a positive per test entry (order of T),
    res["auc"]: bpmf_amd.auc of it against the test labels (NaN for a single class or no test matrix), res["brier"]: the mean
    squared difference of prob and the 0 / 1 label.  The RMSE columns of the trace then compare the latent score u . v with the
    raw label and are not an error measure.

    row_features [nusers, D] / col_features [nmovies, D]: side information.  The prior mean of a user's
    (movie's) factors becomes mu + beta^T f with a link matrix beta (D x K) that is sampled too, its rows N(0, (lambda_beta
    Lambda)^-1) a priori; lambda_beta is fixed (5 is a default, not a tuned number).  Either or both.  The loop is then the plain
    one over engine.link_sample (blocking, both sides); pipelined=True, probit=True and noise="adaptive" are refused with
    features.  res["beta_rows"] / res["beta_cols"]: the mean of beta over the post-burn-in samples (None without such samples).

    A scipy.sparse feature matrix (any D) takes the CG path of DESIGN.md section 14: beta is drawn by conjugate gradients on the
    device to the relative residual link_tol in at most link_max_iter iterations.  res["link_cg_iters"]: per iteration the CG
    iterations of (movies, users), None for a side without sparse features; res["link_cg_hit_max_iter"]: whether any draw ran
    into link_max_iter.  A dense ndarray keeps the dense path; nothing is converted either way.

    lambda_beta_prior=(A0, B0): lambda_beta is sampled too, per side with features: prior Gamma(shape A0,
    rate B0), conditional Gamma(A0 + D K / 2, B0 + tr(Lambda beta^T beta) / 2), drawn at the start of every half-iteration but
    the first, for which `lambda_beta` is the initial value.  (5e-4, 5e-4) is a weak default, not a tuned number.  The chain
    starts at beta = 0, so the first draws are large (10^2 .. 10^3) and take tens of iterations to come down: the burn-in has to
    cover that.  res["lambda_beta_rows"] / res["lambda_beta_cols"]: the value each half-iteration used, one per iteration (None
    for a side without features).  None (the default): lambda_beta stays fixed and nothing changes.

    censored=C: some training ratings are bounds, not measurements.  C is a CSC triple of M's shape: an
    entry > 0 says that the rating of that cell is a lower bound of the true value, an entry < 0 an upper bound (bpmf_amd.
    censor_flags; every entry must be a stored cell of M).  Both sides get their flags (engine.set_censored, tags 5 = movies,
    6 = users; those of Mt from C transposed) and redraw the latent values of their censored cells ahead of every sampler launch,
    on the device, without a host wait: the pipelined loop does not drain.  Any alpha > 0, with or without topn; the test matrix
    is taken as exact values.  probit=True, noise="adaptive" and features are refused with censored.  res["censored"] = (lower
    bounds, upper bounds).  None (the default): nothing changes.

    new_row_features [n_new, D] / new_col_features [n_new, D]: users (movies) that are NOT in the training matrix, predicted from
    their features alone.  Needs row_features (col_features) of the same kind and D, and nsims > burnin.
    Every post-burn-in iteration projects them with that iteration's mu and beta (engine.newrows_add; nsims - burnin slots) and
    keeps the other side's factors in its sample ring (reserved here when topn did not).  res["new_rows"] = dict(mean, std),
    [n_new, nmovies] each, res["new_cols"] = dict(mean, std), [nusers, n_new] each: the mean over the kept samples of mean_rating
    + (mu_s + beta_s^T f) . v_s and the total deviation -- the spread between the samples joined with the spread of a cold row's
    factors around their conditional mean, (1/S) sum_s v_s^T Lambda_s^-1 v_s.  The observation noise 1 / alpha is not part of std.
    With topn=N also res["new_rows_topn"] / res["new_cols_topn"] = (idx, mean, std), [n_new, N] each, the new entities as the
    queries.  These two are ALWAYS ranked by the posterior mean, also when topn_score ranks res["topn"] by another key: the score
    of a new entity would need the w[c] / S term of its variance (out of scope).  None (the default):
    nothing changes.

    foldin=True: the run keeps what bpmf_amd.fold_in(res, ...) needs to give users (movies) that arrive AFTER it, with a few ratings
    and no features, their factors: the sample rings of both sides and, per side without features, the
    hyper-parameters (alpha, mu, Lambda) every post-burn-in iteration ran with (engine.hyper_add, where samples_add sits; nsims -
    burnin slots; with noise="adaptive" the iteration's own alpha).  The engine must stay open for fold_in.  Needs nsims > burnin;
    refused with probit=True and when both sides have features.  res["foldin"] = True.  False (the default): nothing changes.

    weights=W: a precision weight per training rating, r ~ N(mean + u . v, 1 / (alpha w)).  W is a CSC triple
    of M's shape: the rating of a listed cell takes that entry (finite, > 0) as its weight, every other rating the weight 1
    (bpmf_amd.rating_weights; every entry must be a stored cell of M).  Both sides get their weights once (engine.set_weights;
    those of Mt from W transposed) and run the weighted form of their sampler: nothing is enqueued per iteration, the pipelined
    loop does not drain.  With or without topn, topn_score, foldin (a folded-in row's own ratings have weight 1); the test matrix
    is unweighted.  probit=True, censored, noise="adaptive", features and an fp32 engine are refused with weights.  res["weights"]
    = (cells whose weight is not 1, smallest weight, largest weight).  None (the default): nothing changes.

    robust=NU: Student-t noise with NU >= 1 degrees of freedom (1: Cauchy) instead of Gaussian noise, location mean + u . v, scale
    1 / sqrt(alpha): r | w ~ N(mean + u . v, 1 / (alpha w)), w ~ Gamma(NU / 2, rate NU / 2).  Both sides
    become robust sides (engine.set_robust, tags 9 = movies, 10 = users) and redraw the weights of their ratings ahead of every
    sampler launch, on the device, without a host wait: the pipelined loop does not drain.  A gross outlier draws a small weight
    and stops dragging its factors.  Every post-burn-in iteration adds the movies' weights to their running sums
    (engine.robust_add, enqueue only).  res["robust"] = dict(nu=NU, weight_mean=the posterior-mean weight of every training
    rating in M's CSC order (zeros without a kept sample), kept=the samples in it).  With or without topn, foldin (a folded-in
    row's own ratings are Gaussian with weight 1) and topn_score ("ucb" only: the sigma = 1 / sqrt(alpha) of "prob" and "ei"
    assumes Gaussian noise).  weights, probit=True, censored, noise="adaptive", features and an fp32 engine are refused with
    robust.  None (the default): nothing changes.

    ordinal=True | levels: the ratings are ordered categories under the ordinal probit likelihood with sampled cutpoints (DESIGN.md
    section 23).  The training values take one of C levels (True: the distinct training values; or the 2 <= C <= 16 level values,
    increasing, of which some may be absent from the training set); a rating at level c has a latent score between the cutpoints
    g_{c-1} and g_c.  Both sides are created with mean rating 0 and turned into ordinal sides (engine.set_ordinal, tags 11 =
    movies, 12 = users), alpha is 1.  Every iteration but the first starts with a Metropolis-Hastings step of all cutpoints given
    the factors (engine.ordinal_cut_step: one pass over the training ratings on the device, the pipelined loop drains once per
    iteration for it, as noise="adaptive" does).  Its proposal step s starts at 1 / sqrt(nnz) and follows log s += (accepted -
    0.35) / sqrt(iter + 1) during the burn-in, frozen afterwards: start, target and schedule are defaults, not tuned numbers.
    ordinal_step=F fixes s = F and disables the adaptation.  cutpoints=[g_1 .. g_{C-1}]: the cutpoints are fixed at these values,
    there is no step and no drain (None: they start at Phi^-1 of the cumulative level frequencies and are sampled).  Every
    post-burn-in sample adds the level probabilities of the test entries (engine.ordinal_add, enqueue only).  res["ordinal"] =
    dict(levels, cutpoints = the cutpoints every iteration ran with [nsims, C - 1], accepted = per iteration whether its proposal
    was accepted, step = the s of every iteration); res["cat_prob"] [ntest, C]: the posterior-mean probability of every level,
    res["expected"] = sum_c l_c p_c, res["logp"]: the mean log probability of the true level (a test value that is not a level is
    refused).  The RMSE columns of the trace compare the latent score u . v with the raw value and are not an error measure.  topn
    ranks by the latent score, and the thresholds of topn_score "prob" / "ei" are on that scale.  foldin, features,
    noise="adaptive", censored, weights, robust and probit=True are refused with ordinal.  None / False (the default): nothing
    changes.

    implicit=W0: implicit feedback.  EVERY cell of the matrix is observed with precision alpha w: a cell that
    M does not store as r = 0 with w = W0 (finite, > 0), a stored cell with its value and the confidence w = 1 -- or, with weights=W,
    the listed entry of W, which must be > W0 (as must 1 when a stored cell is not listed).  Both sides are created with mean
    rating 0, become implicit sides (engine.set_implicit) and are stepped with engine.implicit_sample, the blocking half-iteration
    that forms G = sum of u u^T over all columns of the other side on the device and samples under the prior precision Lambda +
    alpha W0 G; the column samplers are the weighted ones, unchanged.  With or without topn, topn_score "ucb" and rank_eval; the
    RMSE columns are over the test cells as given.  pipelined=True, probit=True, ordinal, robust, censored, noise="adaptive",
    features, foldin, topn_score "prob" / "ei" and an fp32 engine are refused with implicit.  res["implicit"] = dict(w0, observed =
    the stored cells, cells = nusers * nmovies, weights = (confidences that are not 1, smallest, largest)).  None (the default):
    nothing changes.

    rank_eval=N (1 .. 1000): ranked evaluation of the test cells after the chain.  Needs nsims > burnin; the
    sample rings are reserved as for topn.  rank_by="rows": the users are the queries and the movies the candidates ("cols": the
    other way round).  The held-out items are the test cells with a value > rank_threshold (None: every test cell, or value > 0
    under implicit); engine.rank_eval gives each its rank among the candidates its query has not rated in M, by topn's score.
    res["rank"] = bpmf_amd.rank_metrics(...) at N (recall, ndcg, mrr, mpr, auc, queries, entries) plus n = N, by, rank = the
    rank per test cell in T's order (0 for a cell the threshold left out) and ncand = the candidates left per query.  A test cell
    that is also a training cell is refused.  Works with every likelihood topn works with.  None (the default): nothing changes.

    save_model=DIR: the run keeps the sample rings of both sides and, unless probit=True, the hyper-parameters of both sides (as
    topn and foldin=True do), and writes them as a model directory after the chain (bpmf_amd.save_model): what
    bpmf_amd.load_model and `bpmf --model DIR` serve top-N lists, ranked evaluation, blocks, fold-in and single cells from without a
    chain.  Needs nsims > burnin.  Goes with plain Gaussian runs, any alpha, weights, robust, censored, probit=True, noise="adaptive"
    and an fp32 engine; refused with ordinal, implicit and features (serving them would need state the format does not store).
    None (the default): nothing changes.

    similar=N: the sample rings are kept as for topn, and after the chain res["similar"] = dict(by, kind, kappa, idx, score, mean,
    std) holds engine.similar's lists: the N nearest neighbours of every movie (similar_by="cols") or user
    ("rows") among the entities of the same side, by the posterior mean of the per-sample cosine (similar_kind="cosine") or negative
    squared distance ("euclid") minus similar_kappa >= 0 times its spread -- quantities no rotation of the latent space changes.
    Entities with fewer than similar_min_ratings training ratings are not listed (their factors are close to prior draws); they are
    still queries.  It reads only the ring, so it goes with every likelihood topn goes with, and is independent of topn.  Needs
    nsims > burnin.  None (the default): nothing changes.

    bias=True | LAMBDA: row and column bias terms, r = mean + b_user + c_movie + u . v with b, c ~ N(0, 1 / LAMBDA) (True: 1;
    DESIGN.md section 28).  Both sides get their biases (engine.set_bias, tags 13 = movies, 14 = users, roles 0 / 1) and redraw them
    on the device ahead of every sampler launch; the evaluation adds both to every prediction.  res["bias"] = dict(rows_mean,
    cols_mean: the posterior means of the users' / movies' biases; lambda_rows, lambda_cols: the precision every iteration's step
    ran with, nsims values each; kept).  bias_prior=(A0, B0): LAMBDA is sampled instead, Gamma(A0, rate B0) a priori, on the device at
    the start of every half-iteration of a side but its first (engine.bias_prior); bias then gives the starting value.  topn (every
    score), rank_eval and engine.predict_block / predict_cells work on top: the sample rings of both sides carry two more rows per
    sample, (b, 1) and (1, c), so that the ring dot product is u . v + b + c.  Refused with every other likelihood and add-on (probit,
    ordinal, censored, weights, robust, implicit, features, noise="adaptive"), with foldin, save_model and similar (a folded-in row has
    no bias, the model format stores none, the bias rows would enter the cosine), with pipelined=True, an fp32 engine, a communicator,
    and, together with a sample ring, num_latent > 126.  None / False (the default): nothing changes.

    diagnose=True | (rows, cols): convergence diagnostics of predictions.  The sample rings are kept as for
    topn, and after the chain res["diag"] = bpmf_amd.diagnose's dict for the test cells in the order of T (True) or for the cells
    (rows[i], cols[i]) -- user, movie, 0-based: per cell mean, std, the split-Rhat and the effective sample size (ESS) of the trace
    of its prediction over the kept samples, mcse = std / sqrt(ess), and "summary" (bpmf_amd.diag_summary).  res["diag"]["scalars"] =
    dict(rmse, norm_u, norm_m, and alpha under noise="adaptive"): (rhat, ess) of the post-burn-in per-iteration traces res[key],
    through engine.diag_traces.  Predictions are identified where the factors are not (they rotate along the chain).  Needs 8 ..
    4096 kept samples (nsims - burnin).  It reads only the rings, so it goes with every likelihood topn goes with, and with bias.
    None (the default): nothing changes.

    score=True: model comparison.  The sample rings are kept as for topn, and after the chain res["score"] =
    dict(train=, test=), each bpmf_amd.score_cells's dict.  "test": the log pointwise predictive density of the cells of T (the log
    score of held-out data; absent without a test matrix).  "train": the same over every training cell in the order of M, with the
    run's weights= and censored= flags, whose elpd = lpd - pwaic summed is WAIC's estimate of the out-of-sample log density
    (summary["waic"] = -2 elpd).  The likelihood is the run's: Gaussian with the alpha every kept iteration ran with (noise="adaptive":
    res["alpha"] of that iteration), Student-t with nu degrees of freedom under robust=nu (the marginal density, the weights integrated
    out), probit under probit=True; bias terms are part of the rings.  Refused: ordinal (it has res["logp"]), implicit, a
    communicator, BPMF_REDUCE, fewer than 2 kept samples.  False (the default): nothing changes.

    intervals=True | levels: predictive intervals and their calibration.  The sample rings are kept as for
    score, and after the chain res["intervals"] = dict(test=bpmf_amd.predict_intervals's dict over the cells of T with their values):
    per test cell the central intervals lo / hi of the posterior predictive mixture at the 1 .. 4 levels (True: 0.9), the probability
    integral transform pit of its held-out value, and "summary" (bpmf_amd.calibration_summary: coverage per level, mean width, PIT
    histogram, Kolmogorov distance).  alpha is that of every kept iteration (noise="adaptive": res["alpha"] of that iteration); test
    cells have weight 1; bias terms are part of the rings.  Needs a test matrix and 1 .. 4096 kept samples.  Refused: probit, ordinal,
    implicit, robust (a mixture of Student-t distributions is out of scope), a communicator, BPMF_REDUCE.  None (the default):
    nothing changes.

    loo=True: PSIS-LOO cross-validation of the training cells.  The sample rings are kept as for score, and
    after the chain res["loo"] = bpmf_amd.loo_cells's dict over the cells of M with the run's weights and censoring flags: per
    training cell elpd_loo (the log predictive density a model fitted without the cell would give it, by Pareto-smoothed importance
    sampling), khat (the diagnostic that says whether that estimate can be trusted: <= 0.7), lpd, p_loo, and "summary"
    (bpmf_amd.loo_summary: the sum with its standard error, p_loo, looic = -2 elpd_loo, the khat classes).  It replaces WAIC where the
    variance of the log density is large (score's "var > 0.4").  The likelihood is score's; so are the refusals: ordinal, implicit, a
    communicator, BPMF_REDUCE, fewer than 2 kept samples; and more than 4096.  False (the default): nothing changes.

    chain=c (0 .. 63): an independent chain of the same model: the run restarted from the same initial factors
    with its random numbers taken at the half-iteration indices c * 2^20, c * 2^20 + 1, .. (engine.side_set_chain on both sides; the
    host-keyed draws, noise="adaptive" among them, get the offset index).  res["chain"] = c.  chain=0 (the default) is the run as it
    was, bit for bit.  Goes with Gaussian runs at any alpha, noise="adaptive", weights, robust, probit=True and censored, on fp64 and
    fp32 engines.  Refused before the device is used: features, ordinal, bias, implicit, a communicator, BPMF_REDUCE, nsims > 2^20.
    bpmf_amd.run_chains runs several and pools them; bpmf_amd.diagnose of the pool is the rank-normalised multi-chain estimator.

    keep_rings=True: the sample rings of both sides and the hyper-parameters are kept as save_model=DIR keeps them, and nothing is
    written (bpmf_amd.run_chains, bpmf_amd.pool_models read them back).  It is refused where save_model is, under its own name."""
    keeps_model = save_model is not None or bool(keep_rings)
    keeps_what = "save_model" if save_model is not None else "keep_rings"
    chain = _check_chain(engine, chain, nsims, row_features is not None or col_features is not None or new_row_features is not None
                         or new_col_features is not None, ordinal, bias, bias_prior, implicit)
    loo_on = bool(loo)
    if loo_on:                                       # (refused before the engine is used)
        for on, what, why in ((ordinal is not None and ordinal is not False, "ordinal", "its held-out log density is res['logp']"),
                              (implicit is not None, "implicit", "its likelihood runs over every cell of the matrix"),
                              (getattr(engine, "comm_nranks", lambda: 1)() > 1, "a communicator", "the rings of both sides must be whole on one GPU"),
                              (_os.environ.get("BPMF_REDUCE", "0") not in ("", "0"), "BPMF_REDUCE", "the rings of both sides must be whole on one GPU")):
            if on:
                raise ValueError("loo does not go together with %s (%s)" % (what, why))
        if not (2 <= nsims - burnin <= _engine.HipEngine.LOO_MAX_SAMPLES):
            raise ValueError("loo needs 2 .. %d post-burn-in samples (nsims - burnin = %d)" % (_engine.HipEngine.LOO_MAX_SAMPLES, nsims - burnin))
    intervals_on = intervals is not None and intervals is not False
    if intervals_on:                                 # (refused before the engine is used)
        from .model import interval_taus as _interval_taus
        interval_levels = _interval_taus((0.9,) if intervals is True else intervals)[0]
        for on, what, why in ((bool(probit), "probit", "its predictive is a probability, not an interval"),
                              (ordinal is not None and ordinal is not False, "ordinal", "its predictive is over levels"),
                              (implicit is not None, "implicit", "its likelihood runs over every cell of the matrix"),
                              (robust is not None, "robust", "a mixture of Student-t distributions needs an incomplete beta function on the device: out of scope"),
                              (getattr(engine, "comm_nranks", lambda: 1)() > 1, "a communicator", "the rings of both sides must be whole on one GPU"),
                              (_os.environ.get("BPMF_REDUCE", "0") not in ("", "0"), "BPMF_REDUCE", "the rings of both sides must be whole on one GPU")):
            if on:
                raise ValueError("intervals does not go together with %s (%s)" % (what, why))
        if T is None:
            raise ValueError("intervals needs a test matrix (its cells get the intervals, its values the calibration)")
        if not (1 <= nsims - burnin <= _engine.HipEngine.INTERVAL_MAX_SAMPLES):
            raise ValueError("intervals needs 1 .. %d post-burn-in samples (nsims - burnin = %d)" % (_engine.HipEngine.INTERVAL_MAX_SAMPLES, nsims - burnin))
    score_on = bool(score)
    if score_on:                                     # (refused before the engine is used)
        for on, what, why in ((ordinal is not None and ordinal is not False, "ordinal", "its held-out log density is res['logp']"),
                              (implicit is not None, "implicit", "its likelihood runs over every cell of the matrix"),
                              (getattr(engine, "comm_nranks", lambda: 1)() > 1, "a communicator", "the rings of both sides must be whole on one GPU"),
                              (_os.environ.get("BPMF_REDUCE", "0") not in ("", "0"), "BPMF_REDUCE", "the rings of both sides must be whole on one GPU")):
            if on:
                raise ValueError("score does not go together with %s (%s)" % (what, why))
        if nsims - burnin < 2:
            raise ValueError("score needs at least 2 post-burn-in samples (nsims - burnin = %d)" % (nsims - burnin))
    diag_on = diagnose is not None and diagnose is not False
    if diag_on:                                      # (refused before the engine is used)
        kept = nsims - burnin
        if not (_engine.HipEngine.DIAG_MIN_SAMPLES <= kept <= _engine.HipEngine.DIAG_MAX_SAMPLES):
            raise ValueError("diagnose needs %d .. %d post-burn-in samples (nsims - burnin = %d)"
                             % (_engine.HipEngine.DIAG_MIN_SAMPLES, _engine.HipEngine.DIAG_MAX_SAMPLES, kept))
        if diagnose is True:
            if T is None:
                raise ValueError("diagnose=True needs a test matrix (or give the cells: diagnose=(rows, cols))")
            diag_rows = np.ascontiguousarray(T[1], np.int32)
            diag_cols = np.repeat(np.arange(len(T[0]) - 1, dtype=np.int32), np.diff(np.asarray(T[0], np.int64)))
        else:
            try:
                diag_rows, diag_cols = (np.ascontiguousarray(v, np.int32) for v in diagnose)
            except (TypeError, ValueError):
                raise ValueError("diagnose must be True or a pair (rows, cols)")
            if diag_rows.ndim != 1 or diag_rows.shape != diag_cols.shape:
                raise ValueError("diagnose = (rows, cols): two one-dimensional arrays of the same length")
    bias_on = bias is not None and bias is not False
    if bias_prior is not None and not bias_on:
        raise ValueError("bias_prior needs bias")
    if bias_on:                                      # (refused before the engine is used)
        bias_lambda = 1.0 if bias is True else bias
        try:
            bias_lambda = float(bias_lambda)
        except (TypeError, ValueError):
            bias_lambda = float("nan")
        if not (math.isfinite(bias_lambda) and bias_lambda > 0):
            raise ValueError("bias = %r: True, or a finite lambda > 0" % (bias,))
        if bias_prior is not None:
            try:
                bias_a0, bias_b0 = (float(v) for v in bias_prior)
            except (TypeError, ValueError):
                raise ValueError("bias_prior must be a pair (A0, B0)")
            if not (bias_a0 > 0 and bias_b0 >= 0 and math.isfinite(bias_a0) and math.isfinite(bias_b0)):
                raise ValueError("bias_prior = (A0, B0) needs a finite A0 > 0 and a finite B0 >= 0")
        for on, what, why in ((pipelined, "pipelined=True", "the evaluation of an iteration reads the bias vectors the next one overwrites: the loop is blocking"),
                              (probit, "probit=True", "a side has one latent step"),
                              (ordinal is not None and ordinal is not False, "ordinal", "a side has one latent step"),
                              (censored is not None, "censored", "a side has one latent step"),
                              (robust is not None, "robust", "a side has one latent step"),
                              (weights is not None, "weights", "the bias conditional is unweighted"),
                              (implicit is not None, "implicit", "the bias conditional would run over every cell"),
                              (row_features is not None or col_features is not None, "row_features / col_features", "the residuals would have to be formed from the bias-free values"),
                              (new_row_features is not None or new_col_features is not None, "new_row_features / new_col_features", "they need features"),
                              (noise == "adaptive", "noise='adaptive'", "the training residuals leave the biases out"),
                              (foldin, "foldin=True", "a folded-in row would need a bias of its own"),
                              (keeps_model, "save_model" if save_model is not None else "keep_rings", "the model format stores no biases"),
                              (similar is not None, "similar", "the two bias rows of the sample ring would enter the cosine"),
                              (getattr(engine, "dtype", "f64") == "f32", "an fp32 engine", "the bias kernels are fp64"),
                              (getattr(engine, "comm_nranks", lambda: 1)() > 1, "a communicator", "the bias step needs both sides whole on one GPU")):
            if on:
                raise ValueError("bias does not go together with %s (%s)" % (what, why))
        if alpha is not None and not (float(alpha) > 0 and math.isfinite(float(alpha))):
            raise ValueError("bias needs a finite alpha > 0")
    if similar is not None:                          # (refused before the engine is used)
        if not (isinstance(similar, (int, np.integer)) and 1 <= int(similar) <= 32):
            raise ValueError("similar = %r: the list length must be an integer in 1 .. 32" % (similar,))
        if similar_by not in ("cols", "rows"):
            raise ValueError("similar_by must be 'cols' or 'rows', not %r" % (similar_by,))
        if similar_kind not in ("cosine", "euclid"):
            raise ValueError("similar_kind must be 'cosine' or 'euclid', not %r" % (similar_kind,))
        if not (isinstance(similar_kappa, (int, float)) and math.isfinite(similar_kappa) and similar_kappa >= 0):
            raise ValueError("similar_kappa = %r must be finite and >= 0" % (similar_kappa,))
        if not (isinstance(similar_min_ratings, (int, np.integer)) and similar_min_ratings >= 0):
            raise ValueError("similar_min_ratings = %r must be an integer >= 0" % (similar_min_ratings,))
        if nsims - burnin < 1:
            raise ValueError("similar needs at least one post-burn-in sample (nsims > burnin)")
    if keeps_model:                                  # (refused before the engine is used)
        for on, what in ((ordinal is not None and ordinal is not False, "ordinal"), (implicit is not None, "implicit"),
                         (row_features is not None or col_features is not None, "row_features / col_features")):
            if on:
                raise ValueError("%s does not go together with %s (serving it would need state that model format 1 does not store)" % (keeps_what, what))
        if nsims - burnin < 1:
            raise ValueError("%s needs at least one post-burn-in sample (nsims > burnin)" % keeps_what)
    if implicit is not None:                         # (refused before the engine is used)
        try:
            implicit = float(implicit)
        except (TypeError, ValueError):
            raise ValueError("implicit must be a number: the weight w0 of an unobserved cell")
        if not (math.isfinite(implicit) and implicit > 0.0):
            raise ValueError("implicit = %r: w0 must be finite and > 0" % (implicit,))
        for on, what, why in ((pipelined, "pipelined=True", "the implicit loop is blocking: G of the other side is formed ahead of every half-iteration"),
                              (probit, "probit=True", "a side has one likelihood"),
                              (ordinal is not None and ordinal is not False, "ordinal", "a side has one likelihood"),
                              (robust is not None, "robust", "the weights of a robust side are redrawn in every half-iteration"),
                              (censored is not None, "censored", "the latent draw would need the confidence of its cell"),
                              (noise == "adaptive", "noise='adaptive'", "alpha | r would need the residuals of every cell"),
                              (row_features is not None or col_features is not None, "row_features / col_features",
                               "the link matrix would need the weighted residuals"),
                              (foldin, "foldin=True", "a folded-in row would need G"),
                              (isinstance(topn_score, (tuple, list)) and len(topn_score) > 0 and topn_score[0] in ("prob", "ei"),
                               "topn_score 'prob' / 'ei'", "their sigma = 1 / sqrt(alpha) is not the noise of a cell; 'ucb' is fine"),
                              (getattr(engine, "dtype", "f64") == "f32", "an fp32 engine", "the weighted samplers are fp64")):
            if on:
                raise ValueError("implicit does not go together with %s (%s)" % (what, why))
        if alpha is not None and not (float(alpha) > 0 and math.isfinite(float(alpha))):
            raise ValueError("implicit needs a finite alpha > 0")
    if rank_eval is not None:                        # (refused before the engine is used)
        if isinstance(rank_eval, bool) or int(rank_eval) != rank_eval or not (1 <= int(rank_eval) <= 1000):
            raise ValueError("rank_eval = %r: the list length N must be an integer 1 .. 1000" % (rank_eval,))
        rank_eval = int(rank_eval)
        if rank_by not in ("rows", "cols"):
            raise ValueError("rank_by must be 'rows' or 'cols', not %r" % (rank_by,))
        if rank_threshold is not None and not math.isfinite(float(rank_threshold)):
            raise ValueError("rank_threshold must be finite")
        if nsims - burnin < 1:
            raise ValueError("rank_eval needs at least one post-burn-in sample (nsims > burnin)")
        if T is None:
            raise ValueError("rank_eval needs a test matrix")
        if rank_threshold is None and implicit is not None:
            rank_threshold = 0.0
        rk_tptr, rk_tcand, rk_cell = held_out_lists(T, nusers if rank_by == "rows" else nmovies, rank_by, rank_threshold)
    elif rank_by != "rows" or rank_threshold is not None:
        raise ValueError("rank_by / rank_threshold need rank_eval=N")
    ordinal_on = ordinal is not None and ordinal is not False
    if ordinal_on:                                   # (refused before the engine is used)
        for on, what, why in ((probit, "probit=True", "a side has one likelihood"),
                              (foldin, "foldin=True", "levels would need a latent iteration of their own"),
                              (noise == "adaptive", "noise='adaptive'", "the latent scores have unit variance"),
                              (censored is not None, "censored", "levels have no bounds"),
                              (weights is not None, "weights", "the latent scores have unit variance"),
                              (robust is not None, "robust", "the latent scores have unit variance"),
                              (row_features is not None or col_features is not None, "row_features / col_features",
                               "the residuals would have to be formed from the latent scores")):
            if on:
                raise ValueError("ordinal does not go together with %s (%s)" % (what, why))
        if alpha is not None and float(alpha) != 1.0:
            raise ValueError("ordinal runs with alpha = 1, not %r" % (alpha,))
        ord_levels = np.unique(np.asarray(M[2], np.float64)) if ordinal is True else np.array(ordinal, np.float64)
        if ord_levels.ndim != 1 or not (2 <= len(ord_levels) <= 16):
            raise ValueError("ordinal: %d levels (2 .. 16 are supported)" % (ord_levels.size if ord_levels.ndim == 1 else -1,))
        if not (np.all(np.isfinite(ord_levels)) and np.all(np.diff(ord_levels) > 0)):
            raise ValueError("ordinal: the levels must be finite and strictly increasing")
        if not np.all(np.isin(np.asarray(M[2], np.float64), ord_levels)):
            raise ValueError("ordinal: a training value is not one of the levels %s" % (ord_levels.tolist(),))
        if T is not None and not np.all(np.isin(np.asarray(T[2], np.float64), ord_levels)):
            raise ValueError("ordinal: a test value is not one of the levels %s" % (ord_levels.tolist(),))
        if cutpoints is not None:
            cutpoints = np.array(cutpoints, np.float64)
            if cutpoints.ndim != 1 or len(cutpoints) != len(ord_levels) - 1:
                raise ValueError("ordinal: %d levels need %d cutpoints" % (len(ord_levels), len(ord_levels) - 1))
            if not (np.all(np.isfinite(cutpoints)) and np.all(np.diff(cutpoints) > 0)):
                raise ValueError("ordinal: the cutpoints must be finite and strictly increasing")
        elif len(M[2]) == 0:
            raise ValueError("ordinal: a training matrix without ratings has no default cutpoints")
        if ordinal_step is not None:
            ordinal_step = float(ordinal_step)
            if not (ordinal_step > 0 and math.isfinite(ordinal_step)):
                raise ValueError("ordinal_step must be positive and finite")
        alpha = 1.0
    elif cutpoints is not None or ordinal_step is not None:
        raise ValueError("cutpoints / ordinal_step need ordinal")
    if robust is not None:                           # (refused before the engine is used)
        try:
            robust = float(robust)
        except (TypeError, ValueError):
            raise ValueError("robust must be a number: the degrees of freedom nu >= 1")
        if not (math.isfinite(robust) and robust >= 1.0):
            raise ValueError("robust = %r: the degrees of freedom nu must be finite and >= 1" % (robust,))
        if weights is not None:
            raise ValueError("robust does not go together with weights (the weights of a robust side are redrawn in every half-iteration)")
        if probit:
            raise ValueError("robust does not go together with probit=True (the latent scores have unit variance)")
        if censored is not None:
            raise ValueError("robust does not go together with censored (the latent draw would need the weight of its cell)")
        if noise == "adaptive":
            raise ValueError("robust does not go together with noise='adaptive' (alpha | r would need the weighted residuals)")
        if row_features is not None or col_features is not None:
            raise ValueError("robust does not go together with row_features / col_features (the link matrix would need the weighted residuals)")
        if getattr(engine, "dtype", "f64") == "f32":
            raise ValueError("robust needs an fp64 engine")
        if topn_score is not None and isinstance(topn_score, (tuple, list)) and len(topn_score) > 0 and topn_score[0] in ("prob", "ei"):
            raise ValueError("robust does not go together with topn_score %r (its sigma = 1 / sqrt(alpha) assumes Gaussian noise; "
                             "'ucb' is fine)" % (topn_score[0],))
        if alpha is not None and not (float(alpha) > 0 and math.isfinite(float(alpha))):
            raise ValueError("robust needs a finite alpha > 0")
    if weights is not None and implicit is None:     # (refused before the engine is used)
        if probit:
            raise ValueError("weights does not go together with probit=True (the latent scores have unit variance)")
        if censored is not None:
            raise ValueError("weights does not go together with censored (the latent draw would need the weight of its cell)")
        if noise == "adaptive":
            raise ValueError("weights does not go together with noise='adaptive' (alpha | r would need the weighted residuals)")
        if row_features is not None or col_features is not None:
            raise ValueError("weights does not go together with row_features / col_features (the link matrix would need the weighted residuals)")
        if getattr(engine, "dtype", "f64") == "f32":
            raise ValueError("weights needs an fp64 engine")
    if foldin:                                       # (refused before the engine is used)
        if probit:
            raise ValueError("foldin=True does not go together with probit=True (labels would need a latent iteration of their own)")
        if row_features is not None and col_features is not None:
            raise ValueError("foldin=True: both sides have features, so neither can be folded into (the prior mean of a new row "
                             "needs its features: new_row_features / new_col_features)")
        if nsims - burnin < 1:
            raise ValueError("foldin=True needs at least one post-burn-in sample (nsims > burnin)")
    if topn_score is not None:                       # (refused before the engine is used)
        if topn is None:
            raise ValueError("topn_score needs topn=N (it ranks the top-N lists)")
        try:
            score_kind, score_param = topn_score
            score_param = float(score_param)
        except (TypeError, ValueError):
            raise ValueError("topn_score must be a pair (kind, parameter): ('ucb', kappa), ('prob', t) or ('ei', t)")
        if score_kind not in ("ucb", "prob", "ei"):
            raise ValueError("topn_score: unknown kind %r (one of 'ucb', 'prob', 'ei')" % (score_kind,))
        if not math.isfinite(score_param):
            raise ValueError("topn_score: the parameter of %r must be finite" % (score_kind,))
        if score_kind != "ucb" and noise == "adaptive":
            raise ValueError("topn_score %r does not go together with noise='adaptive' (alpha is not a single number, and sigma = "
                             "1 / sqrt(alpha) is part of the score)" % (score_kind,))
    for new, have, nn, hn in ((new_row_features, row_features, "new_row_features", "row_features"),
                              (new_col_features, col_features, "new_col_features", "col_features")):
        if new is None:
            continue
        if have is None:
            raise ValueError("%s needs %s (the link matrix is fitted on the training entities' features)" % (nn, hn))
        if _engine._is_sparse(new) != _engine._is_sparse(have):
            raise ValueError("%s and %s must be of the same kind (both dense or both sparse)" % (nn, hn))
        if not _engine._is_sparse(new):
            new = np.asarray(new, np.float64)
        if new.ndim != 2 or new.shape[0] < 1 or new.shape[1] != np.shape(have)[1]:
            raise ValueError("%s must be [n_new >= 1, %d]: the D of %s" % (nn, np.shape(have)[1], hn))
        if not np.all(np.isfinite(new.data if _engine._is_sparse(new) else new)):
            raise ValueError("%s holds a value that is not finite" % nn)
        if nsims - burnin < 1:
            raise ValueError("%s needs at least one post-burn-in sample (nsims > burnin)" % nn)
    linked = row_features is not None or col_features is not None
    if censored is not None:
        if probit:
            raise ValueError("censored does not go together with probit=True (labels have no bounds)")
        if noise == "adaptive":
            raise ValueError("censored does not go together with noise='adaptive' (alpha | y needs a fresh draw of every censored "
                             "value from the newest factors of both sides)")
        if linked:
            raise ValueError("censored does not go together with row_features / col_features (the residuals would have to be "
                             "formed from the latent values)")
    if linked:
        if pipelined:
            raise ValueError("pipelined=True does not go together with row_features / col_features (the features loop is blocking)")
        if probit:
            raise ValueError("probit=True does not go together with row_features / col_features")
        if noise == "adaptive":
            raise ValueError("noise='adaptive' does not go together with row_features / col_features")
        if not (float(lambda_beta) > 0 and math.isfinite(float(lambda_beta))):
            raise ValueError("lambda_beta must be positive and finite")
        if not (0.0 < float(link_tol) < 1.0) or int(link_max_iter) < 1:
            raise ValueError("link_tol must lie in (0, 1) and link_max_iter must be >= 1")
    if lambda_beta_prior is not None:
        if not linked:
            raise ValueError("lambda_beta_prior needs row_features or col_features")
        try:
            lb_a0, lb_b0 = (float(v) for v in lambda_beta_prior)
        except (TypeError, ValueError):
            raise ValueError("lambda_beta_prior must be a pair (A0, B0)")
        if not (lb_a0 > 0 and lb_b0 >= 0 and math.isfinite(lb_a0) and math.isfinite(lb_b0)):
            raise ValueError("lambda_beta_prior = (A0, B0) needs a finite A0 > 0 and a finite B0 >= 0")
    if topn is not None and nsims - burnin < 1:
        raise ValueError("topn needs at least one post-burn-in sample (nsims > burnin)")
    if noise not in ("fixed", "adaptive"):
        raise ValueError("noise must be 'fixed' or 'adaptive', not %r" % (noise,))
    adaptive = noise == "adaptive"
    if probit:
        if adaptive:
            raise ValueError("probit=True does not go together with noise='adaptive' (the latent scores have unit variance)")
        if alpha is not None and float(alpha) != 1.0:
            raise ValueError("probit=True runs with alpha = 1, not %r" % (alpha,))
        if not math.isfinite(float(threshold)):
            raise ValueError("threshold must be finite")
        alpha = 1.0
    elif alpha is None:
        alpha = 2.0
    a0, b0 = (float(alpha_prior[0]), float(alpha_prior[1])) if adaptive else (0.0, 0.0)
    if adaptive and not (a0 > 0 and b0 >= 0):
        raise ValueError("alpha_prior = (a0, b0) needs a0 > 0 and b0 >= 0")
    if censored is not None:                         # (checked before a side is created)
        if not (float(alpha) > 0 and math.isfinite(float(alpha))):
            raise ValueError("censored needs a finite alpha > 0")
        cflags = (censor_flags(M, censored), censor_flags(Mt, transpose_csc(censored, nusers)))
    if weights is not None:                          # (checked before a side is created)
        wts = (rating_weights(M, weights), rating_weights(Mt, transpose_csc(weights, nusers)))
    if implicit is not None:
        if weights is None:
            wts = (np.ones(len(M[2])), np.ones(len(Mt[2])))
        low = ~(wts[0] > implicit)
        if low.any():
            raise ValueError("implicit: the confidence %r of training rating %d is not > w0 = %r" % (float(wts[0][int(np.argmax(low))]), int(np.argmax(low)), implicit))
    Sys.nsims, Sys.burnin, Sys.alpha = nsims, burnin, alpha
    movies = Sys("movs", engine, M, nmovies, nusers, T=T, mean_rating=0.0 if probit or ordinal_on or implicit is not None else None)
    users = Sys("users", engine, Mt, nusers, nmovies, T=Tt, mean_rating=0.0 if probit or ordinal_on or implicit is not None else None)
    if chain:
        engine.side_set_chain(movies.side, chain); engine.side_set_chain(users.side, chain)
        movies.key_offset = users.key_offset = chain * CHAIN_STRIDE
    if ordinal_on:
        engine.set_ordinal(movies.side, ord_levels, cutpoints, ORDINAL_TAGS[0])
        engine.set_ordinal(users.side, ord_levels, engine.ordinal_cut_get(movies.side), ORDINAL_TAGS[1])   # (the same bits on both sides)
        ord_sampled = cutpoints is None
        ord_s = ordinal_step if ordinal_step is not None else 1.0 / math.sqrt(max(len(M[2]), 1))
    if probit:
        engine.set_probit(movies.side, threshold, 1)
        engine.set_probit(users.side, threshold, 2)
    if censored is not None:
        engine.set_censored(movies.side, cflags[0], 5)
        engine.set_censored(users.side, cflags[1], 6)
    if implicit is not None:
        engine.set_implicit(movies.side, implicit, wts[0])
        engine.set_implicit(users.side, implicit, wts[1])
        movies.implicit = users.implicit = True
    elif weights is not None:
        engine.set_weights(movies.side, wts[0])
        engine.set_weights(users.side, wts[1])
    if robust is not None:
        engine.set_robust(movies.side, robust, ROBUST_TAGS[0])
        engine.set_robust(users.side, robust, ROBUST_TAGS[1])
    if bias_on:
        engine.set_bias(movies.side, bias_lambda, BIAS_TAGS[0], 0)
        engine.set_bias(users.side, bias_lambda, BIAS_TAGS[1], 1)
        if bias_prior is not None:
            engine.bias_prior(movies.side, bias_a0, bias_b0)
            engine.bias_prior(users.side, bias_a0, bias_b0)
    if linked:
        if col_features is not None:
            engine.set_features(movies.side, col_features, lambda_beta, 3)
        if row_features is not None:
            engine.set_features(users.side, row_features, lambda_beta, 4)
        movies.linked = users.linked = True
        movies.linked_features, users.linked_features = col_features is not None, row_features is not None
        sparse_sides = [sd for sd, F in ((movies, col_features), (users, row_features)) if F is not None and _engine._is_sparse(F)]
        for sd in sparse_sides:
            engine.link_cg_set(sd.side, link_tol, link_max_iter)
        if lambda_beta_prior is not None:
            for sd, F in ((movies, col_features), (users, row_features)):
                if F is not None:
                    engine.link_lambda_prior(sd.side, lb_a0, lb_b0)
    if Tt is not None:
        movies.set_twin(users)                       # users.predict(movies) rides with movies.predict(users)
    res = dict(rmse=[], rmse_avg=[], norm_u=[], norm_m=[], secs=[], samples=[], chain=chain)
    ring_movies = topn is not None or new_row_features is not None or foldin or rank_eval is not None or keeps_model or similar is not None or diag_on or score_on or intervals_on or loo_on   # a side's sample ring: topn, or the other side's new entities
    ring_users = topn is not None or new_col_features is not None or foldin or rank_eval is not None or keeps_model or similar is not None or diag_on or score_on or intervals_on or loo_on
    hyper_sides = [sd for sd, F in ((users, row_features), (movies, col_features)) if (foldin or (keeps_model and not probit)) and F is None]
    for sd in hyper_sides:
        engine.hyper_reserve(sd.side, nsims - burnin)
    if ring_movies:
        engine.samples_reserve(movies.side, nsims - burnin)
    if ring_users:
        engine.samples_reserve(users.side, nsims - burnin)
    if new_row_features is not None:
        engine.newrows_set(users.side, new_row_features, nsims - burnin)
    if new_col_features is not None:
        engine.newrows_set(movies.side, new_col_features, nsims - burnin)

    if linked and sparse_sides:
        res["link_cg_iters"] = []
        res["link_cg_hit_max_iter"] = False
    if lambda_beta_prior is not None:
        res["lambda_beta_rows"] = [] if row_features is not None else None
        res["lambda_beta_cols"] = [] if col_features is not None else None

    def keep(i):                                     # where the -o aggregation sits (bpmf_main.cpp)
        if ring_users and i >= burnin:
            engine.samples_add(users.side)
        if ring_movies and i >= burnin:
            engine.samples_add(movies.side)
        if i >= burnin:
            for sd in hyper_sides:                   # (mu, Lambda) this iteration's half-iteration of the side ran with, and its alpha
                engine.hyper_add(sd.side, Sys.alpha)
        if new_row_features is not None and i >= burnin:
            engine.newrows_add(users.side, movies.side)
        if new_col_features is not None and i >= burnin:
            engine.newrows_add(movies.side, users.side)
        if robust is not None and i >= burnin:
            engine.robust_add(movies.side)
        if bias_on and i >= burnin:
            engine.bias_add(movies.side)
            engine.bias_add(users.side)
        if probit and i >= burnin and movies.test is not None:
            engine.probit_add(movies.test, movies.side, users.side)
        if ordinal_on and i >= burnin and movies.test is not None:
            engine.ordinal_add(movies.test, movies.side, users.side)
        if linked and i >= burnin:
            if col_features is not None:
                engine.link_add(movies.side)
            if row_features is not None:
                engine.link_add(users.side)
        if lambda_beta_prior is not None:
            if col_features is not None:
                res["lambda_beta_cols"].append(engine.link_lambda_get(movies.side)[0])
            if row_features is not None:
                res["lambda_beta_rows"].append(engine.link_lambda_get(users.side)[0])
        if linked and sparse_sides:
            st = [engine.link_cg_stats(sd.side) if sd in sparse_sides else None for sd in (movies, users)]
            res["link_cg_iters"].append(tuple(None if t is None else t["iters_last"] for t in st))
            res["link_cg_hit_max_iter"] = res["link_cg_hit_max_iter"] or any(t is not None and t["hit_max_iter"] for t in st)

    if adaptive:
        res["alpha"], res["train_rmse"] = [], []
    if ordinal_on:
        res["ordinal"] = dict(levels=ord_levels.copy(), cutpoints=[engine.ordinal_cut_get(movies.side)], accepted=[False], step=[ord_s])

    def cut(i):                                      # after both sides of iteration i: the cutpoints of iteration i + 1
        nonlocal ord_s
        if not ordinal_on or i + 1 >= nsims:
            return
        acc = False
        if ord_sampled:
            acc = engine.ordinal_cut_step(movies.side, users.side, i + 1, ord_s)
        o = res["ordinal"]
        o["accepted"].append(acc); o["step"].append(ord_s)
        o["cutpoints"].append(engine.ordinal_cut_get(movies.side) if acc else o["cutpoints"][-1])
        if ord_sampled and ordinal_step is None and i + 1 < burnin:
            ord_s = math.exp(math.log(ord_s) + ((1.0 if acc else 0.0) - 0.35) / math.sqrt(i + 2))

    def adapt(i):                                    # after both sides of iteration i: the alpha of iteration i + 1
        if not adaptive:
            return
        res["alpha"].append(Sys.alpha)
        sse, n = engine.train_sse(movies.side, users.side)
        res["train_rmse"].append(math.sqrt(sse / n))
        if i + 1 < nsims:
            Sys.alpha = engine.noise_sample(a0, b0, sse, n, i + chain * CHAIN_STRIDE, alpha_max)
    nnz = movies.local_nnz

    def line(it, secs, norm_u, norm_m):
        ips = (users.num() + movies.num()) / secs
        if out is not None:
            saved, movies.iter = movies.iter, it
            out.write(movies.format_line(ips, nnz / secs, math.sqrt(norm_u), math.sqrt(norm_m)))
            movies.iter = saved
        res["rmse"].append(movies.rmse); res["rmse_avg"].append(movies.rmse_avg)
        res["norm_u"].append(math.sqrt(norm_u)); res["norm_m"].append(math.sqrt(norm_m))
        res["secs"].append(secs)

    if pipelined and not keep_samples and hasattr(engine, "sys_norm"):
        mark = time.perf_counter()
        for i in range(nsims):
            movies.sample(users)
            users.sample(movies)
            keep(i)
            adapt(i)
            cut(i)
            if i > 0:
                norm_m = engine.sys_norm(movies.side, i - 1)
                norm_u = engine.sys_norm(users.side, i - 1)
                movies.predict_finish()
                if Tt is not None:
                    users.predict_finish()
                now = time.perf_counter()
                line(i - 1, now - mark, norm_u, norm_m)
                mark = now
            movies.predict_launch(users)
        if nsims > 0:
            movies.predict_finish()
            if Tt is not None:
                users.predict_finish()
            movies.refresh(); users.refresh()
            line(nsims - 1, time.perf_counter() - mark, users.norm, movies.norm)
    else:
        for i in range(nsims):
            start = time.perf_counter()
            movies.sample(users)
            users.sample(movies)
            keep(i)
            adapt(i)
            cut(i)
            movies.predict(users)
            if Tt is not None:
                users.predict(movies)                # c++/bpmf.cpp:190 (nothing reads its results; Tt = None leaves it out)
            stop = time.perf_counter()
            movies.refresh(); users.refresh()
            line(i, stop - start, users.norm, movies.norm)
            if keep_samples:
                res["samples"].append((users.items(), movies.items()))
    movies.predict(users, True)                      # c++/bpmf.cpp:242 (the extra call of Q6)
    if Tt is not None:
        users.predict(movies)                        # (the twin was evaluated with it: collect its sums)
    res["final_rmse_avg"] = movies.rmse_avg
    res["num_predict"] = movies.num_predict
    res["U"] = users.items(); res["V"] = movies.items()
    if similar is not None:
        sim_side, sim_M = (movies, M) if similar_by == "cols" else (users, Mt)
        ok = np.diff(np.asarray(sim_M[0])) >= similar_min_ratings if similar_min_ratings > 0 else None
        idx, score, mean, std = engine.similar(sim_side.side, int(similar), similar_kind, float(similar_kappa), cand_ok=ok)
        res["similar"] = dict(by=similar_by, kind=similar_kind, kappa=float(similar_kappa), idx=idx, score=score, mean=mean, std=std)
    if topn is not None:
        if topn_score is None:
            res["topn"] = engine.topn(users.side, movies.side, movies.mean_rating, topn)
        else:
            sigma = 0.0 if score_kind == "ucb" else 1.0 / math.sqrt(float(alpha))
            res["topn"] = engine.topn_scored(users.side, movies.side, movies.mean_rating, topn, score_kind, score_param, sigma)
    if probit:
        have = movies.test is not None and movies.T_nnz > 0 and nsims > burnin
        res["prob"] = engine.probit_get(movies.test)[0] if have else np.zeros(0)
        label = (np.asarray(T[2]) > threshold).astype(np.float64) if have else np.zeros(0)
        res["auc"] = _engine.auc(res["prob"], label, 0.5) if have else float("nan")
        res["brier"] = float(np.mean((res["prob"] - label) ** 2)) if have else float("nan")
    if ordinal_on:
        o = res["ordinal"]
        o["cutpoints"] = np.array(o["cutpoints"][:max(nsims, 1)]).reshape(-1, len(ord_levels) - 1)
        have = movies.test is not None and movies.T_nnz > 0 and nsims > burnin
        res["cat_prob"] = engine.ordinal_get(movies.test)[0] if have else np.zeros((0, len(ord_levels)))
        res["expected"] = res["cat_prob"] @ ord_levels
        if have:
            true = np.searchsorted(ord_levels, np.asarray(T[2], np.float64))
            with np.errstate(divide="ignore"):
                res["logp"] = float(np.mean(np.log(res["cat_prob"][np.arange(len(true)), true])))
        else:
            res["logp"] = float("nan")
    if censored is not None:
        res["censored"] = engine.censored_count(movies.side)
    if rank_eval is not None:
        qs, cs = (users, movies) if rank_by == "rows" else (movies, users)
        rk, ncand = engine.rank_eval(qs.side, cs.side, rk_tptr, rk_tcand, movies.mean_rating)
        per_cell = np.zeros(len(T[2]), np.int32)
        per_cell[rk_cell] = rk
        res["rank"] = dict(rank_metrics(rk, rk_tptr, ncand, rank_eval), n=rank_eval, by=rank_by, rank=per_cell, ncand=ncand)
    if implicit is not None:
        res["implicit"] = dict(w0=implicit, observed=len(M[2]), cells=int(nusers) * int(nmovies), weights=engine.weights_count(movies.side))
    elif weights is not None:
        res["weights"] = engine.weights_count(movies.side)
    if robust is not None:
        kept = max(nsims - burnin, 0)
        wm = engine.robust_get(movies.side)[0] if kept > 0 else np.zeros(len(M[2]))
        res["robust"] = dict(nu=robust, weight_mean=wm, kept=kept)
    if bias_on:
        kept = max(nsims - burnin, 0)
        res["bias"] = dict(rows_mean=engine.bias_mean(users.side)[0] if kept > 0 else np.zeros(nusers),
                           cols_mean=engine.bias_mean(movies.side)[0] if kept > 0 else np.zeros(nmovies),
                           lambda_rows=engine.bias_lambda(users.side, nsims)[1], lambda_cols=engine.bias_lambda(movies.side, nsims)[1], kept=kept)
    if linked:
        res["beta_rows"] = engine.link_mean(users.side)[0] if row_features is not None and nsims > burnin else None
        res["beta_cols"] = engine.link_mean(movies.side)[0] if col_features is not None and nsims > burnin else None
    if new_row_features is not None:
        mean, std = engine.newrows_predict(users.side, movies.side, movies.mean_rating)
        res["new_rows"] = dict(mean=mean, std=std)
        if topn is not None:
            res["new_rows_topn"] = engine.newrows_topn(users.side, movies.side, movies.mean_rating, topn)
    if new_col_features is not None:
        mean, std = engine.newrows_predict(movies.side, users.side, movies.mean_rating)
        res["new_cols"] = dict(mean=mean.T.copy(), std=std.T.copy())
        if topn is not None:
            res["new_cols_topn"] = engine.newrows_topn(movies.side, users.side, movies.mean_rating, topn)
    if foldin:
        res["foldin"] = True
    res["movies"], res["users"] = movies, users
    plain = not ordinal_on and implicit is None and not linked      # what bpmf_amd.save_model can store of this run
    res["model_info"] = dict(alpha=float(alpha), probit=bool(probit), probit_threshold=float(threshold) if probit else 0.0, plain=plain,
                             why="ordinal, implicit and feature models are not stored by model format 1",
                             nu=float(robust) if robust is not None else None,                       # (bpmf_amd.score_cells: the likelihood ..
                             alpha_samples=[float(a) for a in res["alpha"][burnin:nsims]] if adaptive else None,   # .. and the alpha of every kept sample)
                             scored=not ordinal_on and implicit is None)
    if save_model is not None:
        from .model import save_model as _save_model
        _save_model(res, save_model)
    if diag_on:
        from .model import diagnose as _diagnose
        res["diag"] = _diagnose(res, diag_rows, diag_cols)
        keys = ["rmse", "norm_u", "norm_m"] + (["alpha"] if adaptive else [])
        rhat, ess = engine.diag_traces(np.array([res[k][burnin:nsims] for k in keys], np.float64))
        res["diag"]["scalars"] = {k: (float(rhat[i]), float(ess[i])) for i, k in enumerate(keys)}
    if score_on:
        from .model import score_cells as _score_cells
        res["score"] = {}
        if T is not None:
            t_cols = np.repeat(np.arange(len(T[0]) - 1, dtype=np.int32), np.diff(np.asarray(T[0], np.int64)))
            res["score"]["test"] = _score_cells(res, T[1], t_cols, T[2])
        m_cols = np.repeat(np.arange(len(M[0]) - 1, dtype=np.int32), np.diff(np.asarray(M[0], np.int64)))
        res["score"]["train"] = _score_cells(res, M[1], m_cols, M[2], weights=wts[0] if weights is not None else None,
                                             flags=cflags[0] if censored is not None else None)
    if intervals_on:
        from .model import predict_intervals as _predict_intervals
        t_cols = np.repeat(np.arange(len(T[0]) - 1, dtype=np.int32), np.diff(np.asarray(T[0], np.int64)))
        res["intervals"] = dict(test=_predict_intervals(res, T[1], t_cols, interval_levels, values=T[2]))
    if loo_on:
        from .model import loo_cells as _loo_cells
        m_cols = np.repeat(np.arange(len(M[0]) - 1, dtype=np.int32), np.diff(np.asarray(M[0], np.int64)))
        res["loo"] = _loo_cells(res, M[1], m_cols, M[2], weights=wts[0] if weights is not None else None,
                                flags=cflags[0] if censored is not None else None)
    if out is not None:
        out.write("Final Avg RMSE: %g\n" % movies.rmse_avg)
    return res


FOLDIN_TAGS = {"rows": 7, "cols": 8}                 # the random streams of folded-in users / movies (1 .. 6 and 9, 10 are taken: gibbs)
ORDINAL_TAGS = (11, 12)                              # the random streams of the latent scores of ordinal sides: movies, users
BIAS_TAGS = (13, 14)                                 # the random streams of the bias draws: movies, users
ROBUST_TAGS = (9, 10)                                # the random streams of the weights of Student-t noise: movies, users


def fold_in(res, new_rows=None, new_cols=None, topn=None, draw=True):
    """Predictions for users / movies that arrived after the run `res` = gibbs(..., foldin=True), from their ratings alone (DESIGN.md
    section 19).  new_rows: scipy.sparse [n_new, nmovies], the ratings of new users; new_cols: scipy.sparse [nusers, n_new], the
    ratings of new movies (oriented as the training matrix).  Every kept sample gives one draw of an entity's factors from their
    conditional given that sample of the other side (draw=False: the conditional mean); mean and std are those of the predictions
    over the samples (the observation noise 1 / alpha is not part of std).

    Returns a dict with "rows": dict(mean, std), [n_new, nmovies] each, and / or "cols": dict(mean, std), [nusers, n_new] each;
    with topn=N each also has "topn": (idx, mean, std), [n_new, N] each, the new entities as the queries and their own ratings
    excluded (the format of res["new_rows_topn"]).  The engine of the run must still be open."""
    if not isinstance(res, dict) or not res.get("foldin"):
        raise ValueError("fold_in needs the result of gibbs(..., foldin=True) (the kept samples and hyper-parameters)")
    if new_rows is None and new_cols is None:
        raise ValueError("fold_in: give new_rows and / or new_cols")
    if topn is not None and int(topn) < 1:
        raise ValueError("fold_in: topn must be >= 1")
    users, movies = res["users"], res["movies"]
    jobs = []
    for key, new, side, cand in (("rows", new_rows, users, movies), ("cols", new_cols, movies, users)):
        if new is None:
            continue
        if not _engine._is_sparse(new):
            raise ValueError("fold_in: new_%s must be a scipy.sparse matrix" % key)
        if getattr(side, "linked_features", False):
            raise ValueError("fold_in: the %s have features: the prior mean of a new one needs its features (gibbs(new_%s_features=))"
                             % ("users" if key == "rows" else "movies", "row" if key == "rows" else "col"))
        R = new.tocsr() if key == "rows" else new.T.tocsr()
        if R.shape[1] != cand.num() or R.shape[0] < 1:
            raise ValueError("fold_in: new_%s must be %s" % (key, "[n_new >= 1, %d]" % cand.num() if key == "rows" else "[%d, n_new >= 1]" % cand.num()))
        if not np.all(np.isfinite(R.data)):
            raise ValueError("fold_in: new_%s holds a rating that is not finite" % key)
        jobs.append((key, R, side, cand))
    out = {}
    for key, R, side, cand in jobs:
        engine = side.engine
        engine.foldin(side.side, cand.side, movies.mean_rating, R, FOLDIN_TAGS[key], draw)
        mean, std = engine.foldin_predict(side.side, cand.side, movies.mean_rating)
        out[key] = dict(mean=mean, std=std) if key == "rows" else dict(mean=mean.T.copy(), std=std.T.copy())
        if topn is not None:
            out[key]["topn"] = engine.foldin_topn(side.side, cand.side, movies.mean_rating, int(topn))
    return out


if __name__ == "__main__":
    _sys.exit("use the `bpmf` executable (bpmf_amd/csrc) or bench.py")
