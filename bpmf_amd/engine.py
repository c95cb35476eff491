"""HipEngine: numpy-facing wrapper of the C ABI (device = one MI355X).

The engine interface (side_create / sample_side / predict / items get/set /
hyper_sample) is what `Sys` is written against.
"""
import ctypes as C

import numpy as np

from . import _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class _Side:
    def __init__(self, handle, K, ncols, nrows, col_from, col_to, keep):
        self.handle, self.K, self.ncols, self.nrows = handle, K, ncols, nrows
        self.col_from, self.col_to = col_from, col_to
        self.nnz = 0               # ratings of the local columns (set by side_create / side_create_dev)
        self._keep = keep          # arrays / tensors that must outlive the handle


class _Tensor:
    def __init__(self, handle, dims, nnz, mean_rating, sides):
        self.handle, self.dims, self.nnz, self.mean_rating = handle, dims, nnz, mean_rating
        self.sides = sides         # the three modes as sides (owned by the tensor: get_items / set_items / aggr_add / kernel_name ...)
        self.tests = []            # [handle, entries] of its live test sets


class HipEngine:
    """One context = one GPU + one stream.  `stream` is an integer hipStream_t or None."""

    name = "hip"

    def __init__(self, K, device=0, stream=None, dtype="f64"):
        """dtype "f64": the reference's arithmetic, any num_latent 1 .. 128 (8, 16, 32, 64, 128 have kernels of their own, any other
        K runs on the next of those sizes with zero rows in the extra dimensions: ld()); "f32": the opt-in large-K mixed
        precision path, num_latent 65 .. 128 (fp32 factors / Gram / factorisation, fp64 everything else)."""
        self.lib = _lib.load_library()
        self.K = int(K)
        self.dtype = dtype
        code = {"f64": 0, "f32": 1}[dtype]
        h = C.c_void_p()
        _lib.check(self.lib.bpmf_hip_ctx_create_ex(int(device), self.K, code, C.c_void_p(stream) if stream else None, C.byref(h)))
        self.ctx = h
        self.device = device
        self._sides = []

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            for t in getattr(self, "_tests", []):
                if t[0]:
                    self.lib.bpmf_hip_test_destroy(t[0])
                    t[0] = None
            for t in getattr(self, "_tensors", []):
                self.tensor_destroy(t)
            for s in self._sides:
                if s.handle:
                    self.lib.bpmf_hip_side_destroy(s.handle)
                    s.handle = None
            self.lib.bpmf_hip_ctx_destroy(self.ctx)
            self.ctx = None

    def set_no_covariance(self, on):
        """The reference's BPMF_NO_COVARIANCE build as a switch: diagonal Lambda* only."""
        _lib.check(self.lib.bpmf_hip_ctx_set_no_covariance(self.ctx, 1 if on else 0))

    def sync(self):
        _lib.check(self.lib.bpmf_hip_ctx_sync(self.ctx))

    # -- multi-GPU (RCCL inside the library) -------------------------------------
    def comm_unique_id(self):
        buf = (C.c_char * 128)()
        _lib.check(self.lib.bpmf_hip_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, unique_id):
        buf = (C.c_char * 128).from_buffer_copy(unique_id)
        _lib.check(self.lib.bpmf_hip_ctx_comm_init(self.ctx, int(nranks), int(rank), buf))
        self.nranks, self.rank = int(nranks), int(rank)

    def comm_streams(self):
        """0 = no communicator, 1 = one, 2 = a second one split off for the statistics / evaluation streams (ncclCommSplit)"""
        return int(self.lib.bpmf_hip_ctx_comm_streams(self.ctx))

    def comm_nranks(self):
        """Ranks of the communicator as the communication library counts them (1 without one)."""
        return int(self.lib.bpmf_hip_ctx_comm_nranks(self.ctx))

    def side_set_ranges(self, side, bounds):
        b = np.ascontiguousarray(bounds, np.int64)
        _lib.check(self.lib.bpmf_hip_side_set_ranges(side.handle, _ptr(b)))

    def side_set_overlap(self, side, nparts):
        """Cut every rank's range into `nparts` parts: part c is exchanged while part c + 1 is sampled (collective)."""
        _lib.check(self.lib.bpmf_hip_side_set_overlap(side.handle, int(nparts)))

    def side_set_staleness(self, side, k):
        """Bounded-staleness exchange: a part of the side travels every (k + 1)-th half-iteration only (include/bpmf_hip.h)."""
        _lib.check(self.lib.bpmf_hip_side_set_staleness(side.handle, int(k)))

    def sys_set_reduce(self, a, b, on=True):
        """BPMF_REDUCE formulation for the pair of sides (preComputeMuLambda + reduce onto the owners; include/bpmf_hip.h)."""
        _lib.check(self.lib.bpmf_hip_sys_set_reduce(a.handle, b.handle, 1 if on else 0))

    def side_set_conn(self, side, send_ptr=None, send_cols=None, recv_ptr=None, recv_cols=None):
        """Connectivity-aware exchange lists (include/bpmf_hip.h); all None: back to the all-gather form."""
        if send_ptr is None:
            _lib.check(self.lib.bpmf_hip_side_set_conn(side.handle, None, None, None, None))
            return
        sp = np.ascontiguousarray(send_ptr, np.int64); sc = np.ascontiguousarray(send_cols, np.int32)
        rp = np.ascontiguousarray(recv_ptr, np.int64); rc = np.ascontiguousarray(recv_cols, np.int32)
        _lib.check(self.lib.bpmf_hip_side_set_conn(side.handle, _ptr(sp), _ptr(sc) if len(sc) else None,
                                                   _ptr(rp), _ptr(rc) if len(rc) else None))

    def side_exchange(self, side):
        _lib.check(self.lib.bpmf_hip_side_exchange(side.handle))

    # -- sides ----------------------------------------------------------------
    def side_create(self, ncols, nrows, colptr, rowidx, vals, mean_rating, col_from=0, col_to=None):
        col_to = ncols if col_to is None else col_to
        colptr = np.ascontiguousarray(colptr, np.int64)
        rowidx = np.ascontiguousarray(rowidx, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        assert len(colptr) == col_to - col_from + 1
        h = C.c_void_p()
        _lib.check(self.lib.bpmf_hip_side_create(self.ctx, ncols, nrows, col_from, col_to, _ptr(colptr), _ptr(rowidx),
                                                 _ptr(vals), float(mean_rating), C.byref(h)))
        s = _Side(h, self.K, ncols, nrows, col_from, col_to, None)
        s.nnz = int(colptr[-1])
        self._sides.append(s)
        return s

    def side_create_dev(self, ncols, nrows, colptr_host, rowidx_dev_ptr, vals_dev_ptr, mean_rating, col_from=0,
                        col_to=None, keep=None):
        col_to = ncols if col_to is None else col_to
        colptr_host = np.ascontiguousarray(colptr_host, np.int64)
        h = C.c_void_p()
        _lib.check(self.lib.bpmf_hip_side_create_dev(self.ctx, ncols, nrows, col_from, col_to, _ptr(colptr_host),
                                                     C.c_void_p(rowidx_dev_ptr), C.c_void_p(vals_dev_ptr),
                                                     float(mean_rating), C.byref(h)))
        s = _Side(h, self.K, ncols, nrows, col_from, col_to, keep)
        s.nnz = int(colptr_host[-1])
        self._sides.append(s)
        return s

    def side_destroy(self, side):
        for t in getattr(self, "_tests", []):                      # test matrices go before the side they sit on
            if t[0] and t[2] is side:
                self.test_destroy(t)
        if side.handle:
            _lib.check(self.lib.bpmf_hip_side_destroy(side.handle))
            side.handle = None

    def items_dev_ptr(self, side):
        return self.lib.bpmf_hip_side_items_dev(side.handle)

    def ld(self):
        """Rows per column of the context's DEVICE arrays (bpmf_hip_ctx_ld): K for 8 / 16 / 32 / 64 / 128, else the next of those."""
        return int(self.lib.bpmf_hip_ctx_ld(self.ctx))

    def bind_items(self, side, dev_ptr, keep=None, ld=None, nbytes=None):
        """`ld` / `nbytes`: what the caller allocated (default: the caller's K x ncols doubles); the library refuses storage
        whose leading dimension is not the context's or that is too small (a padded num_latent needs ld() rows per column)."""
        ld = self.K if ld is None else int(ld)
        nbytes = 8 * ld * side.ncols if nbytes is None else int(nbytes)
        _lib.check(self.lib.bpmf_hip_side_bind_items(side.handle, C.c_void_p(dev_ptr), ld, nbytes))
        side._items_keep = keep

    def items_tensor(self, side, device):
        """Allocates the factor matrix as a torch tensor [ncols, ld()] on `device` (rows num_latent .. ld()-1 of every column
        stay zero), binds the side to it (bpmf_hip_side_bind_items) and returns the WHOLE tensor, so that RCCL collectives move
        full device rows in place; t[:, :K] are the factors."""
        import torch
        ld = self.ld()
        t = torch.zeros((side.ncols, ld), dtype=torch.float64, device=device)
        self.bind_items(side, t.data_ptr(), keep=t, ld=ld, nbytes=t.numel() * 8)
        return t

    def factors_view(self, t):
        """The num_latent factor rows of a tensor items_tensor() returned: t[:, :K].  WRITE through this view, never through the
        whole tensor: with a padded num_latent (20 on the K = 32 kernels) the rows K .. ld()-1 of every column must stay zero --
        the kernels read them as factor entries (`U.copy_(randn(U.shape))` filled them)."""
        return t[:, :self.K]

    def set_prop_posterior(self, side, Lambda):
        """Per-column prior precisions of the side's local columns: [ncols_local, K*K] (each row a
        column-major K x K matrix, as in *-Lambda.ddm), or None to remove them."""
        if Lambda is None:
            _lib.check(self.lib.bpmf_hip_side_set_prop_posterior(side.handle, None, None))
            return
        L = np.ascontiguousarray(Lambda, np.float64).reshape(side.col_to - side.col_from, self.K * self.K)
        _lib.check(self.lib.bpmf_hip_side_set_prop_posterior(side.handle, None, _ptr(L)))

    def get_items(self, side):
        """[ncols, K] C-order array = the K x ncols column-major factor matrix."""
        out = np.empty((side.ncols, self.K), np.float64)
        _lib.check(self.lib.bpmf_hip_side_get_items(side.handle, _ptr(out)))
        return out

    def set_items(self, side, items):
        items = np.ascontiguousarray(items, np.float64)
        assert items.shape == (side.ncols, self.K)
        _lib.check(self.lib.bpmf_hip_side_set_items(side.handle, _ptr(items)))

    # -- independent chains -------------------------------------------------------
    CHAIN_STRIDE, CHAIN_MAX = 1 << 20, 63

    def side_set_chain(self, side, chain):
        """Makes `side` chain `chain` (0 .. 63) of its model: sys_sample keys the random numbers of its half-iteration i by
        i + chain * 2^20 (include/bpmf_hip.h).  Before the side's first half-iteration; both sides of a pair get
        the same chain.  Chain 0 is the run as it was."""
        _lib.check(self.lib.bpmf_hip_side_set_chain(side.handle, int(chain)))

    def side_chain(self, side):
        return int(self.lib.bpmf_hip_side_chain(side.handle))

    # -- hot path ---------------------------------------------------------------
    def sample_side_launch(self, side, other, it, alpha, mu, LambdaF):
        mu = np.ascontiguousarray(mu, np.float64)
        LF = np.asfortranarray(LambdaF, np.float64)
        _lib.check(self.lib.bpmf_hip_sample_side_launch(side.handle, other.handle, int(it), float(alpha), _ptr(mu), _ptr(LF)))

    def sample_side_finish(self, side):
        K = self.K
        s = np.empty(K); prod = np.empty((K, K), order="F"); nrm = np.empty(1)
        _lib.check(self.lib.bpmf_hip_sample_side_finish(side.handle, _ptr(s), _ptr(prod), _ptr(nrm)))
        return s, prod, float(nrm[0])

    def sample_side(self, side, other, it, alpha, mu, LambdaF):
        """Returns (sum[K], prod[K,K], norm) over the columns [col_from,col_to) of `side`."""
        self.sample_side_launch(side, other, it, alpha, mu, LambdaF)
        return self.sample_side_finish(side)

    def sys_sample(self, side, other, alpha):
        """Sys::sample(Sys&) with the state (iter, cov, hp) kept inside the library."""
        _lib.check(self.lib.bpmf_hip_sys_sample(side.handle, other.handle, float(alpha)))

    def sys_state(self, side):
        """(iter, norm, cov, mu, LambdaF, LambdaU) of a side driven by sys_sample."""
        K = self.K
        it = C.c_int(); nrm = C.c_double()
        cov = np.empty((K, K), order="F"); mu = np.empty(K); LF = np.empty((K, K), order="F"); LU = np.empty((K, K), order="F")
        _lib.check(self.lib.bpmf_hip_sys_state(side.handle, C.byref(it), C.byref(nrm), _ptr(cov), _ptr(mu), _ptr(LF), _ptr(LU)))
        return it.value, nrm.value, cov, mu, LF, LU

    def sys_norm(self, side, it):
        """Sys::norm of half-iteration `it` of the side (one of its last 8), without draining later half-iterations."""
        nrm = C.c_double()
        _lib.check(self.lib.bpmf_hip_sys_norm(side.handle, int(it), C.byref(nrm)))
        return nrm.value

    def aggr_add(self, side):
        """aggrMu / aggrLambda += r, r r^T of the side's local columns (device)."""
        _lib.check(self.lib.bpmf_hip_side_aggr_add(side.handle))

    def aggr_finalize(self, side, nsamples):
        """Sys::finalize_mu_lambda: (mu [nloc, K], Lambda [nloc, K*K]) of the local columns."""
        nloc = side.col_to - side.col_from
        mu = np.empty((nloc, self.K)); lam = np.empty((nloc, self.K * self.K))
        _lib.check(self.lib.bpmf_hip_side_aggr_finalize(side.handle, int(nsamples), _ptr(mu), _ptr(lam)))
        return mu, lam

    # -- posterior top-N ------------------------------------------------------
    def samples_reserve(self, side, max_samples):
        """Room for max_samples fp64 copies of the side's factors on the device (0 frees it)."""
        _lib.check(self.lib.bpmf_hip_side_samples_reserve(side.handle, int(max_samples)))

    def samples_add(self, side):
        """The current factors into the next slot of the side's sample ring (after a post-burn-in sys_sample)."""
        _lib.check(self.lib.bpmf_hip_side_samples_add(side.handle))

    def samples_count(self, side):
        return int(self.lib.bpmf_hip_side_samples_count(side.handle))

    def samples_get(self, side, s_from=0, s_to=None):
        """Slots s_from .. s_to - 1 of the side's sample ring, [ncols, s_to - s_from, K] (the pad rows of the ring are left out): what
        a saved model stores per side."""
        s_to = self.samples_count(side) if s_to is None else int(s_to)
        out = np.empty((side.ncols, max(0, s_to - int(s_from)), self.K))
        _lib.check(self.lib.bpmf_hip_side_samples_get(side.handle, int(s_from), s_to, _ptr(out)))
        return out

    def samples_set(self, side, samples):
        """The inverse of samples_get: samples [ncols, S, K] become slots 0 .. S - 1 of the side's ring (reserved with max_samples >= S),
        which then counts S.  A value that is not finite is refused with its column and sample."""
        samples = np.ascontiguousarray(samples, np.float64)
        if samples.ndim != 3 or samples.shape[0] != side.ncols or samples.shape[2] != self.K:
            raise ValueError("samples_set: samples must be [%d, S, %d], not %s" % (side.ncols, self.K, samples.shape))
        _lib.check(self.lib.bpmf_hip_side_samples_set(side.handle, samples.shape[1], _ptr(samples)))

    def predict_cells(self, query, cand, mean_rating, q, c, threshold=None, sigma=0.0):
        """(mean, std) or, with a threshold t, (mean, std, prob) of the cells (q[i], c[i]) -- column q[i] of `query` against column c[i]
        of `cand` -- over the samples of the two rings: mean and std as topn defines them (std leaves 1 / alpha
        out), prob = the mean over the samples of Phi((p_s - t) / sigma) (sigma = 0: the share of samples with p_s > t).  Any order,
        repeats allowed, an empty list allowed; an index out of range is refused naming the cell.  The bits of a cell do not depend on
        the other cells or on its place in the list."""
        q = np.ascontiguousarray(q, np.int32); c = np.ascontiguousarray(c, np.int32)
        if q.ndim != 1 or q.shape != c.shape:
            raise ValueError("predict_cells: q and c must be one-dimensional and of the same length")
        n = len(q)
        mean = np.empty(n); std = np.empty(n); prob = np.empty(n) if threshold is not None else None
        hold = np.zeros(1, np.int32)
        _lib.check(self.lib.bpmf_hip_predict_cells(query.handle, cand.handle, float(mean_rating), n, _ptr(q if n else hold), _ptr(c if n else hold),
                                                   0 if threshold is None else 1, 0.0 if threshold is None else float(threshold), float(sigma),
                                                   _ptr(mean if n else np.zeros(1)), _ptr(std if n else np.zeros(1)),
                                                   _ptr(prob if n or prob is None else np.zeros(1))))
        return (mean, std) if threshold is None else (mean, std, prob)

    def predict_cells_last_ms(self, query):
        """Device time of the newest launch of the cell kernel with `query` as the queries, between two events (tools/model_bench.py)."""
        ms = C.c_float()
        _lib.check(self.lib.bpmf_hip_predict_cells_last_ms(query.handle, C.byref(ms)))
        return ms.value

    # -- convergence diagnostics ------------------------------------------------
    DIAG_MIN_SAMPLES, DIAG_MAX_SAMPLES = 8, 4096

    def diag_traces(self, X):
        """(rhat, ess), [n] each: split-Rhat and the effective sample size of the n traces X [n, S] (one trace: [S]), every trace in
        chronological order, 8 <= S <= 4096, by the split-chain estimator without rank normalisation.  A
        constant trace and one with a value that is not finite give NaN for both."""
        X = np.ascontiguousarray(X, np.float64)
        if X.ndim == 1:
            X = X[None, :]
        if X.ndim != 2:
            raise ValueError("diag_traces: X must be [n, S]")
        n, S = X.shape
        rhat = np.empty(n); ess = np.empty(n)
        hold = np.zeros(1)
        _lib.check(self.lib.bpmf_hip_diag_traces(self.ctx, n, S, _ptr(X if n else hold), _ptr(rhat if n else hold), _ptr(ess if n else hold)))
        return rhat, ess

    def diag_cells(self, query, cand, mean_rating, q, c):
        """dict(mean, std, rhat, ess), [n] each, of the cells (q[i], c[i]) over the samples of the two rings: mean and std are
        predict_cells's, bit for bit; rhat and ess are diag_traces's of the cell's predictions in the order the samples were kept.
        The list is as predict_cells takes it; the rings must hold 8 .. 4096 samples."""
        q = np.ascontiguousarray(q, np.int32); c = np.ascontiguousarray(c, np.int32)
        if q.ndim != 1 or q.shape != c.shape:
            raise ValueError("diag_cells: q and c must be one-dimensional and of the same length")
        n = len(q)
        out = [np.empty(n) for _ in range(4)]
        hold = np.zeros(1, np.int32)
        _lib.check(self.lib.bpmf_hip_diag_cells(query.handle, cand.handle, float(mean_rating), n, _ptr(q if n else hold), _ptr(c if n else hold),
                                                *[_ptr(a if n else np.zeros(1)) for a in out]))
        return dict(mean=out[0], std=out[1], rhat=out[2], ess=out[3])

    DIAG_MAX_CHAINS = 64

    def diag_traces_mc(self, X, chains):
        """(rhat, ess_bulk, ess_tail), [n] each: the rank-normalised split-Rhat, the bulk and the tail effective sample size
        (Vehtari et al. 2021) of the n traces X [n, chains * S] (one trace: [chains * S]),
        chain-major: chain c is X[i, c S : (c + 1) S], chronological inside.  1 <= chains <= 64, S >= 8, chains * S <= 4096.  A
        trace with a value that is not finite gives NaN for all three; see bpmf_hip.h for the other NaN rules."""
        X = np.ascontiguousarray(X, np.float64)
        chains = int(chains)
        if X.ndim == 1:
            X = X[None, :]
        if X.ndim != 2:
            raise ValueError("diag_traces_mc: X must be [n, chains * S]")
        n, L = X.shape
        if chains < 1 or L % chains:
            raise ValueError("diag_traces_mc: %d values per trace are not %d chains of one length" % (L, chains))
        out = [np.empty(n) for _ in range(3)]
        hold = np.zeros(1)
        _lib.check(self.lib.bpmf_hip_diag_traces_mc(self.ctx, n, chains, L // chains, _ptr(X if n else hold), *[_ptr(a if n else hold) for a in out]))
        return tuple(out)

    def diag_cells_mc(self, query, cand, mean_rating, q, c, chains):
        """dict(mean, std, rhat, ess_bulk, ess_tail), [n] each, of the cells (q[i], c[i]) over two rings that hold the samples of
        `chains` chains of one length one after the other (bpmf_amd.pool_models): mean and std are predict_cells's, bit for bit; the
        other three are diag_traces_mc's of the cell's predictions."""
        q = np.ascontiguousarray(q, np.int32); c = np.ascontiguousarray(c, np.int32)
        if q.ndim != 1 or q.shape != c.shape:
            raise ValueError("diag_cells_mc: q and c must be one-dimensional and of the same length")
        n = len(q)
        out = [np.empty(n) for _ in range(5)]
        hold = np.zeros(1, np.int32)
        _lib.check(self.lib.bpmf_hip_diag_cells_mc(query.handle, cand.handle, float(mean_rating), n, _ptr(q if n else hold), _ptr(c if n else hold),
                                                   int(chains), *[_ptr(a if n else np.zeros(1)) for a in out]))
        return dict(mean=out[0], std=out[1], rhat=out[2], ess_bulk=out[3], ess_tail=out[4])

    def diag_batch_cells(self, cells):
        """Cells per batch of diag_cells (0: automatic, from the size of the trace buffer).  For tests: results do not depend on it."""
        _lib.check(self.lib.bpmf_hip_diag_batch_cells(int(cells)))

    def diag_last_ms(self, query):
        """Device time of the kernels of the newest diag_cells with `query` as the queries, between two events (tools/diag_bench.py)."""
        ms = C.c_float()
        _lib.check(self.lib.bpmf_hip_diag_last_ms(query.handle, C.byref(ms)))
        return ms.value

    # -- model comparison ---------------------------------------------------------
    LOGDENS_KINDS = {"gaussian": 0, "student": 1, "probit": 2}

    def score_cells(self, query, cand, mean_rating, q, c, y, alpha, kind="gaussian", nu=0.0, w=None, flag=None):
        """dict(lpd, pwaic, mean, std), [n] each, of the observed cells (q[i], c[i]) with the values y[i] over the S samples of the
        two rings: lpd the log of the mean over the samples of the predictive density of y[i], pwaic the
        variance over the samples of its log; mean and std are predict_cells's, bit for bit.  kind: "gaussian" (w: per-cell weights,
        flag: int8 -1 / 0 / +1, a censored cell whose y is a bound), "student" (nu >= 1) or "probit" (y > 0: a positive label).
        alpha: the noise precision, one number or S values in ring-slot order."""
        if kind not in self.LOGDENS_KINDS:
            raise ValueError("score_cells: kind must be one of %s, not %r" % (sorted(self.LOGDENS_KINDS), kind))
        q = np.ascontiguousarray(q, np.int32); c = np.ascontiguousarray(c, np.int32); y = np.ascontiguousarray(y, np.float64)
        if q.ndim != 1 or q.shape != c.shape or y.shape != q.shape:
            raise ValueError("score_cells: q, c and y must be one-dimensional and of the same length")
        n = len(q)
        alpha = np.ascontiguousarray(np.atleast_1d(alpha), np.float64)
        if alpha.ndim != 1 or len(alpha) < 1:
            raise ValueError("score_cells: alpha must be one number or one per sample")
        if w is not None:
            w = np.ascontiguousarray(w, np.float64)
            if w.shape != q.shape:
                raise ValueError("score_cells: w must have one weight per cell")
        if flag is not None:
            flag = np.ascontiguousarray(flag, np.int8)
            if flag.shape != q.shape:
                raise ValueError("score_cells: flag must have one flag per cell")
        out = [np.empty(n) for _ in range(4)]
        hold = np.zeros(1, np.int32)

        def opt(a):
            return None if a is None else _ptr(a if n else np.zeros(1, a.dtype))
        _lib.check(self.lib.bpmf_hip_score_cells(query.handle, cand.handle, float(mean_rating), n, _ptr(q if n else hold), _ptr(c if n else hold),
                                                 _ptr(y if n else np.zeros(1)), opt(w), opt(flag), self.LOGDENS_KINDS[kind], float(nu), len(alpha),
                                                 _ptr(alpha), *[_ptr(a if n else np.zeros(1)) for a in out]))
        return dict(lpd=out[0], pwaic=out[1], mean=out[2], std=out[3])

    def score_batch_cells(self, cells):
        """Cells per launch of score_cells (0: automatic).  For tests: results do not depend on it."""
        _lib.check(self.lib.bpmf_hip_score_batch_cells(int(cells)))

    def score_last_ms(self, query):
        """Device time of the kernels of the newest score_cells with `query` as the queries, between two events (tools/score_bench.py)."""
        ms = C.c_float()
        _lib.check(self.lib.bpmf_hip_score_last_ms(query.handle, C.byref(ms)))
        return ms.value

    # -- predictive intervals ------------------------------------------------------
    INTERVAL_MAX_SAMPLES, INTERVAL_MAX_QUANTILES = 4096, 8

    @staticmethod
    def _interval_args(who, n, y, w, alpha, tau):
        """The optional arrays of interval_cells / interval_traces as contiguous float64 (None stays None), alpha and tau as vectors."""
        def per_item(a, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float64)
            if a.shape != (n,):
                raise ValueError("%s: %s must have one value per item" % (who, what))
            return a
        alpha = np.ascontiguousarray(np.atleast_1d(alpha), np.float64)
        if alpha.ndim != 1 or len(alpha) < 1:
            raise ValueError("%s: alpha must be one number or one per sample" % who)
        tau = np.ascontiguousarray(np.atleast_1d(tau) if tau is not None else np.zeros(0), np.float64)
        if tau.ndim != 1:
            raise ValueError("%s: tau must be a vector" % who)
        return per_item(y, "y"), per_item(w, "w"), alpha, tau

    def interval_traces(self, D, alpha, tau=(), y=None, w=None, mean_rating=0.0):
        """(pit [n] or None, quant [n, nq]) of the mixtures (1/S) sum_s N(mean_rating + D[i, s], 1 / (alpha_s w[i])) around the n traces
        D [n, S] (one trace: [S]), 1 <= S <= 4096: pit[i] = F_i(y[i]) (y None: no pit), quant[i, j] =
        F_i^-1(tau[j]) for up to 8 strictly increasing tau in [0.001, 0.999].  alpha: one number or S values.  A trace holding a value
        that is not finite gives NaN."""
        D = np.ascontiguousarray(D, np.float64)
        if D.ndim == 1:
            D = D[None, :]
        if D.ndim != 2:
            raise ValueError("interval_traces: D must be [n, S]")
        n, S = D.shape
        y, w, alpha, tau = self._interval_args("interval_traces", n, y, w, alpha, tau)
        nq = len(tau)
        pit = np.empty(n) if y is not None else None
        quant = np.empty((n, nq))
        hold = np.zeros(1)

        def opt(a):
            return None if a is None else _ptr(a if a.size else hold)
        _lib.check(self.lib.bpmf_hip_interval_traces(self.ctx, n, S, _ptr(D if D.size else hold), float(mean_rating), opt(y), opt(w), len(alpha),
                                                     _ptr(alpha), nq, _ptr(tau if nq else hold), opt(pit), _ptr(quant if quant.size else hold)))
        return pit, quant

    def interval_cells(self, query, cand, mean_rating, q, c, alpha, tau=(), y=None, w=None):
        """dict(pit, quant, mean, std) of the cells (q[i], c[i]) over the S samples of the two rings: the
        probability integral transform pit [n] of the observed values y (None without y) and the quantiles quant [n, nq] at tau of the
        posterior predictive mixture, as interval_traces defines them around p_s = mean_rating + u_s . v_s; mean and std are
        predict_cells's, bit for bit.  alpha: the noise precision, one number or S values in ring-slot order; w: per-cell weights."""
        q = np.ascontiguousarray(q, np.int32); c = np.ascontiguousarray(c, np.int32)
        if q.ndim != 1 or q.shape != c.shape:
            raise ValueError("interval_cells: q and c must be one-dimensional and of the same length")
        n = len(q)
        y, w, alpha, tau = self._interval_args("interval_cells", n, y, w, alpha, tau)
        nq = len(tau)
        pit = np.empty(n) if y is not None else None
        quant = np.empty((n, nq)); mean = np.empty(n); std = np.empty(n)
        hold = np.zeros(1); holdi = np.zeros(1, np.int32)

        def opt(a):
            return None if a is None else _ptr(a if a.size else hold)
        _lib.check(self.lib.bpmf_hip_interval_cells(query.handle, cand.handle, float(mean_rating), n, _ptr(q if n else holdi), _ptr(c if n else holdi),
                                                    opt(y), opt(w), len(alpha), _ptr(alpha), nq, _ptr(tau if nq else hold), opt(pit),
                                                    _ptr(quant if quant.size else hold), opt(mean), opt(std)))
        return dict(pit=pit, quant=quant, mean=mean, std=std)

    def interval_batch_cells(self, cells):
        """Cells per batch of interval_cells and interval_traces (0: automatic, from the size of the trace buffer).  For tests: results do
        not depend on it."""
        _lib.check(self.lib.bpmf_hip_interval_batch_cells(int(cells)))

    def interval_last_ms(self, query):
        """Device time of the kernels of the newest interval_cells with `query` as the queries, between two events (tools/interval_bench.py)."""
        ms = C.c_float()
        _lib.check(self.lib.bpmf_hip_interval_last_ms(query.handle, C.byref(ms)))
        return ms.value

    # -- PSIS-LOO ------------------------------------------------------------------
    LOO_MAX_SAMPLES = 4096

    def loo_traces(self, L, want_lpd=True):
        """dict(elpd_loo, khat, lpd), [n] each, of the n traces L [n, S] (one trace: [S]) of log densities l_s, 1 <= S <= 4096, by
        Pareto-smoothed importance sampling: the leave-one-out log predictive density, the shape khat of the
        generalised Pareto distribution fitted to the tail of the importance ratios (+inf where nothing is smoothed: S < 25, a
        constant tail) and lpd = log mean_s exp l_s (None without want_lpd).  A trace holding a value that is not finite gives NaN."""
        L = np.ascontiguousarray(L, np.float64)
        if L.ndim == 1:
            L = L[None, :]
        if L.ndim != 2:
            raise ValueError("loo_traces: L must be [n, S]")
        n, S = L.shape
        elpd = np.empty(n); khat = np.empty(n); lpd = np.empty(n) if want_lpd else None
        hold = np.zeros(1)
        _lib.check(self.lib.bpmf_hip_loo_traces(self.ctx, n, S, _ptr(L if L.size else hold), _ptr(elpd if n else hold), _ptr(khat if n else hold),
                                                None if lpd is None else _ptr(lpd if n else hold)))
        return dict(elpd_loo=elpd, khat=khat, lpd=lpd)

    def loo_cells(self, query, cand, mean_rating, q, c, y, alpha, kind="gaussian", nu=0.0, w=None, flag=None, want=("lpd", "mean", "std")):
        """dict(elpd_loo, khat, lpd, mean, std), [n] each, of the observed cells (q[i], c[i]) with the values y[i] over the S <= 4096
        samples of the two rings: loo_traces's rule on the log densities score_cells's likelihoods give the
        cell under every sample (kind, nu, w, flag and alpha as there); lpd is score_cells's up to rounding, mean and std are
        predict_cells's, bit for bit.  want: which of lpd, mean and std are read back (the others are None)."""
        if kind not in self.LOGDENS_KINDS:
            raise ValueError("loo_cells: kind must be one of %s, not %r" % (sorted(self.LOGDENS_KINDS), kind))
        q = np.ascontiguousarray(q, np.int32); c = np.ascontiguousarray(c, np.int32); y = np.ascontiguousarray(y, np.float64)
        if q.ndim != 1 or q.shape != c.shape or y.shape != q.shape:
            raise ValueError("loo_cells: q, c and y must be one-dimensional and of the same length")
        n = len(q)
        alpha = np.ascontiguousarray(np.atleast_1d(alpha), np.float64)
        if alpha.ndim != 1 or len(alpha) < 1:
            raise ValueError("loo_cells: alpha must be one number or one per sample")
        if w is not None:
            w = np.ascontiguousarray(w, np.float64)
            if w.shape != q.shape:
                raise ValueError("loo_cells: w must have one weight per cell")
        if flag is not None:
            flag = np.ascontiguousarray(flag, np.int8)
            if flag.shape != q.shape:
                raise ValueError("loo_cells: flag must have one flag per cell")
        out = dict(elpd_loo=np.empty(n), khat=np.empty(n))
        for name in ("lpd", "mean", "std"):
            out[name] = np.empty(n) if name in want else None
        hold = np.zeros(1, np.int32)

        def opt(a):
            return None if a is None else _ptr(a if n else np.zeros(1, a.dtype))
        _lib.check(self.lib.bpmf_hip_loo_cells(query.handle, cand.handle, float(mean_rating), n, _ptr(q if n else hold), _ptr(c if n else hold),
                                               _ptr(y if n else np.zeros(1)), opt(w), opt(flag), self.LOGDENS_KINDS[kind], float(nu), len(alpha),
                                               _ptr(alpha), *[opt(out[name]) for name in ("elpd_loo", "khat", "lpd", "mean", "std")]))
        return out

    def loo_batch_cells(self, cells):
        """Cells per batch of loo_cells and loo_traces (0: automatic, from the size of the trace buffer).  For tests: results do not
        depend on it."""
        _lib.check(self.lib.bpmf_hip_loo_batch_cells(int(cells)))

    def loo_last_ms(self, query):
        """Device time of the kernels of the newest loo_cells with `query` as the queries, between two events (tools/loo_bench.py)."""
        ms = C.c_float()
        _lib.check(self.lib.bpmf_hip_loo_last_ms(query.handle, C.byref(ms)))
        return ms.value

    def topn(self, query, cand, mean_rating, n, q_from=0, q_to=None, exclude_rated=True):
        """The n best columns of `cand` by posterior-mean score for every column q_from .. q_to - 1 of `query`:
        (idx int32[nq, n], mean f64[nq, n], std f64[nq, n]); empty slots have idx -1, mean 0, std 0."""
        q_to = query.ncols if q_to is None else int(q_to)
        nq = max(0, q_to - int(q_from))
        idx = np.empty((nq, int(n)), dtype=np.int32)
        mean = np.empty((nq, int(n)))
        std = np.empty((nq, int(n)))
        _lib.check(self.lib.bpmf_hip_topn(query.handle, cand.handle, float(mean_rating), int(n), int(q_from), int(q_to),
                                          1 if exclude_rated else 0, _ptr(idx), _ptr(mean), _ptr(std)))
        return idx, mean, std

    def rank_eval(self, query, cand, tptr, tcand, mean_rating=0.0, q_from=0, q_to=None, exclude_rated=True):
        """Ranks of held-out candidates by topn's score and order.  Query q_from + q holds out the candidates
        tcand[tptr[q] : tptr[q + 1]], ascending and distinct.  Returns (rank int32[len(tcand)], ncand int32[nq]): rank is 1 + the
        number of other candidates the query has not rated (exclude_rated) that come before the entry, ncand the number of
        candidates the query has not rated.  A held-out entry that is a rated cell of the query is refused."""
        q_to = query.ncols if q_to is None else int(q_to)
        nq = max(0, q_to - int(q_from))
        tptr = np.ascontiguousarray(tptr, np.int64)
        tcand = np.ascontiguousarray(tcand, np.int32)
        if tptr.ndim != 1 or len(tptr) != nq + 1:
            raise ValueError("rank_eval: tptr must hold %d entries (one per query, plus one), not %s" % (nq + 1, tptr.shape))
        if tcand.ndim != 1 or len(tcand) != int(tptr[-1]):
            raise ValueError("rank_eval: tcand holds %d entries, tptr ends at %d" % (tcand.size, int(tptr[-1])))
        rank = np.empty(len(tcand), dtype=np.int32)
        ncand = np.empty(nq, dtype=np.int32)
        tc = tcand if len(tcand) else np.zeros(1, np.int32)
        rk = rank if len(rank) else np.zeros(1, np.int32)
        nc = ncand if nq else np.zeros(1, np.int32)
        _lib.check(self.lib.bpmf_hip_rank_eval(query.handle, cand.handle, float(mean_rating), int(q_from), int(q_to),
                                               1 if exclude_rated else 0, _ptr(tptr), _ptr(tc), _ptr(rk), _ptr(nc)))
        return rank, ncand

    SCORE_KINDS = {"ucb": 0, "prob": 1, "ei": 2}     # BPMF_HIP_SCORE_*

    def topn_scored(self, query, cand, mean_rating, n, kind, param, sigma=0.0, q_from=0, q_to=None, exclude_rated=True):
        """The n best columns of `cand` by an acquisition score of the per-sample predictions for every
        column q_from .. q_to - 1 of `query`: kind "ucb" (mean + param std; param = kappa, negative for a lower bound), "prob"
        (the posterior probability that a rating with noise deviation sigma exceeds param = t) or "ei" (the expected excess over
        t).  (idx int32[nq, n], score, mean, std f64[nq, n]); mean and std of a pick are predict_block's, bit for bit; empty slots
        have idx -1 and zeros."""
        if kind not in self.SCORE_KINDS:
            raise ValueError("topn_scored: kind must be one of 'ucb', 'prob', 'ei', not %r" % (kind,))
        q_to = query.ncols if q_to is None else int(q_to)
        nq = max(0, q_to - int(q_from))
        idx = np.empty((nq, int(n)), dtype=np.int32)
        score = np.empty((nq, int(n)))
        mean = np.empty((nq, int(n)))
        std = np.empty((nq, int(n)))
        _lib.check(self.lib.bpmf_hip_topn_scored(query.handle, cand.handle, float(mean_rating), int(n), int(q_from), int(q_to),
                                                 1 if exclude_rated else 0, self.SCORE_KINDS[kind], float(param), float(sigma),
                                                 _ptr(idx), _ptr(score), _ptr(mean), _ptr(std)))
        return idx, score, mean, std

    SIM_KINDS = {"cosine": 0, "euclid": 1}           # BPMF_HIP_SIM_*

    def similar(self, side, n, kind="cosine", kappa=0.0, q_from=0, q_to=None, cand_ok=None):
        """The n nearest neighbours of every column q_from .. q_to - 1 of `side` among the side's own columns, by a similarity no
        rotation of the latent space changes: per kept sample the cosine between the two columns ("cosine")
        or their negative squared distance ("euclid"), then score = mean - kappa std over the samples (kappa >= 0).  A query is
        never its own neighbour; cand_ok (one truth value per column, None: all) says which columns may be listed.
        (idx int32[nq, n], score, mean, std f64[nq, n]), score descending, lower index first; mean and std of a pick are
        similar_block's, bit for bit; empty slots have idx -1 and zeros."""
        if kind not in self.SIM_KINDS:
            raise ValueError("similar: kind must be one of 'cosine', 'euclid', not %r" % (kind,))
        q_to = side.ncols if q_to is None else int(q_to)
        nq = max(0, q_to - int(q_from))
        ok = None
        if cand_ok is not None:
            ok = np.ascontiguousarray(np.asarray(cand_ok) != 0, np.uint8)
            if ok.shape != (side.ncols,):
                raise ValueError("similar: cand_ok must hold one entry per column (%d), not %s" % (side.ncols, ok.shape))
        idx = np.empty((nq, int(n)), dtype=np.int32)
        score = np.empty((nq, int(n)))
        mean = np.empty((nq, int(n)))
        std = np.empty((nq, int(n)))
        _lib.check(self.lib.bpmf_hip_similar(side.handle, self.SIM_KINDS[kind], float(kappa), int(n), int(q_from), int(q_to),
                                             None if ok is None else _ptr(ok), _ptr(idx), _ptr(score), _ptr(mean), _ptr(std)))
        return idx, score, mean, std

    def similar_block(self, side, kind="cosine", q_from=0, q_to=None, c_from=0, c_to=None):
        """(mean, std), [q_to - q_from, c_to - c_from] each: the posterior mean and spread of the similarity of every pair of
        columns of the block, the diagonal included, with the bits `similar` lists."""
        if kind not in self.SIM_KINDS:
            raise ValueError("similar_block: kind must be one of 'cosine', 'euclid', not %r" % (kind,))
        q_to = side.ncols if q_to is None else int(q_to)
        c_to = side.ncols if c_to is None else int(c_to)
        mean = np.empty((max(0, q_to - int(q_from)), max(0, c_to - int(c_from))))
        std = np.empty_like(mean)
        _lib.check(self.lib.bpmf_hip_similar_block(side.handle, self.SIM_KINDS[kind], int(q_from), int(q_to), int(c_from), int(c_to),
                                                   _ptr(mean), _ptr(std)))
        return mean, std

    def similar_last_ms(self, side):
        """Device time of the newest `similar` of the side, between two events (tools/similar_bench.py)."""
        ms = C.c_float()
        _lib.check(self.lib.bpmf_hip_similar_last_ms(side.handle, C.byref(ms)))
        return ms.value

    def predict_block(self, query, cand, mean_rating, q_from=0, q_to=None, c_from=0, c_to=None):
        """(mean, std), [q_to - q_from, c_to - c_from] each: the posterior-mean prediction and its spread over the samples of the
        two sides' rings for every pair of the block, in one kernel.  The bits of an element do not depend
        on the ranges.  std does not include the observation noise 1 / alpha."""
        q_to = query.ncols if q_to is None else int(q_to)
        c_to = cand.ncols if c_to is None else int(c_to)
        mean = np.empty((max(0, q_to - int(q_from)), max(0, c_to - int(c_from))))
        std = np.empty_like(mean)
        _lib.check(self.lib.bpmf_hip_predict_block(query.handle, cand.handle, float(mean_rating), int(q_from), q_to, int(c_from), c_to,
                                                   _ptr(mean), _ptr(std)))
        return mean, std

    def predict_block_device(self, query, cand, mean_rating, mean_ptr, std_ptr, q_from=0, q_to=None, c_from=0, c_to=None):
        """predict_block into two device addresses of (q_to - q_from) (c_to - c_from) doubles each on the engine's device, written
        in place by the kernel: for a consumer on the device (tools/predblock_bench.py)."""
        q_to = query.ncols if q_to is None else int(q_to)
        c_to = cand.ncols if c_to is None else int(c_to)
        _lib.check(self.lib.bpmf_hip_predict_block_device(query.handle, cand.handle, float(mean_rating), int(q_from), q_to, int(c_from), c_to,
                                                          C.c_void_p(int(mean_ptr)), C.c_void_p(int(std_ptr))))

    # -- rows unseen in training ----------------------------------------------
    def newrows_set(self, side, F, max_samples):
        """Gives a side with features the feature rows F [n_new, D] of entities that are not in the training matrix, and room for
        max_samples projected samples of them.  F is of the kind of the side's features (a dense ndarray
        or a scipy.sparse matrix) with the same D.  Calling again replaces them; F = None or max_samples = 0 frees them."""
        if F is None or int(max_samples) == 0:
            _lib.check(self.lib.bpmf_hip_side_newrows_set(side.handle, 0, None, 0))
            side.newrows_n = 0
            return
        D = getattr(side, "link_d", None)
        if D is None:
            raise ValueError("newrows_set: the side has no features (set_features)")
        if not _is_sparse(F):
            F = np.asarray(F, np.float64)
        if _is_sparse(F) != bool(getattr(side, "link_sparse", False)):
            raise ValueError("newrows_set: the side's features are %s, the new rows' must be of the same kind"
                             % ("sparse" if getattr(side, "link_sparse", False) else "dense"))
        if F.ndim != 2 or F.shape[1] != D:
            raise ValueError("newrows_set: F must be [n_new, %d], the side's features have D = %d" % (D, D))
        if F.shape[0] < 1:
            raise ValueError("newrows_set: n_new must be >= 1")
        if _is_sparse(F):
            rowptr, colidx, vals = csr_arrays(F)
            _lib.check(self.lib.bpmf_hip_side_newrows_set_sparse(side.handle, int(F.shape[0]), _ptr(rowptr), _ptr(colidx), _ptr(vals),
                                                                 int(max_samples)))
        else:
            F = np.ascontiguousarray(F, np.float64)
            _lib.check(self.lib.bpmf_hip_side_newrows_set(side.handle, int(F.shape[0]), _ptr(F), int(max_samples)))
        side.newrows_n = int(F.shape[0])

    def newrows_add(self, side, other):
        """Projects the side's new rows with its current beta and mu into the next slot and adds v^T Lambda^-1 v of the other side's
        current factors to w (where link_add sits: after a post-burn-in iteration, both sides sampled)."""
        _lib.check(self.lib.bpmf_hip_side_newrows_add(side.handle, other.handle))

    def newrows_count(self, side):
        return int(self.lib.bpmf_hip_side_newrows_count(side.handle))

    def newrows_get(self, side, padded=False):
        """(E [n_new, S, K]: the projected factors mu_s + beta_s^T f of every new row and kept sample, w [nrows of the side]:
        (1/S) sum_s v_s(c)^T Lambda_s^-1 v_s(c) per column of the other side).  padded=True: E alone as the ring stores it,
        [n_new, S, Kp] with Kp = K rounded up to a multiple of 4; the components k >= K are the ring's zero padding."""
        S = self.newrows_count(side)
        if padded:
            E = np.empty((getattr(side, "newrows_n", 0), S, (self.K + 3) // 4 * 4))
            _lib.check(self.lib.bpmf_hip_side_newrows_get_padded(side.handle, _ptr(E)))
            return E
        E = np.empty((getattr(side, "newrows_n", 0), S, self.K)); w = np.empty(side.nrows)
        _lib.check(self.lib.bpmf_hip_side_newrows_get(side.handle, _ptr(E), _ptr(w)))
        return E, w

    def newrows_predict(self, side, cand, mean_rating, q_from=0, q_to=None, c_from=0, c_to=None):
        """(mean, std), [q_to - q_from, c_to - c_from] each, of the side's new rows [q_from, q_to) against the columns [c_from, c_to)
        of `cand` (the side's partner, with a sample ring of as many samples).  std joins the spread between the samples with the
        spread of a cold row's factors around their conditional mean; it does not include the observation noise 1 / alpha."""
        q_to = getattr(side, "newrows_n", 0) if q_to is None else int(q_to)
        c_to = cand.ncols if c_to is None else int(c_to)
        mean = np.empty((max(0, q_to - int(q_from)), max(0, c_to - int(c_from))))
        std = np.empty_like(mean)
        _lib.check(self.lib.bpmf_hip_newrows_predict(side.handle, cand.handle, float(mean_rating), int(q_from), q_to, int(c_from), c_to,
                                                     _ptr(mean), _ptr(std)))
        return mean, std

    def newrows_topn(self, side, cand, mean_rating, n, new_are_queries=True):
        """(idx int32, mean, std), [n_new, n] each: the n best columns of `cand` for every new row of `side`; or, with
        new_are_queries=False, [cand.ncols, n]: the n best new rows for every column of `cand`.  Nothing is excluded (new rows
        rated nothing); std is the total one of newrows_predict.  Empty slots: idx -1, mean 0, std 0."""
        nq = getattr(side, "newrows_n", 0) if new_are_queries else cand.ncols
        idx = np.empty((nq, int(n)), dtype=np.int32)
        mean = np.empty((nq, int(n)))
        std = np.empty((nq, int(n)))
        _lib.check(self.lib.bpmf_hip_newrows_topn(side.handle, cand.handle, float(mean_rating), int(n), 1 if new_are_queries else 0,
                                                  _ptr(idx), _ptr(mean), _ptr(std)))
        return idx, mean, std

    # -- fold-in: new rows from their ratings -------------------------------------
    def hyper_reserve(self, side, max_samples):
        """Room for the hyper-parameters (alpha, mu, Lambda) of max_samples kept samples of the side (0 frees
        it): what a fold-in into this side reads beside the other side's sample ring."""
        _lib.check(self.lib.bpmf_hip_side_hyper_reserve(side.handle, int(max_samples)))

    def hyper_add(self, side, alpha, mu=None, LambdaF=None):
        """The next slot of the side's hyper ring: the hyper-parameters its newest sys_sample ran with (mu = LambdaF = None; where
        samples_add of the other side sits), or explicit mu [K] and a symmetric LambdaF [K, K] (tests, a caller's own loop)."""
        if (mu is None) != (LambdaF is None):
            raise ValueError("hyper_add: mu and LambdaF are given together or not at all")
        if mu is not None:
            mu = np.ascontiguousarray(mu, np.float64); LambdaF = np.asfortranarray(LambdaF, np.float64)
            if mu.shape != (self.K,) or LambdaF.shape != (self.K, self.K):
                raise ValueError("hyper_add: mu must be [%d] and LambdaF [%d, %d]" % (self.K, self.K, self.K))
        _lib.check(self.lib.bpmf_hip_side_hyper_add(side.handle, float(alpha), _ptr(mu), _ptr(LambdaF)))

    def hyper_count(self, side):
        return int(self.lib.bpmf_hip_side_hyper_count(side.handle))

    def hyper_get(self, side):
        """(alpha [S], mu [S, K], LambdaF [S, K, K]) of the side's hyper ring"""
        S = self.hyper_count(side)
        alpha = np.empty(S); mu = np.empty((S, self.K)); LF = np.empty((S, self.K, self.K))
        _lib.check(self.lib.bpmf_hip_side_hyper_get(side.handle, _ptr(alpha), _ptr(mu), _ptr(LF)))
        return alpha, mu, np.ascontiguousarray(np.transpose(LF, (0, 2, 1)))      # (column-major slots)

    def foldin_chunk(self):
        """Ratings the fold-in kernel stages per pass over the Gram (kFoldinChunk; the tests sit on its edges)."""
        return int(self.lib.bpmf_hip_foldin_chunk())

    def foldin(self, side, cand, mean_rating, rows, tag, draw=True):
        """Folds new rows of `side` in from their ratings: rows is a scipy.sparse matrix [n_new, cand.ncols]
        (stored zeros are ratings of 0; entries of one cell are NOT summed: the library refuses a cell listed twice) or a CSR triple
        (rowptr, colidx, vals).  Every kept sample s of cand's ring and slot s of the side's hyper ring give one draw of each row's
        factors -- draw=False: the conditional mean -- from the streams named by tag >= 1.  Replaces an earlier set; rows = None
        frees it.  A row whose Lambda* has a pivot that is not positive raises BpmfHipError (code -4) naming it; its factors are
        stored as zeros."""
        if rows is None:
            _lib.check(self.lib.bpmf_hip_foldin(side.handle, cand.handle if cand is not None else None, 0.0, 0, None, None, None, 1, 0))
            return
        rowptr, colidx, vals = foldin_csr(rows, cand.ncols)
        _lib.check(self.lib.bpmf_hip_foldin(side.handle, cand.handle, float(mean_rating), len(rowptr) - 1, _ptr(rowptr), _ptr(colidx), _ptr(vals),
                                            int(tag), 1 if draw else 0))

    def foldin_last_ms(self, side):
        """Device time of the newest launch of the fold-in kernel of the side, between two events (tools/foldin_bench.py)."""
        ms = C.c_float()
        _lib.check(self.lib.bpmf_hip_foldin_last_ms(side.handle, C.byref(ms)))
        return ms.value

    def foldin_count(self, side):
        return int(self.lib.bpmf_hip_foldin_count(side.handle))

    def foldin_get(self, side, padded=False):
        """The folded-in factors u_is, [n_new, S, K]; padded=True: as the ring stores them, [n_new, S, Kp] with Kp = K rounded up to a
        multiple of 4 (the pad components are zeros)."""
        n, S = self.foldin_count(side), int(self.lib.bpmf_hip_foldin_samples(side.handle))
        if padded:
            E = np.empty((n, S, (self.K + 3) // 4 * 4))
            _lib.check(self.lib.bpmf_hip_foldin_get_padded(side.handle, _ptr(E)))
            return E
        E = np.empty((n, S, self.K))
        _lib.check(self.lib.bpmf_hip_foldin_get(side.handle, _ptr(E)))
        return E

    def foldin_predict(self, side, cand, mean_rating, q_from=0, q_to=None, c_from=0, c_to=None):
        """(mean, std), [q_to - q_from, c_to - c_from] each, of the folded-in rows [q_from, q_to) of `side` against the columns
        [c_from, c_to) of `cand`: predict_block with the fold-in ring as the queries.  The observation noise 1 / alpha is not part of
        std."""
        q_to = self.foldin_count(side) if q_to is None else int(q_to)
        c_to = cand.ncols if c_to is None else int(c_to)
        mean = np.empty((max(0, q_to - int(q_from)), max(0, c_to - int(c_from))))
        std = np.empty_like(mean)
        _lib.check(self.lib.bpmf_hip_foldin_predict(side.handle, cand.handle, float(mean_rating), int(q_from), q_to, int(c_from), c_to,
                                                    _ptr(mean), _ptr(std)))
        return mean, std

    def foldin_topn(self, side, cand, mean_rating, n, exclude_rated=True):
        """(idx int32, mean, std), [n_new, n] each: the n best columns of `cand` for every folded-in row by posterior mean, without
        the columns the row itself rated (exclude_rated).  Empty slots: idx -1, mean 0, std 0."""
        nq = self.foldin_count(side)
        idx = np.empty((nq, int(n)), dtype=np.int32)
        mean = np.empty((nq, int(n)))
        std = np.empty((nq, int(n)))
        _lib.check(self.lib.bpmf_hip_foldin_topn(side.handle, cand.handle, float(mean_rating), int(n), 1 if exclude_rated else 0,
                                                 _ptr(idx), _ptr(mean), _ptr(std)))
        return idx, mean, std

    # -- adaptive noise precision ----------------------------------------------
    def train_sse(self, side, other):
        """(SSE, n): the sum of squared training residuals (v - mean - x_c . y_r)^2 over the n ratings of `side`, with the
        current factors of both sides (behind the newest sampler; waits for the result)."""
        sse = C.c_double()
        n = C.c_int64()
        _lib.check(self.lib.bpmf_hip_train_sse(side.handle, other.handle, C.byref(sse), C.byref(n)))
        return sse.value, n.value

    def noise_sample(self, a0, b0, sse, n, it, alpha_max=None):
        """The noise precision after iteration `it`: g / (b0 + sse / 2), g ~ Gamma(a0 + n / 2, 1) on the Philox stream
        BPMF_NOISE_COUNTER(it), capped at alpha_max (None: no cap).  Host only."""
        return noise_sample(a0, b0, sse, n, it, alpha_max)

    # -- probit likelihood -------------------------------------------------------
    def set_probit(self, side, threshold=0.5, tag=1):
        """Turns `side` (created with mean_rating 0) into a probit side: a rating is a label, positive if > threshold, and every
        sampler launch of the side is preceded by the draw of its latent scores (include/bpmf_hip.h).  tag >= 1 names the
        side's random streams: give the two sides of a model different tags.  Such a side is sampled with alpha = 1."""
        _lib.check(self.lib.bpmf_hip_side_set_probit(side.handle, float(threshold), int(tag)))

    def probit_latent(self, side, nnz):
        """The latent scores the side's newest sampler launch read, in the order of its ratings (waits)."""
        z = np.empty(int(nnz))
        _lib.check(self.lib.bpmf_hip_side_probit_latent(side.handle, _ptr(z)))
        return z

    def probit_add(self, test, side, other):
        """Adds Phi(x . y) of the current factors to the running sums of the test matrix' entries (enqueue only)."""
        _lib.check(self.lib.bpmf_hip_test_probit_add(test[0], side.handle, other.handle))

    def probit_get(self, test):
        """(prob, nsamples): the mean probability of a positive per test entry, in the order given to test_create."""
        prob = np.empty(test[1])
        n = C.c_int()
        _lib.check(self.lib.bpmf_hip_test_probit_get(test[0], _ptr(prob), C.byref(n)))
        return prob, n.value

    # -- ordinal probit likelihood -------------------------------------------------
    def set_ordinal(self, side, levels, cutpoints=None, tag=11):
        """Turns `side` (created with mean_rating 0) into an ordinal side (include/bpmf_hip.h): its ratings
        take one of the C = len(levels) values `levels` (strictly increasing, 2 <= C <= 16), and every sampler launch of the side is
        preceded by the draw of its latent scores, truncated to the interval of each rating's level at the side's current
        cutpoints.  cutpoints: the C - 1 initial cutpoints, or None for Phi^-1 of the cumulative level frequencies.  tag >= 1 names
        the side's random streams (gibbs: 11 = movies, 12 = users).  Such a side is sampled with alpha = 1."""
        lv = np.ascontiguousarray(levels, np.float64)
        if lv.ndim != 1:
            raise ValueError("set_ordinal: the levels must be one array")
        cp = None
        if cutpoints is not None:
            cp = np.ascontiguousarray(cutpoints, np.float64)
            if cp.ndim != 1 or len(cp) != len(lv) - 1:
                raise ValueError("set_ordinal: %d levels need %d cutpoints" % (len(lv), len(lv) - 1))
        _lib.check(self.lib.bpmf_hip_side_set_ordinal(side.handle, _ptr(lv), len(lv), _ptr(cp), int(tag)))

    def ordinal_info(self, side):
        """(levels, log-likelihood passes enqueued so far) of an ordinal side."""
        n, runs = C.c_int(), C.c_int64()
        lv = np.zeros(16)
        _lib.check(self.lib.bpmf_hip_side_ordinal_info(side.handle, C.byref(n), _ptr(lv), C.byref(runs)))
        return lv[:n.value].copy(), runs.value

    def ordinal_latent(self, side, nnz):
        """The latent scores the side's newest sampler launch read, in the order of its ratings (waits)."""
        z = np.empty(int(nnz))
        _lib.check(self.lib.bpmf_hip_side_ordinal_latent(side.handle, _ptr(z)))
        return z

    def ordinal_cut_get(self, side):
        """The side's C - 1 cutpoints."""
        cp = np.zeros(15)
        _lib.check(self.lib.bpmf_hip_side_ordinal_cut_get(side.handle, _ptr(cp)))
        return cp[:len(self.ordinal_info(side)[0]) - 1].copy()

    def ordinal_cut_set(self, side, cutpoints):
        """Replaces the side's cutpoints (waits for the work in flight first)."""
        cp = np.ascontiguousarray(cutpoints, np.float64)
        if cp.ndim != 1 or len(cp) != len(self.ordinal_info(side)[0]) - 1:
            raise ValueError("ordinal_cut_set: the side has %d cutpoints" % (len(self.ordinal_info(side)[0]) - 1))
        _lib.check(self.lib.bpmf_hip_side_ordinal_cut_set(side.handle, _ptr(cp)))

    def ordinal_loglik(self, side, other, cutpoints_prop):
        """(l(g), l(g')): the log-likelihood of the side's ratings at its cutpoints g and at `cutpoints_prop`, the latent scores
        integrated out, from one pass over the ratings at the newest factors of both sides (waits)."""
        cp = np.ascontiguousarray(cutpoints_prop, np.float64)
        if cp.ndim != 1 or len(cp) != len(self.ordinal_info(side)[0]) - 1:
            raise ValueError("ordinal_loglik: the side has %d cutpoints" % (len(self.ordinal_info(side)[0]) - 1))
        out = np.zeros(2)
        _lib.check(self.lib.bpmf_hip_ordinal_loglik(side.handle, other.handle, _ptr(cp), _ptr(out)))
        return float(out[0]), float(out[1])

    def ordinal_cut_step(self, movies, users, it, step):
        """One Metropolis-Hastings step of the cutpoints of both sides given their factors (Cowles 1996; include/bpmf_hip.h has
        the proposal, the acceptance ratio and the random streams).  Returns whether the proposal was accepted (waits)."""
        acc = C.c_int()
        _lib.check(self.lib.bpmf_hip_ordinal_cut_step(movies.handle, users.handle, int(it), float(step), C.byref(acc)))
        return bool(acc.value)

    def ordinal_add(self, test, side, other):
        """Adds the level probabilities of the current factors and cutpoints to the running sums of the test matrix' entries
        (enqueue only)."""
        _lib.check(self.lib.bpmf_hip_test_ordinal_add(test[0], side.handle, other.handle))

    def ordinal_get(self, test):
        """(prob [entries, C], nsamples): the mean probability of every level per test entry, in the order given to test_create."""
        buf = np.empty(test[1] * 16)                 # (room for the largest C: the library says how many levels it wrote)
        n, c = C.c_int(), C.c_int()
        _lib.check(self.lib.bpmf_hip_test_ordinal_get(test[0], _ptr(buf), C.byref(c), C.byref(n)))
        return buf[:test[1] * c.value].reshape(test[1], c.value).copy(), n.value

    # -- censored ratings ----------------------------------------------------------
    def set_censored(self, side, flags, tag):
        """Marks ratings of `side` as bounds: flags holds one int8 per rating in the side's order, 0 = the value is the measurement,
        +1 = the true value is at least the recorded one, -1 = at most (bpmf_amd.censor_flags builds them from a sparse matrix).
        Every sampler launch of the side is then preceded by the draw of the latent values of its censored ratings
        (include/bpmf_hip.h).  tag >= 1 names the side's random streams: different per side, and apart from
        the tags of probit sides and features (gibbs: 5 = movies, 6 = users).  Any alpha > 0."""
        f = np.asarray(flags)
        if f.dtype != np.int8:
            if f.size and not np.all((f == -1) | (f == 0) | (f == 1)):
                raise ValueError("set_censored: the flags must be -1, 0 or +1")
            f = f.astype(np.int8)
        f = np.ascontiguousarray(f)
        if f.ndim != 1:
            raise ValueError("set_censored: the flags must be one array, one flag per rating of the side")
        if len(f) != side.nnz:
            raise ValueError("set_censored: %d flags for a side of %d ratings" % (len(f), side.nnz))
        _lib.check(self.lib.bpmf_hip_side_set_censored(side.handle, _ptr(f), int(tag)))

    def censored_count(self, side):
        """(lower bounds, upper bounds) of a censored side."""
        r, l = C.c_int64(), C.c_int64()
        _lib.check(self.lib.bpmf_hip_side_censored_count(side.handle, C.byref(r), C.byref(l)))
        return r.value, l.value

    def censored_latent(self, side):
        """The values the side's newest sampler launch read in place of its ratings, in their order: the ratings at the exact
        positions, the newest draws at the censored ones (waits)."""
        z = np.empty(side.nnz)
        _lib.check(self.lib.bpmf_hip_side_censored_latent(side.handle, _ptr(z)))
        return z

    # -- per-rating precision weights ---------------------------------------------
    def set_weights(self, side, w):
        """Gives every rating of `side` a precision weight: w holds one float64 per rating in the side's order, finite and > 0
        (bpmf_amd.rating_weights builds them from a sparse matrix); rating p is then observed with the precision alpha w[p].  The
        side's sampler launches run the weighted form of their kernel from now on (include/bpmf_hip.h).  A
        second call replaces the weights.  fp64 contexts, one GPU; not with probit, censored ratings, features, propagated priors
        or BPMF_REDUCE."""
        w = np.ascontiguousarray(w, np.float64)
        if w.ndim != 1:
            raise ValueError("set_weights: the weights must be one array, one weight per rating of the side")
        if len(w) != side.nnz:
            raise ValueError("set_weights: %d weights for a side of %d ratings" % (len(w), side.nnz))
        if len(w) == 0:
            w = np.ones(1)
        _lib.check(self.lib.bpmf_hip_side_set_weights(side.handle, _ptr(w)))

    # -- implicit feedback ----------------------------------------------------------
    def set_implicit(self, side, w0, w=None):
        """Makes `side` an implicit side: every cell of the matrix is observed, an unobserved one as a zero
        of weight w0, rating p with its value and the confidence w[p] > w0 (None: every confidence is 1, which needs w0 < 1).  The
        side's mean rating must be 0.  Both sides of a model are implicit and are stepped with implicit_sample.  weights_get
        returns sqrt(w - w0) and w r / sqrt(w - w0).  fp64 contexts, one GPU; not with weights, Student-t noise, a probit, ordinal
        or censored likelihood, features, propagated priors, BPMF_REDUCE or fold-in."""
        if w is not None:
            w = np.ascontiguousarray(w, np.float64)
            if w.ndim != 1 or len(w) != side.nnz:
                raise ValueError("set_implicit: %s confidences for a side of %d ratings" % (w.shape, side.nnz))
            if len(w) == 0:
                w = None
        _lib.check(self.lib.bpmf_hip_side_set_implicit(side.handle, float(w0), _ptr(w) if w is not None else None))

    def implicit_w0(self, side):
        """w0 of an implicit side, 0.0 for any other side."""
        return float(self.lib.bpmf_hip_side_implicit_w0(side.handle))

    def implicit_gram(self, side):
        """G (K x K) of the side's newest implicit_sample: the sum of u u^T over every column of the other side."""
        G = np.empty((self.K, self.K))
        _lib.check(self.lib.bpmf_hip_side_implicit_gram(side.handle, _ptr(G)))
        return G

    def implicit_sample(self, side, other, alpha):
        """One blocking half-iteration of an implicit side: hyper-parameters, G of `other` on the device, the weighted samplers
        under the prior precision Lambda + alpha w0 G (bpmf_hip_implicit_sample)."""
        _lib.check(self.lib.bpmf_hip_implicit_sample(side.handle, other.handle, float(alpha)))

    def weights_get(self, side):
        """(sw, zw) of a side with weights as the device holds them: sqrt(w) and sqrt(w) (r - mean_rating), in the ratings' order."""
        sw, zw = np.empty(side.nnz), np.empty(side.nnz)
        _lib.check(self.lib.bpmf_hip_side_weights_get(side.handle, _ptr(sw), _ptr(zw)))
        return sw, zw

    def weights_count(self, side):
        """(ratings whose weight is not 1, the smallest weight, the largest weight) of a side with weights."""
        n, lo, hi = C.c_int64(), C.c_double(), C.c_double()
        _lib.check(self.lib.bpmf_hip_side_weights_count(side.handle, C.byref(n), C.byref(lo), C.byref(hi)))
        return n.value, lo.value, hi.value

    # -- Student-t noise ------------------------------------------------------------
    def set_robust(self, side, nu, tag):
        """Makes `side` a robust side: Student-t noise with nu >= 1 degrees of freedom as a scale mixture (include/bpmf_hip.h, DESIGN.md
        section 21).  The side gets per-rating weights that start at 1 and are redrawn on the device ahead of every one of its
        sampler launches, on the Philox streams `tag` (>= 1; one per side, used by nothing else in the run).  fp64 contexts, one
        GPU; not with set_weights, probit, censored ratings, features, propagated priors or BPMF_REDUCE."""
        _lib.check(self.lib.bpmf_hip_side_set_robust(side.handle, float(nu), int(tag)))

    def robust_add(self, side):
        """Adds the weights the newest launch of a robust side read to their running sums (enqueue only, no host wait)."""
        _lib.check(self.lib.bpmf_hip_side_robust_add(side.handle))

    def robust_get(self, side):
        """(posterior-mean weight per rating in the side's order, samples added, nu) of a robust side."""
        w = np.empty(side.nnz)
        n, nu = C.c_int(), C.c_double()
        _lib.check(self.lib.bpmf_hip_side_robust_get(side.handle, _ptr(w), C.byref(n), C.byref(nu)))
        return w, n.value, nu.value

    # -- row and column bias terms ----------------------------------------------------
    def set_bias(self, side, lam=1.0, tag=13, role=0):
        """Gives `side` one bias per column, b_a ~ N(0, 1 / lam) (include/bpmf_hip.h): r = mean + b[col] + c[row]
        + x . y.  The biases start at 0 and are redrawn on the device ahead of every sampler launch of the side, on the Philox
        streams `tag` (>= 1; one per side, used by nothing else in the run); both sides of a pair carry biases or neither does, with
        different roles (0 / 1).  fp64 contexts, one GPU; not with probit, ordinal, censored ratings, weights, Student-t noise,
        features, propagated priors, BPMF_REDUCE, a sample ring or fold-in."""
        _lib.check(self.lib.bpmf_hip_side_set_bias(side.handle, float(lam), int(tag), int(role)))

    def bias_get(self, side):
        """The current biases of the side, one per column (waits)."""
        b = np.empty(side.ncols)
        _lib.check(self.lib.bpmf_hip_side_bias_get(side.handle, _ptr(b)))
        return b

    def bias_set(self, side, b):
        """Replaces the biases of the side (one finite value per column)."""
        b = np.ascontiguousarray(b, np.float64)
        if b.shape != (side.ncols,):
            raise ValueError("bias_set: %r values for a side of %d columns" % (b.shape, side.ncols))
        _lib.check(self.lib.bpmf_hip_side_bias_set(side.handle, _ptr(b)))

    def bias_latent(self, side):
        """The values the newest sampler launch of a side with biases read in place of its ratings: (r - b[col]) - c[row] (waits)."""
        z = np.empty(side.nnz)
        _lib.check(self.lib.bpmf_hip_side_bias_latent(side.handle, _ptr(z)))
        return z

    def bias_add(self, side):
        """Adds the current biases to their running sums (enqueue only, no host wait)."""
        _lib.check(self.lib.bpmf_hip_side_bias_add(side.handle))

    def bias_mean(self, side):
        """(posterior-mean bias per column, samples added)"""
        m = np.empty(side.ncols)
        n = C.c_int()
        _lib.check(self.lib.bpmf_hip_side_bias_mean(side.handle, _ptr(m), C.byref(n)))
        return m, n.value

    def bias_prior(self, side, a0, b0):
        """Samples the precision of the side's biases instead of fixing it: prior Gamma(a0, rate b0), drawn on the device at the start
        of every half-iteration of the side but its first (include/bpmf_hip.h)."""
        _lib.check(self.lib.bpmf_hip_side_bias_prior(side.handle, float(a0), float(b0)))

    def bias_lambda(self, side, n=0):
        """(current lambda of the side's biases, the lambda the steps of iterations 0 .. n - 1 ran with, bias steps enqueued so far,
        lambda draws enqueued so far); waits."""
        lam, steps, draws = C.c_double(), C.c_int64(), C.c_int64()
        trace = np.empty(max(int(n), 0))
        _lib.check(self.lib.bpmf_hip_side_bias_lambda_get(side.handle, C.byref(lam), _ptr(trace) if n > 0 else None, max(int(n), 0), C.byref(steps),
                                                          C.byref(draws)))
        return lam.value, trace, steps.value, draws.value

    # -- sparse tensor factorisation -----------------------------------------------
    @staticmethod
    def _tensor_entries(who, idx, vals):
        idx = np.asarray(idx)
        if idx.ndim != 2 or idx.shape[1] != 3:
            raise ValueError("%s: idx must be [nnz, 3], one 0-based index per mode" % who)
        if idx.size and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
            raise ValueError("%s: an index does not fit 32 bits" % who)
        vals = np.ascontiguousarray(vals, np.float64)
        if vals.shape != (idx.shape[0],):
            raise ValueError("%s: %d entries with %s values" % (who, idx.shape[0], vals.shape))
        cols = [np.ascontiguousarray(idx[:, m], np.int32) for m in range(3)]
        if idx.shape[0] == 0:
            cols, vals = [np.zeros(1, np.int32)] * 3, np.zeros(1)
        return cols, vals, int(idx.shape[0])

    def tensor_create(self, idx, vals, dims, mean_rating):
        """A sparse tensor of order 3 for Bayesian CP factorisation (include/bpmf_hip.h): idx [nnz, 3] holds the
        0-based indices of every entry, vals its value, dims the three sizes.  Every mode becomes a side (tensor.sides[m]) behind the
        Khatri-Rao rows of the other two modes.  fp64 engines, one GPU."""
        cols, v, nnz = self._tensor_entries("tensor_create", idx, vals)
        d = np.ascontiguousarray(dims, np.int64)
        if d.shape != (3,):
            raise ValueError("tensor_create: dims must hold three sizes (tensors of order 3 only)")
        h = C.c_void_p()
        _lib.check(self.lib.bpmf_hip_tensor_create(self.ctx, 3, _ptr(d), nnz, _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(v),
                                                   float(mean_rating), C.byref(h)))
        sides = []
        for m in range(3):
            sd = _Side(C.c_void_p(self.lib.bpmf_hip_tensor_side(h, m)), self.K, int(d[m]), max(nnz, 1), 0, int(d[m]), None)
            sd.nnz = nnz
            sides.append(sd)
        t = _Tensor(h, tuple(int(x) for x in d), nnz, float(mean_rating), sides)
        if not hasattr(self, "_tensors"):
            self._tensors = []
        self._tensors.append(t)
        return t

    def tensor_destroy(self, tensor):
        if tensor.handle:
            for tt in tensor.tests:
                self.tensor_test_destroy(tt)
            _lib.check(self.lib.bpmf_hip_tensor_destroy(tensor.handle))
            tensor.handle = None
            for sd in tensor.sides:
                sd.handle = None

    def tensor_sample(self, tensor, mode, it, alpha, mu, LambdaF):
        """One blocking half-iteration of a mode: its Khatri-Rao rows, then its sampler.  Returns (sum[K], prod[K,K], norm)."""
        K = self.K
        mu = np.ascontiguousarray(mu, np.float64)
        LF = np.asfortranarray(LambdaF, np.float64)
        s = np.empty(K); prod = np.empty((K, K), order="F"); nrm = np.empty(1)
        _lib.check(self.lib.bpmf_hip_tensor_sample(tensor.handle, int(mode), int(it), float(alpha), _ptr(mu), _ptr(LF), _ptr(s), _ptr(prod),
                                                   _ptr(nrm)))
        return s, prod, float(nrm[0])

    def tensor_product(self, tensor, mode):
        """[nnz, ld] array: row e holds the Khatri-Rao row of the entry at position e of the mode's order (the entries sorted stably
        by their index in that mode), as the mode's next sampler launch would read it; columns K .. ld - 1 are the zero padding."""
        out = np.empty((max(tensor.nnz, 1), self.ld()), np.float64)
        _lib.check(self.lib.bpmf_hip_tensor_product(tensor.handle, int(mode), _ptr(out)))
        return out[:tensor.nnz]

    def tensor_product_run(self, tensor, mode):
        """Runs the Khatri-Rao kernel of a mode and waits, without the copy to the host (measurements)."""
        _lib.check(self.lib.bpmf_hip_tensor_product(tensor.handle, int(mode), None))

    def tensor_last_ms(self, tensor):
        """Device time in ms of the newest Khatri-Rao launch of a mode of the tensor (waits for it)."""
        ms = C.c_float()
        _lib.check(self.lib.bpmf_hip_tensor_last_ms(tensor.handle, C.byref(ms)))
        return ms.value

    def tensor_test(self, tensor, idx, vals):
        """The test entries of a tensor (idx [n, 3] 0-based, vals [n]) for tensor_predict."""
        cols, v, n = self._tensor_entries("tensor_test", idx, vals)
        h = C.c_void_p()
        _lib.check(self.lib.bpmf_hip_tensor_test_create(tensor.handle, n, _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(v), C.byref(h)))
        tt = [h, n, tensor]
        tensor.tests.append(tt)
        return tt

    def tensor_test_destroy(self, test):
        if test[0]:
            _lib.check(self.lib.bpmf_hip_tensor_test_destroy(test[0]))
            test[0] = None

    def tensor_predict(self, test, n):
        """(se, se_avg, count) of the test entries against the current factors; n as in predict (0 during burn-in, then the number
        of samples already averaged)."""
        se = C.c_double(); sea = C.c_double(); cnt = C.c_int64()
        _lib.check(self.lib.bpmf_hip_tensor_predict(test[0], int(n), C.byref(se), C.byref(sea), C.byref(cnt)))
        return se.value, sea.value, cnt.value

    def tensor_test_get(self, test):
        """(Pavg, Pm2) of the test entries, in the order they were passed."""
        pavg = np.empty(max(test[1], 1)); pm2 = np.empty(max(test[1], 1))
        _lib.check(self.lib.bpmf_hip_tensor_test_get(test[0], _ptr(pavg), _ptr(pm2)))
        return pavg[:test[1]], pm2[:test[1]]

    # -- side information ---------------------------------------------------------
    def set_features(self, side, F, lambda_beta=5.0, tag=3):
        """Gives `side` the feature matrix F [ncols, D] (one row per column of the side), a link matrix beta (D x K, 0) and the
        fixed lambda_beta.  tag >= 1 names the random stream of the link draw: different per side.  From then on the side -- and
        its partner -- are stepped with link_sample.  A dense ndarray (D <= 1024) takes the dense path of DESIGN.md section 13; a
        scipy.sparse matrix (any D, tag < 0x10000) is converted to canonical CSR and takes the CG path of section 14.  Nothing is
        converted from dense to sparse or back."""
        if _is_sparse(F):
            if F.ndim != 2 or F.shape[0] != side.ncols:
                raise ValueError("set_features: F must be [%d, D], one row per column of the side" % side.ncols)
            rowptr, colidx, vals = csr_arrays(F)
            _lib.check(self.lib.bpmf_hip_side_set_features_sparse(side.handle, int(F.shape[1]), _ptr(rowptr), _ptr(colidx), _ptr(vals),
                                                                  float(lambda_beta), int(tag)))
            side.link_d = int(F.shape[1]); side.link_sparse = True
            return
        F = np.asarray(F, np.float64)
        if F.ndim != 2 or F.shape[0] != side.ncols:
            raise ValueError("set_features: F must be [%d, D], one row per column of the side" % side.ncols)
        row_major = not (F.flags.f_contiguous and not F.flags.c_contiguous)
        F = np.asfortranarray(F) if not row_major else np.ascontiguousarray(F)
        _lib.check(self.lib.bpmf_hip_side_set_features(side.handle, _ptr(F), int(F.shape[1]), 1 if row_major else 0, float(lambda_beta), int(tag)))
        side.link_d = int(F.shape[1])

    def link_sample(self, side, other, alpha):
        """The blocking half-iteration of a model with side information (both sides go through it; include/bpmf_hip.h)."""
        _lib.check(self.lib.bpmf_hip_link_sample(side.handle, other.handle, float(alpha)))

    def link_lambda_prior(self, side, a0=5e-4, b0=5e-4):
        """Switches the sampling of the side's lambda_beta on: prior Gamma(shape a0, rate b0), one draw at the start of every
        half-iteration but the side's first.  Only before the side's first half-iteration.  A side with
        dense features factors G(lambda_beta) on the device from then on."""
        _lib.check(self.lib.bpmf_hip_side_link_lambda_prior(side.handle, float(a0), float(b0)))

    def link_lambda_set(self, side, lam):
        """Sets lambda_beta for the following draws of beta (a chain continued from stored state; tests).  A side with dense
        features factors G(lambda_beta) on the device from then on; without a prior the value stays fixed."""
        _lib.check(self.lib.bpmf_hip_side_link_lambda_set(side.handle, float(lam)))

    def link_lambda_get(self, side):
        """(lambda_beta, the trace tr(Lambda beta^T beta) of its newest draw or NaN, whether it is sampled)."""
        lam, tr, on = C.c_double(), C.c_double(), C.c_int()
        _lib.check(self.lib.bpmf_hip_side_link_lambda_get(side.handle, C.byref(lam), C.byref(tr), C.byref(on)))
        return lam.value, tr.value, bool(on.value)

    def link_chol_solve(self, A, P, E=None, want_factor=False):
        return link_chol_solve(A, P, E, want_factor, self.device)

    def link_cg_set(self, side, tol=1e-6, max_iter=1000):
        """The stopping rule of the CG draw of a side with sparse features: relative residual tol, at most max_iter iterations."""
        _lib.check(self.lib.bpmf_hip_side_link_cg_set(side.handle, float(tol), int(max_iter)))

    def link_cg_stats(self, side):
        """dict(iters_last, iters_total, relres_max_last, hit_max_iter) of the CG draws of a side with sparse features."""
        it, tot, rel, hit = C.c_int(), C.c_int64(), C.c_double(), C.c_int()
        _lib.check(self.lib.bpmf_hip_side_link_cg_stats(side.handle, C.byref(it), C.byref(tot), C.byref(rel), C.byref(hit)))
        return dict(iters_last=it.value, iters_total=tot.value, relres_max_last=rel.value, hit_max_iter=bool(hit.value))

    def link_get(self, side):
        """(beta [D, K], offsets M = F beta [ncols, K]) of a side with features."""
        beta = np.empty((getattr(side, "link_d", 0), self.K)); offs = np.empty((side.ncols, self.K))
        _lib.check(self.lib.bpmf_hip_side_link_get(side.handle, _ptr(beta), _ptr(offs)))
        return beta, offs

    def link_set(self, side, beta):
        """Sets beta [D, K]; the offsets are recomputed on the device."""
        beta = np.ascontiguousarray(beta, np.float64)
        assert beta.shape == (side.link_d, self.K)
        _lib.check(self.lib.bpmf_hip_side_link_set(side.handle, _ptr(beta)))

    def link_add(self, side):
        """Adds the current beta to the side's running sum (where aggr_add sits)."""
        _lib.check(self.lib.bpmf_hip_side_link_add(side.handle))

    def link_mean(self, side):
        """(mean of the added beta [D, K], samples added)."""
        beta = np.empty((getattr(side, "link_d", 0), self.K)); n = C.c_int()
        _lib.check(self.lib.bpmf_hip_side_link_mean(side.handle, _ptr(beta), C.byref(n)))
        return beta, n.value

    def link_residual(self, side, other, nnz):
        """r - m_c . y_r of the side's ratings for its current offsets and the other side's current factors (tests, tools)."""
        r = np.empty(int(nnz))
        _lib.check(self.lib.bpmf_hip_side_link_residual(side.handle, other.handle, _ptr(r)))
        return r

    def link_shift(self, side):
        """U += M on the side's current factors; returns sum |u|^2 (tests, tools)."""
        nrm = C.c_double()
        _lib.check(self.lib.bpmf_hip_side_link_shift(side.handle, C.byref(nrm)))
        return nrm.value

    def kernel_name(self, side):
        """The kernel(s) one sampler launch of the side consists of, as a profile names them."""
        buf = C.create_string_buffer(512)
        _lib.check(self.lib.bpmf_hip_side_kernel_name(side.handle, buf, 512))
        return buf.value.decode()

    def kernel_resources(self, side):
        """[{kernel, lds_bytes_per_workgroup, threads_per_workgroup, workgroups_per_cu, vgprs}] of the kernels one sampler
        launch of the side consists of (asked of the library's dispatch logic; nothing is launched)."""
        out = np.zeros(32, np.int64)
        names = C.create_string_buffer(1024)
        n = self.lib.bpmf_hip_side_kernel_resources(side.handle, _ptr(out), 8, names, 1024)
        if n < 0:
            _lib.check(n)
        spelt = names.value.decode().split(";") if n else []
        listed = [x.strip() for x in self.kernel_name(side).split(" + ")]
        res = []
        for i in range(n):
            nm = spelt[i] if i < len(spelt) else "?"
            if nm in ("kernel", "?") and len(listed) == n:            # (launched through a generic lambda: the name list says which)
                nm = listed[i]
            rec = {"kernel": nm, "lds_bytes_per_workgroup": int(out[4 * i]), "threads_per_workgroup": int(out[4 * i + 1]),
                   "workgroups_per_cu": int(out[4 * i + 2]), "vgprs": int(out[4 * i + 3])}
            # the probe asks the unfused dispatch; a fused launch (k_sample1s<64> = the same device code + the statistics rider
            # of kernels_slab.h) is reported under the name the side launches, with the probed twin named beside it
            if n == 1 and len(listed) == 1 and listed[0].split("<")[0] != nm.split("<")[0]:
                rec["kernel"], rec["probed_as"] = listed[0], nm
            res.append(rec)
        return res

    def schedule_info(self, side):
        out = np.zeros(16, np.int64)
        _lib.check(self.lib.bpmf_hip_side_schedule_info(side.handle, _ptr(out), 16))
        keys = ("mode", "work_items", "chunks", "chunked_columns", "light_columns", "other_items", "pf_le3", "pf_4to6", "pf_7to16",
                "lr_columns", "parts", "local_columns", "local_ratings", "pf_ratings", "pf_ratings_sq", "chunk")
        return {k: int(v) for k, v in zip(keys, out)}

    def stat_info(self, side):
        """The side's column statistics pass (bpmf_hip_side_stat_info): form "waves" / "workgroups" / "tiles", units (waves,
        workgroups or slices), columns per wave or slice, empty ranges, passes enqueued as riders / stand-alone."""
        out = np.zeros(8, np.int64)
        _lib.check(self.lib.bpmf_hip_side_stat_info(side.handle, _ptr(out), 8))
        return {"form": ("waves", "workgroups", "tiles")[int(out[0])], "units": int(out[1]), "per": int(out[2]), "empty": int(out[3]),
                "rider_passes": int(out[4]), "alone_passes": int(out[5])}

    def schedule_items(self, side):
        """The side's work items in launch order: (local column, ratings, heavy-column ordinal or -1) arrays."""
        n = C.c_int64()
        _lib.check(self.lib.bpmf_hip_side_schedule_items(side.handle, None, None, None, 0, C.byref(n)))
        col = np.zeros(n.value, np.int32); ln = np.zeros(n.value, np.int32); heavy = np.zeros(n.value, np.int32)
        if n.value:
            _lib.check(self.lib.bpmf_hip_side_schedule_items(side.handle, _ptr(col), _ptr(ln), _ptr(heavy), n.value, None))
        return col, ln, heavy

    def kernel_ms_sum(self, side):
        """(sampler ms, statistics ms, launches) summed over the half-iterations run through sys_sample."""
        a = C.c_double(); b = C.c_double(); n = C.c_int64()
        _lib.check(self.lib.bpmf_hip_side_kernel_ms_sum(side.handle, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def last_kernel_ms(self, side):
        a = C.c_float(); b = C.c_float()
        _lib.check(self.lib.bpmf_hip_side_last_kernel_ms(side.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- prediction -----------------------------------------------------------
    def test_create(self, side, tcolptr, trowidx, tvals):
        tcolptr = np.ascontiguousarray(tcolptr, np.int64)
        trowidx = np.ascontiguousarray(trowidx, np.int32)
        tvals = np.ascontiguousarray(tvals, np.float64)
        h = C.c_void_p()
        _lib.check(self.lib.bpmf_hip_test_create(side.handle, _ptr(tcolptr), _ptr(trowidx), _ptr(tvals), C.byref(h)))
        t = [h, int(tcolptr[-1]), side]
        if not hasattr(self, "_tests"):
            self._tests = []
        self._tests.append(t)
        return t

    def test_set_twin(self, test, twin):
        """users.predict(movies): `twin` (a test matrix of the other side) is evaluated whenever `test` is."""
        _lib.check(self.lib.bpmf_hip_test_set_twin(test[0], twin[0] if twin is not None else None))

    def test_destroy(self, test):
        if test[0]:
            _lib.check(self.lib.bpmf_hip_test_destroy(test[0]))
            test[0] = None

    def predict(self, test, side, other, n):
        se = C.c_double(); sea = C.c_double(); cnt = C.c_int64()
        _lib.check(self.lib.bpmf_hip_predict(test[0], side.handle, other.handle, int(n), C.byref(se), C.byref(sea), C.byref(cnt)))
        return se.value, sea.value, cnt.value

    def predict_launch(self, test, side, other, n):
        _lib.check(self.lib.bpmf_hip_predict_launch(test[0], side.handle, other.handle, int(n)))

    def predict_finish(self, test):
        se = C.c_double(); sea = C.c_double(); cnt = C.c_int64()
        _lib.check(self.lib.bpmf_hip_predict_finish(test[0], C.byref(se), C.byref(sea), C.byref(cnt)))
        return se.value, sea.value, cnt.value

    def test_get(self, test):
        pavg = np.empty(test[1]); pm2 = np.empty(test[1])
        _lib.check(self.lib.bpmf_hip_test_get(test[0], _ptr(pavg), _ptr(pm2)))
        return pavg, pm2

    # -- host-side hyper parameters (also in the library, not device code) -------
    def hyper_sample(self, N, cov, counter, Um=None, extra_scatter=None, extra_dof=0):
        return hyper_sample(self.K, N, cov, counter, Um, extra_scatter, extra_dof)

    def randn_device(self, counter, n):
        out = np.empty(n)
        _lib.check(self.lib.bpmf_hip_randn_stream(self.ctx, int(counter) & 0xFFFFFFFF, int(n), _ptr(out)))
        return out


def noise_sample(a0, b0, sse, n, it, alpha_max=None):
    """bpmf_hip_noise_sample (host only: needs the library, not a GPU)."""
    out = C.c_double()
    _lib.check(_lib.load_library().bpmf_hip_noise_sample(float(a0), float(b0), float(sse), int(n), int(it),
                                                         0.0 if alpha_max is None else float(alpha_max), C.byref(out)))
    return out.value


def link_lambda_counter(it, tag):
    """BPMF_LINK_LAMBDA_COUNTER(it, tag) of include/bpmf_hip.h: the Philox stream of the lambda_beta draw of half-iteration `it`."""
    return (0x80000000 + 16 * int(it) + (int(tag) & 15)) & 0xFFFFFFFF


def link_lambda_sample(a0, b0, trace, count, it, tag):
    """bpmf_hip_link_lambda_sample (host only): g / (b0 + trace / 2), g ~ Gamma(a0 + count / 2, 1) on the Philox stream
    BPMF_LINK_LAMBDA_COUNTER(it, tag).  count = D K, trace = tr(Lambda beta^T beta)."""
    if int(tag) < 0:
        raise ValueError("link_lambda_sample: tag must be 1 .. 15")
    out = C.c_double()
    _lib.check(_lib.load_library().bpmf_hip_link_lambda_sample(float(a0), float(b0), float(trace), int(count), int(it), int(tag), C.byref(out)))
    return out.value


def auc(score, value, threshold=0.5):
    """bpmf_hip_auc (host only): area under the ROC curve of `score` against the labels value > threshold, ties counted half;
    NaN when one class is empty."""
    score = np.ascontiguousarray(score, np.float64)
    value = np.ascontiguousarray(value, np.float64)
    if score.shape != value.shape or score.ndim != 1:
        raise ValueError("auc: score and value must be vectors of one length")
    out = C.c_double()
    _lib.check(_lib.load_library().bpmf_hip_auc(_ptr(score), _ptr(value), len(score), float(threshold), C.byref(out)))
    return out.value


def hyper_sample(K, N, cov, counter, Um=None, extra_scatter=None, extra_dof=0):
    """HyperParams::sample on the host (c++/bpmf.h:98-103): returns mu[K], LambdaU[K,K], LambdaF[K,K].
    extra_scatter [K, K] / extra_dof: added to the posterior scale matrix / the Wishart degrees of freedom (side information:
    lambda_beta beta^T beta and D); None and 0: the plain draw."""
    lib = _lib.load_library()
    cov = np.asfortranarray(cov, np.float64)
    mu = np.empty(K); LU = np.empty((K, K), order="F"); LF = np.empty((K, K), order="F")
    um = np.ascontiguousarray(Um, np.float64) if Um is not None else None
    if extra_scatter is not None or extra_dof:
        sc = np.asfortranarray(extra_scatter, np.float64) if extra_scatter is not None else None
        if sc is not None and sc.shape != (K, K):
            raise ValueError("extra_scatter must be [K, K]")
        _lib.check(lib.bpmf_hyper_sample_ex(int(K), int(N), _ptr(cov), _ptr(um), _ptr(sc), int(extra_dof), int(counter) & 0xFFFFFFFF,
                                            _ptr(mu), _ptr(LU), _ptr(LF)))
        return mu, LU, LF
    _lib.check(lib.bpmf_hyper_sample(int(K), int(N), _ptr(cov), _ptr(um), int(counter) & 0xFFFFFFFF, _ptr(mu), _ptr(LU), _ptr(LF)))
    return mu, LU, LF


def cov_from_sums(K, N, s, prod):
    lib = _lib.load_library()
    s = np.ascontiguousarray(s, np.float64); prod = np.asfortranarray(prod, np.float64)
    cov = np.empty((K, K), order="F")
    lib.bpmf_cov_from_sums(int(K), int(N), _ptr(s), _ptr(prod), _ptr(cov))
    return cov


def randn_host(counter, n, tag=0):
    """n normals of the host stream `counter`; tag: key word 1 of the stream (0: the samplers' streams)."""
    lib = _lib.load_library()
    out = np.empty(n)
    if tag:
        lib.bpmf_randn_stream_tag(int(counter) & 0xFFFFFFFF, int(tag) & 0xFFFFFFFF, int(n), _ptr(out))
    else:
        lib.bpmf_randn_stream(int(counter) & 0xFFFFFFFF, int(n), _ptr(out))
    return out


def link_gemm_tn(A, B=None, bvec=None, device=0):
    """A^T (B - 1 bvec^T) on the device through k_link_gemm_tn (B = None: A^T A).  Row-major fp64 host arrays; tests and tools."""
    A = np.ascontiguousarray(A, np.float64)
    N, D = A.shape
    n = D if B is None else B.shape[1]
    Bc = np.ascontiguousarray(B, np.float64) if B is not None else None
    v = np.ascontiguousarray(bvec, np.float64) if bvec is not None else None
    out = np.empty((D, n))
    _lib.check(_lib.load_library().bpmf_hip_link_gemm_tn(int(device), _ptr(A), N, D, _ptr(Bc), n, _ptr(v), _ptr(out)))
    return out


def link_gemm_nn(A, B, device=0):
    """A B on the device through k_link_gemm_nn (B: D x n, n <= 128).  Row-major fp64 host arrays; tests and tools."""
    A = np.ascontiguousarray(A, np.float64); B = np.ascontiguousarray(B, np.float64)
    N, D = A.shape
    out = np.empty((N, B.shape[1]))
    _lib.check(_lib.load_library().bpmf_hip_link_gemm_nn(int(device), _ptr(A), N, D, _ptr(B), B.shape[1], _ptr(out)))
    return out


def link_chol_solve(A, P, E=None, want_factor=False, device=0):
    """X = L^-T (L^-1 P + E) with A = L L^T, by the blocked Cholesky and the two blocked triangular solves of kernels_link_chol.h
    (A: D x D symmetric positive definite, D <= 1024; P, E: D x n, n <= 128).  Returns X, or (X, L) with want_factor.  Row-major
    fp64 host arrays; tests and tools."""
    A = np.ascontiguousarray(A, np.float64); P = np.ascontiguousarray(P, np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or P.ndim != 2 or P.shape[0] != A.shape[0]:
        raise ValueError("link_chol_solve: A must be [D, D] and P [D, n]")
    Ec = np.ascontiguousarray(E, np.float64) if E is not None else None
    if Ec is not None and Ec.shape != P.shape:
        raise ValueError("link_chol_solve: E must have the shape of P")
    D, n = P.shape
    X = np.empty((D, n)); Lo = np.empty((D, D)) if want_factor else None
    _lib.check(_lib.load_library().bpmf_hip_link_chol_solve(int(device), _ptr(A), D, _ptr(P), _ptr(Ec), n, _ptr(X), _ptr(Lo)))
    return (X, Lo) if want_factor else X


def _is_sparse(F):
    """a scipy.sparse matrix or array (without importing scipy for a dense caller)"""
    return hasattr(F, "tocsr") and hasattr(F, "nnz") and not isinstance(F, np.ndarray)


def csr_arrays(F):
    """(rowptr int64, colidx int32, vals float64 or None) of a scipy.sparse matrix in canonical CSR: duplicates summed, indices
    sorted within a row.  Stored zeros are kept (they are part of the pattern).  vals is None when every stored value is 1."""
    F = F.tocsr().astype(np.float64)
    if not F.has_canonical_format:
        F = F.copy()
        F.sum_duplicates()
    rowptr = np.ascontiguousarray(F.indptr, np.int64)
    colidx = np.ascontiguousarray(F.indices, np.int32)
    vals = np.ascontiguousarray(F.data, np.float64)
    if len(colidx) == 0:
        colidx = np.zeros(1, np.int32)
    return rowptr, colidx, (None if len(vals) and np.all(vals == 1.0) else (vals if len(vals) else None))


def foldin_csr(rows, ncols):
    """(rowptr int64, colidx int32, vals float64) of the new rows of a fold-in: a scipy.sparse matrix [n_new, ncols] with its
    indices sorted within a row and NOTHING summed (a cell stored twice stays twice, for the library to refuse), or a CSR triple
    passed through."""
    if _is_sparse(rows):
        if rows.ndim != 2 or rows.shape[1] != ncols:
            raise ValueError("foldin: the new rows must be [n_new, %d], one column per column of the candidate side" % ncols)
        R = rows.tocsr().astype(np.float64)
        if not R.has_sorted_indices:
            R = R.copy()
            R.sort_indices()
        rowptr, colidx, vals = R.indptr, R.indices, R.data
    else:
        rowptr, colidx, vals = rows
    rowptr = np.ascontiguousarray(rowptr, np.int64)
    colidx = np.ascontiguousarray(colidx, np.int32)
    vals = np.ascontiguousarray(vals, np.float64)
    if rowptr.ndim != 1 or len(rowptr) < 1 or len(colidx) != len(vals) or (len(rowptr) and int(rowptr[-1]) != len(colidx)):
        raise ValueError("foldin: (rowptr, colidx, vals) is not a CSR triple")
    if len(colidx) == 0:
        colidx = np.zeros(1, np.int32); vals = np.zeros(1)
    return rowptr, colidx, vals


def link_spmm_nn(F, V, device=0):
    """F V on the device through k_sp_rows (F: scipy.sparse N x D, V: D x n, n <= 128); tests and tools."""
    V = np.ascontiguousarray(V, np.float64)
    rowptr, colidx, vals = csr_arrays(F)
    N, D = F.shape
    out = np.empty((N, V.shape[1]))
    _lib.check(_lib.load_library().bpmf_hip_link_spmm_nn(int(device), N, D, _ptr(rowptr), _ptr(colidx), _ptr(vals), _ptr(V), V.shape[1], _ptr(out)))
    return out


def link_spmm_tn(F, X, lam=0.0, P=None, device=0):
    """F^T X (+ lam P) on the device (F: scipy.sparse N x D, X: N x n, P: D x n, n <= 128); tests and tools."""
    X = np.ascontiguousarray(X, np.float64)
    Pc = np.ascontiguousarray(P, np.float64) if P is not None else None
    rowptr, colidx, vals = csr_arrays(F)
    N, D = F.shape
    out = np.empty((D, X.shape[1]))
    _lib.check(_lib.load_library().bpmf_hip_link_spmm_tn(int(device), N, D, _ptr(rowptr), _ptr(colidx), _ptr(vals), _ptr(X), X.shape[1], float(lam),
                                                         _ptr(Pc), _ptr(out)))
    return out


def link_cg_solve(F, lam, RHS, tol=1e-6, max_iter=1000, device=0):
    """(X, iters per column, hit_max_iter): (F^T F + lam I) X = RHS by the device's lockstep CG (RHS: D x n, n <= 128)."""
    RHS = np.ascontiguousarray(RHS, np.float64)
    rowptr, colidx, vals = csr_arrays(F)
    N, D = F.shape
    n = RHS.shape[1]
    X = np.empty((D, n)); iters = np.zeros(n, np.int32); hit = C.c_int()
    _lib.check(_lib.load_library().bpmf_hip_link_cg_solve(int(device), N, D, _ptr(rowptr), _ptr(colidx), _ptr(vals), float(lam), _ptr(RHS), n,
                                                          float(tol), int(max_iter), _ptr(X), _ptr(iters), C.byref(hit)))
    return X, iters, bool(hit.value)


def link_noise_rows(nrows, K, it, key_word, Rinv=None, device=0):
    """Rows 0 .. nrows - 1 of the device's noise matrix of iteration `it` and key word `key_word` [nrows, K], times R^-T when Rinv
    (K x K, upper triangular) is given."""
    R = np.ascontiguousarray(Rinv, np.float64) if Rinv is not None else None
    out = np.empty((int(nrows), int(K)))
    _lib.check(_lib.load_library().bpmf_hip_link_noise_rows(int(device), int(nrows), int(K), int(it) & 0xFFFFFFFF, int(key_word) & 0xFFFFFFFF,
                                                            _ptr(R), _ptr(out)))
    return out
