"""CPU restatement of the acquisition scores of the scored top-N ranking in numpy longdouble, the error
bounds the GPU tests judge the device by, and the checks of a device list that do not depend on how near ties fall.

With p_s = mean_rating + u_s(q) . v_s(c) over the S kept samples, mean and std as tests/newrows_ref.predict (w = None) and
z_s = (p_s - t) / sigma:
    ucb    mean + kappa std
    prob   (1/S) sum_s Phi(z_s)                                 sigma = 0: (1/S) #{s : p_s > t}
    ei     (1/S) sum_s [(p_s - t) Phi(z_s) + sigma phi(z_s)]    sigma = 0: (1/S) sum_s max(p_s - t, 0)
Phi is scipy.special.ndtr.

Bounds b(q, c) on |device score - reference|, with u = 2^-53, eps = 2^-52 and
    delta = max_s (Kp + 2) u sum_k |u_k v_k|        the forward error allowed to one p_s (mean_rating is NOT part of the sum)
  ucb   mean_bound + |kappa| * db_std + 3 u (|mean| + |kappa| std), where db_std bounds the error of the square root of a variance
        known to var_bound: |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= min(var_bound / std, sqrt(var_bound))
  prob  (0.3989 / sigma) delta + 8 eps              |dPhi/dp| <= phi(0) / sigma; 8 eps: erfc, the S additions, the division
  ei    delta + 8 eps (|mean - t| + sigma)          |d ei / dp| = Phi <= 1
"""
import numpy as np

from tests import newrows_ref as nr

LD = np.longdouble
U53 = 2.0 ** -53
EPS = 2.0 ** -52
KINDS = ("ucb", "prob", "ei")


def per_sample(Es, Vs, mean_rating):
    """(p [S, nq, nc] longdouble, max_s sum_k |u_k v_k| [nq, nc]) of Es [S, nq, K], Vs [S, nc, K]"""
    Es, Vs = np.asarray(Es, LD), np.asarray(Vs, LD)
    P = LD(mean_rating) + np.einsum("sqk,sck->sqc", Es, Vs)
    A = np.einsum("sqk,sck->sqc", np.abs(Es), np.abs(Vs))
    return P, A.max(0)


def reference(Es, Vs, mean_rating, Kp, kind, param, sigma=0.0):
    """dict(score, bound, mean, std) [nq, nc]: the reference score in longdouble and the bound of the module docstring"""
    from scipy.special import ndtr
    good = nr.predict(Es, Vs, mean_rating)
    mean, var = good["mean"], good["var"]
    std = np.sqrt(var)
    P, absmax = per_sample(Es, Vs, mean_rating)
    S = P.shape[0]
    delta = (Kp + 2) * U53 * absmax
    if kind == "ucb":
        vb = np.asarray(nr.var_bound(good, Kp), LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            db_std = np.where(std > 0, np.minimum(vb / np.where(std > 0, std, 1), np.sqrt(vb)), np.sqrt(vb))
        score = mean + LD(param) * std
        bound = nr.mean_bound(good, Kp, mean_rating) + abs(param) * db_std + 3.0 * U53 * (np.abs(mean) + abs(param) * std)
    elif kind == "prob":
        d = P - LD(param)
        if sigma == 0:
            score = (d > 0).sum(0) / LD(S)
            bound = np.zeros_like(score)
        else:
            score = np.asarray(ndtr(np.asarray(d / LD(sigma), np.float64)), LD).sum(0) / LD(S)
            bound = (0.3989 / sigma) * delta + 8.0 * EPS
    elif kind == "ei":
        d = P - LD(param)
        if sigma == 0:
            score = np.maximum(d, 0).sum(0) / LD(S)
            bound = delta
        else:
            z = d / LD(sigma)
            Phi = np.asarray(ndtr(np.asarray(z, np.float64)), LD)
            phi = np.exp(-z * z / 2) / np.sqrt(2 * LD(np.pi))
            score = (d * Phi + LD(sigma) * phi).sum(0) / LD(S)
            bound = delta + 8.0 * EPS * (np.abs(mean - LD(param)) + sigma)
    else:
        raise ValueError(kind)
    return dict(score=score, bound=np.asarray(bound, LD), mean=mean, std=std)


def exact_scores(Us, Vs, mean_rating, kind, param):
    """the sigma = 0 forms (and ucb with kappa = 0) in plain fp64, for inputs on which every sum is exact"""
    P = mean_rating + np.einsum("sqk,sck->sqc", Us, Vs)
    S = P.shape[0]
    if kind == "prob":
        return (P > param).sum(0) / float(S)
    if kind == "ei":
        return np.maximum(P - param, 0.0).sum(0) / float(S)
    return P.sum(0) / float(S)


def ranked(score, n, rated=None, q_from=0):
    """(idx, score) [nq, n]: the n best columns of every row by (score descending, id ascending) among those not in rated[q_from + i];
    padding: idx -1, score 0"""
    nq, nc = score.shape
    idx = np.full((nq, n), -1, np.int32); out = np.zeros((nq, n))
    for i in range(nq):
        ok = np.ones(nc, bool)
        if rated is not None:
            ok[list(rated[q_from + i])] = False
        cand = np.nonzero(ok)[0]
        order = cand[np.lexsort((cand, -score[i, cand]))][:n]
        idx[i, :len(order)] = order
        out[i, :len(order)] = score[i, order]
    return idx, out


def check_lists(idx, score, ref, n, rated=None, q_from=0, tag=None):
    """The three checks of a device list against a reference that no near tie can flake: (i) every listed score within its bound;
    (ii) every list sorted by (device score descending, id ascending), without an excluded or a duplicate id, and as long as the
    eligible candidates allow; (iii) every eligible candidate not listed has a reference score <= the list's last device score + its
    own bound.  Returns max over the picks of err / bound (0 where the bound is 0 and the error too)."""
    want, bound = ref["score"], ref["bound"]
    nc = want.shape[1]
    worst = 0.0
    for i in range(idx.shape[0]):
        q = q_from + i
        ok = np.ones(nc, bool)
        if rated is not None:
            ok[list(rated[q])] = False
        k = min(n, int(ok.sum()))
        ids = idx[i, :k]
        assert (ids >= 0).all() and (idx[i, k:] == -1).all() and (score[i, k:] == 0).all(), (tag, q)
        assert ok[ids].all() and len(set(ids.tolist())) == k, (tag, q)
        err = np.abs(LD(1) * score[i, :k] - want[q, ids])
        assert (err <= bound[q, ids]).all(), (tag, q, np.asarray(err, float), np.asarray(bound[q, ids], float))
        nz = bound[q, ids] > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[q, ids][nz]).max()))
        for r in range(k - 1):
            assert score[i, r] > score[i, r + 1] or (score[i, r] == score[i, r + 1] and ids[r] < ids[r + 1]), (tag, q, r)
        if k == n and k < ok.sum():
            ok[ids] = False
            rest = np.nonzero(ok)[0]
            assert (want[q, rest] <= LD(1) * score[i, n - 1] + bound[q, rest]).all(), (tag, q)
    return worst
