"""CPU restatement of the similar-columns ranking in numpy longdouble, the error bounds the GPU tests judge the
device by, the checks of a device list that do not depend on how near ties fall, and the planted experiment.

One side is both the query and the candidate.  With v_s(c) column c of kept sample s (Vs [S, nc, K]):
    d_s = v_s(q) . v_s(c)      n_s(c) = |v_s(c)|^2      r_s(c) = 1 / sqrt(n_s(c)), 0 where n_s(c) = 0
    cosine  x_s = clamp(d_s r_s(q) r_s(c), -1, 1)        euclid  x_s = -max(n_s(q) + n_s(c) - 2 d_s, 0)
    mean = (1/S) sum_s x_s     std = sqrt(sum_s (x_s - mean)^2 / (S - 1)), 0 for S = 1     score = mean - kappa std

Bounds, with u = 2^-53 and A_s = sum_k |v_s(q)_k v_s(c)_k|.  The project allows a dot product of Kp terms the forward error
(Kp + 2) u A; a norm is such a dot product with A = n, so n^ = n (1 + t), |t| <= (Kp + 2) u.
  cosine, one sample: r^ = r (1 + t / 2 + 2 u) (sqrt and the division, correctly rounded), the product of the two inverse norms one
    more rounding, the product with d another:  |x^ - x| <= (Kp + 2) u A r r' + |x| ((Kp + 2) u + 6 u); the clamp only moves x^ towards
    the true value, which lies in [-1, 1].       b_s = u [(Kp + 3) A_s r_s(q) r_s(c) + (Kp + 9) |x_s|]       (one u each for second order)
  euclid, one sample: the two norms, their sum, twice the dot product (2 d is exact), the subtraction:
                                                 b_s = u [(Kp + 3) (n_s(q) + n_s(c)) + 2 (Kp + 2) A_s + |x_s|] (1 + 2^-20)
  mean:  (1/S) sum_s b_s + (S + 1) u (1/S) sum_s |x_s|              the S - 1 additions and the division
    With A r r' <= 1 and |x| <= 1 this is at most (2 Kp + 13 + S) u for cosine -- inside the cap (2 Kp + 16 + S) u.  For euclid,
    2 A <= n + n' and |x| <= 2 (n + n') give (2 Kp + 9 + 2 S) u max_s (n_s(q) + n_s(c)), inside the same cap for S <= 7.
  std:   newrows_ref.var_bound's argument -- the first-order perturbation of a two-pass variance by errors |e_s| <= e = max_s b_s, the
    factor 4 for a one-pass scheme's constant -- carried to second order, because a pair of parallel columns has x_s = 1 in every
    sample, so that the first-order term vanishes while the device's x_s still differ in their last bits:
        vb = 4 (4 e dev1 + (S + 3) u dev2 + S e^2) / (S - 1) + 4 u var,      dev1 = sum_s |x_s - mean|, dev2 = sum_s (x_s - mean)^2
        |std^ - std| <= min(vb / std, sqrt(vb)) + 3 u std
  score: mean bound + kappa std bound + 3 u (|mean| + kappa std)
"""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
KINDS = ("cosine", "euclid")


def per_sample(Vs, kind, q_from=0, q_to=None):
    """dict(x, A, nsum) [S, nq, nc] in longdouble: the per-sample similarity; A_s of the module docstring (for cosine already times
    r_s(q) r_s(c)); n_s(q) + n_s(c)"""
    Vs = np.asarray(Vs, LD)
    S, nc, _ = Vs.shape
    q_to = nc if q_to is None else q_to
    Q = Vs[:, q_from:q_to]
    d = np.einsum("sqk,sck->sqc", Q, Vs)
    A = np.einsum("sqk,sck->sqc", np.abs(Q), np.abs(Vs))
    n = (Vs * Vs).sum(2)                                                   # [S, nc]
    nq_, nc_ = n[:, q_from:q_to, None], n[:, None, :]
    if kind == "cosine":
        with np.errstate(divide="ignore"):
            r = np.where(n > 0, 1 / np.sqrt(np.where(n > 0, n, 1)), LD(0))
        rr = r[:, q_from:q_to, None] * r[:, None, :]
        x = np.clip(d * rr, -1, 1)
        return dict(x=x, A=A * rr, nsum=nq_ + nc_)
    if kind == "euclid":
        x = -np.maximum(nq_ + nc_ - 2 * d, 0)
        return dict(x=x, A=A, nsum=nq_ + nc_)
    raise ValueError(kind)


def reference(Vs, Kp, kind, kappa=0.0, q_from=0, q_to=None):
    """dict(score, bound, mean, mean_bound, std, std_bound, cap) [nq, nc] in longdouble, by the module docstring; cap: what the
    mean's bound may not exceed"""
    ps = per_sample(Vs, kind, q_from, q_to)
    x, A, nsum = ps["x"], ps["A"], ps["nsum"]
    S = x.shape[0]
    if kind == "cosine":
        b = U53 * ((Kp + 3) * A + (Kp + 9) * np.abs(x))
        cap = np.full(x.shape[1:], (2 * Kp + 16 + S) * U53, LD)
    else:
        b = U53 * ((Kp + 3) * nsum + 2 * (Kp + 2) * A + np.abs(x)) * (1 + 2.0 ** -20)
        cap = (2 * Kp + 16 + S) * U53 * nsum.max(0)
    mean = x.sum(0) / LD(S)
    mean_bound = b.sum(0) / LD(S) + (S + 1) * U53 * np.abs(x).sum(0) / LD(S)
    dev = x - mean
    if S > 1:
        var = (dev * dev).sum(0) / LD(S - 1)
        e = b.max(0)
        vb = 4 * (4 * e * np.abs(dev).sum(0) + (S + 3) * U53 * (dev * dev).sum(0) + S * e * e) / LD(S - 1) + 4 * U53 * var
    else:
        var = np.zeros_like(mean); vb = np.zeros_like(mean)
    std = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        std_bound = np.where(std > 0, np.minimum(vb / np.where(std > 0, std, 1), np.sqrt(vb)), np.sqrt(vb)) + 3 * U53 * std
    score = mean - LD(kappa) * std
    bound = mean_bound + kappa * std_bound + 3 * U53 * (np.abs(mean) + kappa * std)
    return dict(score=score, bound=np.asarray(bound, LD), mean=mean, mean_bound=mean_bound, std=std, std_bound=std_bound, cap=cap)


def plain(Vs, kind):
    """(mean, std) [nc, nc] in plain fp64 numpy: the definitions restated with the library's roundings where they are stated (the
    product of the inverse norms first, the sum of the norms first), a two-pass variance"""
    Vs = np.asarray(Vs, np.float64)
    S = Vs.shape[0]
    xs = []
    for V in Vs:
        d = V @ V.T
        n = (V * V).sum(1)
        if kind == "cosine":
            with np.errstate(divide="ignore"):
                r = np.where(n > 0, 1.0 / np.sqrt(np.where(n > 0, n, 1.0)), 0.0)
            xs.append(np.clip(d * (r[:, None] * r[None, :]), -1.0, 1.0))
        else:
            xs.append(-np.maximum((n[:, None] + n[None, :]) - 2.0 * d, 0.0))
    x = np.stack(xs)
    acc = np.zeros_like(xs[0])
    for xi in xs:                                                          # s ascending from +0.0, as the device adds them
        acc = acc + xi
    mean = acc / float(S)
    std = np.sqrt(((x - mean) ** 2).sum(0) / float(S - 1)) if S > 1 else np.zeros_like(mean)
    return mean, std


def eligible(nc, q, cand_ok=None):
    ok = np.ones(nc, bool) if cand_ok is None else np.asarray(cand_ok) != 0
    ok = ok.copy()
    ok[q] = False                                                          # a query is never its own neighbour
    return ok


def ranked(score, n, cand_ok=None, q_from=0):
    """idx [nq, n]: the n best eligible columns of every row of score [nq, nc] by (score descending, id ascending); padding -1"""
    nq, nc = score.shape
    idx = np.full((nq, n), -1, np.int32)
    for i in range(nq):
        cand = np.nonzero(eligible(nc, q_from + i, cand_ok))[0]
        order = cand[np.lexsort((cand, -score[i, cand]))][:n]
        idx[i, :len(order)] = order
    return idx


def check_lists(idx, score, mean, std, ref, n, cand_ok=None, q_from=0, tag=None, moments=True):
    """The checks of a device list against reference() that no near tie can flake: (i) every listed score, mean and std within its
    bound; (ii) every list sorted by (device score descending, id ascending), free of the query itself, of masked columns and of
    duplicates, and as long as the eligible candidates allow, padding slots -1 and zeros; (iii) every eligible candidate not listed
    has a reference score <= the list's last device score + its own bound.  ref covers queries q_from .. q_from + len(idx) - 1 as
    rows 0 ...  moments=False: mean and std are not looked at (a list of another route).  Returns max over the picks of score
    error / bound."""
    want, bound = ref["score"], ref["bound"]
    nc = want.shape[1]
    worst = 0.0
    for i in range(idx.shape[0]):
        ok = eligible(nc, q_from + i, cand_ok)
        k = min(n, int(ok.sum()))
        ids = idx[i, :k]
        assert (ids >= 0).all() and (idx[i, k:] == -1).all(), (tag, i)
        assert (score[i, k:] == 0).all() and (not moments or ((mean[i, k:] == 0).all() and (std[i, k:] == 0).all())), (tag, i)
        assert ok[ids].all() and len(set(ids.tolist())) == k, (tag, i)
        err = np.abs(LD(1) * score[i, :k] - want[i, ids])
        assert (err <= bound[i, ids]).all(), (tag, i, np.asarray(err, float), np.asarray(bound[i, ids], float))
        if moments:
            assert (np.abs(LD(1) * mean[i, :k] - ref["mean"][i, ids]) <= ref["mean_bound"][i, ids]).all(), (tag, i)
            assert (np.abs(LD(1) * std[i, :k] - ref["std"][i, ids]) <= ref["std_bound"][i, ids]).all(), (tag, i)
        nz = bound[i, ids] > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[i, ids][nz]).max()))
        for r in range(k - 1):
            assert score[i, r] > score[i, r + 1] or (score[i, r] == score[i, r + 1] and ids[r] < ids[r + 1]), (tag, i, r)
        if k == n and k < ok.sum():
            ok[ids] = False
            rest = np.nonzero(ok)[0]
            assert (want[i, rest] <= LD(1) * score[i, n - 1] + bound[i, rest]).all(), (tag, i)
    return worst


def normalised(Vs):
    """every column of every sample divided by its norm in fp64 (a zero column stays zero): the ring of the normalised-copy route"""
    Vs = np.asarray(Vs, np.float64)
    n = np.sqrt((Vs * Vs).sum(2, keepdims=True))
    return np.where(n > 0, Vs / np.where(n > 0, n, 1.0), 0.0)


def rotate_samples(Vs, seed):
    """an independent random orthogonal matrix applied to every sample, in longdouble: Q from the QR factorisation of a Gaussian
    matrix, made orthogonal to longdouble precision by three Newton steps Q <- Q (3 I - Q^T Q) / 2.  Returns longdouble."""
    Vs = np.asarray(Vs, LD)
    K = Vs.shape[2]
    rng = np.random.default_rng(seed)
    out = np.empty_like(Vs)
    for s in range(Vs.shape[0]):
        Q = np.asarray(np.linalg.qr(rng.standard_normal((K, K)))[0], LD)
        for _ in range(3):
            Q = Q @ (3 * np.eye(K, dtype=LD) - Q.T @ Q) / 2
        out[s] = Vs[s] @ Q
    return out


def cosine_of_mean(Vs):
    """what a user of U-mu.ddm / V-mu.ddm computes: the cosine between the posterior-mean factors, [nc, nc] longdouble"""
    m = np.asarray(Vs, LD).mean(0)
    n = np.sqrt((m * m).sum(1))
    r = np.where(n > 0, 1 / np.where(n > 0, n, 1), LD(0))
    return (m @ m.T) * r[:, None] * r[None, :]


BIG = {"cosine": 300, "euclid": 200}


def inputs(nc, K, S, seed, big=300):
    """Vs [S, nc, K] fp64: standard normal factors; column 1 all zero in every sample, column 5 zero in sample 0 only, column 3
    scaled by 1.37 * 2^big and column 4 by 0.73 * 2^-big where they exist.  BIG[kind] is the exponent the tests use: squared norms
    of 2^+-600 for cosine (supported: 2^+-900) and 2^+-400 for euclid (supported: 2^+-500 -- its variance squares a squared norm)"""
    rng = np.random.default_rng(seed)
    Vs = rng.standard_normal((S, nc, K))
    if nc > 1:
        Vs[:, 1] = 0.0
    if nc > 3:
        Vs[:, 3] *= 1.37 * 2.0 ** big
    if nc > 4:
        Vs[:, 4] *= 0.73 * 2.0 ** -big
    if nc > 5:
        Vs[0, 5] = 0.0
    return Vs


# shapes of the GPU tests: (columns, K, S); 300 and 600 columns at K = 10 only (two and three candidate splits)
SHAPES = [(1, 3, 1), (2, 10, 2), (63, 32, 5), (65, 64, 2), (130, 128, 5), (130, 3, 2), (65, 10, 5), (63, 128, 1), (300, 10, 2), (600, 10, 5)]


# ---- the planted experiment ------------------------------------------------------------------------------------------------------------

# Chosen on the CPU with the oracle's chain (oracle.gibbs, alpha = 2, K = 8): the raw rating columns give a same-group share of 0.179
# among 10 neighbours (chance: 9 / 299 = 0.030); the cosine of the chain's 40th sample alone gives 0.762, its 60th 0.823, its 20th 0.401.
PLANTED = dict(nusers=1500, nitems=300, groups=30, K=8, per_item=60, spread=0.2, noise=0.3, seed=11)
PLANTED_CHAIN = dict(nsims=40, burnin=30)


def planted_data(nusers, nitems, groups, K, per_item, spread, noise, seed):
    """Items in `groups` groups of equal size share a factor centre: v_i = centre[g(i)] + spread N(0, I); users u ~ N(0, I); every
    item is rated by per_item random users, r = u . v + noise N(0, 1).  Two items of a group are seldom rated by the same users
    (per_item / nusers of them), which is why the cosine of two raw rating columns says little.  Returns (M, Mt, T, Tt, group):
    the CSC arrays of tests/util (one column per item; T holds one held-out rating per item) and the group of every item."""
    import scipy.sparse as sp
    from tests import util
    rng = np.random.default_rng(seed)
    group = np.arange(nitems) % groups
    centre = rng.standard_normal((groups, K))
    V = centre[group] + spread * rng.standard_normal((nitems, K))
    U = rng.standard_normal((nusers, K))
    rows, cols = [], []
    for i in range(nitems):
        us = rng.choice(nusers, size=per_item + 1, replace=False)
        rows.extend(int(u) for u in us); cols.extend([i] * (per_item + 1))
    rows, cols = np.asarray(rows), np.asarray(cols)
    vals = (U[rows] * V[cols]).sum(1) + noise * rng.standard_normal(len(rows))
    test = np.zeros(len(rows), bool)
    test[::per_item + 1] = True                                            # the first rating of every item is held out
    M = sp.coo_matrix((vals[~test], (rows[~test], cols[~test])), shape=(nusers, nitems)).tocsc()
    T = sp.coo_matrix((vals[test], (rows[test], cols[test])), shape=(nusers, nitems)).tocsc()
    return util.csc_arrays(M), util.csc_arrays(M.T.tocsc()), util.csc_arrays(T), util.csc_arrays(T.T.tocsc()), group


def same_group_share(idx, group):
    """the mean share of listed neighbours (idx >= 0) that belong to the query's group"""
    idx = np.asarray(idx)
    hit = (group[np.where(idx >= 0, idx, 0)] == group[:len(idx), None]) & (idx >= 0)
    return float(hit.sum() / max(int((idx >= 0).sum()), 1))


def raw_column_neighbours(M, nusers, n):
    """the n nearest items of every item by the cosine between the raw rating columns (unobserved cells as zeros), the order of `ranked`"""
    import scipy.sparse as sp
    A = sp.csc_matrix((M[2], M[1], M[0]), shape=(nusers, len(M[0]) - 1)).toarray()
    nrm = np.sqrt((A * A).sum(0))
    C = (A.T @ A) / np.where(nrm > 0, nrm, 1.0)[:, None] / np.where(nrm > 0, nrm, 1.0)[None, :]
    return ranked(C, n)
