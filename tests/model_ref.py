"""Helpers of the saved-model tests (tests/test_model_host.py, tests/test_gpu_model.py): the references of
bpmf_hip_predict_cells gathered from the block references the suite already has (tests/newrows_ref.py, tests/topn_score_ref.py --
their bounds are the bounds here, no new constant), the inputs that discriminate a cancelling variance, and small random models.
"""
import numpy as np
import scipy.sparse as sp

from tests import newrows_ref as nr
from tests import topn_score_ref as ts
from tests import util

LD = np.longdouble
f64 = lambda a: np.asarray(a, np.float64)


def kp_of(K):
    return (K + 3) // 4 * 4


def pair_of_sides(eng, nq, nc):
    """a side of nq columns and its partner of nc columns with one rating between them"""
    A = sp.coo_matrix((np.array([3.0]), (np.array([0]), np.array([0]))), shape=(nc, nq)).tocsc()
    return eng.side_create(nq, nc, *util.csc_arrays(A), 0.0), eng.side_create(nc, nq, *util.csc_arrays(A.T.tocsc()), 0.0)


def random_model(K, rows, cols, S, seed, hyper=True, probit=False):
    """the dict bpmf_amd.write_model takes, with random values"""
    rng = np.random.default_rng(seed)

    def hyp():
        A = rng.standard_normal((S, K, K))
        return (1.0 + rng.random(S), rng.standard_normal((S, K)), A @ np.transpose(A, (0, 2, 1)) + K * np.eye(K))
    return dict(num_latent=K, rows=rows, cols=cols, samples=S, mean_rating=0.0 if probit else 3.25, alpha=1.0 if probit else 2.0,
                probit=probit, probit_threshold=0.5 if probit else 0.0, dtype="f64", U=rng.standard_normal((rows, S, K)),
                V=rng.standard_normal((cols, S, K)), U_hyper=hyp() if hyper else None, V_hyper=hyp() if hyper else None)


def golden_model():
    """tests/golden/model_v1: K = 3, 4 x 5, S = 2, every value a small dyadic number stated here"""
    K, rows, cols, S = 3, 4, 5, 2
    U = np.array([[[(r + 1) + s / 2.0 + k / 4.0 for k in range(K)] for s in range(S)] for r in range(rows)])
    V = np.array([[[-(c + 1) / 8.0 + s - k / 2.0 for k in range(K)] for s in range(S)] for c in range(cols)])

    def hyp(shift):
        alpha = np.array([2.0, 2.5]) + shift
        mu = np.array([[0.5 * k + s + shift for k in range(K)] for s in range(S)])
        lam = np.array([[[(2.0 + s if i == j else 0.25 * (i + 2 * j)) + shift for j in range(K)] for i in range(K)] for s in range(S)])
        return alpha, mu, lam
    return dict(num_latent=K, rows=rows, cols=cols, samples=S, mean_rating=3.5, alpha=2.0, probit=False, probit_threshold=0.0, dtype="f64",
                U=U, V=V, U_hyper=hyp(0.0), V_hyper=hyp(0.125))


GOLDEN_TXT = ("bpmf_model 1\nnum_latent 3\nrows 4\ncols 5\nsamples 2\nmean_rating 3.5\nalpha 2\nlikelihood gaussian\nprobit_threshold 0\n"
              "dtype f64\nhyper 1\n")


def cancelling_case(nq, nc, K, S, seed):
    """d_s = D + delta_s with D ~ 900 .. 961 and a spread of ~1e-3, carried by the factors themselves: e_s = (a_q, g_qs),
    v_s = (b_c, h_cs), a, b in [30, 31), g, h ~ 1e-2 N(0, 1) -- under mean_rating = 1e6 every |p_s| is 1e9 times the spread"""
    rng = np.random.default_rng(seed)
    Es = 1e-2 * rng.standard_normal((S, nq, K)); Vs = 1e-2 * rng.standard_normal((S, nc, K))
    Es[:, :, 0] = (30.0 + rng.random(nq)) * (1.0 + 1e-6 * rng.standard_normal((S, nq)))
    Vs[:, :, 0] = 30.0 + rng.random(nc)
    return Es, Vs


def block_reference(Es, Vs, mean_rating, Kp, threshold=None, sigma=0.0):
    """the references of every cell of the nq x nc block, computed once: newrows_ref.predict and its bounds and, with a threshold,
    topn_score_ref.reference's prob and bound at sigma and the counting form (prob0, exact)"""
    good = nr.predict(Es, Vs, mean_rating)
    out = dict(mean=good["mean"], var=good["var"], mean_bound=f64(nr.mean_bound(good, Kp, mean_rating)), var_bound=f64(nr.var_bound(good, Kp)),
               S=good["S"])
    if threshold is not None:
        ref = ts.reference(Es, Vs, mean_rating, Kp, "prob", threshold, sigma)
        out["prob"] = ref["score"]; out["prob_bound"] = f64(ref["bound"])
        out["prob0"] = f64(((LD(mean_rating) + np.einsum("sqk,sck->sqc", np.asarray(Es, LD), np.asarray(Vs, LD)) - LD(threshold)) > 0).sum(0) / LD(good["S"]))
    return out


def cells_reference(block, q, c):
    """a block_reference taken at the cells (q[i], c[i])"""
    return {k: (v if k == "S" else v[q, c]) for k, v in block.items()}


def check_cells(got, ref, tag):
    """the device's (mean, std[, prob]) against cells_reference; returns the worst err / bound of (mean, var, prob)"""
    mean, std = got[0], got[1]
    em = np.abs(mean - f64(ref["mean"])); ev = np.abs(std * std - f64(ref["var"]))
    assert (em <= ref["mean_bound"]).all(), (tag, "mean", float((em / ref["mean_bound"]).max()))
    worst = [float((em / ref["mean_bound"]).max()) if len(em) else 0.0, 0.0, 0.0]
    if ref["S"] == 1:
        assert (std == 0.0).all(), (tag, "std of one sample")
    else:
        assert (ev <= ref["var_bound"]).all(), (tag, "var", float((ev / np.maximum(ref["var_bound"], 1e-300)).max()))
        worst[1] = float((ev / np.maximum(ref["var_bound"], 1e-300)).max()) if len(ev) else 0.0
    if "prob" in ref:
        ep = np.abs(got[2] - f64(ref["prob"]))
        assert (ep <= ref["prob_bound"]).all(), (tag, "prob", float(ep.max()))
        assert ((got[2] >= 0) & (got[2] <= 1)).all(), tag
        nz = ref["prob_bound"] > 0
        worst[2] = float((ep[nz] / ref["prob_bound"][nz]).max()) if nz.any() else 0.0
    return worst


def small_ratings(seed=11):
    """60 users x 40 movies: (M, Mt, T, Tt, nusers, nmovies), the layout of tests/util.py"""
    return util.blocks(nusers=60, nmovies=40, per_user=8, cross=6, seed=seed)


def new_entities(n, nother, per, seed):
    """scipy.sparse [n, nother]: `per` ratings 1 .. 5 per new entity"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per)
    cols = np.concatenate([rng.choice(nother, size=per, replace=False) for _ in range(n)])
    return sp.csr_matrix((rng.integers(1, 6, size=n * per).astype(np.float64), (rows, cols)), shape=(n, nother))
