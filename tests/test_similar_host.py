"""The reference of the similar-columns ranking (tests/similar_ref.py) checked on the CPU:

  1. the plain fp64 numpy restatement stays inside the module's bounds on the inputs of the GPU tests, and the bounds are not
     vacuous: the mean's never exceeds (2 Kp + 16 + S) 2^-53 (cosine) or that factor times max_s (n_s(q) + n_s(c)) (euclid)
  2. an independent random orthogonal matrix applied to every sample leaves the reference mean and std unchanged to those bounds,
     while the cosine between the posterior-mean factors -- what U-mu.ddm / V-mu.ddm invite -- moves by orders of magnitude more
  3. the checks of a list accept the reference's own ranking and refuse a list with the query, a masked column, a wrong order
"""
import numpy as np
import pytest

from tests import similar_ref as sr

LD = sr.LD


def kp_of(K):
    return (K + 3) // 4 * 4


@pytest.mark.parametrize("kind", sr.KINDS)
def test_plain_fp64_is_inside_the_bounds(kind):
    worst_mean = worst_std = tightest = 0.0
    for nc, K, S in sr.SHAPES:
        if nc > 130:
            continue                                                           # (the same code at more columns)
        Vs = sr.inputs(nc, K, S, seed=1000 * K + 10 * nc + S, big=sr.BIG[kind])
        ref = sr.reference(Vs, kp_of(K), kind)
        assert (ref["mean_bound"] <= ref["cap"]).all(), (kind, nc, K, S)       # not vacuous
        mean, std = sr.plain(Vs, kind)
        em, es = np.abs(LD(1) * mean - ref["mean"]), np.abs(LD(1) * std - ref["std"])
        assert (em <= ref["mean_bound"]).all(), (kind, nc, K, S, float((em - ref["mean_bound"]).max()))
        assert (es <= ref["std_bound"]).all(), (kind, nc, K, S, float((es - ref["std_bound"]).max()))
        nz = ref["mean_bound"] > 0
        if nz.any():
            worst_mean = max(worst_mean, float((em[nz] / ref["mean_bound"][nz]).max()))
            tightest = max(tightest, float((ref["mean_bound"][nz] / ref["cap"][nz]).max()))
        nz = ref["std_bound"] > 0
        if nz.any():
            worst_std = max(worst_std, float((es[nz] / ref["std_bound"][nz]).max()))
        if nc > 1:                                                             # the all-zero column: cosine 0 with everything, itself included
            assert kind != "cosine" or ((ref["mean"][1] == 0).all() and (mean[1] == 0).all() and (ref["mean_bound"][1] == 0).all())
    print("%s: fp64 numpy max err / bound: mean %.3g std %.3g; largest mean bound / cap %.3g" % (kind, worst_mean, worst_std, tightest))


@pytest.mark.parametrize("kind", sr.KINDS)
def test_rotations_leave_the_reference_unchanged(kind):
    for nc, K, S in ((63, 32, 5), (65, 10, 5), (130, 3, 2)):
        Vs = sr.inputs(nc, K, S, seed=7 * K + S, big=sr.BIG[kind])
        a = sr.reference(Vs, kp_of(K), kind)
        b = sr.reference(sr.rotate_samples(Vs, seed=K), kp_of(K), kind)
        assert (np.abs(a["mean"] - b["mean"]) <= a["mean_bound"]).all(), (kind, nc, K, S)
        assert (np.abs(a["std"] - b["std"]) <= a["std_bound"]).all(), (kind, nc, K, S)


def test_the_cosine_of_the_mean_factors_is_not_invariant():
    nc, K, S = 65, 10, 5
    Vs = sr.inputs(nc, K, S, seed=3)[:, 6:]                                    # (without the zero and the scaled columns)
    a = sr.reference(Vs, kp_of(K), "cosine")
    rot = sr.rotate_samples(Vs, seed=4)
    b = sr.reference(rot, kp_of(K), "cosine")
    moved_posterior = float(np.abs(a["mean"] - b["mean"]).max())
    off = ~np.eye(nc - 6, dtype=bool)
    moved_of_mean = np.abs(sr.cosine_of_mean(Vs) - sr.cosine_of_mean(rot))[off]
    bound = float(a["mean_bound"].max())
    assert moved_posterior <= bound
    assert float(np.median(moved_of_mean)) > 1e6 * bound                       # ~0.1 against ~1e-15: the first section of the issue as an assertion
    print("rotation moves the posterior cosine by %.3g (bound %.3g), the cosine of the mean factors by %.3g (median)"
          % (moved_posterior, bound, float(np.median(moved_of_mean))))


def test_check_lists_accepts_the_reference_and_refuses_bad_lists():
    nc, K, S, n = 65, 10, 5, 10
    Vs = sr.inputs(nc, K, S, seed=5)
    ok = np.ones(nc, bool); ok[::7] = False
    for kind in sr.KINDS:
        for kappa in (0.0, 1.0):
            ref = sr.reference(Vs, kp_of(K), kind, kappa)
            score = np.asarray(ref["score"], np.float64)
            idx = sr.ranked(score, n, ok)
            rows = np.arange(nc)[:, None]
            pick = lambda a: np.asarray(a, np.float64)[rows, idx]
            sc, mu, sd = pick(ref["score"]), pick(ref["mean"]), pick(ref["std"])
            sr.check_lists(idx, sc, mu, sd, ref, n, ok)
            assert (idx != rows).all() and ok[idx].all()
            bad = idx.copy(); bad[3, 0] = 3                                    # the query itself
            with pytest.raises(AssertionError):
                sr.check_lists(bad, sc, mu, sd, ref, n, ok)
            bad = idx.copy(); bad[3, 0] = 0 if 3 != 0 else 7                   # a masked column (0 is masked)
            with pytest.raises(AssertionError):
                sr.check_lists(bad, sc, mu, sd, ref, n, ok)
            with pytest.raises(AssertionError):                                # reversed: not sorted
                sr.check_lists(idx[:, ::-1].copy(), sc[:, ::-1].copy(), mu[:, ::-1].copy(), sd[:, ::-1].copy(), ref, n, ok)
            with pytest.raises(AssertionError):                                # the best candidate left out
                sr.check_lists(sr.ranked(score, n + 1, ok)[:, 1:], pick2(ref["score"], rows, score, n, ok), mu, sd, ref, n, ok)


def pick2(a, rows, score, n, ok):
    idx = sr.ranked(score, n + 1, ok)[:, 1:]
    return np.asarray(a, np.float64)[rows, idx]


def test_planted_design_separates_groups_from_raw_columns():
    """the design only (no chain here): the raw-column baseline of the planted experiment is far from perfect and far above chance"""
    P = sr.PLANTED
    M, Mt, T, Tt, group = sr.planted_data(**P)
    raw = sr.same_group_share(sr.raw_column_neighbours(M, P["nusers"], 10), group)
    print("planted: same-group share of the raw rating columns %.3f" % raw)
    assert abs(raw - 0.179) < 0.01                                             # the figure the design was chosen at
