"""tests/ranking_ref.py on the CPU: the split geometry the GPU cases are chosen for, the 64 KB boundary of the lists' LDS at 13 | 14,
the occurrence of every exclusion pattern, exact lists one can write down by hand, the structure of the exact fields, and the
derived bounds of plain top-N held against two honest fp64 orders before the device is asked (tests/test_gpu_ranking_edges.py)."""
import numpy as np
import pytest

from tests import ranking_ref as rr
from tests import similar_ref as sr
from tests import topn_score_ref as tr

LD = rr.LD


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_cu", [6, 64, 256, 304])
def test_split_geometry(num_cu):
    for nc, want in rr.SPLIT_NC.items():
        for nq in (1, 63, 65, 130, 192):                                   # at most three query blocks
            assert rr.splits(num_cu, nq, nc) == want, (num_cu, nq, nc)
    nsplit, cspan = rr.splits(num_cu, 65, 257)
    assert 257 - (nsplit - 1) * cspan == 65                                # the last split of the first size that splits holds 65
    nsplit, cspan = rr.splits(num_cu, 65, 769)
    assert 769 - (nsplit - 1) * cspan == 1                                 # ... ONE candidate: fewer than any n > 1
    for nc in (1, 63, 64, 65, 130, 256):
        assert rr.splits(num_cu, 65, nc) == (1, (nc + 63) // 64 * 64), nc
    # many query blocks on a small device leave the candidates whole
    assert rr.splits(6, 64 * 13, 769)[0] == 1


def test_lds_boundary_is_13_14():
    # kernels_topn_score.h: 41 472 + 1 792 n; kernels_similar.h: 40 960 + 1 792 n
    for n in range(1, rr.MAX_N + 1):
        assert rr.scored_lds(n) == 41472 + 1792 * n and rr.similar_lds(n) == 40960 + 1792 * n
    assert rr.scored_lds(10) == 59392 and rr.scored_lds(32) == 98816 and rr.similar_lds(10) == 58880 and rr.similar_lds(32) == 98304
    for lds in (rr.scored_lds, rr.similar_lds):
        assert lds(13) <= 65536 < lds(14)
    assert 13 in rr.LIST_LENGTHS and 14 in rr.LIST_LENGTHS and 14 in rr.SPLIT_LENGTHS
    assert max(rr.LIST_LENGTHS) == rr.MAX_N and rr.MAX_N - 1 in rr.LIST_LENGTHS
    assert {n % 4 for n in rr.LIST_LENGTHS} == {0, 1, 2, 3}


# ---- exclusion patterns -----------------------------------------------------------------------------------------------------------------

CASES = [(63, 65), (65, 130), (130, 130), (63, 257), (65, 600), (65, 769)]


@pytest.mark.parametrize("nq,nc", CASES)
@pytest.mark.parametrize("n", [1, 3, 14, 32])
def test_every_pattern_occurs(nq, nc, n):
    nsplit, cspan = rr.splits(256, nq, nc)
    rated, names = rr.edge_rated(nq, nc, n, cspan, names=True)
    assert len(rated) == nq and len(rr.edge_patterns(nc, n, cspan)) <= 63
    every = set(range(nc))
    by = {}
    for q, (r, name) in enumerate(zip(rated, names)):
        assert r <= every
        by.setdefault(name, []).append((q, r))
    first = lambda name: by[name][0][1]
    assert first("none") == set() and first("all") == every
    for q, r in by["all-but-one"]:
        assert len(r) == nc - 1
    assert len({tuple(sorted(every - r)) for q, r in by["all-but-one"]}) == len(by["all-but-one"])      # the free candidate moves
    left = every - first("all-but-n-1")
    assert len(left) == min(n - 1, nc) and (n < 3 or {0, nc - 1} <= left)  # exactly one padding slot (n = 1: nothing is left)
    assert first("tile-63-64") == {63, 64}
    assert first("tile-127-128") == ({127, 128} if nc > 128 else {127} & every)
    assert first("split-boundary") == ({cspan - 1, cspan} if nsplit > 1 else {cspan - 1} & every)
    ends = {0, nc - 1}
    for s in range(1, nsplit):
        ends |= {s * cspan - 1, s * cspan}
    assert first("split-ends") == ends and first("ends") == {0, nc - 1}
    assert first("step-64-127") == set(range(64, min(128, nc)))
    for r in range(4):
        assert first("residue-%d" % r) == set(range(r, nc, 4))
    # runs of every length mod 4 that start on either side of the tile boundary and cross it
    lens = set()
    for s in rr.RUN_STARTS:
        for ln in rr.RUN_LENGTHS:
            run = first("run-%d-len-%d" % (s, ln))
            assert run == set(range(s, min(s + ln, nc)))
            if min(run) <= 63 and max(run) >= 64:
                lens.add((s, len(run) % 4))
    assert nc < 73 or lens == {(s, m) for s in rr.RUN_STARTS for m in range(4)}      # (65 candidates cut the runs at 64)
    # the two sides are one pattern
    Q, Cs = rr.sides_csc(rated, nq, nc)
    assert len(Q[0]) == nq + 1 and len(Cs[0]) == nc + 1 and Q[0][-1] == Cs[0][-1] == sum(len(r) for r in rated)
    for q in (0, 1, nq - 1):
        assert set(Q[1][Q[0][q]:Q[0][q + 1]].tolist()) == rated[q]
    ok = rr.eligible_of(rated, nc, 1, nq - 1)
    assert ok.shape == (nq - 2, nc) and not ok[0].any() and ok[1].sum() == 1        # query 1 rated everything, query 2 all but one


# ---- exact lists ------------------------------------------------------------------------------------------------------------------------

def test_exact_lists_by_hand():
    nq, nc, n = 3, 70, 5
    ids = np.arange(nc)
    ok = np.ones((nq, nc), bool)
    ok[1, :3] = False                                                      # query 1 may not list 0, 1, 2
    ok[2] = False; ok[2, [7, 66]] = True                                   # query 2 has two eligible candidates
    equal = np.full((nq, nc), 0.5)
    idx, val = rr.exact_lists(equal, n, ok)
    assert idx.tolist() == [[0, 1, 2, 3, 4], [3, 4, 5, 6, 7], [7, 66, -1, -1, -1]]
    assert val.tolist() == [[0.5] * 5, [0.5] * 5, [0.5, 0.5, 0, 0, 0]]
    inc = np.tile(ids / 8.0, (nq, 1))
    idx, val = rr.exact_lists(inc, n, ok)
    assert idx.tolist() == [[69, 68, 67, 66, 65], [69, 68, 67, 66, 65], [66, 7, -1, -1, -1]]
    assert val[0].tolist() == [69 / 8, 68 / 8, 67 / 8, 66 / 8, 65 / 8]
    dec = -inc
    idx, val = rr.exact_lists(dec, n, ok)
    assert idx.tolist() == [[0, 1, 2, 3, 4], [3, 4, 5, 6, 7], [7, 66, -1, -1, -1]]
    idx, _ = rr.exact_lists(dec, n)
    assert idx.tolist() == [[0, 1, 2, 3, 4]] * 3
    # twins across the tile boundary: equal scores, lower id first, wherever they stand
    tw = dec.copy(); tw[:, 63] = tw[:, 64] = 1.0
    assert rr.exact_lists(tw, 3)[0].tolist() == [[63, 64, 0]] * 3


@pytest.mark.parametrize("field", rr.FIELDS)
def test_exact_lists_are_the_ranked_of_the_references(field):
    nq, nc, n, K, S = 9, 140, 7, 8, 3
    Us, Vs = rr.exact_factors(field, nq, nc, K, S, 64, seed=5)
    score = tr.exact_scores(Us, Vs, 0.5, "ucb", 0.0)
    rated = rr.edge_rated(nq, nc, n, 64)
    wi, ws = tr.ranked(score, n, rated)
    idx, val = rr.exact_lists(score, n, rr.eligible_of(rated, nc))
    assert np.array_equal(idx, wi) and val.tobytes() == ws.tobytes()
    # the one-sided form: a mask without the query itself
    sq = score @ score.T                                                   # any square matrix will do
    mask = np.ones(nq, bool); mask[::3] = False
    ok = np.tile(mask, (nq, 1)); ok[np.arange(nq), np.arange(nq)] = False
    assert np.array_equal(rr.exact_lists(sq, 4, ok)[0], sr.ranked(sq, 4, mask))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("K", [8, 10, 128])
def test_exact_fields(K, S):
    nq, nc, cspan = 5, 300, 192
    ids = np.arange(nc)
    for field in rr.FIELDS:
        Us, Vs = rr.exact_factors(field, nq, nc, K, S, cspan, seed=K + S)
        assert np.array_equal(Us * 8, np.round(Us * 8)) and np.array_equal(Vs * 8, np.round(Vs * 8))
        P = np.einsum("sqk,sck->sqc", Us, Vs)
        assert np.array_equal(P * 64, np.round(P * 64))                    # exact: multiples of 1/64
        exact = np.einsum("sqk,sck->qc", np.asarray(Us, LD), np.asarray(Vs, LD))
        assert np.array_equal(np.asarray(P.sum(0), LD), exact)
        score = 0.5 + P.sum(0) / S
        d = np.diff(score, axis=1)
        if field == "equal":
            assert (d == 0).all() and rr.exact_lists(score, 4)[0].tolist() == [[0, 1, 2, 3]] * nq
        if field == "increasing":
            assert (d > 0).all() and rr.exact_lists(score, 3)[0].tolist() == [[nc - 1, nc - 2, nc - 3]] * nq
        if field == "decreasing":
            assert (d < 0).all() and rr.exact_lists(score, 3)[0].tolist() == [[0, 1, 2]] * nq
        if field == "twins":
            pairs = rr.twin_pairs(nc, cspan)
            assert pairs == [(63, 64), (127, 128), (191, 192), (255, 256), (298, 299)]
            top, _ = rr.exact_lists(score, 2 * len(pairs))
            for q in range(nq):
                assert set(top[q].tolist()) == {c for p in pairs for c in p}          # the twins lead every list ...
                for r in range(0, 2 * len(pairs), 2):
                    a, b = int(top[q, r]), int(top[q, r + 1])
                    same = [p for p in pairs if score[q, p[0]] == score[q, a]]         # (two pairs may tie with each other)
                    assert score[q, a] == score[q, b] and a < b and ((a, b) in pairs or len(same) > 1), (q, r)
    for field in rr.SIM_FIELDS:
        Vs = rr.exact_columns(field, nc, K, S, cspan, seed=K + S)
        mean, _ = sr.plain(Vs, "euclid")
        exact = -(((np.asarray(Vs, LD)[:, :, None, :] - np.asarray(Vs, LD)[:, None, :, :]) ** 2).sum(3)).sum(0) / LD(S)
        assert np.array_equal(np.asarray(mean, LD), np.asarray(np.asarray(exact, np.float64), LD))   # one rounding: the division
        if field == "equal":
            assert (mean == 0).all()
            assert sr.ranked(mean, 3).tolist()[:3] == [[1, 2, 3], [0, 2, 3], [0, 1, 3]]
        if field == "line":
            assert (np.diff(mean[0]) < 0).all() and (np.diff(mean[nc - 1]) > 0).all()
            assert sr.ranked(mean, 4)[100].tolist() == [99, 101, 98, 102]
        if field == "twins":
            for a, b in rr.twin_pairs(nc, cspan):
                assert mean[a, b] == 0 and np.array_equal(np.delete(mean[:, a], [a, b]), np.delete(mean[:, b], [a, b]))
        if field == "random":
            assert len(np.unique(mean)) <= 64 * K * S + 1


# ---- the derived bounds admit plain fp64 ------------------------------------------------------------------------------------------------

def rounded_cases():
    for K in rr.ROUNDED_K:
        for S in rr.ROUNDED_S:
            yield "gauss", 17, 65, K, S
    yield "gauss", 65, 257, 10, 37
    yield "cancel", 17, 65, 10, 5
    yield "cancel", 17, 65, 128, 5
    yield "scales", 17, 65, 10, 2
    yield "scales", 65, 257, 64, 2


@pytest.mark.parametrize("kind,nq,nc,K,S", list(rounded_cases()))
def test_plain_fp64_is_inside_the_derived_bounds(kind, nq, nc, K, S):
    Us, Vs, mr = rr.rounded_inputs(kind, nq, nc, K, S, seed=100 * K + S)
    ref = rr.topn_reference(Us, Vs, mr, rr.kp_of(K))
    assert np.isfinite(np.asarray(ref["mean_bound"], float)).all() and np.isfinite(np.asarray(ref["std_bound"], float)).all()
    if S == 1:
        assert (ref["std"] == 0).all() and (ref["std_bound"] == 0).all()
    if kind == "cancel":
        rel = np.asarray(ref["std"] / np.abs(ref["mean"]), float)
        assert np.median(rel) < 1e-7                                       # the spread is a tiny share of the mean ...
        assert float((ref["std_bound"] / ref["std"]).min()) > 1e-7         # ... and the derived bound is NOT a relative 1e-12
    if kind == "scales":
        ratio = np.asarray(ref["mean_bound"].max(0), float)
        assert ratio[-1] / ratio[0] > 1e4                                  # the bound follows the column scales
    for order in ("sequential", "per-sample"):
        mean, std = rr.plain_topn(Us, Vs, mr, order)
        em, es = np.abs(LD(1) * mean - ref["mean"]), np.abs(LD(1) * std - ref["std"])
        print("%s %d x %d K = %d S = %d %s: max err / bound  mean %.3g  std %.3g" % (
            kind, nq, nc, K, S, order, rr.worst_ratio(em, ref["mean_bound"]), rr.worst_ratio(es, ref["std_bound"])))
        assert (em <= ref["mean_bound"]).all(), (order, float((em / ref["mean_bound"]).max()))
        assert (es <= ref["std_bound"]).all(), (order, float(rr.worst_ratio(es, ref["std_bound"])))
