"""The three ranking selections (bpmf_hip_topn, bpmf_hip_topn_scored, bpmf_hip_similar) at list, tile, split and mask edges, with the
inputs and references of tests/ranking_ref.py (tests/test_ranking_host.py checks those on the CPU).

  1. the selection, exactly: on score fields whose fp64 sums are exact (all equal, strictly increasing, strictly decreasing, twins
     across every tile and split boundary, random with ties) the lists of all three entry points must EQUAL the numpy ranking -- for
     list lengths 1 .. 32 that are no multiples of 4, next to the maximum and on either side of the 64 KB LDS boundary 13 | 14, for
     candidate counts around the 64-wide step and with two, three and four splits (the last split of 769 holds ONE candidate), with
     the deterministic exclusion patterns of ranking_ref.edge_rated (for `similar`: their complements as cand_ok), on the whole query
     range and on a slice.  topn_scored runs prob and ei with sigma = 0 and ucb with kappa = 0, which must be topn's lists bit for
     bit; mean and std of its picks are predict_block's bits.  similar runs euclid (exact) and cosine with kappa = 0, whose list must
     equal the numpy ranking of the device's own similar_block -- the score of a pick is asserted to be the bits of its mean first
  2. against k_rank_eval without a tolerance: a held-out candidate on either side of every step and split boundary has rank <= 32
     exactly when it is entry rank - 1 of topn(..., 32), on Gaussian factors at K = 10, S = 3 (L = 36 is no multiple of 16)
  3. query slices and repeated calls give the same bytes at 769 candidates (four splits) and n = 32, for all three entry points
  4. plain topn on rounded inputs within the DERIVED bounds of ranking_ref.topn_reference: mean and std, Gaussian factors, samples
     that nearly agree (the subtraction of k_topn_std cancels nine digits) and column scales over six orders of magnitude
  5. a NaN in a candidate column makes that candidate ineligible and nothing else; a NaN in a query column empties that query's list

Every case asserts and prints the split geometry it was chosen for.
"""
import subprocess
import sys

import numpy as np
import pytest

from tests import ranking_ref as rr
from tests import similar_ref as sr
from tests import topn_score_ref as tr

pytestmark = pytest.mark.gpu

LD = rr.LD
MR = 0.5


@pytest.fixture(scope="module")
def num_cu():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process once per module: torch brings a HIP
    runtime of its own, and in a process where the library's runtime was there first torch finds no GPU"""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.split()[-1])


def geometry(num_cu, nq, nc, what):
    """the split geometry of the call, asserted to be the one the case was chosen for"""
    nsplit, cspan = rr.splits(num_cu, nq, nc)
    assert (nsplit, cspan) == rr.SPLIT_NC.get(nc, (1, (nc + 63) // 64 * 64)), (what, num_cu, nq, nc, nsplit, cspan)
    print("%s: %d queries x %d candidates on %d CUs: %d split(s) of %d, the last holds %d" % (
        what, nq, nc, num_cu, nsplit, cspan, nc - (nsplit - 1) * cspan))
    return nsplit, cspan


def lengths(nq, nc):
    if (nq, nc) == (65, 130):
        return rr.LIST_LENGTHS
    return rr.SPLIT_LENGTHS if nc in rr.SPLIT_NC else (2, 5, 32)


def ranges(nq):
    return [(0, nq)] + ([(1, nq - 1)] if nq >= 3 else [])


class Pair:
    """a query side and a candidate side over one rating pattern, destroyed on exit"""

    def __init__(self, eng, rated, nq, nc):
        Q, Cs = rr.sides_csc(rated, nq, nc)
        self.eng, self.nq, self.nc = eng, nq, nc
        self.sq = eng.side_create(nq, nc, *Q, 0.0)
        self.sc = eng.side_create(nc, nq, *Cs, 0.0)

    def fill(self, Us, Vs):
        """the samples through set_items + samples_add (an fp32 context widens them on the device); returns what the device holds"""
        eng, S = self.eng, len(Us)
        eng.samples_reserve(self.sq, S + 1); eng.samples_reserve(self.sc, S)        # (rings of different capacity: the strides differ)
        Ub, Vb = [], []
        for U, V in zip(Us, Vs):
            eng.set_items(self.sq, U); eng.set_items(self.sc, V)
            Ub.append(eng.get_items(self.sq)); Vb.append(eng.get_items(self.sc))
            eng.samples_add(self.sq); eng.samples_add(self.sc)
        return np.stack(Ub), np.stack(Vb)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.side_destroy(self.sq); self.eng.side_destroy(self.sc)


def empty_side(eng, nc):
    return eng.side_create(nc, 1, np.zeros(nc + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), 0.0)


def load_ring(eng, side, Vs, spare=2, through_items=False):
    """Vs [S, nc, K] into slots 0 .. S - 1 of a ring reserved for S + spare samples; through_items: by set_items + samples_add, the
    way of a chain (an fp32 context then widens the factors on the device), instead of samples_set"""
    eng.samples_reserve(side, Vs.shape[0] + spare)
    if not through_items:
        eng.samples_set(side, np.ascontiguousarray(np.transpose(Vs, (1, 0, 2))))
        return
    for V in Vs:
        eng.set_items(side, V)
        assert np.array_equal(eng.get_items(side), V)                      # (multiples of 1/8 below 2^7: exact in fp32 too)
        eng.samples_add(side)


# ---- 1. the selection, exactly ----------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (63, 63), (130, 64), (1, 65), (65, 130), (63, 257), (65, 600), (65, 769)]
GRID = [(nq, nc, K, S, "f64") for nq, nc in SHAPES for K, S in ((8, 1), (10, 3))] + [(65, 130, 128, 3, "f64"), (65, 130, 128, 3, "f32")]
GRID_IDS = ["q%d-c%d-k%d-s%d-%s" % g for g in GRID]


def exact_case(eng, num_cu, nq, nc, K, S, what, check):
    """check(pair, n, rated, field, Ud, Vd, dots, tag) for every list length and field of the case"""
    nsplit, cspan = geometry(num_cu, nq, nc, what)
    for q0, q1 in ranges(nq)[1:]:
        assert rr.splits(num_cu, q1 - q0, nc) == (nsplit, cspan)
    for n in lengths(nq, nc):
        rated = rr.edge_rated(nq, nc, n, cspan)
        with Pair(eng, rated, nq, nc) as pair:
            for f, field in enumerate(rr.FIELDS):
                Us, Vs = rr.exact_factors(field, nq, nc, K, S, cspan, seed=1000 * nc + 10 * n + f)
                Ud, Vd = pair.fill(Us, Vs)
                assert np.array_equal(Ud, Us) and np.array_equal(Vd, Vs)       # multiples of 1/8 below 2^7: exact in fp32 too
                dots = np.einsum("sqk,sck->sqc", Ud, Vd)
                check(pair, n, rated, field, Ud, Vd, dots, (what, nq, nc, K, S, n, field))


@pytest.mark.parametrize("nq,nc,K,S,dtype", GRID, ids=GRID_IDS)
def test_topn_selection_exact(hip_engine_factory, num_cu, nq, nc, K, S, dtype):
    """idx and mean EQUAL the numpy ranking; std is 0 for S = 1 and within the derived bound of ranking_ref.topn_reference otherwise"""
    eng = hip_engine_factory(K, dtype)

    def check(pair, n, rated, field, Ud, Vd, dots, tag):
        score = MR + dots.sum(0) / S                                        # exact sum, one division, one addition: the device's roundings
        ref = rr.topn_reference(Ud, Vd, MR, rr.kp_of(K)) if S > 1 else None
        for excl in (True, False):
            wi, wm = rr.exact_lists(score, n, rr.eligible_of(rated, nc) if excl else None)
            for q0, q1 in ranges(nq):
                idx, mean, std = eng.topn(pair.sq, pair.sc, MR, n, q0, q1, exclude_rated=excl)
                assert np.array_equal(idx, wi[q0:q1]), tag + (excl, q0, q1, np.nonzero((idx != wi[q0:q1]).any(1))[0][:5])
                assert np.array_equal(mean, wm[q0:q1]), tag + (excl, q0, q1)
                if S == 1:
                    assert (std == 0).all(), tag + (excl, q0, q1)
                else:
                    listed = idx >= 0
                    rows = np.arange(q0, q1)[:, None]
                    safe = np.where(listed, idx, 0)
                    err = np.abs(LD(1) * std - ref["std"][rows, safe])
                    assert (err[listed] <= ref["std_bound"][rows, safe][listed]).all() and (std[~listed] == 0).all(), tag + (excl, q0, q1)

    exact_case(eng, num_cu, nq, nc, K, S, "topn", check)


@pytest.mark.parametrize("nq,nc,K,S,dtype", GRID, ids=GRID_IDS)
def test_topn_scored_selection_exact(hip_engine_factory, num_cu, nq, nc, K, S, dtype):
    """prob and ei with sigma = 0 EQUAL the numpy ranking of topn_score_ref.exact_scores (ei with sigma = 0 at n >= 14 is the
    instantiation that had never run with the enlarged LDS); ucb with kappa = 0 is topn's lists bit for bit; mean and std of every
    pick are the bits of predict_block"""
    eng = hip_engine_factory(K, dtype)

    def check(pair, n, rated, field, Ud, Vd, dots, tag):
        t = float(np.median(MR + dots))                                     # a value of the field (or the middle of two): p_s == t occurs
        bm, bs = eng.predict_block(pair.sq, pair.sc, MR)
        for kind in ("prob", "ei", "ucb"):
            want = tr.exact_scores(Ud, Vd, MR, kind, t) if kind != "ucb" else None
            for excl in (True, False):
                if want is not None:
                    wi, ws = rr.exact_lists(want, n, rr.eligible_of(rated, nc) if excl else None)
                for q0, q1 in ranges(nq):
                    param = 0.0 if kind == "ucb" else t
                    idx, score, mean, std = eng.topn_scored(pair.sq, pair.sc, MR, n, kind, param, 0.0, q0, q1, exclude_rated=excl)
                    at = tag + (kind, excl, q0, q1)
                    if kind == "ucb":
                        ti, tm, _ = eng.topn(pair.sq, pair.sc, MR, n, q0, q1, exclude_rated=excl)
                        assert np.array_equal(idx, ti) and mean.tobytes() == tm.tobytes() and score.tobytes() == tm.tobytes(), at
                    else:
                        assert np.array_equal(idx, wi[q0:q1]), at + (np.nonzero((idx != wi[q0:q1]).any(1))[0][:5],)
                        assert np.array_equal(score, ws[q0:q1]), at
                    listed = idx >= 0
                    rows = np.arange(q0, q1)[:, None]
                    safe = np.where(listed, idx, 0)
                    assert np.array_equal(mean[listed], bm[rows, safe][listed]) and np.array_equal(std[listed], bs[rows, safe][listed]), at
                    assert (score[~listed] == 0).all() and (mean[~listed] == 0).all() and (std[~listed] == 0).all(), at

    exact_case(eng, num_cu, nq, nc, K, S, "topn_scored", check)


SIM_SHAPES = [1, 63, 64, 65, 130, 257, 600, 769]
SIM_GRID = [(nc, K, S, "f64") for nc in SIM_SHAPES for K, S in ((8, 1), (10, 3))] + [(130, 128, 3, "f64"), (130, 128, 3, "f32")]


def similar_calls(nc, n, cspan, turn):
    """[(name, cand_ok or None, q0, q1)] of one (field, kind, n): no mask on the whole range, on all but the ends and on four queries
    across the first tile boundary; then the complements of the exclusion patterns as masks: all-but-n-1 and six more, a different
    six every turn, so that a test meets every pattern several times.  Up to 130 columns a masked call asks for every query; with
    more columns for 66 queries around the start, the first tile boundary, the first split boundary or the end, in turn."""
    pats = rr.edge_patterns(nc, n, cspan)[1:]                              # ("none" is the call without a mask)
    out = [("no mask", None, 0, nc)]
    if nc >= 3:
        out.append(("no mask", None, 1, nc - 1))
    if nc >= 66:
        out.append(("no mask", None, 62, 66))
    picked = [p for p in pats if p[0] == "all-but-n-1"] + [pats[(6 * turn + i) % len(pats)] for i in range(6)]
    windows = [(0, 66), (31, 97), (cspan - 33, cspan + 33), (nc - 66, nc)]
    for i, (name, ids) in enumerate(picked):
        ok = np.ones(nc, bool)
        ok[ids] = False
        q0, q1 = (0, nc) if nc <= 130 else windows[(turn + i) % 4]
        out.append((name, ok, q0, q1))
    return out


@pytest.mark.parametrize("nc,K,S,dtype", SIM_GRID, ids=["c%d-k%d-s%d-%s" % g for g in SIM_GRID])
def test_similar_selection_exact(hip_engine_factory, num_cu, nc, K, S, dtype):
    """euclid on the exact fields: similar_block is the plain numpy restatement bit for bit, so the lists EQUAL its numpy ranking.
    cosine with kappa = 0: the score of every pick is the bits of its mean (asserted first), so the list must equal the numpy
    ranking of the device's own similar_block.  The query is every column, so the self-exclusion meets the diagonal at 63 | 64 and
    at every split boundary."""
    eng = hip_engine_factory(K, dtype)
    nsplit, cspan = geometry(num_cu, nc, nc, "similar")
    side = empty_side(eng, nc)
    try:
        turn = 0
        for f, field in enumerate(rr.SIM_FIELDS):
            Vs = rr.exact_columns(field, nc, K, S, cspan, seed=1000 * nc + f)
            load_ring(eng, side, Vs, through_items=(dtype == "f32" or f % 2 == 1))
            want_mean, _ = sr.plain(Vs, "euclid")
            for kind in sr.KINDS:
                bm, bs = eng.similar_block(side, kind)
                if kind == "euclid":
                    assert bm.tobytes() == want_mean.tobytes(), (nc, K, S, field)
                for n in lengths(65 if nc == 130 else 0, nc):
                    turn += 1
                    for name, ok, q0, q1 in similar_calls(nc, n, cspan, turn):
                        tag = (nc, K, S, field, kind, n, name, q0, q1)
                        idx, score, mean, std = eng.similar(side, n, kind, 0.0, q0, q1, cand_ok=ok)
                        listed = idx >= 0
                        assert score.tobytes() == mean.tobytes(), tag          # kappa = 0: the score is the mean, bit for bit
                        wi = sr.ranked(bm[q0:q1], n, ok, q0)
                        assert np.array_equal(idx, wi), tag + (np.nonzero((idx != wi).any(1))[0][:5],)
                        rows = np.arange(q0, q1)[:, None]
                        safe = np.where(listed, idx, 0)
                        assert np.array_equal(mean[listed], bm[rows, safe][listed]) and np.array_equal(std[listed], bs[rows, safe][listed]), tag
                        assert (mean[~listed] == 0).all() and (std[~listed] == 0).all(), tag
    finally:
        eng.side_destroy(side)


# ---- 2. against k_rank_eval, without a tolerance ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", sorted(rr.SPLIT_NC))
def test_boundary_ranks_are_the_top_n_lists(hip_engine_factory, num_cu, nc):
    """K = 10, S = 3: the stacked inner dimension 36 is no multiple of 16.  Held out, for every query: the candidates on either side
    of every 64-candidate step and every split boundary, the first and the last (without the query's rated ones when they are
    excluded).  rank <= 32 exactly when the entry is number rank - 1 of the top-32 list: no tolerance."""
    K, S, nq, n = 10, 3, 65, 32
    eng = hip_engine_factory(K)
    nsplit, cspan = geometry(num_cu, nq, nc, "rank_eval / topn")
    held = sorted({0, nc - 1} | {b - 1 for b in range(64, nc, 64)} | set(range(64, nc, 64)) |
                  {b - 1 for b in range(cspan, nc, cspan)} | set(range(cspan, nc, cspan)))
    rated = rr.edge_rated(nq, nc, n, cspan)
    rng = np.random.default_rng(700 + nc)
    with Pair(eng, rated, nq, nc) as pair:
        pair.fill(rng.standard_normal((S, nq, K)), rng.standard_normal((S, nc, K)))
        for excl in (True, False):
            per_q = [[c for c in held if not (excl and c in rated[q])] for q in range(nq)]
            tptr = np.concatenate([[0], np.cumsum([len(p) for p in per_q])]).astype(np.int64)
            tcand = np.array([c for p in per_q for c in p], np.int32)
            rank, ncand = eng.rank_eval(pair.sq, pair.sc, tptr, tcand, 0.25, exclude_rated=excl)
            idx, mean, std = eng.topn(pair.sq, pair.sc, 0.25, n, exclude_rated=excl)
            listed = 0
            for q in range(nq):
                assert ncand[q] == (nc - len(rated[q]) if excl else nc)
                for p in range(tptr[q], tptr[q + 1]):
                    if rank[p] <= n:
                        assert idx[q, rank[p] - 1] == tcand[p], (excl, q, tcand[p], rank[p], idx[q])
                        listed += 1
                    else:
                        assert tcand[p] not in idx[q], (excl, q, tcand[p], rank[p])
            assert listed > 0


# ---- 3. slices and repeated calls: the same bytes ---------------------------------------------------------------------------------------

def test_slices_and_calls_do_not_change_a_bit(hip_engine_factory, num_cu):
    """769 candidates (four splits, the last of one candidate), n = 32, Gaussian factors at K = 10, S = 3 with twin columns: the
    concatenation of two query slices is the whole call, and a second call is the first, byte for byte -- all three entry points"""
    K, S, nq, nc, n = 10, 3, 65, 769, 32
    eng = hip_engine_factory(K)
    nsplit, cspan = geometry(num_cu, nq, nc, "slices")
    assert rr.splits(num_cu, 17, nc) == (nsplit, cspan) and rr.splits(num_cu, nq - 17, nc) == (nsplit, cspan)
    rng = np.random.default_rng(31)
    Vs = rng.standard_normal((S, nc, K))
    for a, b in rr.twin_pairs(nc, cspan):
        Vs[:, b] = Vs[:, a]
    rated = rr.edge_rated(nq, nc, n, cspan)
    calls = []
    with Pair(eng, rated, nq, nc) as pair:
        pair.fill(rng.standard_normal((S, nq, K)), Vs)
        for excl in (True, False):
            calls.append(("topn", excl, nq, lambda q0, q1, excl=excl: eng.topn(pair.sq, pair.sc, 1.25, n, q0, q1, exclude_rated=excl)))
            for kind, param, sigma in (("ucb", 1.0, 0.0), ("prob", 1.5, 1.0), ("ei", 1.5, 0.5), ("ei", 1.5, 0.0)):
                calls.append(("topn_scored " + kind, excl, nq, lambda q0, q1, excl=excl, kind=kind, param=param, sigma=sigma:
                              eng.topn_scored(pair.sq, pair.sc, 1.25, n, kind, param, sigma, q0, q1, exclude_rated=excl)))
        check_slices(calls)
    side = empty_side(eng, nc)
    try:
        geometry(num_cu, nc, nc, "slices, similar")
        assert rr.splits(num_cu, 17, nc) == rr.splits(num_cu, nc - 17, nc) == (nsplit, cspan)
        load_ring(eng, side, Vs)
        ok = np.ones(nc, bool); ok[dict(rr.edge_patterns(nc, n, cspan))["split-ends"]] = False      # without the first and last candidate of every split
        calls = [("similar " + kind, mask is not None, nc, lambda q0, q1, kind=kind, mask=mask: eng.similar(side, n, kind, 1.0, q0, q1, cand_ok=mask))
                 for kind in sr.KINDS for mask in (None, ok)]
        check_slices(calls)
    finally:
        eng.side_destroy(side)


def check_slices(calls):
    for name, flag, nq, call in calls:
        whole, again = call(0, nq), call(0, nq)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again)), (name, flag)
        parts = [call(0, 17), call(17, nq)]
        for f in range(len(whole)):
            assert np.concatenate([p[f] for p in parts]).tobytes() == whole[f].tobytes(), (name, flag, f)
        assert (whole[0] >= 0).any()


# ---- 4. plain topn on rounded inputs, within derived bounds -----------------------------------------------------------------------------

def rounded_cases(K):
    for nq, nc in rr.ROUNDED_SHAPES:
        for S in rr.ROUNDED_S:
            yield "gauss", nq, nc, S
    yield "cancel", 17, 65, 5
    yield "cancel", 65, 257, 5
    yield "scales", 65, 257, 2


@pytest.mark.parametrize("K", rr.ROUNDED_K)
def test_topn_rounded_within_derived_bounds(hip_engine_factory, num_cu, K):
    """The three checks of topn_score_ref.check_lists on the means (nothing is skipped) and every std within its bound.  The bounds
    are derived (tests/ranking_ref.py), not measured.  Measured on one MI355X, max err / bound (informational): mean 0.40, 0.24,
    0.056, 0.027 and std 0.077, 0.037, 0.0065, 0.0014 at K = 3, 10, 64, 128."""
    eng = hip_engine_factory(K)
    Kp = rr.kp_of(K)
    worst = dict(mean=0.0, std=0.0)
    for kind, nq, nc, S in rounded_cases(K):
        nsplit, cspan = geometry(num_cu, nq, nc, "topn rounded %s S = %d" % (kind, S))
        Us, Vs, mr = rr.rounded_inputs(kind, nq, nc, K, S, seed=100 * K + S + nq)
        ref = None
        for n in rr.ROUNDED_N:
            rated = rr.edge_rated(nq, nc, n, cspan)
            with Pair(eng, rated, nq, nc) as pair:
                Ud, Vd = pair.fill(Us, Vs)
                assert np.array_equal(Ud, Us) and np.array_equal(Vd, Vs)
                if ref is None:
                    ref = rr.topn_reference(Ud, Vd, mr, Kp)
                for excl in (True, False):
                    for q0, q1 in ranges(nq):
                        tag = (kind, nq, nc, K, S, n, excl, q0, q1)
                        idx, mean, std = eng.topn(pair.sq, pair.sc, mr, n, q0, q1, exclude_rated=excl)
                        # (i) every listed mean within its bound; (ii) sorted, no excluded or repeated id, full; (iii) nothing better left out
                        worst["mean"] = max(worst["mean"], tr.check_lists(idx, mean, ref, n, rated if excl else None, q0, tag=tag))
                        listed = idx >= 0
                        rows = np.arange(q0, q1)[:, None]
                        safe = np.where(listed, idx, 0)
                        err = np.abs(LD(1) * std - ref["std"][rows, safe])[listed]
                        bound = ref["std_bound"][rows, safe][listed]
                        assert np.isfinite(std).all() and (std[~listed] == 0).all(), tag
                        if S == 1:
                            assert (std == 0).all(), tag
                        ratio = rr.worst_ratio(err, bound)
                        worst["std"] = max(worst["std"], ratio)
                        assert (err <= bound).all(), tag + (ratio,)
        print("K = %d %s %d x %d S = %d: max err / bound so far  mean %.3g  std %.3g" % (K, kind, nq, nc, S, worst["mean"], worst["std"]))
    print("K = %d: max err / bound  mean %.3g  std %.3g" % (K, worst["mean"], worst["std"]))


# ---- 5. non-finite factors stay local ---------------------------------------------------------------------------------------------------

def test_nan_stays_local(hip_engine_factory, num_cu):
    """17 x 65, n = 5, S = 2, no exclusion.  A NaN in one sample of one candidate column: every list is, bit for bit, the list of the
    call in which everyone has rated that candidate and the rated ones are excluded -- a NaN score never survives
    `v != NEG && better(...)` -- and the candidate is never listed.  A NaN in one query column: that query's list is all padding
    (-1 and zeros), every other query keeps its bits.  The same for topn_scored (ucb, kappa = 0)."""
    K, S, nq, nc, n, bad_c, bad_q = 10, 2, 17, 65, 5, 63, 4
    eng = hip_engine_factory(K)
    geometry(num_cu, nq, nc, "nan")
    rng = np.random.default_rng(5)
    Us, Vs = rng.standard_normal((S, nq, K)), rng.standard_normal((S, nc, K))
    Vs[:, bad_c] = 3.0 * np.abs(Us).sum(1).max()                           # the candidate would lead many lists
    Vs[:, bad_c, 1::2] *= -1.0

    def both(pair, excl):
        return (eng.topn(pair.sq, pair.sc, MR, n, exclude_rated=excl),
                eng.topn_scored(pair.sq, pair.sc, MR, n, "ucb", 0.0, exclude_rated=excl))

    with Pair(eng, [{bad_c} for _ in range(nq)], nq, nc) as pair:         # everyone has rated bad_c
        pair.fill(Us, Vs)
        clean = both(pair, False)
        want = both(pair, True)
        assert (clean[0][0] == bad_c).any() and not (want[0][0] == bad_c).any()
        Vn = Vs.copy(); Vn[1, bad_c, 3] = np.nan
        pair.fill(Us, Vn)
        for got, exp, name in zip(both(pair, False), want, ("topn", "topn_scored")):
            assert not (got[0] == bad_c).any(), name
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, exp)), name
        Un = Us.copy(); Un[0, bad_q, 7] = np.nan
        pair.fill(Un, Vs)
        for got, exp, name in zip(both(pair, False), clean, ("topn", "topn_scored")):
            keep = np.arange(nq) != bad_q
            assert (got[0][bad_q] == -1).all() and all((a[bad_q] == 0).all() for a in got[1:]), name
            assert all(a[keep].tobytes() == b[keep].tobytes() for a, b in zip(got, exp)), name
