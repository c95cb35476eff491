"""Edge inputs, the exact ranking and a longdouble reference of plain top-N for the three ranking entry points (bpmf_hip_topn,
bpmf_hip_topn_scored, bpmf_hip_similar; DESIGN.md sections 10, 18 and 27).  Each of them fuses a score product with its own copy of
one selection: four threads per query own the list slots j, j + 4, ..., survivors of a 64-candidate step are placed by rank, a
64-bit exclusion mask per step is built by four threads that walk every fourth entry of the query's sorted rating list, and when
the candidates are split over workgroups a per-query merge joins the per-split lists.  This module holds what the tests of those
copies share (tests/test_ranking_host.py on the CPU, tests/test_gpu_ranking_edges.py on the device):

  splits            the split geometry of a call, restated from topn_splits (capi_topn.hip)
  scored_lds, similar_lds   the dynamic LDS of k_topn_scored / k_similar_topn for lists of n, restated from their headers
  edge_patterns, edge_rated   deterministic rated sets at the list, tile, split and mask edges
  exact fields      factors that are multiples of 1/8, so that every fp64 sum of a score is exact in any order and a list must EQUAL
                    the numpy ranking: all equal, strictly increasing, strictly decreasing, twins across every boundary, random
  exact_lists       that ranking: (score descending, id ascending), padding (-1, 0)
  topn_reference    bpmf_hip_topn's mean and std in longdouble with DERIVED bounds for a device working in fp64

The bounds of topn_reference.  u = 2^-53; L = S Kp the stacked inner dimension; for a pair (q, c)
    A_s = sum_k |u_s(q)_k v_s(c)_k|,   A = sum_s A_s,   p_s = mean_rating + u_s(q) . v_s(c),   mean = mean_rating + (1/S) sum_s (p_s - mean_rating)
Mean.  The device forms acc, the dot product of L terms, in some order, fused or not: |acc - sum| <= g_L A, g_n = n u / (1 - n u)
(Higham, Accuracy and Stability, section 3.1: every term meets at most L roundings, whatever the order).  Then x = fl(acc / S) and
fl(mean_rating + x), one rounding each:
    |x - sum / S| <= (1 + u) g_L A / S + u |sum| / S <= [(1 + u) g_L + u] A / S                      (|sum| <= A)
    |device - mean| <= (1 + u) |x - sum / S| + u |mean| <= (L + 2) u A / S + u |mean|                (L u < 2^-20: the second-order terms are inside)
The tests use mean_bound = (L + 2) u A / S + 2 u |mean|, the form the other references of this project state theirs in; it is not
smaller than what was just derived.
Std (k_topn_std).  One sample's dot product is at most ceil(Kp / 64) fmas per lane and six butterfly additions, so a term meets at
most ceil(Kp / 64) + 6 roundings; T = max(Kp + 2, ceil(Kp / 64) + 6) covers that order and every other order of Kp terms (the host
test holds two plain numpy orders to the same bound).  With m^ the device's mean, |m^ - mean| <= mean_bound:
    p^_s = fl(mean_rating + dot^):  |p^_s - p_s| <= (1 + u) g_T A_s + u |p_s|                         =: ep_s
    d^_s = fl(p^_s - m^):           |d^_s - dev_s| <= (1 + u) (ep_s + mean_bound) + u |dev_s|          =: e_s,    dev_s = p_s - mean
    ss^ = the fma chain over s:     |ss^ - sum d^_s^2| <= g_S sum d^_s^2,   sum d^_s^2 <= (sqrt(D2) + sqrt(E2))^2,   D2 = sum dev_s^2, E2 = sum e_s^2
    |sum d^_s^2 - D2| = |sum (dev_s + e'_s)^2 - sum dev_s^2| <= 2 sqrt(D2) sqrt(E2) + E2               (Cauchy-Schwarz, |e'_s| <= e_s)
    |ss^ - D2| <= 2 sqrt(D2 E2) + E2 + g_S (sqrt(D2) + sqrt(E2))^2                                     =: B_ss
    v^ = fl(ss^ / (S - 1)):         |v^ - var| <= (1 + u) B_ss / (S - 1) + u var                       =: B_var
    std^ = fl(sqrt(v^)):            |std^ - std| <= (1 + u) min(B_var / std, sqrt(B_var)) + u std      (|sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|))
This is the form topn_score_ref.reference uses for ucb.  Where the samples nearly agree (std ~ 1e-9 mean) E2 is of the size of D2 or
above, and the bound says so: it is then sqrt(B_var), about sqrt(S) times the error of one p_s.
The reference's own rounding (longdouble, unit roundoff eps / 2) obeys the same two derivations with that unit and is added to both
bounds; with the 64-bit significand of x86 that is a 2^-11-th of them.  Nothing here is measured on a device.
"""
import numpy as np
import scipy.sparse as sp

from tests import topn_score_ref as tr
from tests import util

LD = np.longdouble
U53 = 2.0 ** -53
ULD = float(np.finfo(LD).eps) / 2.0

MAX_N = 32
LIST_LENGTHS = (1, 2, 3, 4, 5, 13, 14, 31, 32)          # 13 | 14: the 64 KB boundary of the lists' LDS
SPLIT_LENGTHS = (3, 14, 31, 32)                         # the lengths run on the shapes that split
SPLIT_NC = {257: (2, 192), 600: (3, 256), 769: (4, 256)}   # nc -> (nsplit, cspan) for at most three query blocks on >= 6 CUs


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------

def splits(num_cu, nq, nc):
    """(nsplit, cspan) of a call with nq queries and nc candidates on a device of num_cu compute units: topn_splits restated"""
    nqb = (nq + 63) // 64
    nsplit = max(1, min((2 * num_cu + nqb - 1) // nqb, (nc + 255) // 256))
    cspan = ((nc + nsplit - 1) // nsplit + 63) // 64 * 64
    return (nc + cspan - 1) // cspan, cspan


PRED_TILE, PRED_PITCH = 64, 18                          # kPredTile, kPredPitch = kPredStep + 2 (kernels_predtile.h)
STAGE = 4 * PRED_TILE * PRED_PITCH                      # doubles of the staging buffers: 2 operands x 2 buffers


def scored_lds(n):
    """topn_scored_lds (kernels_topn_score.h): staging | 3 double lists | 64 exclusion words | the id list | the rank tile"""
    return 8 * (STAGE + 3 * 64 * n + 64) + 4 * 64 * n + 64 * 64


def similar_lds(n):
    """similar_lds (kernels_similar.h): as scored_lds without the exclusion words"""
    return 8 * (STAGE + 3 * 64 * n) + 4 * 64 * n + 64 * 64


# ---- exclusion patterns -----------------------------------------------------------------------------------------------------------------

RUN_STARTS = (60, 61, 62, 63)
RUN_LENGTHS = tuple(range(1, 10))


def spread(nc, k):
    """k distinct candidates spread over 0 .. nc - 1, the first and the last among them for k >= 2"""
    k = min(k, nc)
    if k <= 0:
        return []
    if k == 1:
        return [nc // 2]
    return [(i * (nc - 1)) // (k - 1) for i in range(k)]


def edge_patterns(nc, n, cspan):
    """[(name, sorted list of rated candidates)]: the rated sets edge_rated cycles through, every id clipped to 0 .. nc - 1.
    all-but-one leaves candidate 64 (nc // 2 where there is none); edge_rated moves it per query."""
    every = set(range(nc))
    clip = lambda ids: sorted(set(int(c) for c in ids if 0 <= c < nc))
    bounds = [b for b in range(cspan, nc, cspan)]                        # first candidate of every split but the first
    out = [("none", []),
           ("all", sorted(every)),
           ("all-but-one", sorted(every - {64 if nc > 64 else nc // 2})),
           ("all-but-n-1", sorted(every - set(spread(nc, n - 1)))),
           ("tile-63-64", clip([63, 64])),
           ("tile-127-128", clip([127, 128])),
           ("split-boundary", clip([cspan - 1, cspan])),
           ("split-ends", clip([0, nc - 1] + bounds + [b - 1 for b in bounds])),
           ("ends", clip([0, nc - 1])),
           ("step-64-127", clip(range(64, 128)))]
    out += [("residue-%d" % r, clip(range(r, nc, 4))) for r in range(4)]
    out += [("run-%d-len-%d" % (s, ln), clip(range(s, s + ln))) for ln in RUN_LENGTHS for s in RUN_STARTS]
    return out


def edge_rated(nq, nc, n, cspan, names=False):
    """a deterministic rated set per query: query q takes pattern q mod (number of patterns) of edge_patterns; the candidate that
    all-but-one leaves moves with q.  names=True: also the pattern's name per query."""
    pats = edge_patterns(nc, n, cspan)
    rated, used = [], []
    for q in range(nq):
        name, ids = pats[q % len(pats)]
        if name == "all-but-one":
            ids = sorted(set(range(nc)) - {(7 * q + 64) % nc})
        rated.append(set(ids)); used.append(name)
    return (rated, used) if names else rated


def eligible_of(rated, nc, q_from=0, q_to=None):
    """[q_to - q_from, nc] bool: candidate c may be listed for query q"""
    q_to = len(rated) if q_to is None else q_to
    ok = np.ones((q_to - q_from, nc), bool)
    for i in range(q_to - q_from):
        ok[i, sorted(rated[q_from + i])] = False
    return ok


def sides_csc(rated, nq, nc):
    """(query side, candidate side) as CSC triples of the pattern in which query q has rated rated[q]: the query side has one column
    per query and nc rows"""
    rows = [c for q in range(nq) for c in sorted(rated[q])]
    cols = [q for q in range(nq) for _ in rated[q]]
    A = sp.coo_matrix((np.full(len(rows), 3.0), (rows, cols)), shape=(nc, nq)).tocsc()
    return util.csc_arrays(A), util.csc_arrays(A.T.tocsc())


# ---- exact score fields -----------------------------------------------------------------------------------------------------------------

FIELDS = ("equal", "increasing", "decreasing", "twins", "random")
SIM_FIELDS = ("equal", "line", "twins", "random")


def twin_pairs(nc, cspan):
    """the pairs (b - 1, b) made twins: across every 64-candidate tile boundary, every split boundary, and the last two candidates"""
    bs = set(range(64, nc, 64)) | set(range(cspan, nc, cspan)) | ({nc - 1} if nc > 1 else set())
    return [(b - 1, b) for b in sorted(bs)]


def exact_factors(field, nq, nc, K, S, cspan, seed):
    """(Us [S, nq, K], Vs [S, nc, K]): multiples of 1/8 such that score(q, c) = mean_rating + (1/S) sum_s u_s(q) . v_s(c) is
      equal        the same for every c (all candidate columns are one vector)
      increasing   strictly increasing in c for every q (u_0 > 0, v_0 = c / 8, the other rows of v common to all c)
      decreasing   strictly decreasing in c
      twins        random with positive queries; the columns of twin_pairs hold one vector of large entries per pair, so both twins
                   are near the top of every list, equal, and must appear lower id first -- across steps and across the merge
      random       k / 8, |k| <= 4, every tenth candidate a copy of its left neighbour
    Every product is a multiple of 1/64 below 2^11 and a sum of S K <= 384 of them is exact in fp64 in any order."""
    rng = np.random.default_rng(seed)
    dy = lambda shape, lo=-4, hi=4: rng.integers(lo, hi + 1, size=shape) / 8.0
    Us, Vs = dy((S, nq, K)), dy((S, nc, K))
    if field == "equal":
        Vs[:] = dy((S, 1, K))
    elif field in ("increasing", "decreasing"):
        ramp = np.arange(nc) if field == "increasing" else np.arange(nc)[::-1]
        Us[:, :, 0] = dy((S, nq), 1, 4)
        Vs[:] = dy((S, 1, K))
        Vs[:, :, 0] = ramp / 8.0
    elif field == "twins":
        Us = dy((S, nq, K), 1, 4)
        for a, b in twin_pairs(nc, cspan):
            Vs[:, a] = dy((S, K), 3, 4)
            Vs[:, b] = Vs[:, a]
    elif field == "random":
        Vs[:, 1::10] = Vs[:, 0::10][:, :Vs[:, 1::10].shape[1]]
    else:
        raise ValueError(field)
    return Us, Vs


def exact_columns(field, nc, K, S, cspan, seed):
    """Vs [S, nc, K] for the one-sided ranking (similar): multiples of 1/8 whose squared distances are exact in fp64
      equal    all columns one vector: every distance 0, every cosine equal -- the list is the n lowest eligible ids
      line     v(c) = (a_s c / 8, w): the distance (a_s (q - c))^2 / 64 falls away from the query on both sides, q - d and q + d tie
               (lower id first); for the first queries the score strictly decreases in c, for the last it strictly increases
      twins    random with the pairs of twin_pairs equal
      random   k / 8, |k| <= 4: at most 64 K + 1 different distances, so ties are everywhere"""
    rng = np.random.default_rng(seed)
    dy = lambda shape, lo=-4, hi=4: rng.integers(lo, hi + 1, size=shape) / 8.0
    Vs = dy((S, nc, K))
    if field == "equal":
        Vs[:] = dy((S, 1, K), 1, 4)
    elif field == "line":
        Vs[:] = dy((S, 1, K), 1, 4)
        Vs[:, :, 0] = (np.arange(S)[:, None] % 2 + 1) * np.arange(nc)[None, :] / 8.0
    elif field == "twins":
        for a, b in twin_pairs(nc, cspan):
            Vs[:, b] = Vs[:, a]
    elif field != "random":
        raise ValueError(field)
    return Vs


def exact_lists(score, n, eligible=None):
    """(idx int32 [nq, n], value [nq, n]): the n best columns of every row of score by (score descending, id ascending) among
    eligible[i] (bool [nq, nc]; None: all); padding: id -1, value 0.  This is topn_score_ref.ranked (and similar_ref.ranked, whose
    eligible set is a mask without the query itself), called with the complement as the rated sets."""
    nq, nc = score.shape
    rated = None if eligible is None else [set(np.nonzero(~np.asarray(eligible[i], bool))[0].tolist()) for i in range(nq)]
    return tr.ranked(np.asarray(score, np.float64), n, rated)


# ---- plain top-N in longdouble ------------------------------------------------------------------------------------------------------------

def kp_of(K):
    return (K + 3) // 4 * 4


def dot_terms(Kp):
    """T of the module docstring"""
    return max(Kp + 2, (Kp + 63) // 64 + 6)


def _gamma(n, u):
    return n * u / (1.0 - n * u)


def _bounds(q, Kp, u):
    """(mean bound, std bound) of the module docstring for arithmetic of unit roundoff u; q: the longdouble quantities"""
    S, L = q["S"], q["S"] * Kp
    mean_b = (L + 2) * u * q["A"] / LD(S) + 2 * u * np.abs(q["mean"])
    if S == 1:
        return mean_b, np.zeros_like(mean_b)
    ep = (1 + u) * _gamma(dot_terms(Kp), u) * q["As"] + u * np.abs(q["P"])
    e = (1 + u) * (ep + mean_b) + u * np.abs(q["dev"])
    D2, E2 = q["D2"], (e * e).sum(0)
    b_ss = 2 * np.sqrt(D2 * E2) + E2 + _gamma(S, u) * (np.sqrt(D2) + np.sqrt(E2)) ** 2
    b_var = (1 + u) * b_ss / LD(S - 1) + u * q["var"]
    std = q["std"]
    with np.errstate(divide="ignore", invalid="ignore"):
        near = np.where(std > 0, np.minimum(b_var / np.where(std > 0, std, 1), np.sqrt(b_var)), np.sqrt(b_var))
    return mean_b, (1 + u) * near + u * std


def topn_reference(Us, Vs, mean_rating, Kp):
    """dict(score = mean, bound = mean_bound, mean, mean_bound, std, std_bound) [nq, nc] in longdouble for Us [S, nq, K],
    Vs [S, nc, K]: bpmf_hip_topn's two outputs for every pair and the derived bounds of the module docstring (the device's at
    u = 2^-53 plus the reference's own)"""
    Us, Vs = np.asarray(Us, LD), np.asarray(Vs, LD)
    S = Us.shape[0]
    D = np.einsum("sqk,sck->sqc", Us, Vs)
    As = np.einsum("sqk,sck->sqc", np.abs(Us), np.abs(Vs))
    mean = LD(mean_rating) + D.sum(0) / LD(S)
    P = LD(mean_rating) + D
    dev = P - mean
    D2 = (dev * dev).sum(0)
    var = D2 / LD(S - 1) if S > 1 else np.zeros_like(mean)
    q = dict(S=S, A=As.sum(0), As=As, P=P, mean=mean, dev=dev, D2=D2, var=var, std=np.sqrt(var))
    mb, sb = _bounds(q, Kp, U53)
    mb_ref, sb_ref = _bounds(q, Kp, ULD)
    mb, sb = np.asarray(mb + mb_ref, LD), np.asarray(sb + sb_ref, LD)
    return dict(score=mean, bound=mb, mean=mean, mean_bound=mb, std=q["std"], std_bound=sb)


def plain_topn(Us, Vs, mean_rating, order):
    """(mean, std) [nq, nc] of every pair in plain fp64 numpy (the zero pad rows of the ring would add exact zeros):
      order = "sequential"   one running sum over the L = S Kp stacked terms, s ascending, k ascending, then / S + mean_rating
      order = "per-sample"   the S dot products (numpy's own summation), added in s order
    std as k_topn_std: d_s = (mean_rating + dot_s) - mean, ss += d_s^2 in s order, sqrt(ss / (S - 1)); dot_s by the same order"""
    Us, Vs = np.asarray(Us, np.float64), np.asarray(Vs, np.float64)
    S, nq, K = Us.shape
    nc = Vs.shape[1]
    if order == "sequential":
        dots, acc = np.zeros((S, nq, nc)), np.zeros((nq, nc))
        for s in range(S):
            for k in range(K):
                term = Us[s, :, k, None] * Vs[s, None, :, k]
                dots[s] += term
                acc += term
    elif order == "per-sample":
        dots = np.stack([Us[s] @ Vs[s].T for s in range(S)])
        acc = np.zeros((nq, nc))
        for s in range(S):
            acc = acc + dots[s]
    else:
        raise ValueError(order)
    mean = mean_rating + acc / float(S)
    if S == 1:
        return mean, np.zeros_like(mean)
    ss = np.zeros_like(mean)
    for s in range(S):
        d = (mean_rating + dots[s]) - mean
        ss = ss + d * d
    return mean, np.sqrt(ss / float(S - 1))


# the rounded inputs of section 3: (name, K, S); the shapes and list lengths are the GPU test's
ROUNDED_K = (3, 10, 64, 128)
ROUNDED_S = (1, 2, 37)
ROUNDED_SHAPES = ((17, 65), (65, 257))
ROUNDED_N = (5, 32)


def rounded_inputs(kind, nq, nc, K, S, seed):
    """(Us [S, nq, K], Vs [S, nc, K], mean_rating) of section 3:
      gauss      standard normal factors, mean_rating 0.25
      cancel     S = 5 samples that are ONE Gaussian draw times (1 + 1e-9 N(0, 1)) entry by entry, mean_rating 3.5: the true std is about
                 1e-9 of the mean, the subtraction (mean_rating + d_s) - m cancels nine digits, and a relative tolerance on std would
                 be the wrong bar
      scales     Gaussian with candidate column c scaled by 10^(-3 + 6 c / (nc - 1)): A / S and |mean| differ by orders of magnitude"""
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((S, nq, K)), rng.standard_normal((S, nc, K)), 0.25
    if kind == "cancel":
        U0, V0 = rng.standard_normal((nq, K)), rng.standard_normal((nc, K))
        return (U0[None] * (1.0 + 1e-9 * rng.standard_normal((S, nq, K))), V0[None] * (1.0 + 1e-9 * rng.standard_normal((S, nc, K))), 3.5)
    if kind == "scales":
        scale = 10.0 ** (-3.0 + 6.0 * np.arange(nc) / max(nc - 1, 1))
        return rng.standard_normal((S, nq, K)), rng.standard_normal((S, nc, K)) * scale[None, :, None], 0.25
    raise ValueError(kind)


def pad_k(X, Kp):
    """X [..., K] with zero rows appended up to Kp"""
    out = np.zeros(X.shape[:-1] + (Kp,), X.dtype)
    out[..., :X.shape[-1]] = X
    return out


def worst_ratio(err, bound):
    """max err / bound over the entries with a positive bound (0 if there is none)"""
    nz = np.asarray(bound > 0)
    return float((np.asarray(err)[nz] / np.asarray(bound)[nz]).max()) if nz.any() else 0.0
