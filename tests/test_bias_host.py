"""Row and column bias terms on the CPU: the restatement of tests/bias_ref.py against plain loops, the shape of the edge side, the
refusals gibbs gives before it touches an engine, the declared entry points, and the planted experiment's recorded pair."""
import math
import os
import re

import numpy as np
import pytest

from tests import bias_ref as ref
from tests import util
from tests.conftest import ROOT


def test_edge_side_has_every_piece_boundary():
    A, nrows = ref.edge_side()
    counts = np.diff(A[0])
    assert nrows == 800 and tuple(counts[33:]) == (0, 1, 16, 17, 63, 64, 65, 255, 256, 257, 3 * ref.PIECE + 1)
    assert counts[:33].min() == 0 and counts[:33].max() == 40 and len(A[1]) == len(A[2]) == A[0][-1]
    for a in range(len(counts)):                                      # rows ascend inside a column, no cell twice
        r = A[1][A[0][a]:A[0][a + 1]]
        assert np.all(np.diff(r) > 0) and (len(r) == 0 or (0 <= r[0] and r[-1] < nrows))
    pieces = np.where(counts > ref.LIGHT, (counts + ref.PIECE - 1) // ref.PIECE, 0)
    assert pieces.max() == 4 and pieces[counts <= 16].sum() == 0 and int(pieces[-3]) == 1 and int(pieces[-2]) == 2
    assert (counts[:33] <= 16).any() and (counts[:33] > 16).any()


def test_step_restatement_against_plain_loops():
    """bias_ref.step against one loop per column in Python floats (math.fsum for the sum), and its bar"""
    A, nrows = ref.edge_side()
    ncols, K, it, alpha, lam = len(A[0]) - 1, 10, 3, 1.7, 2.5
    X, Y = ref.factors(K, ncols, nrows)
    c = np.random.default_rng(1).standard_normal(nrows)
    mean = util.mean_rating(A)
    r = ref.step(A, X, Y, c, it, ref.TAG_MOVIES, alpha, lam, mean)
    xi = ref.normals(np.arange(ncols), it, ref.TAG_MOVIES)
    bar = ref.bar(r, K, alpha, lam)
    for a in range(ncols):
        terms = []
        for p in range(int(A[0][a]), int(A[0][a + 1])):
            terms += [A[2][p] - mean, -c[A[1][p]]] + [-(X[a, k] * Y[A[1][p], k]) for k in range(K)]
        S, n = math.fsum(terms), A[0][a + 1] - A[0][a]
        prec = lam + alpha * n
        want = alpha * S / prec + float(xi[a]) / math.sqrt(prec)
        assert abs(float(r["b"][a]) - want) <= 1e-13 * (1.0 + abs(want)), (a, float(r["b"][a]), want)
        assert float(r["M"][a]) >= abs(S) - 1e-12 and bar[a] > 0.0
    empty = np.flatnonzero(np.diff(A[0]) == 0)
    assert len(empty) >= 2 and np.all(r["mean_part"][empty] == 0) and np.all(r["M"][empty] == 0)
    # the double evaluation of the chain agrees with the longdouble one far inside the bar's scale
    r64 = ref.step(A, X, Y, c, it, ref.TAG_MOVIES, alpha, lam, mean, np.float64)
    assert np.abs(r64["b"] - r["b"].astype(np.float64)).max() < 1e-12


def test_normals_are_standard_and_keyed():
    n = 200_000
    x = ref.normals(np.arange(n), 7, ref.TAG_MOVIES, np.float64)
    assert abs(x.mean()) < 5.0 / math.sqrt(n) and abs(x.var() - 1.0) < 5.0 * math.sqrt(2.0 / n) and np.abs(x).max() < 7.0
    assert np.all(ref.normals(np.arange(1000), 8, ref.TAG_MOVIES, np.float64) != x[:1000])
    assert np.all(ref.normals(np.arange(1000), 7, ref.TAG_USERS, np.float64) != x[:1000])
    big = ref.normals(np.array([2 ** 32 + 5]), 7, ref.TAG_MOVIES, np.float64)     # the high word of the column is part of the key
    assert big[0] != x[5]


def test_values_order_of_operations():
    A = (np.array([0, 2, 3], np.int64), np.array([0, 1, 1], np.int32), np.array([1.0, 2.0 ** -30, 3.0]))
    b, c = np.array([1.0, 2.0 ** -40]), np.array([2.0 ** -53, -1.0])
    z = ref.values(A, b, c)
    assert z[0] == (1.0 - 1.0) - 2.0 ** -53 and z[1] == (2.0 ** -30 - 1.0) + 1.0 and z[2] == (3.0 - 2.0 ** -40) + 1.0


def test_gibbs_refuses_before_the_engine_is_used():
    import bpmf_amd
    none = (np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0))
    cases = [(dict(pipelined=True), "pipelined=True"), (dict(probit=True), "probit=True"), (dict(ordinal=True), "ordinal"),
             (dict(censored=none), "censored"), (dict(robust=4.0), "robust"), (dict(weights=none), "weights"), (dict(implicit=0.1), "implicit"),
             (dict(row_features=np.zeros((1, 1))), "row_features / col_features"), (dict(col_features=np.zeros((1, 1))), "row_features / col_features"),
             (dict(noise="adaptive"), "noise='adaptive'"), (dict(foldin=True), "foldin=True"), (dict(save_model="x"), "save_model"),
             (dict(similar=3), "similar"), (dict(new_row_features=np.zeros((1, 1))), "new_row_features / new_col_features"),
             (dict(new_col_features=np.zeros((1, 1))), "new_row_features / new_col_features")]

    class Ranks:
        def comm_nranks(self):
            return 2
    with pytest.raises(ValueError, match="bias does not go together with a communicator"):
        bpmf_amd.gibbs(Ranks(), none, none, none, 1, 1, nsims=3, burnin=1, bias=True)
    for kw, what in cases:
        with pytest.raises(ValueError, match="bias does not go together with %s" % re.escape(what)):
            bpmf_amd.gibbs(None, none, none, none, 1, 1, nsims=3, burnin=1, bias=True, **kw)

    class F32:
        dtype = "f32"
    with pytest.raises(ValueError, match="bias does not go together with an fp32 engine"):
        bpmf_amd.gibbs(F32(), none, none, none, 1, 1, nsims=3, burnin=1, bias=True)
    for v in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="a finite lambda > 0"):
            bpmf_amd.gibbs(None, none, none, none, 1, 1, bias=v)
    with pytest.raises(ValueError, match="bias_prior needs bias"):
        bpmf_amd.gibbs(None, none, none, none, 1, 1, bias_prior=(1.0, 1.0))
    for bad in ((0.0, 1.0), (1.0, -1.0), (1.0,), "x", (float("inf"), 1.0), 3):
        with pytest.raises(ValueError, match="bias_prior"):
            bpmf_amd.gibbs(None, none, none, none, 1, 1, bias=2.0, bias_prior=bad)
    with pytest.raises(ValueError, match="bias needs a finite alpha > 0"):
        bpmf_amd.gibbs(None, none, none, none, 1, 1, bias=True, alpha=0.0)


def test_cli_refusals(tmp_path):
    """every refusal of `bpmf --bias` in one line with a non-zero status, before a GPU is touched"""
    from tests.test_similar_cli import refused
    files = ["-n", "train.sdm", "-p", "test.sdm"]
    base = files + ["--bias"]
    for extra, why in ((["--probit"], "--probit"), (["--ordinal"], "--ordinal"), (["--censored", "c.sdm"], "--censored"), (["--robust", 4], "--robust"),
                       (["--weights", "w.sdm"], "--weights"), (["--implicit", 0.1], "--implicit"), (["--noise", "adaptive"], "--noise adaptive"),
                       (["--row-features", "f.ddm"], "--row-features / --col-features"), (["--col-features", "f.ddm"], "--row-features / --col-features"),
                       (["--fold-in-rows", "r.sdm"], "--fold-in-rows / --fold-in-cols"), (["--save-model", "m", "-o", "o"], "--save-model / --model"),
                       (["--similar", 5, "-o", "o"], "--similar"), (["--row-features", "f.ddm", "--new-row-features", "g.ddm", "-o", "o"], "--row-features / --col-features"),
                       (["--col-features", "f.ddm", "--new-col-features", "g.ddm", "-o", "o"], "--row-features / --col-features"), (["--fold-in-cols", "r.sdm"], "--fold-in-rows / --fold-in-cols"),
                       (["-m", "a.ddm,b.ddm"], "a propagated posterior (-m / -l)"), (["-l", "a.ddm,b.ddm"], "a propagated posterior (-m / -l)"),
                       (["--fp32", "-d", 128], "--fp32")):
        refused(base + extra, "--bias does not go together with " + why, tmp_path)
    refused(base + ["-g", 1], "--bias runs on one GPU without -g", tmp_path)
    refused(base + ["--model", "m"], "--model does not go together with --bias", tmp_path)      # (the rule of --model: no chain runs)
    refused(base, "--bias does not go together with BPMF_REDUCE=1", tmp_path, {"BPMF_REDUCE": "1"})
    refused(base + ["-a", 0], "--bias needs a noise precision -a F > 0", tmp_path)
    refused(["--tensor", "x.tns", "--bias"], "--tensor does not go together with --bias", tmp_path)
    refused(base + ["--topn", 5, "-o", "o", "-d", 127], "--bias with --topn / --rank-eval needs -d <= 126", tmp_path)
    refused(base + ["--rank-eval", 5, "-d", 128], "--bias with --topn / --rank-eval needs -d <= 126", tmp_path)
    for v in ("1", "0,1", "1,-1", "nan,1", "1,inf", "a,b", "1,2,3", ""):
        refused(base + ["--bias-prior", v], "--bias-prior expects A0,B0 with a finite A0 > 0 and a finite B0 >= 0", tmp_path)
    for v in (0, -1, "nan", "inf", "much", ""):
        refused(base + ["--bias-lambda", v], "--bias-lambda expects the precision of the bias prior, a finite number > 0", tmp_path)
    refused(files + ["--bias-lambda", 2], "--bias-lambda needs --bias", tmp_path)
    refused(files + ["--bias-prior", "1,1"], "--bias-prior needs --bias", tmp_path)


def test_entry_points_are_declared_and_bound():
    from bpmf_amd import _lib
    names = ["bpmf_hip_side_set_bias", "bpmf_hip_side_bias_prior", "bpmf_hip_side_bias_get", "bpmf_hip_side_bias_set", "bpmf_hip_side_bias_latent", "bpmf_hip_side_bias_add",
             "bpmf_hip_side_bias_mean", "bpmf_hip_side_bias_lambda_get"]
    header = open(os.path.join(ROOT, "include", "bpmf_hip.h")).read()
    source = open(os.path.join(ROOT, "bpmf_amd", "csrc", "capi_bias.hip")).read()
    bound = open(os.path.join(ROOT, "bpmf_amd", "_lib.py")).read()
    for n in names:
        assert re.search(r"BPMF_API int %s\(" % n, header) and re.search(r'extern "C" int %s\(' % n, source) and '"%s"' % n in bound, n
    assert sorted(set(re.findall(r"bpmf_hip_\w*bias\w*", header))) == sorted(names)
    assert hasattr(_lib, "check")


def test_planted_experiment_reproduces_and_the_biases_help(oracle):
    rec = ref.planted_recorded()
    assert rec["spread"] == ref.PLANTED["spread"] == 1.0              # the spread of the first attempt: it was not raised
    with_bias, plain = ref.planted_measure(oracle)
    print("planted: with biases %.12g, plain %.12g" % (with_bias, plain))
    # (the bar of the chain-parity tests: the oracle's sums depend on its thread count the way the device's depend on its grid)
    assert abs(with_bias - rec["rmse_bias"]) < 1e-6 and abs(plain - rec["rmse_plain"]) < 1e-6
    assert with_bias < plain
