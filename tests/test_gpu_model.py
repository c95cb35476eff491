"""Saved models on the device: the read-back and load of the sample rings, the cell kernel, and the served
products against what the training process produced.

  1. ring round trip: samples_get equals get_items after every samples_add, bit for bit; samples_set into a fresh context gives the
     same bytes back, and bpmf_hip_topn over the loaded rings the same bytes as over the original ones (which proves the pad rows);
     range errors and values that are not finite are refused and the context goes on working
  2. predict_cells against tests/newrows_ref.py::predict in longdouble at the cells, within newrows_ref.mean_bound / var_bound and
     the prob bound of tests/topn_score_ref.py::reference (the project's own bounds for these quantities): 70 queries x 130
     candidates, K in {1, 8, 20, 32, 64, 128}, S in {1, 2, 5, 33}; an empty list, one cell, every cell of one query five times over
     (repeats; more than a workgroup's share at every K), the last row and column, a random list; |p| >> spread (mean_rating = 1e6,
     spread 1e-3), where newrows_ref.predict_naive breaks var_bound and the device must not; an fp32 context
  3. the bits of a cell do not depend on the list: a permutation, a subset, another mix, a second call
  4. gibbs(save_model=DIR) then load_model on a second engine: topn, topn_scored of every kind, rank_eval, predict_block and fold_in
     (rows and cols, with topn) byte-identical to the run's own; K = 8, a padded K = 20, an fp32 run at K = 72 served from fp64
  5. bpmf --save-model DIR, then bpmf --model DIR: topn.csv and the three fold-in files byte-identical; --predict within mean_bound
     of the longdouble mean over the saved samples; a probit model's prob column in [0, 1] and within the reference bound

Every test of this file fails on the commit before the feature (missing entry points / arguments).
"""
import os
import subprocess

import numpy as np
import pytest
import bpmf_amd
from bpmf_amd import io as bio
from bpmf_amd.rank import held_out_lists
from tests import model_ref as mr
from tests import newrows_ref as nr
from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")
f64 = mr.f64


# ---- 1. ring round trip ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [8, 20, 64])
def test_ring_round_trip(hip_engine_factory, K):
    nc, nq, S = 37, 9, 3
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, nq, nc)
    other = bpmf_amd.HipEngine(K)
    try:
        rng = np.random.default_rng(K)
        eng.samples_reserve(sq, 5); eng.samples_reserve(sc, 5)
        for s in range(S):
            for side, n in ((sq, nq), (sc, nc)):
                eng.set_items(side, rng.standard_normal((n, K)))
                eng.samples_add(side)
                assert eng.samples_get(side, s, s + 1)[:, 0, :].tobytes() == eng.get_items(side).tobytes(), (K, s)
        Q, Cn = eng.samples_get(sq), eng.samples_get(sc)
        assert Q.shape == (nq, S, K) and Cn.shape == (nc, S, K)
        assert eng.samples_get(sc, 1, 3).tobytes() == np.ascontiguousarray(Cn[:, 1:3]).tobytes()
        assert eng.samples_get(sc, 2, 2).shape == (nc, 0, K)
        # into a fresh context: the same bytes back, and the same ranking (the pad rows of the loaded ring are zeros)
        oq, oc = mr.pair_of_sides(other, nq, nc)
        other.samples_reserve(oq, 4); other.samples_reserve(oc, 3)
        other.samples_set(oq, Q); other.samples_set(oc, Cn)
        assert other.samples_count(oq) == S and other.samples_count(oc) == S
        assert other.samples_get(oq).tobytes() == Q.tobytes() and other.samples_get(oc).tobytes() == Cn.tobytes()
        for ex in (True, False):
            a = eng.topn(sq, sc, 1.5, 6, exclude_rated=ex); b = other.topn(oq, oc, 1.5, 6, exclude_rated=ex)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (K, ex)
        # refusals, and the context keeps working
        for lo, hi in ((0, S + 1), (-1, 1), (2, 1)):
            with pytest.raises(bpmf_amd.BpmfHipError, match="out of range") as e:
                eng.samples_get(sc, lo, hi)
            assert e.value.code == -1
        bad = Cn.copy(); bad[11, 2, K - 1] = np.nan
        with pytest.raises(bpmf_amd.BpmfHipError, match="column 11, sample 2") as e:
            other.samples_set(oc, bad)
        assert e.value.code == -1
        bad[11, 2, K - 1] = np.inf
        with pytest.raises(bpmf_amd.BpmfHipError, match="not finite"):
            other.samples_set(oc, bad)
        with pytest.raises(bpmf_amd.BpmfHipError, match="do not fit"):
            other.samples_set(oc, np.zeros((nc, 4, K)))
        assert other.samples_get(oc).tobytes() == Cn.tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(eng.topn(sq, sc, 1.5, 6), other.topn(oq, oc, 1.5, 6)))
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)
        other.close()


# ---- 2. the cell kernel against longdouble ----------------------------------------------------------------------------------------------

NQ, NC = 70, 130


def cell_lists(rng):
    """name -> (q, c): the lists of the module docstring"""
    q1 = 37
    every = (np.full(5 * NC, q1), np.tile(np.arange(NC), 5))
    rand = (rng.integers(0, NQ, 1000), rng.integers(0, NC, 1000))
    return dict(empty=(np.zeros(0, int), np.zeros(0, int)), one=(np.array([5]), np.array([77])), every=every,
                last=(np.array([NQ - 1, 0, NQ - 1]), np.array([NC - 1, NC - 1, 0])), random=rand)


def load_rings(eng, sq, sc, Es, Vs, cap=None):
    S = Es.shape[0]
    eng.samples_reserve(sq, cap or S); eng.samples_reserve(sc, cap or S)
    eng.samples_set(sq, np.transpose(Es, (1, 0, 2))); eng.samples_set(sc, np.transpose(Vs, (1, 0, 2)))


@pytest.mark.parametrize("K,dtype", [(1, "f64"), (8, "f64"), (20, "f64"), (32, "f64"), (64, "f64"), (128, "f64"), (72, "f32")])
def test_predict_cells_against_longdouble(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    mean_rating, t, sigma = 3.5, 3.75, 0.7
    try:
        for S in (1, 2, 5, 33):
            rng = np.random.default_rng(100 * K + S)
            Es, Vs = rng.standard_normal((S, NQ, K)), rng.standard_normal((S, NC, K))
            load_rings(eng, sq, sc, Es, Vs, S + (S % 2))
            block = mr.block_reference(Es, Vs, mean_rating, mr.kp_of(K), t, sigma)
            for name, (q, c) in cell_lists(rng).items():
                ref = mr.cells_reference(block, q, c)
                got = eng.predict_cells(sq, sc, mean_rating, q, c, t, sigma)
                assert all(g.shape == (len(q),) for g in got)
                worst = mr.check_cells(got, ref, (K, dtype, S, name))
                plain = eng.predict_cells(sq, sc, mean_rating, q, c)
                assert len(plain) == 2 and plain[0].tobytes() == got[0].tobytes() and plain[1].tobytes() == got[1].tobytes()
                # the counting form
                got0 = eng.predict_cells(sq, sc, mean_rating, q, c, t, 0.0)
                assert np.array_equal(got0[2], ref["prob0"]), (K, S, name)
                if name == "random":
                    print("K %d %s S %d: err / bound mean %.3g var %.3g prob %.3g" % (K, dtype, S, *worst))
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_predict_cells_survives_cancellation(hip_engine_factory):
    K, S, mean_rating = 8, 5, 1e6
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    try:
        Es, Vs = mr.cancelling_case(NQ, NC, K, S, 3)
        load_rings(eng, sq, sc, Es, Vs)
        q, c = np.divmod(np.arange(NQ * NC), NC)
        ref = mr.cells_reference(mr.block_reference(Es, Vs, mean_rating, 8), q, c)
        spread = np.sqrt(f64(ref["var"]))
        assert (spread > 1e-4).all() and (spread < 1e-2).all() and (np.abs(f64(ref["mean"])) > 1e6).all()
        _, naive = nr.predict_naive(Es, Vs, mean_rating)
        assert (np.abs(naive[q, c] - f64(ref["var"])) > ref["var_bound"]).any()           # the input discriminates
        worst = mr.check_cells(eng.predict_cells(sq, sc, mean_rating, q, c), ref, "cancellation")
        print("cancellation: err / bound mean %.3g var %.3g" % (worst[0], worst[1]))
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


def test_predict_cells_refusals(hip_engine_factory):
    K = 8
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    try:
        with pytest.raises(bpmf_amd.BpmfHipError, match="no sample ring"):
            eng.predict_cells(sq, sc, 0.0, [0], [0])
        rng = np.random.default_rng(1)
        load_rings(eng, sq, sc, rng.standard_normal((2, NQ, K)), rng.standard_normal((2, NC, K)))
        for q, c, cell in (([0, NQ], [0, 0], "cell 1"), ([0, 1, 2], [0, 1, NC], "cell 2"), ([-1], [0], "cell 0")):
            with pytest.raises(bpmf_amd.BpmfHipError, match=cell + " .*out of range") as e:
                eng.predict_cells(sq, sc, 0.0, q, c)
            assert e.value.code == -1
        with pytest.raises(bpmf_amd.BpmfHipError, match="sigma"):
            eng.predict_cells(sq, sc, 0.0, [0], [0], 1.0, -1.0)
        mean, std = eng.predict_cells(sq, sc, 0.0, [0], [0])
        assert np.isfinite(mean).all() and np.isfinite(std).all() and eng.predict_cells_last_ms(sq) >= 0.0
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 3. order independence ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [4, 20, 128])
def test_cell_bits_do_not_depend_on_the_list(hip_engine_factory, K):
    S = 7
    eng = hip_engine_factory(K)
    sq, sc = mr.pair_of_sides(eng, NQ, NC)
    try:
        rng = np.random.default_rng(K)
        load_rings(eng, sq, sc, rng.standard_normal((S, NQ, K)), rng.standard_normal((S, NC, K)))
        q, c = rng.integers(0, NQ, 3000), rng.integers(0, NC, 3000)
        base = eng.predict_cells(sq, sc, 2.5, q, c, 2.0, 0.5)
        again = eng.predict_cells(sq, sc, 2.5, q, c, 2.0, 0.5)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base, again))
        perm = rng.permutation(len(q))
        got = eng.predict_cells(sq, sc, 2.5, q[perm], c[perm], 2.0, 0.5)
        assert all(a[perm].tobytes() == b.tobytes() for a, b in zip(base, got))
        sub = np.sort(rng.choice(len(q), 41, replace=False))
        got = eng.predict_cells(sq, sc, 2.5, q[sub], c[sub], 2.0, 0.5)
        assert all(a[sub].tobytes() == b.tobytes() for a, b in zip(base, got))
        # another mix: the shared cells among every cell of three queries, in reverse
        qq = np.repeat([int(q[0]), int(q[1]), NQ - 1], NC); cc = np.tile(np.arange(NC)[::-1], 3)
        mix = eng.predict_cells(sq, sc, 2.5, qq, cc, 2.0, 0.5)
        where = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(qq, cc))}
        shared = [(i, where[(int(a), int(b))]) for i, (a, b) in enumerate(zip(q, c)) if (int(a), int(b)) in where]
        assert len(shared) > 20
        i0, i1 = np.array(shared).T
        assert all(a[i0].tobytes() == b[i1].tobytes() for a, b in zip(base, mix))
    finally:
        eng.side_destroy(sq); eng.side_destroy(sc)


# ---- 4. served equals in-process ---------------------------------------------------------------------------------------------------------

def products(engine, res, T, new_rows, new_cols):
    """every served product of a result, as a flat list of arrays"""
    users, movies, mean = res["users"].side, res["movies"].side, res["movies"].mean_rating
    out = list(engine.topn(users, movies, mean, 5))
    for kind, param, sigma in (("ucb", 1.5, 0.0), ("prob", 3.0, 0.7), ("ei", 3.0, 0.7), ("prob", 3.0, 0.0)):
        out += list(engine.topn_scored(users, movies, mean, 5, kind, param, sigma))
    tptr, tcand, _ = held_out_lists(T, res["users"].num(), "rows", None)
    out += list(engine.rank_eval(users, movies, tptr, tcand, mean))
    out += list(engine.predict_block(users, movies, mean))
    out += list(engine.predict_block(movies, users, mean, 3, 17, 5, 44))
    fold = bpmf_amd.fold_in(res, new_rows=new_rows, new_cols=new_cols, topn=5)
    for key in ("rows", "cols"):
        out += [fold[key]["mean"], fold[key]["std"]] + list(fold[key]["topn"])
    cells = bpmf_amd.predict_cells(res, np.arange(60) % 60, np.arange(60) % 40, threshold=3.0)
    return out + [cells["mean"], cells["std"], cells["prob"]]


@pytest.mark.parametrize("K,dtype", [(8, "f64"), (20, "f64"), (72, "f32")])
def test_served_equals_in_process(K, dtype, tmp_path):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    new_rows, new_cols = mr.new_entities(6, nm, 5, 1), mr.new_entities(4, nu, 7, 2).T.tocsc()
    train = bpmf_amd.HipEngine(K, dtype=dtype)
    serve = bpmf_amd.HipEngine(K)
    try:
        res = bpmf_amd.gibbs(train, M, Mt, T, nu, nm, nsims=8, burnin=3, topn=5, foldin=True, save_model=str(tmp_path / "model"), Tt=Tt)
        assert sorted(os.listdir(tmp_path / "model")) == ["U-hyper.ddm", "U-samples.ddm", "V-hyper.ddm", "V-samples.ddm", "model.txt"]
        want = products(train, res, T, new_rows, new_cols)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(res["topn"], want[:3]))
        loaded = bpmf_amd.load_model(serve, str(tmp_path / "model"), M)
        assert loaded["foldin"] and loaded["users"].num() == nu and loaded["movies"].num() == nm
        assert loaded["model_info"]["dtype"] == dtype and loaded["model_info"]["samples"] == 5
        got = products(serve, loaded, T, new_rows, new_cols)
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(want, got)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (K, dtype, i)
        # a model saved again from the loaded rings is the same model
        bpmf_amd.save_model(loaded, str(tmp_path / "again"))
        for name in os.listdir(tmp_path / "model"):
            if name != "model.txt":
                assert (tmp_path / "model" / name).read_bytes() == (tmp_path / "again" / name).read_bytes(), name
    finally:
        train.close(); serve.close()


# ---- 5. the executable -------------------------------------------------------------------------------------------------------------------

def run(args, cwd):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def write_inputs(tmp_path, labels=False):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    vals = (M[2] > 3).astype(np.float64) if labels else M[2]
    bio.write_sparse(tmp_path / "train.sdm", nu, nm, (M[0], M[1], vals))
    bio.write_sparse(tmp_path / "test.sdm", nu, nm, (T[0], T[1], (T[2] > 3).astype(np.float64) if labels else T[2]))
    F = mr.new_entities(6, nm, 5, 1).tocsc()
    bio.write_sparse(tmp_path / "fold.sdm", 6, nm, util.csc_arrays(F))
    return T, nu, nm


def saved_samples(model_dir):
    """(model, Es [S, rows, K], Vs [S, cols, K]) of a model directory"""
    m = bpmf_amd.read_model(model_dir)
    Es, Vs = np.transpose(m["U"], (1, 0, 2)), np.transpose(m["V"], (1, 0, 2))
    return m, Es, Vs


def test_cli_serves_what_the_run_wrote(tmp_path):
    T, nu, nm = write_inputs(tmp_path)
    for d in ("A", "B", "C"):
        os.mkdir(tmp_path / d)
    out = run(["-n", "train.sdm", "-p", "test.sdm", "-d", 20, "-i", 8, "-b", 3, "--topn", 5, "--fold-in-rows", "fold.sdm", "--save-model", "model",
               "-o", "A"], tmp_path)
    assert "save-model: model\n" in out
    out = run(["--model", "model", "-n", "train.sdm", "--topn", 5, "--fold-in-rows", "fold.sdm", "-o", "B"], tmp_path)
    assert out == "model: model, %d x %d, num_latent 20, 5 samples, gaussian\n" % (nu, nm)
    for name in ("topn.csv", "foldin-rows-mean.ddm", "foldin-rows-std.ddm", "foldin-rows-topn.csv"):
        assert (tmp_path / "A" / name).read_bytes() == (tmp_path / "B" / name).read_bytes(), name
    # --predict at the test cells, without the training matrix
    run(["--model", "model", "--predict", "test.sdm", "--predict-threshold", 3.5, "-o", "C"], tmp_path)
    rows = np.loadtxt(tmp_path / "C" / "predict.csv", delimiter=",", skiprows=1, ndmin=2)
    assert (tmp_path / "C" / "predict.csv").read_text().splitlines()[0] == "row,col,mean,std,prob"
    tcol = np.repeat(np.arange(nm), np.diff(T[0]))
    assert np.array_equal(rows[:, 0], T[1] + 1) and np.array_equal(rows[:, 1], tcol + 1)            # the reader's order, 1-based
    m, Es, Vs = saved_samples(tmp_path / "model")
    assert m["alpha"] == 2.0 and not m["probit"]
    ref = mr.cells_reference(mr.block_reference(Es, Vs, m["mean_rating"], 20, 3.5, 1.0 / np.sqrt(m["alpha"])), T[1], tcol)
    mr.check_cells((rows[:, 2], rows[:, 3], rows[:, 4]), ref, "cli --predict")


def test_cli_probit_model_has_a_prob_column(tmp_path):
    T, nu, nm = write_inputs(tmp_path, labels=True)
    os.mkdir(tmp_path / "P")
    run(["-n", "train.sdm", "-p", "test.sdm", "-d", 8, "-i", 6, "-b", 2, "--probit", "--save-model", "model"], tmp_path)
    assert sorted(os.listdir(tmp_path / "model")) == ["U-samples.ddm", "V-samples.ddm", "model.txt"]
    out = run(["--model", "model", "--predict", "test.sdm", "-o", "P"], tmp_path)
    assert out == "model: model, %d x %d, num_latent 8, 4 samples, probit\n" % (nu, nm)
    assert (tmp_path / "P" / "predict.csv").read_text().splitlines()[0] == "row,col,mean,std,prob"
    rows = np.loadtxt(tmp_path / "P" / "predict.csv", delimiter=",", skiprows=1, ndmin=2)
    tcol = np.repeat(np.arange(nm), np.diff(T[0]))
    m, Es, Vs = saved_samples(tmp_path / "model")
    assert m["probit"] and m["mean_rating"] == 0.0 and m["U_hyper"] is None
    ref = mr.cells_reference(mr.block_reference(Es, Vs, 0.0, 8, 0.0, 1.0), T[1], tcol)
    mr.check_cells((rows[:, 2], rows[:, 3], rows[:, 4]), ref, "cli probit --predict")
    with pytest.raises(AssertionError, match="without hyper"):
        run(["--model", "model", "--fold-in-rows", "fold.sdm", "-o", "P"], tmp_path)
