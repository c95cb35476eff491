"""Independent chains on the device: bpmf_hip_side_set_chain, gibbs(chain=), bpmf_amd.run_chains, pool_models
and the multi-chain diagnose.

  1. a pair of sides with set_chain(1) on a 30 x 20 matrix with about 200 ratings takes two sys_sample half-iterations each, K = 8, 64
     and 128 (fp64; K = 128 also fp32): sys_state reports iter 0 / 1, mu and Lambda are bpmf_hyper_sample(.., counter = iter + 2^20) of
     the same inputs byte for byte, the items are the stateless sample_side(iter = t + 2^20) on twin sides given the same
     hyper-parameters and other-side factors byte for byte; chain 0 is a side that never had the call, chain 1 differs from chain 0
  2. gibbs(chain=1) with robust=4, probit=True, censored=, noise="adaptive" and weights runs, differs from chain 0 and repeats bit for
     bit; gibbs(chain=0) is gibbs()
  3. every refusal of set_chain and of the setters after it; sys_sample refuses two sides of different chains
     (a mode of a tensor; in a process of its own, a context with a communicator: set_chain, and sys_sample of a chain set before
     the communicator came)
  4. run_chains(chains=2, nsims=12, burnin=4): the pooled rings are [chain 0's 8 samples, chain 1's 8] byte for byte, chain 0 is a plain
     gibbs with the rings kept, diagnose of the pool is diag_cells_mc called directly; pool_models of two runs; a pool saved chain by
     chain and loaded from the list of directories serves the same figures

  5. the executable: bpmf --chain 0 / 1 --save-model, then bpmf --model A,B -o OUT --predict FILE --diagnose writes the file Python's
     pooled diagnose gives value for value at %.17g; --model A,A is refused; --model A --diagnose alone gives the file it gave before;
     --diagnose-rank in a training run and on one model is C = 1 of the estimator

Every test of this file fails on the commit before the feature (missing entry points / arguments).

At K = 64 in fp64 the columns of this matrix (at most 16 ratings each) take the product form, whose shared factor R0 the stateful path of
chain 0 takes from the Wishart draw (LambdaU) and the stateless sample_side gets by factorising LambdaF: rounding apart.  A chain other than
0 factorises LambdaF too (draw_and_release in capi_sample.hip), which is what makes case 1 hold byte for byte at K = 64.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import bpmf_amd
from bpmf_amd import io as bio
from tests import model_ref as mr
from tests import util
from tests.conftest import ROOT

BPMF = os.path.join(ROOT, "bpmf_amd", "bpmf")

pytestmark = pytest.mark.gpu

STRIDE = 1 << 20
NU, NM, NNZ = 30, 20, 200


def matrix():
    """(M, Mt): about 200 ratings by movie (20 columns, 30 rows) and by user"""
    rng = np.random.default_rng(40)
    cells = rng.choice(NU * NM, NNZ, replace=False)
    vals = rng.integers(1, 6, NNZ).astype(np.float64)
    A = sp.coo_matrix((vals, (cells // NM, cells % NM)), shape=(NU, NM))
    return util.csc_arrays(A), util.csc_arrays(A.T)


def pair(eng, M, Mt, chain=None, mean=None):
    mean = util.mean_rating(M) if mean is None else mean
    movies, users = eng.side_create(NM, NU, *M, mean), eng.side_create(NU, NM, *Mt, mean)
    if chain is not None:
        eng.side_set_chain(movies, chain); eng.side_set_chain(users, chain)
    return movies, users


def two_iterations(eng, movies, users, alpha=2.0):
    for _ in range(2):
        eng.sys_sample(movies, users, alpha)
        eng.sys_sample(users, movies, alpha)
    return eng.get_items(movies), eng.get_items(users)


# ---- 1. what the chain id offsets ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,dtype", [(8, "f64"), (64, "f64"), (128, "f64"), (128, "f32")])
def test_chain_one_is_keyed_at_the_offset_indices(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    M, Mt = matrix()
    alpha = 2.0
    movies, users = pair(eng, M, Mt, 1)
    twin_m, twin_u = pair(eng, M, Mt)
    try:
        assert eng.side_chain(movies) == 1 and eng.side_chain(users) == 1 and eng.side_chain(twin_m) == 0
        cov = {id(movies): np.zeros((K, K)), id(users): np.zeros((K, K))}
        for t in (0, 1):
            for me, ot, tme, tot in ((movies, users, twin_m, twin_u), (users, movies, twin_u, twin_m)):
                pre_me, pre_ot = eng.get_items(me), eng.get_items(ot)
                eng.sys_sample(me, ot, alpha)
                it, nrm, cov_new, mu, LF, LU = eng.sys_state(me)
                assert it == t                                                         # the chain's own index
                want = bpmf_amd.engine.hyper_sample(K, me.ncols, cov[id(me)], t + STRIDE)
                assert mu.tobytes() == want[0].tobytes() and np.asfortranarray(LU).tobytes() == want[1].tobytes() and \
                    np.asfortranarray(LF).tobytes() == want[2].tobytes(), (K, dtype, t)
                plain = bpmf_amd.engine.hyper_sample(K, me.ncols, cov[id(me)], t)
                assert mu.tobytes() != plain[0].tobytes()
                X = eng.get_items(me)
                eng.set_items(tme, pre_me); eng.set_items(tot, pre_ot)
                eng.sample_side(tme, tot, t + STRIDE, alpha, mu, LF)
                twin = eng.get_items(tme)
                print("K %d %s t %d %s: max |stateful - stateless at the offset index| = %.3g" % (K, dtype, t, "movies" if me is movies else "users", np.abs(twin - X).max()))
                assert np.abs(twin - X).max() <= 1e-9 * np.abs(X).max()                # the same streams, whatever the form of the arithmetic
                assert twin.tobytes() == X.tobytes(), (K, dtype, t)
                eng.set_items(tme, pre_me)
                eng.sample_side(tme, tot, t, alpha, mu, LF)
                assert np.abs(eng.get_items(tme) - X).max() > 1e-3                     # other streams
                cov[id(me)] = cov_new
                assert eng.sys_norm(me, t) == nrm
    finally:
        for s in (movies, users, twin_m, twin_u):
            eng.side_destroy(s)


@pytest.mark.parametrize("K,dtype", [(8, "f64"), (64, "f64"), (128, "f32")])
def test_chain_zero_is_the_run_as_it_was(hip_engine_factory, K, dtype):
    eng = hip_engine_factory(K, dtype)
    M, Mt = matrix()
    got = {}
    for chain in (None, 0, 1, 63):
        movies, users = pair(eng, M, Mt, chain)
        try:
            got[chain] = two_iterations(eng, movies, users)
            assert eng.sys_state(movies)[0] == 1
        finally:
            eng.side_destroy(movies); eng.side_destroy(users)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[None], got[0]))
    for c in (1, 63):
        assert all(a.tobytes() != b.tobytes() and np.isfinite(a).all() for a, b in zip(got[c], got[0]))
    assert got[1][0].tobytes() != got[63][0].tobytes()


# ---- 2. gibbs(chain=) ----------------------------------------------------------------------------------------------------------------------

RUN = dict(nsims=5, burnin=2)


def variants(M):
    flags = np.zeros(len(M[2])); flags[3::7] = 1.0; flags[5::11] = -1.0
    keep = flags != 0
    col_of = np.repeat(np.arange(len(M[0]) - 1), np.diff(M[0]))
    C = sp.csc_matrix((flags[keep], (M[1][keep], col_of[keep])), shape=(int(M[1].max()) + 1, len(M[0]) - 1))
    C = (C.indptr.astype(np.int64), C.indices.astype(np.int32), C.data.astype(np.float64))
    W = (M[0], M[1], np.linspace(0.5, 2.0, len(M[2])))
    return dict(plain={}, alpha=dict(alpha=0.7), adaptive=dict(noise="adaptive"), weights=dict(weights=W), robust=dict(robust=4.0),
                probit=dict(probit=True, threshold=3.0), censored=dict(censored=C))


@pytest.mark.parametrize("variant", ["plain", "alpha", "adaptive", "weights", "robust", "probit", "censored"])
def test_gibbs_chain(hip_engine_factory, variant):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    eng = hip_engine_factory(8)
    kw = variants(M)[variant]
    if variant == "censored":
        kw = dict(kw, censored=(kw["censored"][0], kw["censored"][1], kw["censored"][2]))
    run = lambda **more: bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, **RUN, **kw, **more)
    base, zero, one, again = run(), run(chain=0), run(chain=1), run(chain=1)
    assert base["chain"] == 0 and zero["chain"] == 0 and one["chain"] == 1
    for k in ("U", "V"):
        assert base[k].tobytes() == zero[k].tobytes() and one[k].tobytes() == again[k].tobytes()
        assert one[k].tobytes() != base[k].tobytes() and np.isfinite(one[k]).all()
    assert np.array(base["rmse"]).tobytes() == np.array(zero["rmse"]).tobytes()
    assert np.array(one["rmse"]).tobytes() == np.array(again["rmse"]).tobytes() != np.array(base["rmse"]).tobytes()
    if variant == "adaptive":
        assert one["alpha"] == again["alpha"] and one["alpha"][1:] != base["alpha"][1:]
    for r in (base, zero, one, again):
        eng.side_destroy(r["users"].side); eng.side_destroy(r["movies"].side)


def test_gibbs_chain_on_an_fp32_engine(hip_engine_factory):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    eng = hip_engine_factory(128, "f32")
    runs = [bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, chain=c, **RUN) for c in (0, 1, 1)]
    assert runs[1]["U"].tobytes() == runs[2]["U"].tobytes() != runs[0]["U"].tobytes() and np.isfinite(runs[1]["U"]).all()
    for r in runs:
        eng.side_destroy(r["users"].side); eng.side_destroy(r["movies"].side)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_set_chain_refusals(hip_engine_factory):
    eng = hip_engine_factory(8)
    M, Mt = matrix()
    F = np.random.default_rng(23).standard_normal((NM, 3))
    levels = np.array([1.0, 2.0, 3.0, 4.0, 5.0])

    def refused(side, chain, reason):
        with pytest.raises(bpmf_amd.BpmfHipError, match="side_set_chain: " + reason) as e:
            eng.side_set_chain(side, chain)
        assert e.value.code == -1 and "\n" not in str(e.value)

    movies, users = pair(eng, M, Mt)
    try:
        for bad in (-1, 64, 1000):
            refused(movies, bad, "chain %d given, 0 .. 63 allowed" % bad)
        assert eng.lib.bpmf_hip_side_set_chain(None, 1) == -1 and eng.lib.bpmf_hip_side_chain(None) == 0
        eng.side_set_chain(movies, 2)
        with pytest.raises(bpmf_amd.BpmfHipError, match="sys_sample: the sides belong to different chains \\(2 and 0"):
            eng.sys_sample(movies, users, 2.0)
        eng.side_set_chain(users, 2)
        eng.side_set_chain(movies, 5); eng.side_set_chain(movies, 2)                 # (may be changed until the first half-iteration)
        eng.sys_sample(movies, users, 2.0)
        refused(movies, 1, "the side has taken a half-iteration")
        refused(movies, 0, "the side has taken a half-iteration")
        assert eng.side_chain(movies) == 2
        eng.sys_state(movies)
    finally:
        eng.side_destroy(movies); eng.side_destroy(users)

    # a side in a state that only chain 0 runs with refuses the chain; the setter of that state refuses a side whose chain is not 0
    states = dict(
        features=(lambda s, o: eng.set_features(s, F, 5.0, 3), "not together with features"),
        ordinal=(lambda s, o: eng.set_ordinal(s, levels, None, 11), "not on an ordinal side"),
        implicit=(lambda s, o: eng.set_implicit(s, 0.1), "not on a side with implicit feedback"),
        prop_posterior=(lambda s, o: eng.set_prop_posterior(s, np.tile(np.eye(8).ravel(), (NM, 1))), "not together with propagated priors"),
        reduce=(lambda s, o: eng.sys_set_reduce(s, o), "not together with the BPMF_REDUCE formulation"),
        bias=(lambda s, o: eng.set_bias(s, 1.0, 13, 0), "not on a side with bias terms"))
    for name, (setter, sentence) in states.items():
        mean = 0.0 if name in ("ordinal", "implicit") else None                        # (what those two models ask for)
        movies, users = pair(eng, M, Mt, mean=mean)
        try:
            setter(movies, users)
            refused(movies, 1, sentence)
            refused(movies, 0, sentence)
        finally:
            eng.side_destroy(movies); eng.side_destroy(users)
        movies, users = pair(eng, M, Mt, 1, mean=mean)
        try:
            with pytest.raises(bpmf_amd.BpmfHipError, match="not on a side whose chain is not 0 \\(bpmf_hip_side_set_chain\\)") as e:
                setter(movies, users)
            assert e.value.code == -1, name
        finally:
            eng.side_destroy(movies); eng.side_destroy(users)
    # a shard
    n = int(M[0][10])
    shard = eng.side_create(NM, NU, M[0][:11], M[1][:n], M[2][:n], util.mean_rating(M), 0, 10)
    try:
        refused(shard, 1, "not on a shard of a side")
    finally:
        eng.side_destroy(shard)
    # what runs on a chain other than 0 is accepted after the call
    for setter in (lambda s: eng.set_weights(s, np.linspace(0.5, 2.0, s.nnz)), lambda s: eng.set_robust(s, 4.0, 7),
                   lambda s: eng.set_probit(s, 3.0, 1), lambda s: eng.set_censored(s, np.r_[1, np.zeros(NNZ - 1)].astype(np.int8), 5)):
        movies, users = pair(eng, M, Mt, 3, mean=0.0)
        try:
            setter(movies)
        finally:
            eng.side_destroy(movies); eng.side_destroy(users)


# ---- 4. run_chains, pool_models, diagnose of the pool --------------------------------------------------------------------------------------

def test_run_chains(hip_engine_factory, tmp_path):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    eng = hip_engine_factory(8)
    run = dict(nsims=12, burnin=4, alpha=2.0)
    pool = bpmf_amd.run_chains(eng, M, Mt, T, nu, nm, chains=2, Tt=Tt, **run)
    assert pool["chains"] == 2 and [p["chain"] for p in pool["per_chain"]] == [0, 1] and pool["foldin"]
    assert all(len(p["rmse"]) == 12 and np.isfinite(p["final_rmse_avg"]) for p in pool["per_chain"])
    U, V = eng.samples_get(pool["users"].side), eng.samples_get(pool["movies"].side)
    assert U.shape == (nu, 16, 8) and V.shape == (nm, 16, 8)
    singles = [bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, chain=c, keep_rings=True, **run) for c in (0, 1)]
    plain = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, save_model=str(tmp_path / "plain"), **run)
    for c, r in enumerate(singles):
        assert U[:, 8 * c:8 * c + 8].tobytes() == eng.samples_get(r["users"].side).tobytes()
        assert V[:, 8 * c:8 * c + 8].tobytes() == eng.samples_get(r["movies"].side).tobytes()
        assert np.array(r["rmse"]).tobytes() == np.array(pool["per_chain"][c]["rmse"]).tobytes()
    assert eng.samples_get(plain["users"].side).tobytes() == U[:, :8].tobytes() and np.array(plain["rmse"]).tobytes() == np.array(singles[0]["rmse"]).tobytes()
    assert U[:, :8].tobytes() != U[:, 8:].tobytes()
    hyp = eng.hyper_get(pool["users"].side)
    assert all(h[:8].tobytes() == g.tobytes() for h, g in zip(hyp, eng.hyper_get(singles[0]["users"].side)))
    assert all(h[8:].tobytes() == g.tobytes() for h, g in zip(hyp, eng.hyper_get(singles[1]["users"].side)))

    # diagnose of the pool is the multi-chain estimator over the pooled rings
    tcol = np.repeat(np.arange(nm), np.diff(T[0]))
    d = bpmf_amd.diagnose(pool, T[1], tcol)
    direct = eng.diag_cells_mc(pool["users"].side, pool["movies"].side, pool["movies"].mean_rating, T[1], tcol, 2)
    assert sorted(d) == sorted(["rows", "cols", "mean", "std", "rhat", "ess_bulk", "ess_tail", "mcse", "chains", "samples", "summary"])
    assert all(d[k].tobytes() == direct[k].tobytes() for k in ("mean", "std", "rhat", "ess_bulk", "ess_tail"))
    assert d["chains"] == 2 and d["samples"] == 16 and d["mcse"].tobytes() == (d["std"] / np.sqrt(d["ess_bulk"])).tobytes()
    assert d["summary"] == bpmf_amd.diag_summary(d) and d["summary"]["chains"] == 2 and d["summary"]["n_nan"] == 0
    assert np.isfinite(d["rhat"]).all() and (d["ess_bulk"] > 0).all() and (d["ess_tail"] > 0).all()
    pm = bpmf_amd.predict_cells(pool, T[1], tcol)
    assert pm["mean"].tobytes() == d["mean"].tobytes()
    # one chain: the old dict unless rank=True, which is C = 1 of the new estimator
    old = bpmf_amd.diagnose(singles[0], T[1], tcol)
    assert sorted(old) == sorted(["rows", "cols", "mean", "std", "rhat", "ess", "mcse", "samples", "summary"])
    ranked = bpmf_amd.diagnose(singles[0], T[1], tcol, rank=True)
    one = eng.diag_cells_mc(singles[0]["users"].side, singles[0]["movies"].side, singles[0]["movies"].mean_rating, T[1], tcol, 1)
    assert ranked["chains"] == 1 and all(ranked[k].tobytes() == one[k].tobytes() for k in ("rhat", "ess_bulk", "ess_tail"))

    # pool_models of the two runs, and of their saved directories
    p2 = bpmf_amd.pool_models(singles)
    assert p2["chains"] == 2 and p2["U"].tobytes() == U.tobytes() and p2["V"].tobytes() == V.tobytes()
    with pytest.raises(ValueError, match="chain 1 has the first kept sample of chain 0"):
        bpmf_amd.pool_models([singles[0], plain])
    for c, r in enumerate(singles):
        bpmf_amd.save_model(r, str(tmp_path / ("chain%d" % c)))
    serve = bpmf_amd.HipEngine(8)
    try:
        loaded = bpmf_amd.load_model(serve, [str(tmp_path / "chain0"), str(tmp_path / "chain1")])
        assert loaded["chains"] == 2 and serve.samples_get(loaded["users"].side).tobytes() == U.tobytes()
        again = bpmf_amd.diagnose(loaded, T[1], tcol)
        assert all(again[k].tobytes() == d[k].tobytes() for k in ("mean", "std", "rhat", "ess_bulk", "ess_tail"))
        with pytest.raises(ValueError, match="the same chain twice"):
            bpmf_amd.load_model(serve, [str(tmp_path / "chain0"), str(tmp_path / "plain")])
        single = bpmf_amd.load_model(serve, str(tmp_path / "chain0"))
        assert "chains" not in single and sorted(bpmf_amd.diagnose(single, T[1], tcol)) == sorted(old)
    finally:
        serve.close()
    for r in singles + [plain, pool]:
        eng.side_destroy(r["users"].side); eng.side_destroy(r["movies"].side)


def test_set_chain_refuses_a_mode_of_a_tensor(hip_engine_factory):
    eng = hip_engine_factory(8)
    rng = np.random.default_rng(3)
    idx = np.unique(np.stack([rng.integers(0, 6, 40), rng.integers(0, 5, 40), rng.integers(0, 4, 40)], axis=1), axis=0)
    t = eng.tensor_create(idx, rng.standard_normal(len(idx)), (6, 5, 4), 0.0)
    try:
        for side in t.sides:
            for chain in (1, 0):
                with pytest.raises(bpmf_amd.BpmfHipError, match="side_set_chain: not on a mode of a tensor") as e:
                    eng.side_set_chain(side, chain)
                assert e.value.code == -1 and "\n" not in str(e.value)
            assert eng.side_chain(side) == 0
    finally:
        eng.tensor_destroy(t)


_COMM_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bpmf_amd
eng = bpmf_amd.HipEngine(8)
A = (np.array([0, 4, 6], np.int64), np.array([0, 1, 2, 3, 0, 2], np.int32), np.array([2., 3., 7., 4., 5., 1.]))
B = (np.array([0, 2, 3, 5, 6], np.int64), np.array([0, 1, 0, 0, 1, 0], np.int32), np.array([2., 5., 3., 7., 1., 4.]))
early_m, early_u = eng.side_create(2, 4, *A, 3.0), eng.side_create(4, 2, *B, 3.0)
eng.side_set_chain(early_m, 1); eng.side_set_chain(early_u, 1)
eng.comm_init(1, 0, eng.comm_unique_id())
late = eng.side_create(2, 4, *A, 3.0)
for name, call in (("SET", lambda: eng.side_set_chain(late, 1)), ("SET0", lambda: eng.side_set_chain(late, 0)),
                   ("SAMPLE", lambda: eng.sys_sample(early_m, early_u, 2.0))):
    try:
        call()
        print(name, "ACCEPTED")
    except bpmf_amd.BpmfHipError as e:
        print(name, "REFUSED %d %s" % (e.code, e))
print("CHAIN", eng.side_chain(late))
eng.close()
"""


def test_set_chain_refuses_a_context_with_a_communicator():
    """a whole side on a context that has a communicator (one rank, as `bpmf -g 1` makes one), and a chain set before the communicator
    came.  In a process of its own: a communicator is process-wide state of the communication library."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("BPMF_HIP_RCCL_LIBRARY", None)
    r = subprocess.run([sys.executable, "-c", _COMM_CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    for name in ("SET", "SET0"):
        assert re.search(r"^%s REFUSED -1 .*side_set_chain: not on a context with a communicator$" % name, r.stdout, re.M), r.stdout
    assert re.search(r"^SAMPLE REFUSED -1 .*sys_sample: a chain other than 0 not on a context with a communicator$", r.stdout, re.M), r.stdout
    assert re.search(r"^CHAIN 0$", r.stdout, re.M), r.stdout


# ---- 5. the executable -----------------------------------------------------------------------------------------------------------------------

def run(args, cwd, ok=True):
    p = subprocess.run([BPMF] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stdout + p.stderr
    return p


def read_csv(path, header):
    lines = open(path).read().splitlines()
    assert lines[0] == header
    return np.array([ln.split(",") for ln in lines[1:]], dtype=float).reshape(-1, len(header.split(",")))


MC_HEADER = "row,col,mean,std,rhat,ess_bulk,ess_tail,mcse"


def mc_final_lines(s, samples, chains):
    return ["Final ESS: bulk min %.1f median %.1f tail min %.1f median %.1f of %d samples in %d chains (%d cells)"
            % (s["ess_bulk_min"], s["ess_bulk_median"], s["ess_tail_min"], s["ess_tail_median"], samples, chains, s["n"]),
            "Final rank-Rhat: median %.4f max %.4f above 1.01: %.2f%%" % (s["rhat_median"], s["rhat_max"], 100.0 * s["rhat_above"]),
            "Final MCSE/std: median %.4f" % s["mcse_over_std_median"]]


def test_cli_chains(tmp_path):
    M, Mt, T, Tt, nu, nm = mr.small_ratings()
    bio.write_sparse(tmp_path / "train.sdm", nu, nm, M)
    bio.write_sparse(tmp_path / "test.sdm", nu, nm, T)
    for name in ("P", "O", "OA", "OD", "OR", "OT"):
        os.mkdir(tmp_path / name)
    train = ["-n", "train.sdm", "-p", "test.sdm", "-d", 8, "-i", 12, "-b", 4]
    plain = run(train + ["--save-model", "P0"], tmp_path)
    a = run(train + ["--chain", 0, "--save-model", "A"], tmp_path)
    b = run(train + ["--chain", 1, "--save-model", "B"], tmp_path)
    # one more header line, nothing else in stdout changes; chain 0 is the run as it was
    drop = lambda text, *starts: [ln for ln in text.splitlines() if not ln.startswith(("pid: ", "save-model: ", "Average items/sec", "Total") + starts)
                                  and "/sec" not in ln]
    assert "chain: 0 (random streams of half-iterations 0 ...)" in a.stdout.splitlines()
    assert "chain: 1 (random streams of half-iterations 1048576 ...)" in b.stdout.splitlines()
    assert drop(a.stdout, "chain: ") == drop(plain.stdout) and not any(ln.startswith("chain: ") for ln in plain.stdout.splitlines())
    ma, mb, mp = (bpmf_amd.read_model(str(tmp_path / d)) for d in ("A", "B", "P0"))
    assert ma["U"].tobytes() == mp["U"].tobytes() and ma["V"].tobytes() == mp["V"].tobytes() and mb["U"].tobytes() != ma["U"].tobytes()
    # the same chains in Python
    eng = bpmf_amd.HipEngine(8)
    try:
        one = bpmf_amd.gibbs(eng, M, Mt, T, nu, nm, Tt=Tt, nsims=12, burnin=4, chain=1, keep_rings=True)
        assert eng.samples_get(one["users"].side).tobytes() == mb["U"].tobytes() and eng.samples_get(one["movies"].side).tobytes() == mb["V"].tobytes()
        # --model A,B --diagnose: the pooled multi-chain estimator, value for value what Python's pooled diagnose gives
        o = run(["--model", "A,B", "-o", "O", "--predict", "test.sdm", "--diagnose"], tmp_path)
        rec = read_csv(tmp_path / "O" / "diagnostics.csv", MC_HEADER)
        tcol = np.repeat(np.arange(nm), np.diff(T[0]))
        pool = bpmf_amd.load_model(eng, [str(tmp_path / "A"), str(tmp_path / "B")])
        d = bpmf_amd.diagnose(pool, T[1], tcol)
        assert np.array_equal(rec[:, 0], T[1] + 1) and np.array_equal(rec[:, 1], tcol + 1)
        for j, k in enumerate(("mean", "std", "rhat", "ess_bulk", "ess_tail", "mcse")):
            assert rec[:, 2 + j].tobytes() == d[k].tobytes(), k
        assert o.stdout.startswith("model: A,B, ") and o.stdout.splitlines()[0].endswith(", 16 samples, gaussian, 2 chains")
        assert o.stdout.splitlines()[1:] == mc_final_lines(d["summary"], 16, 2)
        pc = read_csv(tmp_path / "O" / "predict.csv", "row,col,mean,std")
        assert pc[:, 2].tobytes() == d["mean"].tobytes()                            # everything --model serves comes from the pooled rings
        # --model A,A is refused, in one line, and so is a list with an empty name
        for lst, reason in (("A,A", "the same chain twice"), ("A,,B", "an empty directory name"), ("A,P0", "the same chain twice")):
            p = run(["--model", lst, "-o", "OA", "--predict", "test.sdm", "--diagnose"], tmp_path, ok=False)
            assert p.returncode == 1 and p.stdout == "" and len(p.stderr.strip().splitlines()) == 1 and reason in p.stderr, p.stderr
        # --model A alone with --diagnose: the file and the lines of one chain, as before
        s1 = run(["--model", "A", "-o", "OD", "--predict", "test.sdm", "--diagnose"], tmp_path)
        single = bpmf_amd.load_model(eng, str(tmp_path / "A"))
        d1 = bpmf_amd.diagnose(single, T[1], tcol)
        r1 = read_csv(tmp_path / "OD" / "diagnostics.csv", "row,col,mean,std,rhat,ess,mcse")
        for j, k in enumerate(("mean", "std", "rhat", "ess", "mcse")):
            assert r1[:, 2 + j].tobytes() == d1[k].tobytes(), k
        assert s1.stdout.splitlines()[0].endswith(", 8 samples, gaussian") and s1.stdout.splitlines()[1].startswith("Final ESS: min ")
        # --diagnose-rank on one model and in a training run: C = 1 of the estimator
        s2 = run(["--model", "A", "-o", "OR", "--predict", "test.sdm", "--diagnose-rank"], tmp_path)
        d2 = bpmf_amd.diagnose(single, T[1], tcol, rank=True)
        r2 = read_csv(tmp_path / "OR" / "diagnostics.csv", MC_HEADER)
        for j, k in enumerate(("mean", "std", "rhat", "ess_bulk", "ess_tail", "mcse")):
            assert r2[:, 2 + j].tobytes() == d2[k].tobytes(), k
        assert s2.stdout.splitlines()[1:] == mc_final_lines(d2["summary"], 8, 1)
        t = run(train + ["--diagnose-rank", "-o", "OT"], tmp_path)
        r3 = read_csv(tmp_path / "OT" / "diagnostics.csv", MC_HEADER)
        assert r3.tobytes() == r2.tobytes()                                         # (the training run of chain 0 is the run that saved A)
        lines = t.stdout.splitlines()
        at = lines.index(mc_final_lines(d2["summary"], 8, 1)[0])
        assert lines[at:at + 3] == mc_final_lines(d2["summary"], 8, 1) and lines[at + 3].startswith("Final trace ESS: RMSE ")
        assert "diagnose: rank-normalised split-Rhat, bulk and tail ESS of the test predictions" in lines
    finally:
        eng.close()
