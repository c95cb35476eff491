"""Worker of test_gpu_reduce.py: the BPMF_REDUCE formulation (bpmf_hip_sys_set_reduce) of the stateful path, in a
process of its own (one-rank RCCL communicator) --
  * single GPU, no communicator: the chain against the oracle's restatement of the reference's BPMF_REDUCE build
    (oracle.gibbs_reduce: preComputeMuLambda / sample from precMu + precLambda, c++/sample.cpp:234-246,289-291,375-377);
  * the same over a one-rank communicator + ranges (the grouped ncclReduce onto the owners runs, as the identity):
    bit for bit the chain without a communicator;
  * switching the formulation off again returns to the gather form.
Arguments: K [alpha [variant]].  variant "diag": all of the above with the diagonal-only precision (set_no_covariance) on, against
oracle.gibbs_reduce(no_covariance=True).  variant "prop": per-column propagated priors (set_prop_posterior) on both sides; the
oracle has no entry for them in this formulation, so the formulation is compared with the gather form under the same priors, GPU
against GPU, at the bar the plain run uses between the two (1e-8 of the scale) -- and over the communicator bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bpmf_amd
    from bpmf_amd import synth
    from bpmf_amd.sys import Sys
    from oracle import oracle as orc
    K = int(sys.argv[1])
    alpha = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0        # (-a F, c++/bpmf.cpp:91: tests/test_gpu_alpha.py)
    variant = sys.argv[3] if len(sys.argv) > 3 else "plain"
    assert variant in ("plain", "diag", "prop"), variant
    nsims = 4
    # one heavy movie (650 ratings), empty columns on both sides
    M, Mt, T, Tt, nu, nm = synth.ratings(700, 500, 30000, seed=3, heavy=(7, 650))
    mean = float(np.sum(M[2])) / len(M[2])
    ref = None
    if variant != "prop":
        ref = orc.Oracle().gibbs_reduce(K, M, Mt, T, alpha=alpha, nsims=nsims, burnin=1, no_covariance=variant == "diag")
    prop = None
    if variant == "prop":                                        # SPD per column, symmetric: B B^T + 2 I, B = 0.2 N(0, 1)
        rng = np.random.default_rng(900 + K)
        prop = []
        for n in (nm, nu):
            B = rng.standard_normal((n, K, K)) * 0.2
            prop.append((np.einsum("nij,nkj->nik", B, B) + 2.0 * np.eye(K)[None]).reshape(n, K * K))

    def run(comm, reduce, nocov=False):
        eng = bpmf_amd.HipEngine(K)
        eng.set_no_covariance(nocov)
        if comm:
            eng.comm_init(1, 0, eng.comm_unique_id())
        Sys.nsims, Sys.burnin, Sys.alpha = nsims, 1, alpha
        movies = Sys("movs", eng, M, nm, nu, T=T, mean_rating=mean)
        users = Sys("users", eng, Mt, nu, nm, mean_rating=mean)
        if comm:
            eng.side_set_ranges(movies.side, [0, nm]); eng.side_set_ranges(users.side, [0, nu])
        if prop is not None:
            eng.set_prop_posterior(movies.side, prop[0]); eng.set_prop_posterior(users.side, prop[1])
        if reduce:
            eng.sys_set_reduce(movies.side, users.side, True)
        rm = []
        for i in range(nsims):
            movies.sample(users); users.sample(movies)
            movies.predict(users)
            rm.append(movies.rmse)
        movies.refresh(); users.refresh()
        out = (np.asarray(rm), users.items().copy(), movies.items().copy())
        if reduce:                                               # off again: one more iteration of the gather form runs
            eng.sys_set_reduce(movies.side, users.side, False)
            movies.sample(users); users.sample(movies); movies.refresh()
            assert np.all(np.isfinite(movies.items()))
        eng.close()
        return out

    nocov = variant == "diag"
    got = run(False, True, nocov)
    if ref is not None:
        scale = max(np.abs(ref["U"]).max(), np.abs(ref["V"]).max())
        eu = np.abs(got[1] - ref["U"]).max() / scale; ev = np.abs(got[2] - ref["V"]).max() / scale
        er = np.abs(got[0] - ref["rmse"]).max()
        print("reduce %s K=%d: against the oracle factors %.3e / %.3e rmse %.3e" % (variant, K, eu, ev, er))
        # fp64: summation order of the Gram, 1/sqrt vs divide, log / sqrt ulps, over `nsims` iterations of the chain
        assert eu < 1e-8 and ev < 1e-8 and er < 1e-9, (eu, ev, er)
    else:
        scale = max(np.abs(got[1]).max(), np.abs(got[2]).max())
        eu = ev = er = float("nan")
    plain = run(False, False, nocov)                             # the default formulation: same chain up to rounding
    pu = np.abs(plain[1] - got[1]).max() / scale; pv = np.abs(plain[2] - got[2]).max() / scale
    print("reduce %s K=%d: against the gather form factors %.3e / %.3e rmse %.3e" % (variant, K, pu, pv, np.abs(plain[0] - got[0]).max()))
    assert pu < 1e-8
    if variant != "plain":
        assert np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2])) and pv < 1e-8
    shard = run(True, True, nocov)
    for a, b in zip(got, shard):
        assert np.array_equal(a, b), "BPMF_REDUCE over a one-rank communicator differs from the plain one"
    if variant == "plain":
        print("REDUCE-OK K=%d alpha=%g factors %.1e / %.1e rmse %.1e" % (K, alpha, eu, ev, er))
    else:
        print("REDUCE-OK K=%d alpha=%g variant=%s factors %.1e / %.1e rmse %.1e gather %.1e / %.1e" % (K, alpha, variant, eu, ev, er, pu, pv))


if __name__ == "__main__":
    main()
