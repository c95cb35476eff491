"""tests/variants_ref.py against the oracle it restates (no GPU).

With no variant the restated chain must BE oracle.gibbs: same hyper draws, same column samples, same running means of the
evaluation -- rmse, U and V to 1e-12 (they are the same operations; only the thread partition of the sums may differ).  With the
diagonal-only precision its first movies half-iteration is the `ml100k_k32_nocov` case of tests/test_oracle_vs_ref.py (V-0.ddm of
the reference's BPMF_NO_COVARIANCE build): the oracle call of that test bit for bit, and the dump itself to that test's 1e-10
wherever the dump has been built.
"""
import os

import numpy as np
import pytest

from tests import util
from tests import variants_ref

_DATA = {"tiny": util.tiny, "synthetic": lambda: util.synthetic(150, 40, 2500, seed=12, heavy=(3, 140))}


@pytest.mark.parametrize("K", [8, 20])
@pytest.mark.parametrize("data", ["tiny", "synthetic"])
def test_restated_chain_without_a_variant_is_oracle_gibbs(oracle, data, K):
    M, Mt, T, Tt, nu, nm = _DATA[data]()
    ref = oracle.gibbs(K, M, Mt, T, Tt, nsims=4, burnin=1)
    got = variants_ref.gibbs(oracle, K, M, Mt, T, Tt, 4, 1, 2.0)
    assert set(got) == set(ref)
    for key in ("rmse", "rmse_avg", "norm_u", "norm_m", "U", "V", "Pavg", "Pm2"):
        assert np.shape(got[key]) == np.shape(ref[key]), key
        assert np.abs(np.asarray(got[key]) - np.asarray(ref[key])).max() <= 1e-12, key
    assert abs(got["final_rmse_avg"] - ref["final_rmse_avg"]) <= 1e-12 and got["num_predict"] == ref["num_predict"]


def test_restated_chain_takes_another_alpha(oracle):
    M, Mt, T, Tt, nu, nm = util.tiny()
    ref = oracle.gibbs(8, M, Mt, T, Tt, alpha=1.5, nsims=3, burnin=0)
    got = variants_ref.gibbs(oracle, 8, M, Mt, T, Tt, 3, 0, 1.5)
    assert np.abs(got["rmse"] - ref["rmse"]).max() <= 1e-12 and np.abs(got["U"] - ref["U"]).max() <= 1e-12


def test_no_covariance_is_the_reference_dump_case(oracle):
    from tests import test_oracle_vs_ref as R
    K = 32
    M, Mt, T, Tt, nu, nm = util.ml100k()
    got = variants_ref.gibbs(oracle, K, M, Mt, T, Tt, 1, 1, 2.0, no_covariance=True)
    # what _nocov_case computes: zero factors on the other side, the hyper-parameters of iteration 0 from a zero cov
    mu, LU, LF = oracle.hyper_sample(K, nm, np.zeros((K, K)), 0)
    V = np.zeros((nm, K))
    oracle.sample_side(K, M, util.mean_rating(M), 2.0, np.zeros((nu, K)), V, 0, mu, LF, no_covariance=True)
    assert np.abs(got["V"] - V).max() <= 1e-12 * max(1.0, np.abs(V).max())
    plain = oracle.gibbs(K, M, Mt, T, Tt, nsims=1, burnin=1)
    assert np.abs(got["V"] - plain["V"]).max() > 1e-3               # (the switch does something)
    d = os.path.join(R.REFOUT, "ml100k_k32_nocov")
    if os.path.isdir(d):                                             # the dump of the real BPMF_NO_COVARIANCE build, where it was built
        ref_v = R.read_ddm(os.path.join(d, "V-0.ddm"))
        assert np.abs(got["V"] - ref_v).max() < 1e-10 * max(1.0, np.abs(ref_v).max())


def test_priors_are_symmetric_positive_definite_and_cached():
    P = variants_ref.prop_priors(7, 20, 3)
    assert P.shape == (7, 20, 20) and np.array_equal(P, P.transpose(0, 2, 1)) and np.linalg.eigvalsh(P).min() >= 2.0 - 1e-12
    assert variants_ref.prop_priors(7, 20, 3) is P and not P.flags.writeable
