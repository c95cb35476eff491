"""The BPMF_REDUCE formulation (Sys::preComputeMuLambda, c++/sample.cpp:234-246; c++/mpi_reduce.h) on
the GPU against the oracle's restatement of that build -- see tests/_reduce_worker.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K", [8, 32, 64])
def test_reduce_formulation_matches_oracle(K):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_reduce_worker.py"), str(K)], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0 and "REDUCE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("variant", ["diag", "prop"])
@pytest.mark.parametrize("K", [8, 32, 64])
def test_reduce_formulation_variants(K, variant):
    """k_sample_prec with a prior variant on (it goes through deposit_column and reads prop_lambda / diag_only).
    diag: the diagonal-only precision against oracle.gibbs_reduce(no_covariance=True) at the worker's own bars, factors 1e-8 of
    the scale and RMSE 1e-9.  prop: per-column priors on both sides -- the oracle has no prec + prop entry, so the formulation is
    compared with the gather formulation under the same priors, GPU against GPU, at the 1e-8 the worker applies between the two
    formulations.  That is a weaker check than an oracle: a defect the two formulations share (deposit_column is common to
    k_sample_prec and the fused K <= 32 forms) would pass it; the gather form itself meets the oracle under per-column priors in
    tests/test_gpu_variant_forms.py.
    Observed on an MI355X (K = 8 | 32 | 64): diag against the oracle, factors 6.6e-16 | 1.1e-15 | 7.5e-16, RMSE 2.2e-15 | 1.1e-15 |
    1.8e-15 (and 1.6e-16 | 5.3e-16 | 3.8e-16 from the gather form); prop against the gather form 1.7e-15 | 3.4e-15 | 5.3e-15.  All six
    passed at the first run."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_reduce_worker.py"), str(K), "2", variant], capture_output=True,
                       text=True, timeout=600, env=env)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and ("REDUCE-OK K=%d alpha=2 variant=%s" % (K, variant)) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_reduce_rejects_fp32():
    import bpmf_amd
    import numpy as np
    eng = bpmf_amd.HipEngine(128, dtype="f32")
    cp = np.zeros(5, np.int64)
    a = eng.side_create(4, 4, cp, np.zeros(0, np.int32), np.zeros(0), 0.0)
    b = eng.side_create(4, 4, cp, np.zeros(0, np.int32), np.zeros(0), 0.0)
    with pytest.raises(Exception, match="fp64"):
        eng.sys_set_reduce(a, b, True)
    eng.side_destroy(a); eng.side_destroy(b); eng.close()
