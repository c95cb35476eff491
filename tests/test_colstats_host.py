"""The net of tests/test_gpu_colstats.py, shown to hold before any GPU is involved (tests/colstats_ref.py: the longdouble sums and
the bound every fp64 evaluation of them meets).

For N in {1, 5, 33, 769, 2049, 100 001} and Kt in {8, 20, 64, 128}: fp64 sums formed wave by wave with the pass's own slicing (per =
roundup4(ceil(N / waves)), trips of 8 columns, partials added afterwards; four waves per partial in the workgroup form) are inside the
bound -- and the same sums with one column dropped, with the last (partial) trip of one wave dropped, or with one partial kept in
fp32 are outside it in at least one element.  Worst error / bound of the correct sums over all cases: 0.038 (N = 5; up to N = 33 the
64 of the bound's factor is most of it), 1.8e-4 at N = 100 001.  Other orders of the same sums (strictly sequential, numpy's own) and
cov through bpmf_cov_from_sums against B_cov are checked too.  The longdouble references of the 100 001-column cases take 2.5 s (Kt =
64) and 4.5 s (Kt = 128) on four host threads, the file about 15 s.
"""
import numpy as np
import pytest

from tests import colstats_ref as R

NS = (1, 5, 33, 769, 2049, 100001)
KTS = (8, 20, 64, 128)
_CACHE = {}


def _kdev(Kt):
    return next(k for k in (8, 16, 32, 64, 128) if k >= Kt)


def _case(N, Kt):
    """(X, longdouble reference): factor-like columns, means of order 1, not representable in fp32.  Computed once, never written."""
    if (N, Kt) not in _CACHE:
        rng = np.random.default_rng(1000 * Kt + N % 997)
        X = rng.standard_normal(Kt) + 0.7 * rng.standard_normal((N, Kt))
        X.setflags(write=False)
        _CACHE[(N, Kt)] = (X, R.sums(X))
    return _CACHE[(N, Kt)]


def test_geometry_is_the_one_the_cases_are_named_for():
    """769 and 20 000 columns leave two and twelve waves of k_colstats without columns, 2049 one slice of the tile form, 100 001
    takes the workgroup form; 3840 -> 3841 is the step from 24 to 25 waves."""
    assert R.geometry(769, 16) == ("waves", 24, 24, 36, 2)
    assert R.geometry(768, 16)[4] == 0
    assert R.geometry(20000, 8) == ("waves", 512, 512, 40, 12)
    assert R.geometry(19999, 8)[4] == 0
    assert R.geometry(3840, 32)[:4] == ("waves", 24, 24, 160) and R.geometry(3841, 32)[:4] == ("waves", 25, 25, 156)
    assert R.geometry(2049, 128) == ("tiles", 32, 32, 68, 1) and R.geometry(2048, 128) == ("tiles", 32, 32, 64, 0)
    assert R.geometry(100000, 8)[:2] == ("waves", 512)
    assert R.geometry(100001, 8) == ("workgroups", 512, 2048, 52, 124)
    for N in range(1, 10):
        assert R.geometry(N, 64)[:2] == ("waves", 1) and R.geometry(N, 128)[:2] == ("tiles", 1)


@pytest.mark.parametrize("Kt", KTS)
@pytest.mark.parametrize("N", NS)
def test_the_bound_holds_for_sliced_fp64_sums_and_catches_three_defects(N, Kt):
    X, ref = _case(N, Kt)
    form, units, waves, per, empty = R.geometry(N, _kdev(Kt))
    group = 4 if form == "workgroups" else 1
    good = R.ratios(*R.sliced_sums(X, waves, per, group), ref)
    print("colstats-host N=%d Kt=%d %s x %d per %d empty %d: error / bound  s %.2e  p %.2e  n %.2e" % ((N, Kt, form, units, per, empty) + good))
    assert max(good) <= 1.0
    s, p, n = R.sliced_sums(X, waves, per, group)
    assert np.array_equal(p, p.T)
    # the defects sit in the last wave that has columns (its last trip is the partial one whenever the side has one)
    w = min(waves - 1 - empty, (N - 1) // per)
    assert w * per < N
    for kind in ("column", "trip", "fp32"):
        bad = R.ratios(*R.sliced_sums(X, waves, per, group, (kind, w)), ref)
        print("colstats-host N=%d Kt=%d with %-6s: error / bound  s %.2e  p %.2e  n %.2e" % ((N, Kt, kind) + bad))
        assert max(bad) > 1.0, kind


@pytest.mark.parametrize("N,Kt", [(2, 8), (33, 20), (769, 64), (20000, 8), (100001, 8)])
def test_sequential_and_numpy_sums_stay_far_inside(N, Kt):
    """Other orders of the same sums: strictly sequential, and numpy's own.  The worst case of N terms is (N - 1) u S against the
    bound's (N + 64) u S, rounding errors that do not conspire give about sqrt(N) u S: both stay far inside (worst seen here 0.046
    at N = 33, 6e-4 at N = 100 001)."""
    X, ref = _case(N, Kt)
    s, p = np.zeros(Kt), np.zeros((Kt, Kt))
    for x in X:
        s += x
        p += np.outer(x, x)
    seq = R.ratios(s, p, float(np.sum(np.diagonal(p))), ref)
    own = R.ratios(X.sum(0), X.T @ X, float((X * X).sum()), ref)
    print("colstats-host N=%d Kt=%d: sequential %.2e %.2e %.2e   numpy %.2e %.2e %.2e" % ((N, Kt) + seq + own))
    assert max(seq) <= 1.0 and max(own) <= 1.0


@pytest.mark.parametrize("N,shift", [(2, 0.0), (33, 1.0), (769, 100.0), (20000, 100.0)])
def test_cov_bound(N, shift):
    """cov through bpmf_cov_from_sums from sequential fp64 sums stays inside B_cov with column means up to 100; the same from sums
    with one column dropped does not."""
    from bpmf_amd import engine
    Kt = 16
    rng = np.random.default_rng(N)
    X = shift * rng.standard_normal(Kt) + rng.standard_normal((N, Kt))
    ref = R.sums(X)
    c_ref, B = R.cov(ref)
    s, p = np.zeros(Kt), np.zeros((Kt, Kt))
    for x in X:
        s += x
        p += np.outer(x, x)
    c = engine.cov_from_sums(Kt, N, s, p)
    worst = float((np.abs(np.asarray(c, R.LD) - c_ref) / B).max())
    print("colstats-host cov N=%d means x %g: error / bound %.2e" % (N, shift, worst))
    assert worst <= 1.0
    c = engine.cov_from_sums(Kt, N, s - X[0], p - np.outer(X[0], X[0]))
    assert float((np.abs(np.asarray(c, R.LD) - c_ref) / B).max()) > 1.0


def test_stat_info_is_exported_bound_and_checks_its_arguments():
    """bpmf_hip_side_stat_info: declared in the header, exported, bound with its signature, and refusing a NULL side or fewer than
    eight words without touching a device."""
    import ctypes as C
    import os
    import bpmf_amd
    from bpmf_amd import _lib
    from tests.conftest import ROOT
    assert "bpmf_hip_side_stat_info" in open(os.path.join(ROOT, "include", "bpmf_hip.h")).read()
    assert "bpmf_hip_side_stat_info" in _lib.exported_signatures()
    lib = bpmf_amd.load_library()
    out = np.full(8, -7, np.int64)
    assert lib.bpmf_hip_side_stat_info(None, out.ctypes.data_as(C.c_void_p), 8) == -1
    assert b"side_stat_info" in lib.bpmf_hip_last_error()
    assert np.all(out == -7)

