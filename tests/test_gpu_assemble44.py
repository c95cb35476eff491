"""assemble44<K> (bpmf_amd/csrc/kernels.h) on its own: the LDS images it leaves, bit for bit.

assemble44 is the hand-over between the 4x4x4 Gram of k_sample1 / k_sample1i / k_sample1w and the factorisation: every lane
(i, b, j) = (lane / 16, lane / 4 % 4, lane % 4) holds, per block (g, g2) of the Gram, the contribution of its b to the entry
(idx(g, i), idx(g2, j)), and per group g its share of the rhs sum idx(g, j).  The four b are added as
(x_b + x_{b^2}) + (x_{b^1} + x_{b^3}), the rhs sums then over the four i as (t_i + t_{i^1}) + the same of i ^ 2, and the totals
go into the symmetric K x LD matrix sA (diagonal blocks as they are, the others mirrored) and into sb.  K = 32 does this with a
packed reduce-scatter, K = 8 and 16 in every lane: the bits must not depend on which.

tools/probes/assemble44_probe.hip runs the function in one wave on inputs from a file; the expected image is computed here in
numpy (IEEE double additions in the order above).  The inputs, normal(0, 1) * exp(normal(0, 3)), span many binades, so that
another association of the four-term sums changes the bits of a good share of the totals -- asserted below, so that a wrong
order cannot pass.  sA's two padding columns (LD = K + 2) are nobody's to write and are not compared.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

KS = (8, 16, 32)
_CACHE = {}


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def _idx(g, x):
    return 8 * (g >> 1) + 2 * x + (g & 1)                            # Geo44<K>::idx (args.h)


def _inputs():
    """K -> (NB + NG) x 64 doubles, register-major: one generator, drawn once, never written."""
    if "in" not in _CACHE:
        rng = np.random.default_rng(44)
        out = {}
        for K in KS:
            ng = K // 4
            shape = (ng * (ng + 1) // 2 + ng, 64)
            x = rng.normal(0.0, 1.0, shape) * np.exp(rng.normal(0.0, 3.0, shape))
            x.setflags(write=False)
            out[K] = x
        _CACHE["in"] = out
    return _CACHE["in"]


def _bank_totals(x):
    """(T, 64) -> (T, i, j): the four b added as (x_b + x_{b^2}) + (x_{b^1} + x_{b^3}), and under two other associations."""
    v = x.reshape(-1, 4, 4, 4)                                       # lane = 16 i + 4 b + j
    want = (v[:, :, 0] + v[:, :, 2]) + (v[:, :, 1] + v[:, :, 3])
    pairs = (v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])
    left = ((v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]) + v[:, :, 3]
    return want, pairs, left


def _expected(K, x):
    """(sA[:, :K], sb) as assemble44 must leave them"""
    ng = K // 4
    nb = ng * (ng + 1) // 2
    tot = _bank_totals(x)[0]
    sA = np.zeros((K, K))
    ii = np.arange(4)
    t = 0
    for g in range(ng):
        for g2 in range(g, ng):
            r, c = _idx(g, ii), _idx(g2, ii)
            sA[np.ix_(r, c)] = tot[t]
            if g2 > g:
                sA[np.ix_(c, r)] = tot[t].T
            t += 1
    assert t == nb
    sb = np.zeros(K)
    for g in range(ng):
        p = tot[nb + g]                                              # (i, j)
        sb[_idx(g, ii)] = (p[0] + p[1]) + (p[2] + p[3])
    return sA, sb


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("assemble44")
    exe = str(d / "assemble44_probe")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=on", "-mllvm", "-pragma-unroll-threshold=4000000",
                           "-I", os.path.join(ROOT, "bpmf_amd", "csrc"), os.path.join(ROOT, "tools", "probes", "assemble44_probe.hip"), "-o", exe])
    return exe, d


@pytest.mark.parametrize("K", KS)
def test_another_association_would_change_the_bits(K):
    want, pairs, left = _bank_totals(_inputs()[K])
    share_pairs = np.mean(want.view(np.uint64) != pairs.view(np.uint64))
    share_left = np.mean(want.view(np.uint64) != left.view(np.uint64))
    print("K %d: %.3f of the totals change bits under (x0 + x1) + (x2 + x3), %.3f left to right" % (K, share_pairs, share_left))
    assert share_pairs >= 0.2 and share_left >= 0.2


@pytest.mark.parametrize("K", KS)
def test_lds_images_bit_for_bit(probe, K):
    exe, d = probe
    x = _inputs()[K]
    fin, fout = str(d / ("in%d.bin" % K)), str(d / ("out%d.bin" % K))
    x.tofile(fin)
    r = subprocess.run([exe, str(K), fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    LD = K + 2
    img = np.fromfile(fout, np.float64)
    assert img.shape == (K * LD + K,)
    sA, sb = img[:K * LD].reshape(K, LD)[:, :K], img[K * LD:]
    wantA, wantb = _expected(K, x)
    badA = np.argwhere(np.ascontiguousarray(sA).view(np.uint64) != wantA.view(np.uint64))
    badb = np.flatnonzero(sb.view(np.uint64) != wantb.view(np.uint64))
    print("K %d: %d of %d entries of sA and %d of %d of sb differ in bits" % (K, len(badA), K * K, len(badb), K))
    assert len(badA) == 0, "sA differs first at %s: %r, expected %r" % (badA[0], sA[tuple(badA[0])], wantA[tuple(badA[0])])
    assert len(badb) == 0, "sb differs first at %d: %r, expected %r" % (badb[0], sb[badb[0]], wantb[badb[0]])
