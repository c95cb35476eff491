"""The column statistics pass restated: sum x, sum x x^T, sum |x|^2 in numpy.longdouble, and the bound that ANY fp64 evaluation of
these sums has to meet, whatever its order and whether its products are fused or not.

    |fl(sum_c t_c) - sum_c t_c| <= gamma_{N-1} sum_c |t_c|,   gamma_m = m u / (1 - m u),  u = 2^-53     (any order of the additions)

and a product x_ci x_cj that is rounded before it is added costs one more u of its magnitude.  With a margin of 64 for the product
roundings and the handful of extra additions of the finishers (partials of waves, quarters, slices):

    B_s  = (N + 64) u S1,   S1_i  = sum_c |x_ci|
    B_p  = (N + 64) u S2,   S2_ij = sum_c |x_ci x_cj|
    B_n  = sum_i B_p,ii                                  (norm is the sum of p's diagonal)

cov = (p - s s^T / N) / (N - 1) (bpmf_cov_from_sums, hyper.cpp) propagates these and adds its own four roundings:

    B_cov = [B_p + (|s_i| B_s,j + |s_j| B_s,i + B_s,i B_s,j) / N + 4 u (|p_ij| + |s_i s_j| / N)] / (N - 1)

The bounds are derived, not measured: nothing in here knows what a kernel returns.  (S2 is itself formed in fp64 and widened: a
sum of non-negative terms, relative error below (N + 1) u <= 1.2e-11, against the factor's own margin of 64 / N.)
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U = np.longdouble(2.0) ** -53
LD = np.longdouble


def sums(X):
    """X: [N, Kt] float64 (what get_items returned).  Returns dict(s, p, n, S1, S2) in longdouble; p, S2 symmetric, formed from the
    upper triangle by 16-row tile rows."""
    X = np.ascontiguousarray(X, np.float64)
    N, Kt = X.shape
    XL = X.astype(LD)
    s = XL.sum(0)
    S1 = np.abs(XL).sum(0)
    p = np.zeros((Kt, Kt), LD)

    def tile_row(i0):
        p[i0:i0 + 16, i0:] = XL[:, i0:i0 + 16].T @ XL[:, i0:]
    rows = list(range(0, Kt, 16))
    if N * Kt * Kt > 1 << 26 and len(rows) > 1:                       # (numpy's longdouble product is a plain loop that releases the GIL)
        with ThreadPoolExecutor(min(4, len(rows))) as pool:
            list(pool.map(tile_row, rows))
    else:
        for i0 in rows:
            tile_row(i0)
    iu = np.triu_indices(Kt, 1)
    p[(iu[1], iu[0])] = p[iu]                                         # (the diagonal tiles were formed in full: both halves agree)
    A = np.abs(X)
    S2 = (A.T @ A).astype(LD)
    n = np.diagonal(p).sum()
    return dict(s=s, p=p, n=n, S1=S1, S2=S2, N=N)


def bounds(ref):
    """(B_s [Kt], B_p [Kt, Kt], B_n) of a sums() result."""
    f = LD(ref["N"] + 64) * U
    Bp = f * ref["S2"]
    return f * ref["S1"], Bp, np.diagonal(Bp).sum()


def cov(ref):
    """(cov, B_cov) in longdouble for N >= 2: cov of bpmf_cov_from_sums from the exact sums, and its bound."""
    N = LD(ref["N"])
    s, p = ref["s"], ref["p"]
    Bs, Bp, _ = bounds(ref)
    c = (p - np.outer(s, s) / N) / (N - 1)
    a = np.abs(s)
    B = (Bp + (np.outer(a, Bs) + np.outer(Bs, a) + np.outer(Bs, Bs)) / N + 4 * U * (np.abs(p) + np.outer(a, a) / N)) / (N - 1)
    return c, B


def ratios(s, p, n, ref):
    """Worst |error| / bound of (s, p's upper triangle, n) against a sums() result; a zero bound with a zero error counts as 0."""
    Bs, Bp, Bn = bounds(ref)
    iu = np.triu_indices(len(Bs))

    def worst(err, B):
        err, B = np.atleast_1d(err), np.atleast_1d(B)
        out = np.zeros(err.shape, LD)
        nz = B > 0
        out[nz] = err[nz] / B[nz]
        out[~nz & (err > 0)] = np.inf
        return float(out.max())
    return (worst(np.abs(np.asarray(s, LD) - ref["s"]), Bs), worst(np.abs(np.asarray(p, LD) - ref["p"])[iu], Bp[iu]),
            worst(abs(LD(n) - ref["n"]), Bn))


def geometry(N, Kdev, num_cu=256):
    """The pass's slicing as build_schedule (capi_side.hip) sets it for N local columns on the kernels of size Kdev: (form, units,
    waves, per, empty).  Used by the host test only; on the device bpmf_hip_side_stat_info is the authority."""
    if Kdev == 128:
        form, units = "tiles", max(1, min((N + 63) // 64, 32))
        waves = units
    else:
        waves = max(1, min((N + 31) // 32, num_cu * (8 if N > 100000 else 2)))
        if N < 20000:
            waves = max(1, min(waves, max((N + 159) // 160, 24)))
        form, units = "waves", waves
        if N > 100000:
            form, units = "workgroups", min((N + 127) // 128, num_cu * 2)
            waves = 4 * units
    per = (-(-N // waves) + 3) // 4 * 4
    empty = sum(1 for w in range(waves) if w * per >= N)
    return form, units, waves, per, empty


def sliced_sums(X, waves, per, group=1, mutate=None):
    """fp64 sums formed as the pass forms them: wave w takes the columns [w per, (w + 1) per) in trips of 8, `group` waves add up to
    one partial (4 in the workgroup form), the partials are added afterwards.  mutate = (kind, w): "column" drops the first column
    of wave w, "trip" drops its last trip (the partial one if it has one), "fp32" keeps the partial that holds wave w in fp32."""
    X = np.ascontiguousarray(X, np.float64)
    N, Kt = X.shape
    kind, mw = mutate if mutate else (None, -1)
    parts = []
    for w in range(waves):
        b, e = min(w * per, N), min((w + 1) * per, N)
        if w == mw and kind == "column":
            b += 1
        if w == mw and kind == "trip" and e > b:
            e = b + (e - b - 1) // 8 * 8
        s, p = np.zeros(Kt), np.zeros((Kt, Kt))
        for c in range(b, e, 8):
            Y = X[c:min(c + 8, e)]
            s += Y.sum(0)
            p += Y.T @ Y
        parts.append((s, p))
    s, p = np.zeros(Kt), np.zeros((Kt, Kt))
    for g in range(0, waves, group):
        gs, gp = np.zeros(Kt), np.zeros((Kt, Kt))
        for q in parts[g:g + group]:
            gs += q[0]; gp += q[1]
        if kind == "fp32" and g <= mw < g + group:
            gs, gp = gs.astype(np.float32).astype(np.float64), gp.astype(np.float32).astype(np.float64)
        s += gs; p += gp
    return s, p, float(np.diagonal(p).sum())
