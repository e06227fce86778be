"""Extended-precision host restatement of the posterior draws (csrc/sample.cpp, kernels_sample.hip): the
instrument test_gpu_sample.py measures k_draw, the sample paths and the per-draw extremum with, and
test_sample_host.py proves against 50-digit arithmetic and shows which failures it can see.

np.longdouble and NumPy only, in the style of posterior_ref.py / design_ref.py; B and its conditioning bB
come from extended_ref.ExtendedRef.  With H = L L^T (posterior_ref.cholesky_ld), theta the posterior mean
and Z the p x S normals the caller supplies:

    Theta = theta 1^T + L^-T Z      by back substitution (backward_ld), no inverse formed
    path  = B Theta                 m x S
    per draw s the eligible row with the smallest (maximize: largest) path value, first among equals; a row
    is eligible when it is not skipped, all its coordinates are finite and its value is finite.

Tolerances follow the project's rule |got - want| <= C x (number of summands) x (magnitudes):

  Theta_ks   p - k + 2 summands (the p - k products X_kj z_js, j >= k, of the upper triangular X = L^-T, theta
             and one for the rounding of X_kj itself) of magnitude |theta_k| + sum_j |X_kj| |z_js|; plus the
             backward error of the float64 factorisation, L^ L^^T = H + dH with |dH| <= gamma(p + 1) |L| |L|^T
             (Higham, theorem 10.3, as posterior_ref carries it) carried to first order through
             dL = L tril(L^-1 dH L^-T) and d(L^-T z) = -L^-T dL^T L^-T z:
             (p + 1) |X| (|L| tril(|L^-1| |L| |L|^T |L^-T|))^T |X z|, and the inversion of the computed factor,
             p |X| |L|^T |X| |z|.
  path_is    p summands of magnitude sum_k |B_ik| |Theta_ks|, plus bB_i . |Theta_s| (the magnitudes inside the
             knot sums of b_i), plus |B_i| . bound(Theta_s).

The unit roundoff is carried by C.  C is never a constant of this module and never measured from the device:
every test measures the float64 host restatement on the same case (host64: NumPy Cholesky, a float64
triangular solve, the float64 oracle's B) and takes extended_ref.constant_from_oracle_ratio of its worst
err / bound: eight times it, at most extended_ref.C_CAP = 2e-13.
"""
import numpy as np

import extended_ref as E
import posterior_ref as P
from extended_ref import ld


def _f64(a):
    return np.asarray(a, dtype=np.float64)


class Case:
    pass


def backward_ld(L, R):
    """inv(L^T) R by back substitution, long double; R is p x S"""
    E.require_extended()
    L, R = np.asarray(L, dtype=ld), np.asarray(R, dtype=ld)
    p = L.shape[0]
    T = np.empty(R.shape, dtype=ld)
    for k in range(p - 1, -1, -1):
        T[k] = (R[k] - L[k + 1:, k] @ T[k + 1:]) / L[k, k]
    return T


def ref_draw(H, theta, Z):
    """(L, Theta, bound of a float64 Theta without C)"""
    p = len(theta)
    L = P.cholesky_ld(H)
    T = backward_ld(L, Z)
    Theta = np.asarray(theta, dtype=ld)[:, None] + T
    L64 = _f64(L)
    aW, aL, aZ = np.abs(P.inverse64(L64)), np.abs(L64), np.abs(_f64(Z))
    aX = aW.T
    mag = np.abs(_f64(theta))[:, None] + aX @ aZ
    nsum = (p - np.arange(p) + 2.0)[:, None]
    dL = aL @ np.tril(aW @ (aL @ aL.T) @ aW.T)
    back = (p + 1) * (aX @ (dL.T @ np.abs(_f64(T)))) + p * (aX @ (aL.T @ (aX @ aZ)))
    return L, Theta, nsum * mag + back


def ref_paths(B, bB, Theta, bTheta):
    """(path, bound of a float64 path without C)"""
    p = B.shape[1]
    aB, aT = np.abs(_f64(B)), np.abs(_f64(Theta))
    return B @ Theta, p * (aB @ aT) + _f64(bB) @ aT + aB @ bTheta


def make_case(om_o, terms, H, theta, Z, x, skip=None):
    """everything the tests need of one problem; H, theta, Z float64 (taken as exact)"""
    import ob_oracle as O
    E.require_extended()
    c = Case()
    knots = [np.asarray(om_o.knots_of(k), dtype=np.float64) for k in range(om_o.d)]
    c.terms, c.H, c.theta, c.Z, c.x = terms, _f64(H), _f64(theta), np.asfortranarray(_f64(Z)), x
    c.p, c.S, c.m = len(terms), Z.shape[1], len(x)
    assert c.H.shape == (c.p, c.p) and c.theta.shape == (c.p,) and Z.shape[0] == c.p
    c.skip = np.zeros(c.m, dtype=np.uint8) if skip is None else np.asarray(skip, dtype=np.uint8)
    c.finite = np.all(np.isfinite(x), axis=1)
    xs = np.where(np.isfinite(x), x, 0.5)                          # a row that is not finite: never eligible
    c.B, c.bB = E.ExtendedRef(om_o.kinds, knots, om_o.hyp, om_o.rotmat, xs).getmat(terms)
    c.Bo = O.ob_getmat(O.OuterBase(om_o, xs), terms)
    c.L, c.Theta, c.bTheta = ref_draw(c.H, c.theta, c.Z)
    c.path, c.bpath = ref_paths(c.B, c.bB, c.Theta, c.bTheta)
    c.elig = c.finite & (c.skip == 0)
    return c


# ---- the per-draw optimum -----------------------------------------------------------------------------
def extremum(path, elig, maximize=False, mutate=None):
    """(index (S, int64; -1: no eligible row), value (S; NaN)) of the columns of path over the rows with
    elig, first among equals.  mutate: "maximize ignored", "highest index on a tie", "skip ignored" (the caller
    passes the rows' finiteness as elig2), "nan wins" -- the failures test_sample_host.py stages."""
    path = np.asarray(path)
    m, S = path.shape
    index, value = np.full(S, -1, dtype=np.int64), np.full(S, np.nan, dtype=path.dtype)
    sgn = -1 if (maximize and mutate != "maximize ignored") else 1
    for s in range(S):
        v = path[:, s]
        fin = np.isfinite(_f64(v))
        if mutate == "nan wins":
            key = np.where(fin, sgn * v, -np.inf)
            ok = np.asarray(elig).copy()
        else:
            key, ok = sgn * v, elig & fin
        if not np.any(ok):
            continue
        key = np.where(ok, key, np.inf)
        best = key.min()
        hits = np.nonzero(ok & (key == best))[0]
        j = int(hits[-1] if mutate == "highest index on a tie" else hits[0])
        index[s], value[s] = j, v[j]
    return index, value


def gap_ratio(c, C, maximize=False, drop=()):
    """smallest (runner-up - best) / (C x (their two bounds)) over the draws, on the reference alone; drop: rows
    left out of the comparison (the deliberate twins); inf when a draw has fewer than two eligible rows"""
    worst = np.inf
    ok = c.elig.copy()
    ok[list(drop)] = False
    sgn = -1 if maximize else 1
    for s in range(c.S):
        v = c.path[:, s]
        idx = np.nonzero(ok & np.isfinite(_f64(v)))[0]
        if len(idx) < 2:
            continue
        key = sgn * v[idx]
        o = np.argsort(_f64(key), kind="stable")[:2]
        gap = float(key[o[1]] - key[o[0]])
        worst = min(worst, gap / (C * (c.bpath[idx[o[0]], s] + c.bpath[idx[o[1]], s])))
    return worst


# ---- the float64 restatement --------------------------------------------------------------------------
def host64(c, mutate=None):
    """(Theta, path) in NumPy float64: LAPACK Cholesky, a float64 triangular solve, the float64 oracle's B.
    mutate: "inverse not transposed" (L^-1 z: the right marginal size, the wrong covariance), "theta dropped"."""
    L = np.linalg.cholesky(c.H)
    T = np.linalg.solve(L, c.Z) if mutate == "inverse not transposed" else np.linalg.solve(L.T, c.Z)
    Theta = T if mutate == "theta dropped" else c.theta[:, None] + T
    return Theta, c.Bo @ Theta


def ratios(c, Theta=None, path=None, C=1.0):
    """{quantity: worst |got - want| / (C x bound)}; rows that are not finite are left out of path"""
    out = {}
    if Theta is not None:
        out["theta"] = E.worst_ratio(Theta, c.Theta, C * c.bTheta)
    if path is not None:
        f = c.finite
        out["path"] = E.worst_ratio(_f64(path)[f], c.path[f], C * c.bpath[f])
    return out


def constant_of(c):
    """(C, r): r = the float64 restatement's own worst err / bound on the case"""
    Theta, path = host64(c)
    r = max(ratios(c, Theta, path).values())
    return E.constant_from_oracle_ratio(r), r


def value_ratio(c, index, value, C):
    """worst |value_s - path[index_s, s]| / (C x bound) over the draws with a pick"""
    s = np.nonzero(np.asarray(index) >= 0)[0]
    if not len(s):
        return 0.0
    j = np.asarray(index)[s]
    return E.worst_ratio(_f64(value)[s], c.path[j, s], C * c.bpath[j, s])


# ---- the cases both test files share ------------------------------------------------------------------
THETA_SCALE = 0.001  # a mean of the size of the draws' spread |L^-T z| in these cases: the optimum moves from draw to draw


def seeded_case(om_o, terms, m, S, seed, x=None, skip=None, theta=None, Z=None):
    """H of design_ref.hessian_of; theta, Z and the rows from np.random.default_rng(seed)"""
    import design_ref as D
    from conftest import sample_x
    rng = np.random.default_rng(seed)
    p = len(terms)
    H, _ = D.hessian_of(om_o, terms, seed + 1)
    th = THETA_SCALE * rng.standard_normal(p)
    z = rng.standard_normal((p, S))
    xs = sample_x(rng, m, om_o.kinds)
    return make_case(om_o, terms, H, th if theta is None else theta, z if Z is None else Z, xs if x is None else x, skip)


# (model, p, m, S, seed): p = 5 (one partial 4-term step), 67, 130; S = 1, 15, 16, 17 around a 16-column block,
# 65 (second pass of the 64-draw chunk of draw, sample and the unfused route) and 129 (second pass of the fused
# kernel's 128 draws); m = 1, 63, 64, 65, 129 around the 64-row tile and 1000
SHAPES = [("d3", 5, 1, 1, 61), ("d3", 5, 63, 15, 62), ("d3", 5, 64, 16, 63), ("d8", 67, 65, 17, 64),
          ("d8", 67, 129, 65, 65), ("d8", 67, 64, 1, 66), ("d5", 130, 129, 17, 67), ("d5", 130, 1000, 65, 68),
          ("d5", 130, 63, 16, 69), ("d5", 130, 65, 15, 70), ("d8", 67, 65, 129, 73)]
WIDE = ("wide", 0, 65, 17, 71)
SEMANTICS = ("d5", 130, 129, 17, 72)
