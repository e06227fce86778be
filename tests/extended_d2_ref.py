"""Extended-precision reference of the design matrix's SECOND derivatives by the inputs and of the
Hessian-vector and Jacobian-vector products of the multi-response predictor taken from them -- the
instrument of test_predict_hvp_host.py (which proves it) and test_gpu_predict_hvp.py (which uses it).
extended_ref and extended_dx_ref are imported unchanged; the rules are theirs.

Per dimension l, with K'' = d2K / dx_l^2 (d2cov_dx2_ld), R = K rot, s = R[:, 0]:

    second-derivative factor  g2_l[:, c] = (K'' rot)[:, c] / s     bound (|K''| |rot| + |g2_l| bs) / |s|

(column 0 included: g2_l[:, 0] = kappa_l).  d2B / dx_l dx_m is B with the level factors of l and m
replaced by g_l and g_m (l != m) or the factor of l by g2_l (l = m), with the first-order bound of
that product (getmat_d2).  For a direction v per row (the rows of V) and coefficients Theta (p x q)

    hv[i, l, j] = sum_m v_im sum_k d2B[i, k, l, m] Theta[k, j]
    jv[i, j]    = sum_l v_il sum_k  dB[i, k, l]    Theta[k, j]

are held to C . (sum_m |v_m| bound_lm @ |Theta|) + gamma_{p d + d} . (sum_m |v_m| |d2B_lm| @ |Theta|)
(the sum has p d summands, each with one more rounded factor v_m), and the contraction with the
weights W to sum_j |W_ij| tol_ilj + gamma_q sum_j |W_ij hv_ilj|: extended_jac_ref.ref_vjp's rule.

The float64 side that C is measured from is NOT the unnormalised product above but a plain NumPy
restatement of the normalised algebra the kernel uses (include/obhip.h at
obhip_predict_hvp_multi_dev; NormBasis, hv_terms_norm): r, r', r'', rho, kappa, prefix-free products
of the level factors.  C = 8 x its own max(err / bound) over the per-(row, term, dimension) entries
therefore reflects what that algebra cancels (kappa_l - rho_l^2, the three-term r''), and is capped
at extended_ref.C_CAP; test_predict_hvp_host.py asserts that it stays strictly below the cap on
every case of the GPU file, so the instrument is known to hold the reference's own form.
"""
import numpy as np

import extended_dx_ref as X
import extended_jac_ref as J
import extended_ref as E

ld = np.longdouble


def _cov012(kind, x, kn, hyp, dt):
    """(K, dK/dx, d2K/dx2) of one dimension, n x m, in the arithmetic dt throughout"""
    x, kn, hyp = np.asarray(x, dtype=dt), np.asarray(kn, dtype=dt), np.asarray(hyp, dtype=dt)
    third = dt(1) / 3
    if kind in ("mat25", "mat25pow"):
        if kind == "mat25":
            els = np.exp(2 * hyp[0])
            t1, t2 = x / els, kn / els
            du, d2u = np.ones_like(x) / els, np.zeros_like(x)
        else:
            powv, els = np.exp(dt(0.25) * hyp[1]), np.exp(2 * hyp[0] + dt(0.25) * hyp[1])
            t1, t2 = np.power(x, powv) / els, np.power(kn, powv) / els
            du, d2u = powv * t1 / x, powv * (powv - 1) * t1 / (x * x)
        h = t1[:, None] - t2[None, :]
        ah = np.abs(h)
        e = np.exp(-ah)
        k1 = -third * (h * (1 + ah) * e)
        k2 = -third * ((1 + ah - h * h) * e)
        return (1 + ah + ah * ah * third) * e, k1 * du[:, None], k2 * (du * du)[:, None] + k1 * d2u[:, None]
    if kind == "mat25ang":
        es, ec = np.exp(2 * hyp[0]), np.exp(2 * hyp[1])
        sn, cs = np.sin(x), np.cos(x)
        hs = (sn / es)[:, None] - (np.sin(kn) / es)[None, :]
        hc = (cs / ec)[:, None] - (np.cos(kn) / ec)[None, :]
        h = np.sqrt(hs * hs + hc * hc)
        e = np.exp(-h)
        cx, sx = (cs / es)[:, None], (sn / ec)[:, None]
        q = hs * cx - hc * sx
        qp = cx * cx + sx * sx - hs * (sn / es)[:, None] - hc * (cs / ec)[:, None]
        return (1 + h + h * h * third) * e, -third * ((1 + h) * e) * q, -third * e * ((1 + h) * qp - q * q)
    raise ValueError("unknown covariance " + str(kind))


def d2cov_dx2_ld(kind, x, kn, hyp):
    """d2K / dx2 of one dimension, n x m, long double throughout"""
    return _cov012(kind, x, kn, hyp, ld)[2]


class ExtendedRefD2(X.ExtendedRefDx):
    """ExtendedRefDx with the second-derivative factors g2[l], bg2[l] by the inputs"""

    def __init__(self, kinds, knots, hyp, rot, x):
        super().__init__(kinds, knots, hyp, rot, x)
        x = np.asarray(x, dtype=np.float64)
        hyp = np.asarray(hyp, dtype=np.float64)
        self.g2, self.bg2 = [], []
        for k in range(self.d):
            m, o = len(knots[k]), int(self.knotptst[k])
            rk = np.asarray(rot[:m, o:o + m], dtype=ld)
            K2 = d2cov_dx2_ld(self.kinds[k], x[:, k], knots[k], hyp[self.hypst[k]:self.hypst[k + 1]])
            T, bT = K2 @ rk, np.abs(K2) @ np.abs(rk)
            s = self.s[k]
            g2 = T / s[:, None]
            self.g2.append(g2)
            self.bg2.append((bT + np.abs(g2) * self.bs[k][:, None]) / np.abs(s)[:, None])

    def getmat_d2(self, terms, l, m):
        """(d2B / dx_l dx_m, bound), n x p: the product with the factors of l and m replaced"""
        terms = np.asarray(terms, dtype=np.int64)
        assert terms.ndim == 2 and terms.shape[1] == self.d
        p = terms.shape[0]
        P0, S0 = self._scale()
        P = np.repeat(P0[:, None], p, axis=1)
        S = np.repeat(S0[:, None], p, axis=1)
        for k in range(self.d):
            lev = terms[:, k]
            if k == l and k == m:
                P, S = self._times(P, S, self.g2[k][:, lev], self.bg2[k][:, lev])
            elif k == l or k == m:
                P, S = self._times(P, S, self.g[k][:, lev], self.bg[k][:, lev])
            else:
                idx = np.nonzero(lev > 0)[0]
                if len(idx):
                    P[:, idx], S[:, idx] = self._times(P[:, idx], S[:, idx], self.r[k][:, lev[idx]],
                                                       self.br[k][:, lev[idx]])
        return P, S

    def hv_terms(self, terms, V):
        """per (row, term, dimension l): T = sum_m v_m d2B_lm, its bound sum_m |v_m| bound_lm and
        sum_m |v_m d2B_lm|; three n x p x d arrays (long double, float64, float64).  d2B_lm = d2B_ml
        is formed once per pair."""
        V = np.asarray(V, dtype=np.float64)
        n, p, d = self.n, len(terms), self.d
        T = np.zeros((n, p, d), dtype=ld)
        bT, aT = np.zeros((n, p, d)), np.zeros((n, p, d))
        Vl, aV = np.asarray(V, dtype=ld), np.abs(V)
        for l in range(d):
            for m in range(l, d):
                if not (np.any(V[:, m]) or np.any(V[:, l])):
                    continue
                D, bD = self.getmat_d2(terms, l, m)
                bD, aD = E._f64(bD), np.abs(E._f64(D))
                for a, b in ((l, m),) if l == m else ((l, m), (m, l)):
                    T[:, :, a] += Vl[:, b:b + 1] * D
                    bT[:, :, a] += aV[:, b:b + 1] * bD
                    aT[:, :, a] += aV[:, b:b + 1] * aD
        return T, bT, aT

    def jv_terms(self, terms, V):
        """per (row, term): sum_l v_l dB_l with its bound and the sum of magnitudes, n x p each"""
        V = np.asarray(V, dtype=np.float64)
        T = np.zeros((self.n, len(terms)), dtype=ld)
        bT, aT = np.zeros(T.shape), np.zeros(T.shape)
        for l in range(self.d):
            D, bD = self.getmat_dx(terms, l)
            T += np.asarray(V[:, l:l + 1], dtype=ld) * D
            bT += np.abs(V[:, l:l + 1]) * E._f64(bD)
            aT += np.abs(V[:, l:l + 1]) * np.abs(E._f64(D))
        return T, bT, aT


def reference_d2_of(om, x):
    """ExtendedRefD2 of an oracle model (ob_oracle.OuterMod) on the rows x"""
    return ExtendedRefD2(om.kinds, [om.knots_of(k) for k in range(om.d)], om.hyp, om.rotmat, x)


def ref_hv(hvt, Theta, C):
    """(hv, tolerance), n x d x q each, from ExtendedRefD2.hv_terms' triple"""
    T, bT, aT = hvt
    Th = np.asarray(Theta, dtype=ld)
    aTh = np.abs(E._f64(Th))
    n, p, d = T.shape
    want = np.stack([T[:, :, l] @ Th for l in range(d)], axis=1)
    tol = np.stack([E._sum_tol(C, bT[:, :, l] @ aTh, p * d + d, aT[:, :, l] @ aTh) for l in range(d)], axis=1)
    return want, tol


def ref_hvp(hvt, Theta, W, C):
    """(hvp, tolerance), n x d each: ref_hv contracted with the float64 weights W (n x q) by ref_vjp's rule"""
    return J.ref_vjp(*ref_hv(hvt, Theta, C), W)


def ref_jvp(jvt, Theta, C, d):
    """(jvp, tolerance), n x q each, from ExtendedRefD2.jv_terms' triple"""
    T, bT, aT = jvt
    Th = np.asarray(Theta, dtype=ld)
    aTh = np.abs(E._f64(Th))
    return T @ Th, E._sum_tol(C, bT @ aTh, T.shape[1] * d + d, aT @ aTh)


# -- the normalised algebra of the kernel, in any arithmetic ------------------------------------------
class NormBasis:
    """s, rho_l, kappa_l and per dimension r, r', r'' (n x m_l, column 0 unused) in the arithmetic dt,
    by the formulas of include/obhip.h.  mutate: "r2" takes r'' without the 2 r' R'_0 term."""

    def __init__(self, kinds, knots, hyp, rot, x, dt, mutate=None):
        x = np.asarray(x, dtype=np.float64)
        hyp = np.asarray(hyp, dtype=np.float64)
        self.d, self.n, self.dt = len(kinds), x.shape[0], dt
        m = [len(k) for k in knots]
        kst = np.concatenate([[0], np.cumsum(m)])
        hst = np.concatenate([[0], np.cumsum([E.NUMHYP[k] for k in kinds])])
        self.s = np.ones(self.n, dtype=dt)
        self.rho, self.kappa, self.r, self.r1, self.r2 = [], [], [], [], []
        for k in range(self.d):
            rk = np.asarray(rot[:m[k], kst[k]:kst[k] + m[k]], dtype=dt)
            K, K1, K2 = _cov012(kinds[k], x[:, k], knots[k], hyp[hst[k]:hst[k + 1]], dt)
            R, R1, R2 = K @ rk, K1 @ rk, K2 @ rk
            s0, d0, e0 = R[:, 0:1], R1[:, 0:1], R2[:, 0:1]
            r = R / s0
            r1 = (R1 - r * d0) / s0
            r2 = (R2 - (0 if mutate == "r2" else 2 * r1 * d0) - r * e0) / s0
            self.s = self.s * R[:, 0]
            self.rho.append(R1[:, 0] / R[:, 0]), self.kappa.append(R2[:, 0] / R[:, 0])
            self.r.append(r), self.r1.append(r1), self.r2.append(r2)


def norm_basis_of(om, x, dt, mutate=None):
    return NormBasis(om.kinds, [om.knots_of(k) for k in range(om.d)], om.hyp, om.rotmat, x, dt, mutate)


def hv_terms_norm(nb, terms, V, mutate=None):
    """(B, jv terms n x p, hv terms n x p x d) by the normalised algebra, per (row, term k):
         B    = s P
         jv   = s ((rho.v) P + dP),                              dP = sum_m v_m E_km r'_m
         hv_l = s ((rho_l (rho.v) + v_l (kappa_l - rho_l^2)) P + rho_l dP
                   + (rho.v) E_kl r'_l + v_l E_kl r''_l + r'_l sum_{m != l} v_m E_klm r'_m)
    mutate: "kappa" puts kappa_l for kappa_l - rho_l^2, "cross" drops the last term."""
    dt, d, n = nb.dt, nb.d, nb.n
    terms = np.asarray(terms, dtype=np.int64)
    p = len(terms)
    V = np.asarray(V, dtype=dt)
    one, zero = np.ones((n, p), dtype=dt), np.zeros((n, p), dtype=dt)
    F0, F1, F2 = [], [], []
    for k in range(d):
        lev = terms[:, k]
        has = (lev > 0)[None, :]
        F0.append(np.where(has, nb.r[k][:, lev], one))
        F1.append(np.where(has, nb.r1[k][:, lev], zero))
        F2.append(np.where(has, nb.r2[k][:, lev], zero))

    def without(skip):
        P = one.copy()
        for k in range(d):
            if k not in skip:
                P = P * F0[k]
        return P
    P = without(())
    E1 = [without((l,)) for l in range(d)]
    rv = np.zeros(n, dtype=dt)
    for l in range(d):
        rv = rv + V[:, l] * nb.rho[l]
    dP = zero.copy()
    for m in range(d):
        dP = dP + V[:, m:m + 1] * (E1[m] * F1[m])
    s = nb.s[:, None]
    hv = np.empty((n, p, d), dtype=dt)
    for l in range(d):
        cross = zero.copy()
        if mutate != "cross":
            for m in range(d):
                if m != l and np.any(terms[:, m] > 0) and np.any(terms[:, l] > 0):
                    cross = cross + V[:, m:m + 1] * (without((l, m)) * F1[m])
        rho, vl = nb.rho[l][:, None], V[:, l:l + 1]
        curv = nb.kappa[l][:, None] - (0 if mutate == "kappa" else rho * rho)
        hv[:, :, l] = s * ((rho * rv[:, None] + vl * curv) * P + rho * dP + rv[:, None] * (E1[l] * F1[l])
                           + vl * (E1[l] * F2[l]) + F1[l] * cross)
    return s * P, s * (rv[:, None] * P + dP), hv


def f64_ratio(ref, om, x, terms, V, parts=None):
    """max(err / bound) of the float64 normalised restatement over B, the JVP terms and the HVP terms
    of this case (and X.f64_ratio's, for the mean and the VJP): what constant_from_oracle_ratio is given.
    parts = (hv_terms, jv_terms) of the reference if the caller has them."""
    hvt, jvt = parts if parts is not None else (ref.hv_terms(terms, V), ref.jv_terms(terms, V))
    B64, jv64, hv64 = hv_terms_norm(norm_basis_of(om, x, np.float64), terms, V)
    worst = max(X.f64_ratio(ref, om, x, terms), E.worst_ratio(B64, *ref.getmat(terms)),
                E.worst_ratio(jv64, jvt[0], jvt[1]), E.worst_ratio(hv64, hvt[0], hvt[1]))
    return worst


def direction_rows(n, d, seed):
    """V (n x d): rows scaled 1e-3 .. 1e3 (period 7, as the responses), entries of both signs; rows
    3, 34 and 70 (where they exist) exactly zero"""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, d)) * J.response_scales(n)[:, None]
    for i in (3, 34, 70):
        if i < n:
            V[i] = 0.0
    return V
