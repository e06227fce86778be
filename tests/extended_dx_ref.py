"""Extended-precision reference of the design matrix's derivative by the inputs, dB / dx_l, and of the
gradients of the predictive mean and variance taken from it -- the instrument the input-gradient
tests measure with (test_predict_grad_host.py proves it, test_gpu_predict_grad.py uses it).
extended_ref is imported unchanged; the rules are its rules.

Per dimension l, with K = cov(x_l, knots_l), K' = dK / dx_l (dcov_dx_ld), R = K rot, s = R[:, 0]:

    gradient factor  g_l[:, c] = (K' rot)[:, c] / s      bound (|K'| |rot| + |g_l| bR[:, 0]) / |s|

(column 0 included: g_l[:, 0] = rho_l).  dB / dx_l is B with dimension l's level factor replaced by
g_l[:, t_l] -- ExtendedRef._product(terms, replace_dim=l, h=l) with the factor lists filled per
dimension instead of per hyper-parameter -- and carries the first-order bound of that product.

    d mean / dx_l = sum_k theta_k dB_kl
    d var / dx_l  = 2 sum_k c_k B_k dB_kl        bound 2 sum_k |c_k| (bB_k |dB_kl| + |B_k| bdB_kl)

each held to C . bound + gamma_p . sum |summands| (extended_ref's rule).  The reference library has
no such function, so the float64 side that C is measured from (where the oracle stands in
constant_from_oracle_ratio) is the plain NumPy restatement below, dB_f64.
"""
import numpy as np

import extended_ref as E

ld = np.longdouble


def dcov_dx_ld(kind, x, kn, hyp):
    """dK / dx of one dimension, n x m, long double throughout"""
    x, kn, hyp = np.asarray(x, dtype=ld), np.asarray(kn, dtype=ld), np.asarray(hyp, dtype=ld)
    third = ld(1) / 3
    if kind in ("mat25", "mat25pow"):
        if kind == "mat25":
            els = np.exp(2 * hyp[0])
            t1, t2 = x / els, kn / els
            dudx = np.ones_like(x) / els
        else:
            powv, els = np.exp(ld(0.25) * hyp[1]), np.exp(2 * hyp[0] + ld(0.25) * hyp[1])
            t1, t2 = np.power(x, powv) / els, np.power(kn, powv) / els
            dudx = powv * t1 / x
        h = t1[:, None] - t2[None, :]
        ah = np.abs(h)
        h2 = h * (1 + ah) * np.exp(-ah)
        return -third * h2 * dudx[:, None]
    if kind == "mat25ang":
        es, ec = np.exp(2 * hyp[0]), np.exp(2 * hyp[1])
        hs = (np.sin(x) / es)[:, None] - (np.sin(kn) / es)[None, :]
        hc = (np.cos(x) / ec)[:, None] - (np.cos(kn) / ec)[None, :]
        h = np.sqrt(hs * hs + hc * hc)
        w = (1 + h) * np.exp(-h)
        return -third * w * (hs * (np.cos(x) / es)[:, None] - hc * (np.sin(x) / ec)[:, None])
    raise ValueError("unknown covariance " + str(kind))


class ExtendedRefDx(E.ExtendedRef):
    """ExtendedRef whose gradient factors are by the INPUTS: g[l], bg[l] for l = 0 .. d-1"""

    def __init__(self, kinds, knots, hyp, rot, x):
        super().__init__(kinds, knots, hyp, rot, x, rotg=None)
        x = np.asarray(x, dtype=np.float64)
        hyp = np.asarray(hyp, dtype=np.float64)
        self.g, self.bg = [], []
        for k in range(self.d):
            m, o = len(knots[k]), int(self.knotptst[k])
            rk = np.asarray(rot[:m, o:o + m], dtype=ld)
            dK = dcov_dx_ld(self.kinds[k], x[:, k], knots[k], hyp[self.hypst[k]:self.hypst[k + 1]])
            T, bT = dK @ rk, np.abs(dK) @ np.abs(rk)
            s = self.s[k]
            g = T / s[:, None]
            self.g.append(g)
            self.bg.append((bT + np.abs(g) * self.bs[k][:, None]) / np.abs(s)[:, None])

    def getmat_dx(self, terms, l):
        """(dB / dx_l, bound), n x p"""
        return self._product(terms, replace_dim=l, h=l)

    def ref_grad_mean(self, terms, theta, C):
        """(d mean / dx, tolerance), n x d each"""
        out = [E.ref_matmul(*self.getmat_dx(terms, l), theta, C) for l in range(self.d)]
        return np.stack([w for w, _ in out], axis=1), np.stack([t for _, t in out], axis=1)

    def ref_grad_var(self, terms, cv, C):
        """(d var / dx, tolerance), n x d each: 2 sum_k c_k B_k dB_kl (the noise term has no gradient)"""
        B, bB = self.getmat(terms)
        c = np.asarray(cv, dtype=ld)
        ac = np.abs(E._f64(c))
        Bf, bBf = np.abs(E._f64(B)), E._f64(bB)
        want, tol = [], []
        for l in range(self.d):
            dB, bdB = self.getmat_dx(terms, l)
            dBf = np.abs(E._f64(dB))
            bound = 2 * ((bBf * dBf + Bf * E._f64(bdB)) @ ac)
            want.append(2 * ((B * dB) @ c))
            tol.append(E._sum_tol(C, bound, B.shape[1], 2 * ((Bf * dBf) @ ac)))
        return np.stack(want, axis=1), np.stack(tol, axis=1)


def reference_dx_of(om, x):
    """ExtendedRefDx of an oracle model (ob_oracle.OuterMod) on the rows x"""
    knots = [om.knots_of(k) for k in range(om.d)]
    return ExtendedRefDx(om.kinds, knots, om.hyp, om.rotmat, x)


# -- the float64 side: the same formulas in plain NumPy ------------------------------------------
def _cov_f64(kind, x, kn, hyp):
    """(K, dK / dx) of one dimension in float64"""
    if kind in ("mat25", "mat25pow"):
        if kind == "mat25":
            els = np.exp(2 * hyp[0])
            t1, t2 = x / els, kn / els
            dudx = np.ones_like(x) / els
        else:
            powv, els = np.exp(0.25 * hyp[1]), np.exp(2 * hyp[0] + 0.25 * hyp[1])
            t1, t2 = np.power(x, powv) / els, np.power(kn, powv) / els
            dudx = powv * t1 / x
        h = t1[:, None] - t2[None, :]
        ah = np.abs(h)
        e = np.exp(-ah)
        return (1 + ah + ah * ah / 3) * e, -(h * (1 + ah) * e) / 3 * dudx[:, None]
    es, ec = np.exp(2 * hyp[0]), np.exp(2 * hyp[1])
    hs = (np.sin(x) / es)[:, None] - (np.sin(kn) / es)[None, :]
    hc = (np.cos(x) / ec)[:, None] - (np.cos(kn) / ec)[None, :]
    h = np.sqrt(hs * hs + hc * hc)
    e = np.exp(-h)
    return ((1 + h + h * h / 3) * e,
            -((1 + h) * e) / 3 * (hs * (np.cos(x) / es)[:, None] - hc * (np.sin(x) / ec)[:, None]))


def dB_f64(kinds, knots, hyp, rot, x, terms):
    """(B, dB) in float64: n x p and n x p x d"""
    x = np.asarray(x, dtype=np.float64)
    terms = np.asarray(terms, dtype=np.int64)
    hyp = np.asarray(hyp, dtype=np.float64)
    d, (n, p) = len(kinds), (x.shape[0], terms.shape[0])
    m = [len(k) for k in knots]
    kst = np.concatenate([[0], np.cumsum(m)])
    hst = np.concatenate([[0], np.cumsum([E.NUMHYP[k] for k in kinds])])
    s, r, g = [], [], []
    for k in range(d):
        rk = np.asarray(rot[:m[k], kst[k]:kst[k] + m[k]], dtype=np.float64)
        K, dK = _cov_f64(kinds[k], x[:, k], np.asarray(knots[k], dtype=np.float64), hyp[hst[k]:hst[k + 1]])
        R, T = K @ rk, dK @ rk
        s.append(R[:, 0]), r.append(R / R[:, 0:1]), g.append(T / R[:, 0:1])
    scale = np.ones(n)
    for k in range(d):
        scale = scale * s[k]

    def product(replace):
        P = np.repeat(scale[:, None], p, axis=1)
        for k in range(d):
            lev = terms[:, k]
            if k == replace:
                P = P * g[k][:, lev]
            else:
                P = P * np.where(lev[None, :] > 0, r[k][:, lev], 1.0)
        return P
    return product(None), np.stack([product(l) for l in range(d)], axis=2)


def dB_f64_of(om, x, terms):
    return dB_f64(om.kinds, [om.knots_of(k) for k in range(om.d)], om.hyp, om.rotmat, x, terms)


def f64_ratio(ref, om, x, terms):
    """max(err / bound) of the float64 restatement over B and every dB / dx_l on this case: what
    constant_from_oracle_ratio is given"""
    B64, dB64 = dB_f64_of(om, x, terms)
    worst = E.worst_ratio(B64, *ref.getmat(terms))
    for l in range(om.d):
        worst = max(worst, E.worst_ratio(dB64[:, :, l], *ref.getmat_dx(terms, l)))
    return worst
