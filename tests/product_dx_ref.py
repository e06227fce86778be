"""Host reference of the gradient by xb on the product of two input blocks (obhip_predict_product_grad_dev,
obhip_product_loglik_grad_dev): NumPy only, long double; product_ref.ProductRef for the values and
extended_dx_ref.ExtendedRefDx on the expanded rows for the derivatives.  test_product_dx_host.py proves it
against central differences of its own sums, test_gpu_product_dx.py measures with it.

Per pair (row i nb + j of the expanded rows) and B dimension l, with C of the ProductRef:
  m' = d mean / d xb_jl   ref_matmul(*getmat_dx(terms, l), theta, C, extra=2d+2): the device multiplies the
                          factors of an entry side by side, as product_ref's mean says, and adds the rho part;
  v' = d var / d xb_jl    2 sum_k c_k B_k dB_kl with the bound of extended_dx_ref.ref_grad_var,
                          2 sum_k |c_k| (bB_k |dB_kl| + |B_k| bdB_kl), held to C . bound + gamma_(p + 4d + 6)
                          . 2 sum_k |c_k B_k dB_kl| (the noise term has no gradient).
Sums over i, in long double, with r = y - mean, v = var + obsvar, u = 2^-53 and the per-pair tolerances tau_m,
tau_v of product_ref.sums, tau_m', tau_v' of the two lines above -- the first-order propagation of the four:
  d chi2 / d xb_jl = sum_i (-2 r m' / v - r^2 v' / v^2)
      -2 r m' / v     2 (|m'| / v tau_m + |r| / v tau_m' + |r m'| / v^2 tau_v)
      r^2 v' / v^2    2 |r v'| / v^2 tau_m + r^2 / v^2 tau_v' + 2 r^2 |v'| / v^3 tau_v
  d logdet / d xb_jl = sum_i v' / v
      v' / v          tau_v' / v + |v'| / v^2 tau_v
and every sum also 4 u |summand| per summand and gamma_na sum_i |summand|.
"""
import numpy as np

import extended_dx_ref as X
import extended_ref as E
import product_ref as P

ld = np.longdouble


class ProductDxRef(P.ProductRef):
    """ProductRef with the derivatives by the columns of xb; m as ProductRef takes it"""

    def __init__(self, m, xa, xb, dims_b, seed=0):
        super().__init__(m, xa, xb, dims_b, seed)
        self.m, self.dims_b, self.L = m, [int(b) for b in dims_b], len(dims_b)
        self._pairs = {}

    def _grid3(self, cols):
        return np.stack([self._grid(c) for c in cols], axis=2)

    def pair_grads(self, theta, cv=None):
        """((m', tol), (v', tol)), na x nb x L each; without cv the second is (0, 0)"""
        key = (np.asarray(theta, dtype=np.float64).tobytes(), None if cv is None else np.asarray(cv).tobytes())
        if key in self._pairs:
            return self._pairs[key]
        m, d, p, extra = self.m, self.d, self.p, 4 * self.d + 6
        wm, tm, wv, tv = ([[] for _ in range(self.L)] for _ in range(4))
        if cv is not None:
            c = np.asarray(cv, dtype=ld)
            ac = np.abs(E._f64(c))
        for r0 in range(0, len(self.x), P.MAX_ROWS):
            ref = X.ExtendedRefDx(m["kinds"], m["knots"], m["hyp"], m["rot"], self.x[r0:r0 + P.MAX_ROWS])
            B, bB = self.B[r0:r0 + P.MAX_ROWS], self.bB[r0:r0 + P.MAX_ROWS]
            Bf, bBf = np.abs(E._f64(B)), E._f64(bB)
            for k, l in enumerate(self.dims_b):
                dB, bdB = ref.getmat_dx(m["terms"], l)
                w, t = E.ref_matmul(dB, bdB, theta, self.C, extra=2 * d + 2)
                wm[k].append(w), tm[k].append(t)
                if cv is not None:
                    dBf = np.abs(E._f64(dB))
                    bound = 2 * ((bBf * dBf + Bf * E._f64(bdB)) @ ac)
                    wv[k].append(2 * ((B * dB) @ c))
                    tv[k].append(E._sum_tol(self.C, bound, p + extra, 2 * ((Bf * dBf) @ ac)))
        cat = lambda parts: self._grid3([np.concatenate(pt) for pt in parts])
        shape = (self.na, self.nb, self.L)
        out = ((cat(wm), cat(tm)),
               (cat(wv), cat(tv)) if cv is not None else (np.zeros(shape, dtype=ld), np.zeros(shape)))
        self._pairs = {key: out}          # the last one only: na nb L long doubles each
        return out

    def sums_grad(self, theta, y, obsvar, cv, sigma):
        """((d chi2, tol), (d logdet, tol)), nb x L each, of ProductRef.sums' two sums"""
        mean, tm = self.mean(theta)
        var, tv = self.var(cv, sigma)
        (dm, tdm), (dv, tdv) = self.pair_grads(theta, cv)
        y = np.asarray(y, dtype=ld)[:, None]
        ov = np.zeros((self.na, 1), dtype=ld) if obsvar is None else np.asarray(obsvar, dtype=ld)[:, None]
        r, v = y - mean, var + ov
        f = lambda a: np.asarray(a, dtype=np.float64)
        rf, vf = np.abs(f(r))[:, :, None], f(v)[:, :, None]
        tau_m = (tm + E.U * (np.abs(f(y)) + np.abs(f(mean))))[:, :, None]
        tau_v = (tv + 2 * E.U * f(v))[:, :, None]
        r, v = r[:, :, None], v[:, :, None]
        s1, s2, s3 = -2 * r * dm / v, -(r * r) * dv / (v * v), dv / v
        adm, adv = np.abs(f(dm)), np.abs(f(dv))
        t1 = 2 * (adm / vf * tau_m + rf / vf * tdm + rf * adm / (vf * vf) * tau_v)
        t2 = 2 * rf * adv / (vf * vf) * tau_m + rf * rf / (vf * vf) * tdv + 2 * rf * rf * adv / vf ** 3 * tau_v
        t3 = tdv / vf + adv / (vf * vf) * tau_v
        g = E.gamma(self.na)
        a12, a3 = np.abs(f(s1)) + np.abs(f(s2)), np.abs(f(s3))
        tol_c = (t1 + t2 + 4 * E.U * a12).sum(0) + g * a12.sum(0)
        tol_l = (t3 + 4 * E.U * a3).sum(0) + g * a3.sum(0)
        return ((s1 + s2).sum(0), tol_c), (s3.sum(0), tol_l)
