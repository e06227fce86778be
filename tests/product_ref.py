"""Host reference of the predictor on the product of two input blocks (obhip_predict_product_dev,
obhip_product_loglik_dev): NumPy only, long double through extended_ref.ExtendedRef on the expanded rows.

Tolerances (extended_ref's docstring explains C, the propagated bound and gamma_k):
  mean      ref_matmul(B, bB, theta, C, extra=2d+2): the device multiplies the factors of an entry in another
            order (each side's product first, the two scales last) -- 2d summands, as
            test_bty_against_the_exact_product argues for its 2d -- and two scale multiplications;
  variance  ref_matmul(B, bB, c, C, squared=True, extra=4d+6) plus the noise term as ref_predict_var handles it;
  sums      with r = y - mean, v = var + obsvar, u = 2^-53 and the per-pair tolerances
            tau_m = (mean's) + u (|y| + |mean|),  tau_v = (variance's) + 2 u v  for forming r and v:
              chi2    sum_i [2 |r| / v tau_m + r^2 / v^2 tau_v + 4 u r^2 / v] + gamma_na sum_i r^2 / v
              logdet  sum_i [tau_v / v + 4 u |log v|] + gamma_na sum_i |log v|
C per case: constant_from_oracle_ratio of the float64 oracle's worst_ratio on the same rows and on a 300-row
probe, as test_gpu_extended.rows does it.
"""
import numpy as np

import extended_ref as E
from conftest import sample_x

ld = np.longdouble
PROBE_ROWS = 300
MAX_ROWS = 2300      # expanded rows per evaluation of the extended reference (long double n x p arrays)


def dims_a_of(d, dims_b):
    return [l for l in range(d) if l not in set(int(b) for b in dims_b)]


def expand(xa, xb, dims_b):
    """the na nb x d rows of the product, row i nb + j = (xa[i] on the other dimensions, xb[j] on dims_b)"""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    na, nb, d = xa.shape[0], xb.shape[0], xa.shape[1] + xb.shape[1]
    X = np.empty((na * nb, d))
    X[:, dims_a_of(d, dims_b)] = np.repeat(xa, nb, axis=0)
    X[:, list(dims_b)] = np.tile(xb, (na, 1))
    return X


def split_x(x, dims_b):
    """(xa, xb) columns of full-width rows x"""
    return x[:, dims_a_of(x.shape[1], dims_b)], x[:, list(dims_b)]


def _oracle_ratio(m, x, B, bB):
    import ob_oracle as O
    return E.worst_ratio(O.ob_getmat(O.OuterBase(m["om_o"], x), m["terms"]), B, bB)


def probe_ratio(m, seed):
    """the oracle's err / bound of the case on PROBE_ROWS sampled rows (once per model dict)"""
    if "_product_probe" not in m:
        x = sample_x(np.random.default_rng(seed), PROBE_ROWS, m["kinds"])
        B, bB = E.ExtendedRef(m["kinds"], m["knots"], m["hyp"], m["rot"], x).getmat(m["terms"])
        m["_product_probe"] = _oracle_ratio(m, x, B, bB)
    return m["_product_probe"]


class ProductRef:
    """m: a model dict (kinds, knots, hyp, rot, terms, om_o) as test_gpu_extended.model returns it"""

    def __init__(self, m, xa, xb, dims_b, seed=0):
        self.na, self.nb, self.d = len(xa), len(xb), len(m["kinds"])
        self.x = expand(xa, xb, dims_b)
        parts, self.ratio = [], 0.0
        for r0 in range(0, len(self.x), MAX_ROWS):
            x = self.x[r0:r0 + MAX_ROWS]
            parts.append(E.ExtendedRef(m["kinds"], m["knots"], m["hyp"], m["rot"], x).getmat(m["terms"]))
            self.ratio = max(self.ratio, _oracle_ratio(m, x, *parts[-1]))
        self.B, self.bB = (np.concatenate([pt[k] for pt in parts]) for k in (0, 1))
        self.C = E.constant_from_oracle_ratio(max(self.ratio, probe_ratio(m, seed)))
        self.p = self.B.shape[1]

    def _grid(self, a):
        return a.reshape(self.na, self.nb)

    def mean(self, theta):
        """(want, tol), na x nb, of one coefficient vector"""
        want, tol = E.ref_matmul(self.B, self.bB, theta, self.C, extra=2 * self.d + 2)
        return self._grid(want), self._grid(tol)

    def var(self, cv, sigma):
        """(want, tol), na x nb; cv None: the noise term alone"""
        noise = np.exp(2 * ld(sigma))
        if cv is None:
            return (np.full((self.na, self.nb), noise, dtype=ld),
                    np.full((self.na, self.nb), E.gamma(2) * float(noise)))
        extra = 4 * self.d + 6
        want, tol = E.ref_matmul(self.B, self.bB, cv, self.C, squared=True, extra=extra)
        return self._grid(want + noise), self._grid(tol + E.gamma(self.p + extra) * float(noise))

    def sums(self, theta, y, obsvar, cv, sigma):
        """((chi2, tol), (logdet, tol)), nb each"""
        mean, tm = self.mean(theta)
        var, tv = self.var(cv, sigma)
        y = np.asarray(y, dtype=ld)[:, None]
        ov = np.zeros((self.na, 1), dtype=ld) if obsvar is None else np.asarray(obsvar, dtype=ld)[:, None]
        r, v = y - mean, var + ov
        f = lambda a: np.asarray(a, dtype=np.float64)
        rf, vf = np.abs(f(r)), f(v)
        tau_m = tm + E.U * (np.abs(f(y)) + np.abs(f(mean)))
        tau_v = tv + 2 * E.U * vf
        t1, t2 = r * r / v, np.log(v)
        g = E.gamma(self.na)
        tol1 = (2 * rf / vf * tau_m + rf * rf / (vf * vf) * tau_v + 4 * E.U * f(t1)).sum(0) + g * f(t1).sum(0)
        tol2 = (tau_v / vf + 4 * E.U * np.abs(f(t2))).sum(0) + g * np.abs(f(t2)).sum(0)
        return (t1.sum(0), tol1), (t2.sum(0), tol2)
