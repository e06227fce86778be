"""Extended-precision host restatement of the design matrix B, its hyper-parameter gradient and the
products taken of them, for d dimensions -- the instrument the parity tests measure kernels with
(test_extended_ref.py proves it against 50-digit arithmetic, test_gpu_extended.py uses it).

Everything is np.longdouble (x87 extended, eps = 1.08e-19); NumPy only, nothing of the float64
oracle takes part in the arithmetic.  The float64 inputs are taken as exact: the rows x, the knots,
the hyper-parameters and the rotation (rotmat, rotmat_gradhyp) that BOTH sides hold, so the
instrument measures kernels and says nothing about the eigen-solver that made the rotation.

Per dimension k (covf::cov / cov_gradhyp of mat25, mat25pow, mat25ang; outermod::buildob with and
without gradients):

    K = cov(x_k, knots_k)            dK_h = dK / d hyp_h
    R = K rot                        bR   = |K| |rot|
    T_h = dK_h rot + K rotg_h        bT_h = |dK_h| |rot| + |K| |rotg_h|

bR and bT are the conditioning of the knot sums: a float64 evaluation of R[i, c] in any order is
wrong by a few eps64 x bR[i, c], however small R[i, c] itself comes out (rot columns carry
1 / eigenvalue, so high levels cancel many digits).  The factors a term is multiplied out of:

    scale factor     s_k = R[:, 0]                      bound bR[:, 0]
    level factor     r_k[:, c] = R[:, c] / R[:, 0]      bound (bR[:, c] + |r_k[:, c]| bR[:, 0]) / |R[:, 0]|
    gradient factor  g_h[:, c] = T_h[:, c] / R[:, 0]    bound (bT_h[:, c] + |g_h[:, c]| bR[:, 0]) / |R[:, 0]|

(column 0 of g_h included: it is not the derivative of the normalised ratio).  Then

    B[i, t]     = prod_k s_k[i] . prod_{k: t_k > 0} r_k[i, t_k]
    bB[i, t]    = sum over its factors f of  bound_f[i] . prod_{g != f} |g[i]|        (first order)
    dB[i, t, h] = the same product with dimension hypmatch[h]'s level factor replaced by
                  g_h[:, t_l] (level 0 included), bounded by the same rule.

A float64 result `got` of a sum S = sum_j s_j of k such entries (B a, B^T v, the Gram, ...) is held to

    |got - S|  <=  C . (propagated bound of the sum)  +  gamma_k . sum_j |s_j|

gamma_k = k u / (1 - k u), u = 2^-53, is the textbook bound of a float64 sum of k summands in ANY
order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), so it covers matrix-core
accumulation, LDS trees and split-row reductions alike.  C is not a constant of this module: each
test measures the float64 oracle's own max(err / bound) on the same case and allows eight times
that (room for another summation order, fused multiply-adds, interval tables, another libm),
never more than 2e-13.
"""
import numpy as np

ld = np.longdouble
EPS = float(np.finfo(ld).eps)
U = 2.0 ** -53
C_CAP = 2e-13
NUMHYP = {"mat25": 1, "mat25pow": 2, "mat25ang": 2}

PRECISION_MESSAGE = ("np.longdouble on this host has eps = %.3g, not the < 2e-19 of an extended format: "
                     "the 'extended' reference would be float64 and pass everything" % EPS)


def require_extended():
    """every entry point calls this: without an extended format the tests FAIL, they do not skip"""
    assert EPS < 2e-19, PRECISION_MESSAGE


def gamma(k):
    return k * U / (1.0 - k * U)


def constant_from_oracle_ratio(ratio):
    """C of the tolerance: eight times the float64 oracle's own max(err / bound), at most 2e-13"""
    return min(8.0 * float(ratio), C_CAP)


def cov_ld(kind, x, kn, hyp):
    """(K, [dK / d hyp_h]) of one dimension, n x m, long double throughout"""
    x, kn, hyp = np.asarray(x, dtype=ld), np.asarray(kn, dtype=ld), np.asarray(hyp, dtype=ld)
    third = ld(1) / 3
    if kind in ("mat25", "mat25pow"):
        if kind == "mat25":
            els = np.exp(2 * hyp[0])
            t1, t2 = x / els, kn / els
        else:
            powv, els = np.exp(ld(0.25) * hyp[1]), np.exp(2 * hyp[0] + ld(0.25) * hyp[1])
            t1, t2 = np.power(x, powv) / els, np.power(kn, powv) / els
        h = t1[:, None] - t2[None, :]
        ah = np.abs(h)
        e = np.exp(-ah)
        K = (1 + ah + ah * ah * third) * e
        h2 = h * (1 + ah) * e
        dK = [2 * third * h * h2]
        if kind == "mat25pow":
            g1 = (np.log(x) * t1)[:, None] - (np.log(kn) * t2)[None, :]
            dK.append(g1 * (-(ld(0.25) * powv * third) * h2) + ld(0.25) * third * h * h2)
        return K, dK
    if kind == "mat25ang":
        es, ec = np.exp(2 * hyp[0]), np.exp(2 * hyp[1])
        hs = (np.sin(x) / es)[:, None] - (np.sin(kn) / es)[None, :]
        hc = (np.cos(x) / ec)[:, None] - (np.cos(kn) / ec)[None, :]
        h = np.sqrt(hs * hs + hc * hc)
        e = np.exp(-h)
        K = (1 + h + h * h * third) * e
        w = e * (h + 1)
        return K, [2 * third * hs * hs * w, 2 * third * hc * hc * w]
    raise ValueError("unknown covariance " + str(kind))


class ExtendedRef:
    """The factors of every dimension on the rows x, and B / dB with their bounds for any terms.

    kinds, knots (one array per dimension), hyp (all hyper-parameters, dimension after dimension),
    rot (mmax x sum m_k, dimension k's m_k x m_k block at column knotptst[k]), rotg (mmax x ng: per
    dimension one block of m_k columns per hyper-parameter, or None without gradients), x (n x d)."""

    def __init__(self, kinds, knots, hyp, rot, x, rotg=None):
        require_extended()
        self.kinds = list(kinds)
        self.d = d = len(self.kinds)
        x = np.asarray(x, dtype=np.float64)
        assert x.ndim == 2 and x.shape[1] == d and len(knots) == d
        self.n = x.shape[0]
        m = [len(k) for k in knots]
        self.knotptst = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
        self.hypst = np.concatenate([[0], np.cumsum([NUMHYP[k] for k in self.kinds])]).astype(np.int64)
        hyp = np.asarray(hyp, dtype=np.float64)
        assert len(hyp) == self.hypst[-1]
        self.nhyp = int(self.hypst[-1])
        self.hypmatch = np.concatenate([[k] * NUMHYP[kd] for k, kd in enumerate(self.kinds)]).astype(np.int64)
        self.grad = rotg is not None
        self.R, self.bR = [], []                # n x m_k: getbase and its bound
        self.s, self.bs = [], []                # scale factors
        self.r, self.br = [], []                # level factors (column 0 unused)
        self.g, self.bg = [None] * self.nhyp, [None] * self.nhyp
        gcol = 0
        for k in range(d):
            o = int(self.knotptst[k])
            rk = np.asarray(rot[:m[k], o:o + m[k]], dtype=ld)
            K, dK = cov_ld(self.kinds[k], x[:, k], knots[k], hyp[self.hypst[k]:self.hypst[k + 1]])
            R, bR = K @ rk, np.abs(K) @ np.abs(rk)
            s = R[:, 0]
            r = R / s[:, None]
            br = (bR + np.abs(r) * bR[:, 0:1]) / np.abs(s)[:, None]
            self.R.append(R), self.bR.append(bR), self.s.append(s), self.bs.append(bR[:, 0])
            self.r.append(r), self.br.append(br)
            for j in range(NUMHYP[self.kinds[k]]):
                if self.grad:
                    rg = np.asarray(rotg[:m[k], gcol:gcol + m[k]], dtype=ld)
                    T = dK[j] @ rk + K @ rg
                    bT = np.abs(dK[j]) @ np.abs(rk) + np.abs(K) @ np.abs(rg)
                    g = T / s[:, None]
                    h = int(self.hypst[k]) + j
                    self.g[h] = g
                    self.bg[h] = (bT + np.abs(g) * bR[:, 0:1]) / np.abs(s)[:, None]
                gcol += m[k]

    # -- the running product of a term's factors and its first-order bound -----------------------
    @staticmethod
    def _times(P, S, f, bf):
        """(P, S) . factor f with bound bf:  S <- S |f| + |P| bf,  P <- P f  -- which unrolls to
        S = sum_f bf prod_{g != f} |g| without ever dividing by a factor"""
        return P * f, S * np.abs(f) + np.abs(P) * bf

    def _scale(self):
        P, S = np.ones(self.n, dtype=ld), np.zeros(self.n, dtype=ld)
        for k in range(self.d):
            P, S = self._times(P, S, self.s[k], self.bs[k])
        return P, S

    def _product(self, terms, replace_dim=None, h=None):
        terms = np.asarray(terms, dtype=np.int64)
        assert terms.ndim == 2 and terms.shape[1] == self.d
        p = terms.shape[0]
        P0, S0 = self._scale()
        P = np.repeat(P0[:, None], p, axis=1)
        S = np.repeat(S0[:, None], p, axis=1)
        for k in range(self.d):
            if k == replace_dim:
                lev = terms[:, k]
                P, S = self._times(P, S, self.g[h][:, lev], self.bg[h][:, lev])
                continue
            idx = np.nonzero(terms[:, k] > 0)[0]
            if len(idx) == 0:
                continue
            lev = terms[idx, k]
            P[:, idx], S[:, idx] = self._times(P[:, idx], S[:, idx], self.r[k][:, lev], self.br[k][:, lev])
        return P, S

    def getbase(self, k):
        """(R, bR) of dimension k (0-based): what getbase returns, s_k r_k = R"""
        return self.R[k], self.bR[k]

    def getmat(self, terms):
        """(B, bB), n x p"""
        return self._product(terms)

    def getmat_gradhyp(self, terms):
        """(dB, bdB), n x p x nhyp"""
        assert self.grad, "built without rotmat_gradhyp"
        terms = np.asarray(terms, dtype=np.int64)
        dB = np.empty((self.n, terms.shape[0], self.nhyp), dtype=ld)
        bdB = np.empty_like(dB)
        for h in range(self.nhyp):
            dB[:, :, h], bdB[:, :, h] = self._product(terms, int(self.hypmatch[h]), h)
        return dB, bdB


# -- sums of entries: (value in long double, tolerance for a float64 result) -----------------------
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _sum_tol(C, bound, k, absum):
    return C * _f64(bound) + gamma(k) * _f64(absum)


def ref_matmul(B, bB, a, C, squared=False, extra=0):
    """B a (or (B o B) a) over the p terms; `extra` more summands for what a caller adds on top"""
    a = np.asarray(a, dtype=ld)
    if squared:
        B, bB = B * B, 2 * np.abs(B) * bB
    aa = np.abs(_f64(a))
    return B @ a, _sum_tol(C, _f64(bB) @ aa, B.shape[1] + extra, np.abs(_f64(B)) @ aa)


def ref_tmatmul(B, bB, v, C, squared=False):
    """B^T v (or (B o B)^T v) over the n rows"""
    v = np.asarray(v, dtype=ld)
    if squared:
        B, bB = B * B, 2 * np.abs(B) * bB
    av = np.abs(_f64(v))
    return B.T @ v, _sum_tol(C, _f64(bB).T @ av, B.shape[0], np.abs(_f64(B)).T @ av)


def ref_sqcolsums(B, bB, C):
    return ref_tmatmul(B, bB, np.ones(B.shape[0]), C, squared=True)


def ref_predict_var(B, bB, cv, sigma, C):
    """(B o B) cv + e^{2 sigma}: the noise term and its libm exponential count as two more summands"""
    want, tol = ref_matmul(B, bB, cv, C, squared=True, extra=2)
    noise = np.exp(2 * ld(sigma))
    return want + noise, tol + gamma(B.shape[1] + 2) * float(noise)


def gram_column_sample(bB, seed):
    """The columns the Gram is compared on: two seeded-random columns of every block of 64, plus the
    64 columns of largest mean bound.  Every 64 x 64 quadrant of every 128 x 128 tile then has at
    least two sampled rows of G; exact symmetry carries that to the transposed blocks."""
    p = bB.shape[1]
    rng = np.random.default_rng(seed)
    cols = []
    for c0 in range(0, p, 64):
        width = min(64, p - c0)
        cols += list(c0 + rng.choice(width, size=min(2, width), replace=False))
    worst = np.argsort(-_f64(bB).mean(axis=0), kind="stable")[:64]
    return np.unique(np.concatenate([np.asarray(cols, dtype=np.int64), worst.astype(np.int64)]))


def gram_bound(B, bB, cols):
    Bf, bf = np.abs(_f64(B)), _f64(bB)
    return bf[:, cols].T @ Bf + Bf[:, cols].T @ bf


def ref_gram(B, bB, cols, C, extra=0):
    """G[cols, :] = B[:, cols]^T B over the n rows, bound sum_i (bB_ik |B_il| + |B_ik| bB_il)"""
    Bf = np.abs(_f64(B))
    return B[:, cols].T @ B, _sum_tol(C, gram_bound(B, bB, cols), B.shape[0] + extra, Bf[:, cols].T @ Bf)


def ref_matmul_gradhyp(dB, bdB, a, C):
    """sum_t a_t dB[:, t, h]: n x nhyp"""
    a = np.asarray(a, dtype=ld)
    aa = np.abs(_f64(a))
    want = np.einsum("ith,t->ih", dB, a)
    return want, _sum_tol(C, np.einsum("ith,t->ih", _f64(bdB), aa), dB.shape[1],
                          np.einsum("ith,t->ih", np.abs(_f64(dB)), aa))


def ref_tmatmul_gradhyp(dB, bdB, v, C):
    """sum_i v_i dB[i, :, h]: p x nhyp"""
    v = np.asarray(v, dtype=ld)
    av = np.abs(_f64(v))
    want = np.einsum("ith,i->th", dB, v)
    return want, _sum_tol(C, np.einsum("ith,i->th", _f64(bdB), av), dB.shape[0],
                          np.einsum("ith,i->th", np.abs(_f64(dB)), av))


def ref_sqcolsums_gradhyp(B, bB, dB, bdB, C):
    """d/d hyp_h sum_i B[i, t]^2 = 2 sum_i B[i, t] dB[i, t, h]: p x nhyp (the factor 2 is exact)"""
    want = 2 * np.einsum("it,ith->th", B, dB)
    Bf, bf, dBf, bdf = np.abs(_f64(B)), _f64(bB), np.abs(_f64(dB)), _f64(bdB)
    bound = 2 * (np.einsum("it,ith->th", bf, dBf) + np.einsum("it,ith->th", Bf, bdf))
    return want, _sum_tol(C, bound, B.shape[0], 2 * np.einsum("it,ith->th", Bf, dBf))


def _sq_grad_cube(B, bB, dB, bdB):
    """d(B^2)/dhyp = 2 B dB per entry (the factor 2 is exact): value, bound, |value| in float64"""
    Bf, bf, dBf, bdf = np.abs(_f64(B)), _f64(bB), np.abs(_f64(dB)), _f64(bdB)
    return 2 * B[:, :, None] * dB, 2 * (bf[:, :, None] * dBf + Bf[:, :, None] * bdf), 2 * Bf[:, :, None] * dBf


def ref_sqtmm_gradhyp(B, bB, dB, bdB, v, C):
    """sum_i v_i 2 B[i, t] dB[i, t, h] with v of any sign: p x nhyp, n summands"""
    S, bS, aS = _sq_grad_cube(B, bB, dB, bdB)
    v = np.asarray(v, dtype=ld)
    av = np.abs(_f64(v))
    return np.einsum("ith,i->th", S, v), _sum_tol(C, np.einsum("ith,i->th", bS, av), B.shape[0],
                                                  np.einsum("ith,i->th", aS, av))


def ref_sqmm_gradhyp(B, bB, dB, bdB, a, C):
    """sum_t a_t 2 B[i, t] dB[i, t, h]: n x nhyp, p summands"""
    S, bS, aS = _sq_grad_cube(B, bB, dB, bdB)
    a = np.asarray(a, dtype=ld)
    aa = np.abs(_f64(a))
    return np.einsum("ith,t->ih", S, a), _sum_tol(C, np.einsum("ith,t->ih", bS, aa), B.shape[1],
                                                  np.einsum("ith,t->ih", aS, aa))


def ref_matmul_gradhyp_dot(dB, bdB, a, v, C):
    """sum_i sum_t v_i a_t dB[i, t, h]: nhyp values, each a double sum of n p summands"""
    a, v = np.asarray(a, dtype=ld), np.asarray(v, dtype=ld)
    aa, av = np.abs(_f64(a)), np.abs(_f64(v))
    want = np.einsum("ith,t,i->h", dB, a, v)
    return want, _sum_tol(C, np.einsum("ith,t,i->h", _f64(bdB), aa, av), dB.shape[0] * dB.shape[1],
                          np.einsum("ith,t,i->h", np.abs(_f64(dB)), aa, av))


def term_var(basisvar, knotptst, terms):
    """om$getvar(terms) = exp(sum_l basisvar[knotptst[l] + t_l]) in long double, and the bound of a float64
    evaluation of it: d additions in the exponent (absolute there, relative here) and one exponential"""
    terms = np.asarray(terms, dtype=np.int64)
    bv = np.asarray(basisvar, dtype=ld)[np.asarray(knotptst, dtype=np.int64)[None, :-1] + terms]
    varc = np.exp(bv.sum(axis=1))
    return varc, _f64(varc) * (gamma(terms.shape[1]) * np.abs(_f64(bv)).sum(axis=1) + 2 * U)


def ref_residvar_gradhyp(B, bB, dB, bdB, varc, bvarc, lv, C):
    """d/dhyp_h (1 - sum_t varc_t B[i, t]^2) = - sum_t varc_t (2 B dB[i, t, h] + B^2 lv[t, h]), lv[t, h] =
    d log varc_t / d hyp_h (float64 data, exact): n x nhyp, 2 p summands and four roundings in forming them.
    bvarc (term_var) enters as it is, not times C: it is a bound of float64 arithmetic, not of conditioning."""
    S, bS, aS = _sq_grad_cube(B, bB, dB, bdB)
    lv = np.asarray(lv, dtype=ld)
    Bf, bf, alv = np.abs(_f64(B)), _f64(bB), np.abs(_f64(lv))
    T = S + (B * B)[:, :, None] * lv[None, :, :]
    bT = bS + (2 * Bf * bf)[:, :, None] * alv[None, :, :]
    aT = aS + (Bf * Bf)[:, :, None] * alv[None, :, :]
    vf = _f64(varc)
    want = -np.einsum("ith,t->ih", T, np.asarray(varc, dtype=ld))
    return want, _sum_tol(C, np.einsum("ith,t->ih", bT, vf), 2 * B.shape[1] + 4, np.einsum("ith,t->ih", aT, vf)) \
        + np.einsum("ith,t->ih", aT, _f64(bvarc))


# -- measuring ---------------------------------------------------------------------------------------
def maxnorm_relerr(got, want):
    """the criterion the older tests use: max |got - want| / max |want|"""
    want = _f64(want)
    return float(np.max(np.abs(_f64(np.asarray(got, dtype=ld) - want))) / max(1e-300, np.max(np.abs(want))))


def ratio_map(got, want, tol, floor=0.0):
    """|got - want| / (tol + floor) per entry (0 where both vanish)"""
    err = _f64(np.abs(np.asarray(got, dtype=ld) - want))
    den = _f64(tol) + floor
    out = np.zeros(err.shape)
    np.divide(err, den, out=out, where=den > 0)
    out[(den <= 0) & (err > 0)] = np.inf
    return out


def worst_ratio(got, want, tol, floor=0.0):
    r = ratio_map(got, want, tol, floor)
    return float(np.max(r)) if r.size else 0.0
