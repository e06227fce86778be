"""Extended-precision host restatement of the model layer (csrc/lpdf.cpp): loglik_gauss / loglik_std,
logpr_gauss, loglik_gda and the diagonal marginal adjustment of lpdfvec, every quantity with the
tolerance a float64 result of it is held to.  The instrument test_gpu_lpdf.py measures the likelihood
classes, vec_ops.h, kernels_misc.hip and the grad_*_dev entries with (test_lpdf_ref_host.py proves it
against the float64 oracle and against its own difference quotients).

np.longdouble and NumPy only; nothing of the float64 oracle takes part in the arithmetic.  B, dB / dhyp
and their bounds bB, bdB come from extended_ref.ExtendedRef, the prior's variances from
posterior_ref.prior_ld.  The float64 inputs (x, y, knots, hyp, rotation and its gradient, coeff, para)
are exact, as in extended_ref's docstring.  It is stateless: every function computes from the model,
the terms, the parameters and the coefficients it is given, never from an earlier answer.

Every result is a Pair (v, b, s): the long double value, the first-order bound `b` that bB / bdB
propagate into it (the part a float64 evaluation of B in any order may be wrong by, in units of C) and
the allowance `s` for the float64 roundings of everything after B.  A float64 result `got` is held to

    |got - v|  <=  C . b  +  s                                     (tol(pair, C))

which is extended_ref's rule C . bound + gamma_k . sum |summands|, carried through +, -, ., /, sqrt, log,
exp and sums by the usual first-order propagation:

    a + c   b = b_a + b_c                       s = s_a + s_c + RU |a + c|
    a . c   b = b_a |c| + |a| b_c               s = s_a |c| + |a| s_c + RU |a c|
    a / c   b = (b_a + |a / c| b_c) / |c|       s = (s_a + |a / c| s_c) / |c| + RU |a / c|
    f(a)    b = |f'(a)| b_a                     s = |f'(a)| s_a + RU |f(a)|          (sqrt, log, exp)
    sum_j   b = sum b_j                         s = sum s_j + gamma_k sum |a_j|      (k summands, any order)

RU = 2 u: one operation of the restatement stands for at most two roundings of the other side, which
may contract a product into an fma, scale before a sum where this file scales after it, or take a
libm function good to one ulp (= 2 u) -- a libm call counts as one more operation, as in
extended_ref.ref_predict_var.  C is never a constant of this module and never measured from the
device: every test measures the float64 oracle on the same case -- its max(err / bound) on the entries
of B and dB themselves (entry_ratio), where the accuracy of a side's B shows unmixed with later
roundings, and the C it needs on top of the allowance on every quantity (oracle_need) -- and takes
extended_ref.constant_from_oracle_ratio of the largest: eight times it, at most 2e-13; an oracle that
alone would need more than the cap fails the test.

The full-Hessian adjustment and predr_std with the full covariance are posterior_ref.ref_margadj and
ref_var on the float64 H BOTH sides hold (the device's Hessian, itself held to `hess`); the predictors
(pred_gauss, predr_std, pred_gda with its residual variance at the new rows) are in predict().
Session holds the state of a pair and the reference's cache rules for the call-order tests.

Rows go through in chunks of at most CHUNK = 32768, so the n x p x nhyp gradient never exists whole.
Row weight N (the likelihood sharded over N simulated ranks that all hold the same rows): every sum
over the rows times N, n_total = N n, para0 from the variance of the rows repeated N times.

Reference lines restated (src/lpdfs of the reference, as cited in csrc/lpdf.cpp):
  loglik_gauss   loglik_gauss.cpp:110-172    loglik_std    loglik_std.cpp:100-173 (the same expressions)
  logpr_gauss    logpr_gauss.cpp:98-160      loglik_gda    loglik_gda.cpp:117-235
  margadj_diag   fit.cpp:252-268, 371-380    para0         loglik_gauss.cpp:48, loglik_gda.cpp:58-60
  margadj_full   fit.cpp:270-299             predictors    loglik_gauss.cpp:196-227, loglik_std.cpp:218-256,
  Session        fit.cpp:208-245, 252-302                  loglik_gda.cpp:247-281
"""
import numpy as np

import extended_ref as E
import posterior_ref as PR
from extended_ref import U, gamma, ld

RU = 2 * U
CHUNK = 32768


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _abs64(v):
    return np.abs(_f64(v))


class Pair:
    """(value, bound propagated from bB, allowance for float64 roundings); see the module docstring"""
    __slots__ = ("v", "b", "s")

    def __init__(self, v, b=0.0, s=0.0):
        self.v = np.asarray(v, dtype=ld)
        self.b = _f64(b)
        self.s = _f64(s)

    @staticmethod
    def of(x):
        return x if isinstance(x, Pair) else Pair(x)

    @property
    def shape(self):
        return self.v.shape

    def __getitem__(self, idx):
        sh = self.v.shape
        return Pair(self.v[idx], np.broadcast_to(self.b, sh)[idx], np.broadcast_to(self.s, sh)[idx])

    def __neg__(self):
        return Pair(-self.v, self.b, self.s)

    def __add__(self, o):
        o = Pair.of(o)
        v = self.v + o.v
        return Pair(v, self.b + o.b, self.s + o.s + RU * _abs64(v))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-Pair.of(o))

    def __rsub__(self, o):
        return Pair.of(o) + (-self)

    def __mul__(self, o):
        o = Pair.of(o)
        v = self.v * o.v
        a, c = _abs64(self.v), _abs64(o.v)
        return Pair(v, self.b * c + a * o.b, self.s * c + a * o.s + RU * _abs64(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Pair.of(o)
        v = self.v / o.v
        q, c = _abs64(v), _abs64(o.v)
        return Pair(v, (self.b + q * o.b) / c, (self.s + q * o.s) / c + RU * q)

    def __rtruediv__(self, o):
        return Pair.of(o) / self

    def scale2(self, k):
        """times an exact power of two: no rounding"""
        return Pair(self.v * k, self.b * abs(k), self.s * abs(k))

    def sqrt(self):
        v = np.sqrt(self.v)
        w = _f64(v)
        return Pair(v, self.b / (2 * w), self.s / (2 * w) + RU * w)

    def log(self):
        v = np.log(self.v)
        a = _abs64(self.v)
        return Pair(v, self.b / a, self.s / a + RU * _abs64(v))

    def exp(self):
        v = np.exp(self.v)
        w = _f64(v)
        return Pair(v, self.b * w, self.s * w + RU * w)

    def sum(self, axis, k=None):
        """sum of k summands along `axis` in any order; k = 0 leaves the gamma term to the caller (Acc)"""
        sh = self.v.shape
        k = sh[axis] if k is None else k
        rest = gamma(k) * _abs64(self.v).sum(axis=axis) if k > 1 else 0.0
        return Pair(self.v.sum(axis=axis), np.broadcast_to(self.b, sh).sum(axis=axis),
                    np.broadcast_to(self.s, sh).sum(axis=axis) + rest)


def exact(x):
    return Pair(x)


def pexp(x):
    """libm exponential of an exact float64"""
    return Pair(x).exp()


def tol(pair, C):
    """the tolerance of a float64 result of `pair`"""
    return C * np.broadcast_to(pair.b, pair.v.shape) + np.broadcast_to(pair.s, pair.v.shape)


class Acc:
    """A sum over the rows taken chunk by chunk: the gamma term is that of ONE sum over all N n rows"""

    def __init__(self):
        self.v = self.b = self.s = self.a = None

    def add(self, pair):
        """pair: rows on axis 0"""
        sh = pair.v.shape
        parts = (pair.v.sum(axis=0), np.broadcast_to(pair.b, sh).sum(axis=0),
                 np.broadcast_to(pair.s, sh).sum(axis=0), _abs64(pair.v).sum(axis=0))
        if self.v is None:
            self.v, self.b, self.s, self.a = parts
        else:
            self.v, self.b, self.s, self.a = (x + y for x, y in zip((self.v, self.b, self.s, self.a), parts))

    def result(self, n, N=1):
        """the sum over the n rows, each repeated N times (one more rounding for the product by N)"""
        k = n * N
        rest = (gamma(k) if k > 1 else 0.0) * self.a + (RU * _abs64(self.v) if N > 1 else 0.0)
        return Pair(self.v * N, self.b * N, (self.s + rest) * N)


# ---- the case: model, rows, response, terms -----------------------------------------------------------
class Case:
    """om: the float64 oracle's model, used for its data only (kinds, knots, hyp, rotmat,
    rotmat_gradhyp, basisvar, logbasisvar_gradhyp and their index tables): what BOTH sides hold"""

    def __init__(self, om, x, y, terms):
        E.require_extended()
        self.om = om
        self.x = np.asarray(x, dtype=np.float64)
        self.y = np.asarray(y, dtype=np.float64)
        self.terms = np.asarray(terms, dtype=np.int64)
        self.n, self.p = self.x.shape[0], self.terms.shape[0]
        self.nhyp = len(om.hypmatch)
        self._kept = {}

    def chunks(self, grad=True):
        """(rows, B, dB) per chunk of at most CHUNK rows, B and dB as Pairs (dB None without grad)"""
        om = self.om
        knots = [np.asarray(om.knots_of(k), dtype=np.float64) for k in range(om.d)]
        for a in range(0, self.n, CHUNK):
            sl = slice(a, min(self.n, a + CHUNK))
            key = (a, bool(grad))
            if key not in self._kept:
                ref = E.ExtendedRef(om.kinds, knots, om.hyp, om.rotmat, self.x[sl], om.rotmat_gradhyp if grad else None)
                B, bB = ref.getmat(self.terms)
                out = (Pair(B, bB), None)
                if grad:
                    dB, bdB = ref.getmat_gradhyp(self.terms)
                    out = (out[0], Pair(dB, bdB))
                if self.n > CHUNK:        # a large case is walked once per call, nothing is kept
                    yield sl, out[0], out[1]
                    continue
                self._kept[key] = out
            yield sl, self._kept[key][0], self._kept[key][1]

    def prior(self, rho):
        """(prec as a Pair, lv exact) of logpr_gauss through posterior_ref.prior_ld"""
        om = self.om
        prec, rel, lv = PR.prior_ld(om.basisvar, om.knotptst, om.logbasisvar_gradhyp, om.gest, om.hypmatch,
                                    self.terms, rho)
        return Pair(prec, 0.0, rel * _f64(prec)), lv

    def varc(self):
        """om.getvar(terms) = 1 / prec at rho = 0 (modandbase.cpp:350-356)"""
        prec, lv = self.prior(0.0)
        return 1.0 / prec, lv


# ---- para0 ------------------------------------------------------------------------------------------------
def sample_var(y, N=1):
    """var() with the n - 1 denominator of the rows y repeated N times, two-pass (loglik_std.cpp:51).  With a
    mean wrong by dm the sum of squares about it is exactly  sum (y - m)^2 + n dm^2,  dm <= gamma(n) sum |y| / n
    + u |m|; the squares and their sum take gamma(n + 3) more.  NaN below two rows."""
    y = np.asarray(y, dtype=ld)
    n = len(y) * N
    if n < 2:
        return Pair(np.nan)
    m = y.sum() / len(y)
    dev = y - m
    ss = (dev * dev).sum() * N
    dm = gamma(n) * float(np.abs(y).sum()) / len(y) + RU * abs(float(m))
    s = n * dm * dm + gamma(n + 3) * float(ss) + 2 * dm * float(np.abs(dev).sum()) * N * RU
    return Pair(ss / (n - 1), 0.0, s / (n - 1) + RU * float(ss) / (n - 1))


def para0_gauss(y, N=1):
    """log(0.01 var(y)) (loglik_gauss.cpp:48, loglik_std.cpp:51)"""
    return (sample_var(y, N) * 0.01).log()


def para0_gda(y):
    """0.5 log(0.01 var(y)) (loglik_gda.cpp:58-60); the second parameter starts at 0"""
    return (sample_var(y) * 0.01).log().scale2(0.5)


# ---- loglik_gauss / loglik_std ------------------------------------------------------------------------------
def loglik_gauss(case, coeff, sigma, g=None, N=1, hess=False, grads=True):
    """{name: Pair} of loglik_gauss::update with every flag set, hessmult(g), diaghess, diaghessgradhyp
    (p x nhyp), diaghessgradpara (p x 1), the sums they are made of (sqcolsums, sqcolsums_gradhyp) and,
    when asked for, hess (loglik_std.cpp:170-173), with the rows weighted by N.  grads = False leaves out what
    needs dB / dhyp (for term sets of many dimensions, where n x p x nhyp is too much)."""
    c = np.asarray(coeff, dtype=ld)
    e2 = pexp(-2.0 * sigma)
    n, ntot = case.n, case.n * N
    ss, gr, gh, sq, dsq, hm, hs = Acc(), Acc(), Acc(), Acc(), Acc(), Acc(), Acc()
    gv = None if g is None else np.asarray(g, dtype=ld)
    for sl, B, dB in case.chunks(grads):
        yhat = (B * c[None, :]).sum(axis=1)
        d = yhat - case.y[sl]
        ss.add(d * d)
        r = -(e2 * d)                                             # :118-119
        gr.add(B * r[:, None])                                    # grad = B^T r
        sq.add(B * B)
        if grads:
            yge = (dB * c[None, :, None]).sum(axis=1)             # matmul_gradhyp(terms, coeff), n x nhyp
            gh.add(yge * r[:, None])
            dsq.add((B[:, :, None] * dB).scale2(2.0))
        if gv is not None:
            w = e2 * (B * gv[None, :]).sum(axis=1)                # :137-145
            hm.add(B * w[:, None])
        if hess:
            hs.add(B[:, :, None] * B[:, None, :])
    SS, SQ = ss.result(n, N), sq.result(n, N)
    out = {"val": (e2 * SS).scale2(-0.5) - exact(float(ntot)) * exact(sigma),
           "grad": gr.result(n, N), "gradpara": (e2 * SS - float(ntot))[None],
           "sqcolsums": SQ, "diaghess": e2 * SQ, "diaghessgradpara": (e2 * SQ).scale2(-2.0)[:, None]}
    if grads:
        DSQ = dsq.result(n, N)
        out.update({"gradhyp": gh.result(n, N), "sqcolsums_gradhyp": DSQ, "diaghessgradhyp": e2 * DSQ})
    if gv is not None:
        out["hessmult"] = hm.result(n, N)
    if hess:
        out["hess"] = e2 * hs.result(n, N)
    return out


# ---- logpr_gauss -------------------------------------------------------------------------------------------
def logpr_gauss(case, coeff, rho, g=None):
    """{name: Pair} of logpr_gauss (logpr_gauss.cpp:98-160) in terms of prec_k = 1 / (coeffsd_k e^rho)^2:
    stdresid^2 = coeff^2 prec and log(coeffsd e^rho) = -1/2 log prec"""
    c = np.asarray(coeff, dtype=ld)
    prec, lv = case.prior(rho)
    p = case.p
    sr2 = exact(c * c) * prec
    lp = prec.log().scale2(0.5)
    out = {"val": sr2.sum(axis=0).scale2(-0.5) + lp.sum(axis=0),
           "grad": -(exact(c) * prec),
           "gradhyp": (exact(lv).scale2(0.5) * (sr2 - 1.0)[:, None]).sum(axis=0),
           "gradpara": (sr2.sum(axis=0) - float(p))[None],
           "diaghess": prec, "diaghessgradhyp": -(exact(lv) * prec[:, None]),
           "diaghessgradpara": prec.scale2(-2.0)[:, None]}
    if g is not None:
        out["hessmult"] = exact(np.asarray(g, dtype=ld)) * prec
    return out


# ---- the diagonal marginal adjustment -------------------------------------------------------------------------
def margadj_diag(lik, pr):
    """lpdfvec::buildhess in its diagonal form (fit.cpp:252-268) from the members' diaghess family:
    val = -1/2 sum log D, gradhyp = -1/2 sum_k dD_k / D_k, gradpara likewise per member
    (gradpara_lik / gradpara_pr), D = the total diagonal (totdiaghess)"""
    D = lik["diaghess"] + pr["diaghess"]
    dD = lik["diaghessgradhyp"] + pr["diaghessgradhyp"]
    return {"totdiaghess": D, "val": D.log().sum(axis=0).scale2(-0.5),
            "gradhyp": (dD / D[:, None]).sum(axis=0).scale2(-0.5),
            "gradpara_lik": (lik["diaghessgradpara"] / D[:, None]).sum(axis=0).scale2(-0.5),
            "gradpara_pr": (pr["diaghessgradpara"] / D[:, None]).sum(axis=0).scale2(-0.5)}


def cat(*pairs):
    sh = [p.v.shape for p in pairs]
    return Pair(np.concatenate([p.v for p in pairs]),
                np.concatenate([np.broadcast_to(p.b, s) for p, s in zip(pairs, sh)]),
                np.concatenate([np.broadcast_to(p.s, s) for p, s in zip(pairs, sh)]))


def lpdfvec_diag(members, domarg=True, full=None):
    """{val, grad, gradhyp, gradpara, diaghess, diaghessgradhyp, diaghessgradpara} of lpdfvec(members[0],
    members[1]) (fit.cpp:323-380): members are (kind, dict) with kind "lik" or "pr"; gradpara and the columns
    of diaghessgradpara in list order.  full: margadj_full's answer, which then replaces the diagonal form of
    the adjustment (fit.cpp:270-299) while the diaghess family stays what buildhess made it."""
    (ka, a), (kb, b) = members
    lik, pr = (a, b) if ka == "lik" else (b, a)
    out = {"val": a["val"] + b["val"], "grad": a["grad"] + b["grad"], "gradhyp": a["gradhyp"] + b["gradhyp"],
           "gradpara": cat(a["gradpara"], b["gradpara"]), "diaghess": a["diaghess"] + b["diaghess"]}
    if domarg:
        m = margadj_diag(lik, pr) if full is None else full
        adj = {"lik": m["gradpara_lik"], "pr": m["gradpara_pr"]}
        out["val"] = out["val"] + m["val"]
        out["gradhyp"] = out["gradhyp"] + m["gradhyp"]
        out["gradpara"] = out["gradpara"] + cat(adj[ka], adj[kb])
        out["diaghessgradhyp"] = a["diaghessgradhyp"] + b["diaghessgradhyp"]
        za, zb = a["diaghessgradpara"], b["diaghessgradpara"]
        out["diaghessgradpara"] = Pair(np.concatenate([za.v, zb.v], axis=1),
                                       np.concatenate([np.broadcast_to(za.b, za.shape), np.broadcast_to(zb.b, zb.shape)], axis=1),
                                       np.concatenate([np.broadcast_to(za.s, za.shape), np.broadcast_to(zb.s, zb.shape)], axis=1))
    return out


def margadj_full(case, H, sigma, rho, N=1):
    """the full-Hessian adjustment (fit.cpp:270-299) by posterior_ref.ref_margadj on the float64 H BOTH sides
    hold (the Hessian the device built, itself held to `hess`), factored in long double; the backward error of a
    float64 factorisation is in the allowance.  Rows weighted by N are rows repeated."""
    assert case.n <= CHUNK
    _, B, dB = next(iter(case.chunks()))
    om = case.om
    prec, rel, lv = PR.prior_ld(om.basisvar, om.knotptst, om.logbasisvar_gradhyp, om.gest, om.hypmatch, case.terms, rho)
    rep = lambda a: np.concatenate([a] * N, axis=0)
    r = PR.ref_margadj(PR.cholesky_ld(H), rep(B.v), rep(B.b), rep(dB.v), rep(dB.b), sigma, rho, prec, rel, lv, True)
    gp = [Pair(r["gradpara"][0][i], r["gradpara"][1][i], r["gradpara"][2][i])[None] for i in (0, 1)]
    return {"val": Pair(*r["val"]), "gradhyp": Pair(*r["gradhyp"]), "gradpara_lik": gp[0], "gradpara_pr": gp[1]}


def oracle_margadj_full(case, H, sigma, rho, N=1):
    """the float64 host route of the same (posterior_ref.host_margadj64)"""
    import ob_oracle as O
    bo = O.OuterBase(case.om, np.tile(case.x, (N, 1)), dograd=True)
    r = PR.host_margadj64(H, O.ob_getmat(bo, case.terms), O.ob_getmat_gradhyp(bo, case.terms), sigma, rho,
                          O.prior_prec(case.om, case.terms, rho), case.om.getlvar_gradhyp(case.terms))
    return {"val": r["val"], "gradhyp": r["gradhyp"], "gradpara_lik": r["gradpara"][:1], "gradpara_pr": r["gradpara"][1:]}


# ---- predictors ------------------------------------------------------------------------------------------------
def predict(case, xnew, coeff, para, kind, D=None, H=None, doda=True):
    """{mean, var} at the rows xnew of pred_gauss (loglik_gauss.cpp:196-227), predr_std (loglik_std.cpp:218-256) and
    pred_gda (loglik_gda.cpp:247-281).  D: the total diagonal the pair handed over (totdiaghess, a Pair; None:
    never set, no coefficient variance); H: the full total Hessian both sides hold (predr_std after optnewton:
    posterior_ref.ref_var).  predr_std without the full Hessian puts totdiaghess ITSELF on the diagonal of the
    coefficient covariance (loglik_std.cpp:228-232), the other two its reciprocal; pred_gda adds e^{2 para[1]}
    residvar at the new rows."""
    new = Case(case.om, xnew, np.zeros(len(xnew)), case.terms)
    c = np.asarray(coeff, dtype=ld)
    _, B, _ = next(iter(new.chunks(grad=False)))
    out = {"mean": (B * c[None, :]).sum(axis=1)}
    if kind == "std" and H is not None:
        want, bound, rest, _ = PR.ref_var(PR.cholesky_ld(H), B.v, B.b, para[0], True)
        out["var"] = Pair(want, bound, rest)
        return out
    noise = pexp(2.0 * para[0])
    Bsq = B * B
    if D is None:
        var = noise + exact(np.zeros(len(xnew)))
    else:
        var = (Bsq * (D if kind == "std" else 1.0 / D)[None, :]).sum(axis=1) + noise
    if kind == "gda" and doda:
        varc, _ = new.varc()
        var = var + pexp(2.0 * para[1]) * (1.0 - (Bsq * varc[None, :]).sum(axis=1))
    out["var"] = var
    return out


# ---- loglik_gda ----------------------------------------------------------------------------------------------
def loglik_gda(case, coeff, para, g=None, doda=True):
    """{name: Pair} of loglik_gda::buildstd + update + the diaghess family (loglik_gda.cpp:117-235).  residvar
    = 1 - B^2 varc is a difference of two numbers near 1 when the expansion explains almost everything: its
    Pair carries bB and the rounding of the sum at the size of B^2 varc, not of the difference, and obssd,
    val and every gradient inherit that."""
    c = np.asarray(coeff, dtype=ld)
    n, nh = case.n, case.nhyp
    e0, e1 = pexp(2.0 * para[0]), pexp(2.0 * para[1])
    varc, lv = case.varc()
    gv = None if g is None else np.asarray(g, dtype=ld)
    acc = {k: Acc() for k in ("q2", "logsd", "grad", "gh1", "gh2", "gp", "dh", "dhgh", "dhgh2", "dhgp", "hm")}
    rows = {"residvar": [], "obssd": [], "residvar_gradhyp": [], "obssd_gradhyp": [], "obssd_gradpara": []}
    for sl, B, dB in case.chunks():
        Bsq = B * B
        rv = 1.0 - (Bsq * varc[None, :]).sum(axis=1)                                # :221, modandbase.cpp:889-895
        obssd = (e0 + e1 * rv).sqrt() if doda else (e0 + exact(np.zeros(rv.shape))).sqrt()
        dBsq = (B[:, :, None] * dB).scale2(2.0)
        rvg = -(dBsq * varc[None, :, None]).sum(axis=1) \
            - (Bsq[:, :, None] * (exact(lv) * varc[:, None])[None, :, :]).sum(axis=1)   # modandbase.cpp:904-925
        ge = rvg * ((e1.scale2(0.5)) / obssd)[:, None]                                # :224-227
        gp0 = e0 / obssd                                                              # :229
        gp1 = e1 * rv / obssd if doda else exact(np.zeros(rv.shape))                  # :230
        gp = Pair(np.stack([gp0.v, gp1.v], axis=1),
                  np.stack([np.broadcast_to(gp0.b, gp0.shape), np.broadcast_to(gp1.b, gp1.shape)], axis=1),
                  np.stack([np.broadcast_to(gp0.s, gp0.shape), np.broadcast_to(gp1.s, gp1.shape)], axis=1))
        rows["residvar"].append(rv), rows["obssd"].append(obssd), rows["residvar_gradhyp"].append(rvg)
        rows["obssd_gradhyp"].append(ge), rows["obssd_gradpara"].append(gp)
        yhat = (B * c[None, :]).sum(axis=1)
        q = (yhat - case.y[sl]) / obssd                                               # :126
        q2 = q * q
        acc["q2"].add(q2), acc["logsd"].add(obssd.log())
        rr = -(q / obssd)
        r2s = q2 / obssd
        acc["grad"].add(B * rr[:, None])
        yge = (dB * c[None, :, None]).sum(axis=1)
        acc["gh1"].add(yge * rr[:, None])
        w = r2s - 1.0 / obssd                                                         # :139-150
        if doda:
            acc["gh2"].add(ge * w[:, None])
        acc["gp"].add(gp * w[:, None])
        w2 = 1.0 / (obssd * obssd)                                                    # :177-180
        acc["dh"].add(Bsq * w2[:, None])
        acc["dhgh"].add(dBsq * w2[:, None, None])
        t2 = w2 * (-2.0 / obssd)                                                      # :187-214
        if doda:
            acc["dhgh2"].add(Bsq[:, :, None] * (ge * t2[:, None])[:, None, :])
        acc["dhgp"].add(Bsq[:, :, None] * (gp * t2[:, None])[:, None, :])
        if gv is not None:
            acc["hm"].add(B * ((B * gv[None, :]).sum(axis=1) * w2)[:, None])          # :160-169
    R = {k: a.result(n) for k, a in acc.items() if a.v is not None}
    out = {k: catrows(v) for k, v in rows.items()}
    out.update({"val": R["q2"].scale2(-0.5) - R["logsd"], "grad": R["grad"],
                "gradhyp": R["gh1"] + R["gh2"] if doda else R["gh1"], "gradpara": R["gp"],
                "diaghess": R["dh"], "diaghessgradhyp": R["dhgh"] + R["dhgh2"] if doda else R["dhgh"],
                "diaghessgradpara": R["dhgp"]})
    if gv is not None:
        out["hessmult"] = R["hm"]
    return out


def catrows(pairs):
    sh = [p.v.shape for p in pairs]
    return Pair(np.concatenate([p.v for p in pairs], axis=0),
                np.concatenate([np.broadcast_to(p.b, s) for p, s in zip(pairs, sh)], axis=0),
                np.concatenate([np.broadcast_to(p.s, s) for p, s in zip(pairs, sh)], axis=0))


# ---- the float64 oracle's answers under the same names (what C is measured from) -----------------------------
def oracle_loglik_gauss(case, coeff, sigma, g=None, N=1, grads=True):
    import math
    import ob_oracle as O
    om, t = case.om, case.terms
    x, y = np.tile(case.x, (N, 1)), np.tile(case.y, N)
    e2 = math.exp(-2 * sigma)
    if not grads:
        bo = O.OuterBase(om, x)
        d = O.ob_mm(bo, t, np.asarray(coeff, dtype=np.float64)) - y
        sq = O.ob_sqcolsums(bo, t)
        out = {"val": -0.5 * e2 * np.sum(d * d) - len(y) * sigma, "grad": O.ob_tmm(bo, t, -e2 * d),
               "gradpara": np.array([e2 * np.sum(d * d) - len(y)]), "sqcolsums": sq, "diaghess": e2 * sq,
               "diaghessgradpara": (-2 * e2 * sq)[:, None]}
        if g is not None:
            out["hessmult"] = e2 * O.ob_tmm(bo, t, O.ob_mm(bo, t, np.asarray(g, dtype=np.float64)))
        return out
    bo = O.OuterBase(om, x, dograd=True)
    val, grad, gh, gp = O.loglik_update(bo, t, y, sigma, np.asarray(coeff, dtype=np.float64))
    sq, dsq = O.ob_sqcolsums(bo, t), O.ob_sqcolsums_gradhyp(bo, t)
    out = {"val": val, "grad": grad, "gradhyp": gh, "gradpara": gp, "sqcolsums": sq, "sqcolsums_gradhyp": dsq,
           "diaghess": e2 * sq, "diaghessgradhyp": e2 * dsq, "diaghessgradpara": (-2 * e2 * sq)[:, None]}
    if g is not None:
        out["hessmult"] = e2 * O.ob_tmm(bo, t, O.ob_mm(bo, t, np.asarray(g, dtype=np.float64)))
    return out


def oracle_logpr_gauss(case, coeff, rho, g=None):
    import ob_oracle as O
    om, t = case.om, case.terms
    val, grad, gh, gp = O.logpr_update(om, t, rho, np.asarray(coeff, dtype=np.float64))
    prec = O.prior_prec(om, t, rho)
    out = {"val": val, "grad": grad, "gradhyp": gh, "gradpara": gp, "diaghess": prec,
           "diaghessgradhyp": -om.getlvar_gradhyp(t) * prec[:, None], "diaghessgradpara": (-2 * prec)[:, None]}
    if g is not None:
        out["hessmult"] = np.asarray(g, dtype=np.float64) * prec
    return out


def oracle_margadj_diag(case, sigma, rho, N=1):
    import ob_oracle as O
    bo = O.OuterBase(case.om, np.tile(case.x, (N, 1)), dograd=True)
    v, gh, gl, gp = O.margadj_diag(bo, case.terms, sigma, rho)
    return {"val": v, "gradhyp": gh, "gradpara_lik": np.array([gl]), "gradpara_pr": np.array([gp])}


def oracle_loglik_gda(case, coeff, para, g=None, doda=True):
    import ob_oracle as O
    bo = O.OuterBase(case.om, case.x, dograd=True)
    r = O.loglik_gda_update(bo, case.terms, case.y, np.asarray(para, dtype=np.float64),
                            np.asarray(coeff, dtype=np.float64), dodiag=doda)
    r["residvar"] = O.ob_residvar(bo, case.terms)
    r["residvar_gradhyp"] = O.ob_residvar_gradhyp(bo, case.terms)
    if g is not None:
        v = O.ob_mm(bo, case.terms, np.asarray(g, dtype=np.float64)) / np.square(r["obssd"])
        r["hessmult"] = O.ob_tmm(bo, case.terms, v)
    return r


# ---- measuring -----------------------------------------------------------------------------------------------
def oracle_ratio(got64, want):
    """{name: the float64 route's max(err / b) over the entries that depend on B (b > 0)} -- the measured C"""
    out = {}
    for name, pair in want.items():
        if name not in got64:
            continue
        b = np.broadcast_to(pair.b, pair.v.shape)
        got = np.reshape(_f64(got64[name]), pair.v.shape)
        err = _f64(np.abs(np.asarray(got, dtype=ld) - pair.v))
        out[name] = float(np.max(err[b > 0] / b[b > 0])) if np.any(b > 0) else 0.0
    return out


def entry_ratio(case, grads=True):
    """{"B", "dB"}: the float64 oracle's max |entry - want| / bound over the entries of B and dB / dhyp themselves
    -- C is the accuracy of a side's evaluation of B in units of bB, and this is where it shows unmixed with any
    later rounding.  C belongs to the case (model, terms), not to its rows: a case of more than CHUNK rows is
    measured on its first chunk, and -- as posterior_ref.var_case does, for its reason: the maximum of err / bound
    over a row or two is noise -- a case of fewer than 65 rows also on posterior_ref.PROBE_ROWS seeded rows of the
    same model and terms."""
    import ob_oracle as O
    sl, B, dB = next(iter(case.chunks(grads)))
    bo = O.OuterBase(case.om, case.x[sl], dograd=grads)
    out = {"B": E.worst_ratio(O.ob_getmat(bo, case.terms), B.v, B.b)}
    if grads:
        out["dB"] = E.worst_ratio(O.ob_getmat_gradhyp(bo, case.terms), dB.v, dB.b)
    if case.n < 65:
        xp = PR.inside_rows(PR.PROBE_ROWS, 9, case.om.kinds)
        probe = entry_ratio(Case(case.om, xp, np.zeros(len(xp)), case.terms), grads)
        out = {k: max(v, probe[k]) for k, v in out.items()}
    return out


def oracle_need(got64, want):
    """{name: the C the float64 route needs on top of the rounding allowance, max (err - s)+ / b} -- for what is built
    on B through further arithmetic (1 - B^2 varc, quotients, logarithms), where err / b alone would charge the
    roundings of that arithmetic to B; inf where an entry without any b misses its allowance"""
    out = {}
    for name, pair in want.items():
        if name not in got64:
            continue
        b, s = np.broadcast_to(pair.b, pair.v.shape), np.broadcast_to(pair.s, pair.v.shape)
        err = _f64(np.abs(np.asarray(np.reshape(_f64(got64[name]), pair.v.shape), dtype=ld) - pair.v))
        over = np.maximum(err - s, 0.0)
        r = float(np.max(over[b > 0] / b[b > 0])) if np.any(b > 0) else 0.0
        out[name] = float("inf") if np.any(over[b <= 0] > 0) else r
    return out


def constant_of(*ratio_dicts):
    """(C, r) of a case from the oracle's ratios of all its quantities"""
    r = max([0.0] + [v for d in ratio_dicts for v in d.values()])
    return E.constant_from_oracle_ratio(r), r


def ratios(got, want, C):
    """{name: worst |got - v| / (C b + s)} over EVERY entry of every quantity both sides name; an entry whose
    tolerance is 0 must be matched exactly (extended_ref.ratio_map), a NaN on either side is inf"""
    out = {}
    for name, pair in want.items():
        if name not in got:
            continue
        g = np.reshape(_f64(got[name]), pair.v.shape)
        r = E.worst_ratio(g, pair.v, tol(pair, C))
        out[name] = r if np.all(np.isfinite(g)) and np.all(np.isfinite(_f64(pair.v))) else float("inf")
    return out


# ---- the pair as a state machine ------------------------------------------------------------------------------------
class Session:
    """lpdfvec(a, b) of one likelihood ("gauss" | "std" | "gda") and logpr_gauss, `order` = ("pr", "lik") or
    ("lik", "pr"), as the sequence of calls of obmod.py's lpdf class sees it.  It holds the STATE (model, terms,
    parameters, coefficients, flags) and the reference's cache rules, never a previous answer: every expected
    quantity is computed from scratch from the current state by the stateless functions above.

    The rules (fit.cpp:208-245, 252-302): buildhess runs inside update() when updateom / updatepara / updateterms
    (or a change of domarg) came since the last one, and what it made -- the diaghess family of the pair and the
    adjustment -- stays until then, so those reads are DEFINED only while nothing has changed since the last
    update(); the adjustment is the full-Hessian one from optnewton on (fullhess), through later updates and
    rebuilds, until optcg, which drops it (LpdfVec::optcg) and returns to the diagonal form.  update() defines
    val / grad under their flags and gradhyp / gradpara only together with grad (loglik_gauss.cpp:120-130 forms
    them from the residual of the gradient pass); optnewton / optcg end in an update with all four.  loglik_gda
    builds its observation standard deviations in update() and in the diaghess family, not in hessmult
    (loglik_gda.cpp:160-169): its hessmult is defined only after one of those at the current state."""

    def __init__(self, om, x, y, terms, kind, order, N=1):
        self.om, self.x, self.y, self.terms, self.kind, self.order, self.N = om, x, y, np.asarray(terms), kind, tuple(order), N
        p0 = para0_gda(y) if kind == "gda" else para0_gauss(y, N)
        self.para = {"lik": [float(p0.v)] + ([0.0] if kind == "gda" else []), "pr": [6.0]}
        self.flags = dict(val=True, grad=True, gradhyp=False, gradpara=False)
        self.domarg, self.fullhess, self.doda = True, False, True
        self.coeff = None
        self.built = self.std_built = False       # buildhess / buildstd hold for the current state
        self.case = Case(om, x, y, self.terms)

    # -- the state changes -------------------------------------------------------------------------------------
    def updatepara(self, para):
        k = len(self.para[self.order[0]])
        self.para[self.order[0]], self.para[self.order[1]] = list(map(float, para[:k])), list(map(float, para[k:]))
        self.built = self.std_built = False

    def updateom(self, om):
        self.om, self.case = om, Case(om, self.x, self.y, self.terms)
        self.built = self.std_built = False

    def updateterms(self, terms):
        self.terms = np.asarray(terms)
        self.case = Case(self.om, self.x, self.y, self.terms)
        self.built = self.std_built = False
        self.coeff = None

    def set_domarg(self, v):
        if v != self.domarg:
            self.built = False
        self.domarg = v

    def set_doda(self, v):
        self.doda, self.std_built = v, False
        self.built = False      # the likelihood's diagonal changes behind the pair's back: rebuilt by the caller's updatepara

    def para_vector(self):
        return self.para[self.order[0]] + self.para[self.order[1]]

    # -- the members and the pair at the current state ------------------------------------------------------------
    def lik(self, coeff, g=None):
        if self.kind == "gda":
            return loglik_gda(self.case, coeff, self.para["lik"], g, self.doda)
        return loglik_gauss(self.case, coeff, self.para["lik"][0], g, self.N, hess=self.kind == "std")

    def pr(self, coeff, g=None):
        return logpr_gauss(self.case, coeff, self.para["pr"][0], g)

    def pair_parts(self, coeff, g=None):
        """the pair without any adjustment"""
        return self.pair(coeff, None, g, adjust=False)

    def pair(self, coeff, H=None, g=None, adjust=True):
        """H: the device's total Hessian, needed while the full adjustment is in force"""
        lik, pr = self.lik(coeff, g), self.pr(coeff, g)
        parts = {"lik": lik, "pr": pr}
        full = None
        if adjust and self.domarg and self.fullhess:
            assert H is not None
            full = margadj_full(self.case, H, self.para["lik"][0], self.para["pr"][0], self.N)
        out = lpdfvec_diag([(k, parts[k]) for k in self.order], adjust and self.domarg, full)
        if g is not None:
            out["hessmult"] = lik["hessmult"] + pr["hessmult"]
        if self.kind == "std":
            p = self.case.p
            out["hess"] = lik["hess"] + Pair(np.diag(pr["diaghess"].v), 0.0, np.diag(np.broadcast_to(pr["diaghess"].s, (p,))))
        return out

    # -- the calls ---------------------------------------------------------------------------------------------------
    def update(self, coeff, H=None):
        """what update(coeff) defines under the current flags"""
        self.coeff = np.asarray(coeff, dtype=np.float64)
        self.built = True
        self.std_built = True
        f = self.flags
        want = self.pair(self.coeff, H)
        names = (["val"] if f["val"] else []) + (["grad"] if f["grad"] else []) + \
            (["gradhyp"] if f["grad"] and f["gradhyp"] else []) + (["gradpara"] if f["grad"] and f["gradpara"] else [])
        return {k: want[k] for k in names}

    def after_opt(self, coeff, newton, H=None):
        """optnewton / optcg ended at the device's coefficients `coeff`: flags as fit.cpp:87-93, 122-128 leave them,
        everything defined"""
        self.fullhess = bool(newton)
        self.flags = dict(val=True, grad=True, gradhyp=False, gradpara=False)
        self.coeff = np.asarray(coeff, dtype=np.float64)
        self.built = self.std_built = True
        want = self.pair(self.coeff, H)
        return {k: want[k] for k in ("val", "grad", "gradhyp", "gradpara")}

    def newton_system(self):
        """(H, r) of the Newton step from zero: hess of the pair and its gradient at coeff = 0, as Pairs"""
        w = self.pair_parts(np.zeros(self.case.p))
        return w["hess"], w["grad"]

    def reads(self, g, H=None):
        """(of the pair, of the likelihood alone): hessmult and the diaghess family, where DEFINED"""
        pair = self.pair(self.coeff if self.coeff is not None else np.zeros(self.case.p), H, g)
        lik = self.lik(self.coeff if self.coeff is not None else np.zeros(self.case.p), g)
        po = {}
        if self.kind != "gda" or self.std_built:
            po["hessmult"] = pair["hessmult"]
        if self.built:
            po["diaghess"] = pair["diaghess"]
            if self.domarg:
                po["diaghessgradhyp"], po["diaghessgradpara"] = pair["diaghessgradhyp"], pair["diaghessgradpara"]
        lo = {k: lik[k] for k in ("diaghess", "diaghessgradhyp", "diaghessgradpara")}
        if self.kind != "gda" or self.std_built:
            lo["hessmult"] = lik["hessmult"]
        return po, lo
