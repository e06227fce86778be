"""Host reference of the GLM fit (include/obhip.h, "weighted, binomial and Poisson responses"): the same
iteration in NumPy, in float64 and in np.longdouble.  It owns nothing of the library: it is fed a design
matrix B, the prior precisions P and the data, and restates the model from the header's formulas.

    F(theta) = sum_i a_i l(y_i, eta_i) - theta^T P theta / 2,   eta = o + B theta

Row pass (rows): mu, w, sqrt(w), the working column u = a (y - mu) (Gaussian: e^{-2 sigma}) / sqrt(w), the
sums (sum a l over the finite rows, the sum of the magnitudes a (|y eta| + |b(eta)|), the rows left out).
Iteration (fit): H = B^T W B + P, g = B^T (a (y - mu)) - P theta, delta = solve(H, g), dec = g^T delta; the
full step and stop when dec <= tol (1 + |F|); otherwise alpha halved from 1 until F(theta + alpha delta) is
finite and >= F(theta) - (n + p + 16) 2^-53 (A + A'), at most 30 halvings.

The long-double variant solves in float64 and refines three times with long-double residuals.
Shared by test_glm_host.py (which proves the float64 restatement against the long-double one on the cases
the GPU tests use) and test_gpu_glm.py.
"""
import functools

import numpy as np

ld = np.longdouble
U = 2.0 ** -53
GAUSSIAN, BINOMIAL, POISSON = 0, 1, 2
FAMILY_NAMES = {GAUSSIAN: "gaussian", BINOMIAL: "binomial", POISSON: "poisson"}
KINDS = ["mat25", "mat25pow", "mat25ang", "mat25"]
SIGMA = float(np.log(0.01))
TOL = 1e-13
MAX_HALVINGS = 30
# (n, p) of the converged-fit cases and the prior's rho: three families each
SIZES = [(1000, 129, 0.0), (3001, 260, 3.0)]
# iterations and halvings of this reference on them, per family (binomial: 5 at the first size, 6 at the second)
EXPECTED = {GAUSSIAN: (2, 0), BINOMIAL: None, POISSON: (6, 2)}


def link(family, eta):
    """mu, d mu / d eta, b(eta) (l = y eta - b) in the dtype of eta, the binomial forms free of overflow"""
    eta = np.asarray(eta)
    if family == BINOMIAL:
        e = np.exp(-np.abs(eta))
        d = 1 + e
        mu = np.where(eta >= 0, 1 / d, e / d)
        return mu, e / (d * d), np.maximum(eta, 0) + np.log1p(e)
    if family == POISSON:
        with np.errstate(over="ignore"):
            mu = np.exp(eta)
        return mu, mu, mu
    return eta, np.ones_like(eta), np.zeros_like(eta)


def rows(family, eta, y, a, sigma=SIGMA, scale=None, dtype=np.float64):
    """the row pass on n rows: dict(mu, w, sw, scale_w, u, l, mag, sums = [sum a l, sum mag, rows left out])"""
    eta, y, a = (np.asarray(v, dtype=dtype) for v in (eta, y, a))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mu, dmu, b = link(family, eta)
        if family == GAUSSIAN:
            e2 = np.exp(-2 * dtype(sigma))
            d = y - eta
            l = -e2 * d * d / 2
            mag = a * np.abs(l)
            w = a * e2
            res = a * d * e2
        else:
            ye = y * eta
            l = ye - b
            mag = a * (np.abs(ye) + np.abs(b))
            w = a * dmu
            res = a * (y - mu)
        al = a * l
        fin = np.isfinite(al) & np.isfinite(mag)
        live = (w > 0) & np.isfinite(w)
        sw = np.where(live, np.sqrt(np.where(live, w, 1)), 0)
        u = np.where(live, res / np.where(live, sw, 1), 0)
    out = dict(mu=mu, w=w, sw=sw, u=u, al=al, mag=mag, fin=fin,
               sums=[np.sum(al[fin]), np.sum(mag[fin]), int(np.sum(~fin))])
    if scale is not None:
        out["scale_w"] = np.asarray(scale, dtype=dtype) * sw
    return out


def saturated(family, y, a, dtype=np.float64):
    y, a = np.asarray(y, dtype=dtype), np.asarray(a, dtype=dtype)

    def xlogx(v):
        return np.where(v > 0, v * np.log(np.where(v > 0, v, 1)), 0)
    if family == BINOMIAL:
        return np.sum(a * (xlogx(y) + xlogx(1 - y)))
    if family == POISSON:
        return np.sum(a * (xlogx(y) - y))
    return dtype(0)


def _solve(H, g, dtype):
    H64 = np.asarray(H, dtype=np.float64)
    np.linalg.cholesky(H64)         # raises LinAlgError where the library returns OBHIP_ERR_NUMERIC
    if dtype is np.float64:
        return np.linalg.solve(H64, np.asarray(g, dtype=np.float64))
    Hi = np.linalg.inv(H64)         # one factorisation for the solve and its three refinements
    t = np.asarray(Hi @ np.asarray(g, dtype=np.float64), dtype=ld)
    for _ in range(3):
        t = t + np.asarray(Hi @ np.asarray(g - H @ t, dtype=np.float64), dtype=ld)
    return t


def fit(B, prec, family, y, a=None, o=None, sigma=SIGMA, tol=TOL, maxit=25, dtype=np.float64, theta0=None,
        hessian64=False):
    """-> dict(theta, eta, mu, iterations, halvings, converged, decs, thresholds, F, deviance, H (the last
    Hessian), w (the weights it was formed with)).  hessian64: the Hessian alone is formed in float64 (for term
    sets too large for a long-double matrix product); the gradient and the row pass stay in dtype, and the
    gradient alone decides where the iteration comes to rest."""
    B = np.asarray(B, dtype=dtype)
    n, p = B.shape
    P = np.asarray(prec, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    a = np.ones(n, dtype=dtype) if a is None else np.asarray(a, dtype=dtype)
    o = np.zeros(n, dtype=dtype) if o is None else np.asarray(o, dtype=dtype)
    theta = np.zeros(p, dtype=dtype) if theta0 is None else np.asarray(theta0, dtype=dtype)
    eta = o + B @ theta
    r = rows(family, eta, y, a, sigma, dtype=dtype)
    assert r["sums"][2] == 0, "F is not finite at the start"
    qtt = theta @ (P * theta)
    lik, mag, F = r["sums"][0], r["sums"][1] + qtt / 2, r["sums"][0] - qtt / 2
    ub = (n + p + 16) * U
    decs, thr, halvings, its, converged, H = [], [], 0, 0, False, None
    for _ in range(maxit):
        Bw = B * r["sw"][:, None]
        if hessian64:
            B64 = np.asarray(Bw, dtype=np.float64)
            H = np.asarray(B64.T @ B64, dtype=dtype) + np.diag(P)
        else:
            H = Bw.T @ Bw + np.diag(P)
        g = Bw.T @ r["u"] - P * theta
        delta = _solve(H, g, dtype)
        w_used = r["w"]
        dec = g @ delta
        qtt, qtd, qdd = theta @ (P * theta), theta @ (P * delta), delta @ (P * delta)
        bd = B @ delta
        decs.append(float(dec))
        thr.append(float(tol * (1 + abs(F))))
        assert np.isfinite(dec) and dec >= 0

        def prior_at(al):
            return (qtt + al * (2 * qtd + al * qdd)) / 2
        last = dec <= tol * (1 + abs(F))
        alpha = 1.0
        if not last:
            k = 0
            while True:
                assert k <= MAX_HALVINGS, "the line search found no step"
                tr = rows(family, eta + dtype(alpha) * bd, y, a, sigma, dtype=dtype)
                pr = prior_at(dtype(alpha))
                Ft = tr["sums"][0] - pr
                if tr["sums"][2] == 0 and np.isfinite(Ft) and Ft >= F - ub * (mag + tr["sums"][1] + pr):
                    break
                alpha *= 0.5
                halvings += 1
                k += 1
        theta = theta + dtype(alpha) * delta
        eta = eta + dtype(alpha) * bd
        r = rows(family, eta, y, a, sigma, dtype=dtype)
        pr = prior_at(dtype(alpha))
        its += 1
        assert r["sums"][2] == 0
        lik, mag, F = r["sums"][0], r["sums"][1] + pr, r["sums"][0] - pr
        if last:
            converged = True
            break
    dev = 2 * (saturated(family, y, a, dtype) - lik)
    return dict(theta=theta, eta=eta, mu=r["mu"], iterations=its, halvings=halvings, converged=converged, decs=decs,
                thresholds=thr, F=float(F), deviance=float(dev), H=H, w=w_used)


def relerr(got, want):
    """max |got - want| / max |want|, taken in long double"""
    got, want = np.asarray(got, dtype=ld), np.asarray(want, dtype=ld)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def threshold_distance(res):
    """how far, as a factor >= 1, the nearest dec of a run lies from its threshold: a dec close to it may fall
    on either side in another arithmetic, and the two runs would then stop an iteration apart"""
    worst = np.inf
    for d, t in zip(res["decs"], res["thresholds"]):
        d = max(d, 1e-300)
        worst = min(worst, max(d / t, t / d))
    return worst


def data(family, n, seed=3, kinds=KINDS):
    """(x, y, a, o) of the family's case on n rows: a smooth signal f of the synthetic response, trials
    1..5 (binomial), exposures 0.5..4 (Poisson), weights 2e3..5e4 (Gaussian)"""
    import ob_oracle as O
    x, ysyn = O.synth_xy(7, 0, n, kinds)
    f = (ysyn - ysyn.mean()) / ysyn.std()
    rng = np.random.default_rng(seed)
    if family == BINOMIAL:
        m = rng.integers(1, 6, n)
        y = rng.binomial(m, 1 / (1 + np.exp(-1.5 * f))) / m
        return x, y, m.astype(np.float64), None
    if family == POISSON:
        o = np.log(rng.uniform(.5, 4, n))
        y = rng.poisson(np.exp(.8 * f + 1 + o)).astype(np.float64)
        return x, y, None, o
    a = 1e4 * rng.uniform(.2, 5, n)
    y = f + .01 * rng.standard_normal(n)
    return x, y, a, None


@functools.lru_cache(maxsize=None)
def oracle_model():
    import ob_oracle as O
    om = O.OuterMod()
    om.setcovfs(KINDS)
    om.setknot(O.bench_knots(KINDS, 20))
    return om


@functools.lru_cache(maxsize=None)
def cpu_case(family, n, p, rho):
    """one converged-fit case on the oracle's B: the float64 and the long-double run, computed once"""
    import ob_oracle as O
    om = oracle_model()
    terms = om.selectterms(p)
    x, y, a, o = data(family, n)
    B = O.ob_getmat(O.OuterBase(om, x), terms)
    prec = O.prior_prec(om, terms, rho)
    r64 = fit(B, prec, family, y, a, o, dtype=np.float64)
    rl = fit(B, prec, family, y, a, o, dtype=ld)
    return dict(terms=terms, x=x, y=y, a=a, o=o, B=B, prec=prec, r64=r64, rl=rl)
