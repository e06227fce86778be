"""Extended-precision host reference of the input gradients of the latent variance and of the acquisition criteria
(csrc/acquire_dx.cpp, kernels_acquire_dx.hip): the instrument test_gpu_acquire_grad.py measures
the device with, and test_acquire_grad_host.py proves against central differences of its own scores and shows which
failures it can see.  acquire_ref, extended_dx_ref and posterior_ref are imported unchanged; the rules are theirs.

np.longdouble, NumPy and mpmath.  B, dB / dx_l and their conditioning bB, bdB come from extended_dx_ref.ExtendedRefDx,
inv(H) = W^T W from posterior_ref.cholesky_ld and inverse_ld (W = inv(L)).  With t_i = inv(H) b_i:

    mu_i = b_i^T theta      dmu_i/dx_l = (db_i/dx_l)^T theta      d_i = b_i^T t_i      dd_i/dx_l = 2 (db_i/dx_l)^T t_i

and the four scores and their gradients from those with Phi and phi from mpmath at 50 digits (gradient_mp):

    EI        -Phi(u) dmu~ + phi(u) dsd                PI         phi(u) (-dmu~ - u dsd) / sd
    LCB       kappa dsd - dmu~                         straddle   kappa dsd - sign(mu~ - level) dmu~

mu~ = sgn mu, dmu~ = sgn dmu, dsd = dd / (2 sd), t = best - xi - mu~, u = t / sd.

Allowances.  Every quantity reaches the device as float64 sums of K = p summands and is held to C x bound + rest with
bound = K x (the sum of the magnitudes of everything added to reach it), as acquire_ref does.  With aB = |b| + bB,
adB_l = |db/dx_l| + bdB_l and G = |W|^T |W| (the magnitudes inside inv(H) as the device forms it, X X^T):

    mu     aB . |theta|                  dmu_l   adB_l . |theta|
    d      aB^T G aB                     dd_l    2 adB_l^T G aB

d is bounded as the device forms it -- b^T (S b), S explicit -- and not as acquire's || L^-1 b ||^2, a sum of squares:
what cancels inside S b is counted.  Each score gradient carries the four bounds through its exact partial
derivatives, as acquire_ref.score_bounds carries those of mu and d through the scores.  With dm, dsd the perturbations
of mu~ and sd (dsd = bound_d / (2 sd)), gm = dmu~_l, gs = dsd_l, and their perturbations dgm = bound_dmu_l and
dgs = bound_dd_l / (2 sd) + |gs| / sd dsd (gs depends on sd through 1 / (2 sd)), u moves by du = (dm + |u| dsd) / sd:

    EI        phi |gm + u gs| du + Phi dgm + phi dgs
    PI        phi / sd |u gm + (u^2 - 1) gs| du + |g| / sd dsd + phi / sd (dgm + |u| dgs)
    LCB, straddle   dgm + kappa dgs

The evaluation term `rest` (not multiplied by C) counts the roundings of forming the gradient in float64 from the
formula, as acquire_ref does for the scores: t = best - xi - mu~ and sd move the ARGUMENT by 2 (|best| + |xi| + |mu|) U
and 3 sd U, which go through the same partials (dm and dsd above); erfc counts 16, exp 3 and its constant 1 and
-u^2 / 2 two (2 u^2 relatively on phi); 1 / (2 sd), its product with dd, the two products with the coefficients and the
sum count 6 on the magnitudes of the two terms.

C is never a constant of this module and never measured from the device: every test measures the float64 restatement
of the device's operation order (restatement64: explicit S = Linv^T Linv, Y = S B^T, d = sum_k Y_k B_k, NumPy on the
float64 oracle's B and extended_dx_ref.dB_f64) on the same case and takes extended_ref.constant_from_oracle_ratio of
its worst (err - rest) / bound over all six outputs: eight times it, at most extended_ref.C_CAP.
"""
import functools

import numpy as np

import acquire_ref as A
import extended_dx_ref as X
import extended_ref as E
import posterior_ref as P
from extended_ref import ld

QUANTITIES = ("score", "grad", "mean", "grad_mean", "var", "grad_var")
MUTATIONS = ["factor 2 of dd dropped", "rho term dropped", "dsd without 1/(2 sd)", "maximize not applied to dmu",
             "sign dropped", "S replaced by diag(c)"]
_f64 = A._f64


class Case:
    pass


def make_case(om_o, terms, n, seed, xrows=None):
    """acquire_ref.seeded_case (H, theta, the rows) with the derivative side added: everything both routes need"""
    a = A.seeded_case(om_o, terms, n, seed, xcand=xrows)
    assert a.finite.all()
    c = Case()
    c.a, c.om_o, c.terms, c.H, c.sigma, c.theta, c.x = a, om_o, terms, a.H, a.sigma, a.theta, a.xcand
    c.n, c.p, c.d = a.m, a.p, om_o.d
    c.ref = X.reference_dx_of(om_o, c.x)
    c.B, c.bB = a.B, a.bB
    dB = [c.ref.getmat_dx(terms, l) for l in range(c.d)]
    c.dB = np.stack([v for v, _ in dB], axis=2)                     # n x p x d
    c.bdB = np.stack([_f64(b) for _, b in dB], axis=2)
    c.L = P.cholesky_ld(c.H)
    c.W = P.inverse_ld(c.L)
    S = c.W.T @ c.W
    th = np.array(c.theta, dtype=ld)
    c.T = c.B @ S                                                   # row i: t_i = S b_i
    c.mu = c.B @ th
    c.dv = np.einsum("ik,ik->i", c.B, c.T)
    c.dmu = np.einsum("ikl,k->il", c.dB, th)
    c.dd = 2 * np.einsum("ikl,ik->il", c.dB, c.T)
    # the magnitudes
    aB, adB = np.abs(_f64(c.B)) + _f64(c.bB), np.abs(_f64(c.dB)) + c.bdB
    aW = np.abs(_f64(c.W))
    G = aW.T @ aW
    GaB = aB @ G                                                    # n x p
    K = c.p
    c.bound = dict(mean=K * (aB @ np.abs(c.theta)), var=K * np.einsum("ik,ik->i", aB, GaB),
                   grad_mean=K * np.einsum("ikl,k->il", adB, np.abs(c.theta)),
                   grad_var=K * 2 * np.einsum("ikl,ik->il", adB, GaB))
    c.Bo64, c.dB64 = a.Bo, X.dB_f64_of(om_o, c.x, terms)[1]
    return c


def configs_of(c):
    """the eight calls of a case: four criteria x two directions.  best is the lower (maximize: upper) decile of the
    latent means, xi a hundredth of their spread, level the float32-rounded midpoint of the two middle latent means"""
    mu = np.sort(_f64(c.mu))
    f = lambda v: float(np.float32(v))
    k = len(mu) // 2
    level = f(0.5 * (mu[k - 1] + mu[k])) if len(mu) > 1 else f(mu[0] + 1.0)
    return [A.Config(crit, best=f(np.quantile(mu, 0.9 if mx else 0.1)), xi=f(0.01 * (mu[-1] - mu[0])), kappa=1.96,
                     level=level, maximize=mx) for crit in A.CRITERIA for mx in (False, True)]


def cfg_index(crit, mx):
    return A.CRITERIA.index(crit) * 2 + int(mx)


# ---- the scores' gradients ----------------------------------------------------------------------------
def coeffs64(cfg, mu, d):
    """float64 (score, A, C, sd): d score = A dmu~ + C dsd, in the device's formulas with its d <= 0 rule -- dsd taken
    as 0 there by the caller, EI: A = -1 where t > 0 and 0 elsewhere, PI: A = C = 0"""
    ms, t, sd, u, Phi, phi = A.parts64(cfg, mu, d, cfg.sgn * cfg.best)
    pos = sd > 0
    with np.errstate(all="ignore"):
        if cfg.criterion == A.LCB:
            return cfg.kappa * sd - ms, -np.ones_like(ms), np.full_like(ms, cfg.kappa), sd
        if cfg.criterion == A.STRADDLE:
            df = ms - cfg.sgn * cfg.level
            return cfg.kappa * sd - np.abs(df), -np.sign(df), np.full_like(ms, cfg.kappa), sd
        if cfg.criterion == A.PI:
            return (np.where(pos, Phi, np.where(t > 0, 1.0, 0.0)), np.where(pos, -phi / sd, 0.0),
                    np.where(pos, -(phi * u) / sd, 0.0), sd)
        return (np.where(pos, t * Phi + sd * phi, np.maximum(t, 0.0)), np.where(pos, -Phi, np.where(t > 0, -1.0, 0.0)),
                np.where(pos, phi, 0.0), sd)


def gradient64(cfg, mu, d, dmu, dd, mutate=None):
    """(score, gradient) in float64 from mu, d (n) and dmu, dd (n x d): the device's epilogue"""
    score, Ac, Cc, sd = coeffs64(cfg, mu, d)
    sgn = 1.0 if mutate == "maximize not applied to dmu" else cfg.sgn
    if mutate == "sign dropped" and cfg.criterion == A.STRADDLE:
        Ac = -np.ones_like(Ac)
    with np.errstate(all="ignore"):
        hsd = np.where(sd > 0, 1.0 / (2.0 * sd), 0.0)
        if mutate == "dsd without 1/(2 sd)":
            hsd = np.where(sd > 0, 1.0, 0.0)
        dsd = np.where(hsd[:, None] == 0.0, 0.0, _f64(dd) * hsd[:, None])
    return score, Ac[:, None] * (sgn * _f64(dmu)) + Cc[:, None] * dsd


def gradient_mp(cfg, mu, d, dmu, dd):
    """(score, gradient) from the long-double mu, d, dmu, dd with mpmath at 50 digits -> long double"""
    mp = A._mp()
    n, dim = dmu.shape
    grad = np.zeros((n, dim), dtype=ld)
    score = A.score_mp(cfg, mu, d, ld(cfg.sgn * cfg.best))
    sgn, xi, kap = mp.mpf(cfg.sgn), mp.mpf(cfg.xi), mp.mpf(cfg.kappa)
    bst, lev = mp.mpf(cfg.sgn * cfg.best), mp.mpf(cfg.sgn * cfg.level)
    r2, c2 = mp.sqrt(2), mp.sqrt(2 * mp.pi)
    for i in range(n):
        ms, di = sgn * A.to_mp(mu[i]), A.to_mp(d[i])
        sd = mp.sqrt(di) if di > 0 else mp.mpf(0)
        t = bst - xi - ms
        if cfg.criterion == A.LCB:
            a, cc = mp.mpf(-1), kap
        elif cfg.criterion == A.STRADDLE:
            a, cc = -mp.sign(ms - lev), kap
        elif sd == 0:
            a, cc = (mp.mpf(-1 if t > 0 else 0) if cfg.criterion == A.EI else mp.mpf(0)), mp.mpf(0)
        else:
            u = t / sd
            Phi, phi = mp.erfc(-u / r2) / 2, mp.exp(-u * u / 2) / c2
            a, cc = (-Phi, phi) if cfg.criterion == A.EI else (-phi / sd, -phi * u / sd)
        for l in range(dim):
            gs = A.to_mp(dd[i, l]) / (2 * sd) if sd > 0 else mp.mpf(0)
            grad[i, l] = A.from_mp(a * sgn * A.to_mp(dmu[i, l]) + cc * gs)
    return score, grad


def gradient_bounds(cfg, mu, d, dmu, dd, bmu, bd, bdmu, bdd, rnd=E.U):
    """(bound, rest) of a score gradient, n x d each: the allowances of mu, d, dmu, dd through the exact partial
    derivatives, and the evaluation term (module docstring)"""
    ms, t, sd, u, Phi, phi = (v[:, None] if np.ndim(v) else v for v in A.parts64(cfg, mu, d, cfg.sgn * cfg.best))
    gm = cfg.sgn * _f64(dmu)
    bmu, bd = _f64(bmu)[:, None], _f64(bd)[:, None]
    with np.errstate(all="ignore"):
        gs = _f64(dd) / (2 * sd)
        au = np.abs(u)
        mag = abs(cfg.best) + abs(cfg.xi) + np.abs(ms)

        def through(dm, dsd, dgm, dgdd):
            dgs = dgdd / (2 * sd) + np.abs(gs) / sd * dsd
            du = (dm + au * dsd) / sd
            if cfg.criterion == A.EI:
                return phi * np.abs(gm + u * gs) * du + Phi * dgm + phi * dgs
            if cfg.criterion == A.PI:
                g = phi * (-gm - u * gs) / sd
                return phi / sd * np.abs(u * gm + (u * u - 1) * gs) * du + np.abs(g) / sd * dsd + phi / sd * (dgm + au * dgs)
            return dgm + cfg.kappa * dgs
        bound = through(bmu, bd / (2 * sd), _f64(bdmu), _f64(bdd))
        rest = through(2 * mag, 3 * sd, 0.0, 0.0)
        if cfg.criterion == A.EI:
            rest = rest + 16 * Phi * np.abs(gm) + (4 + 2 * u * u) * phi * np.abs(gs) + 6 * (Phi * np.abs(gm) + phi * np.abs(gs))
        elif cfg.criterion == A.PI:
            rest = rest + (4 + 2 * u * u + 6 + 2) * phi / sd * (np.abs(gm) + au * np.abs(gs))
        else:
            rest = rest + 6 * (np.abs(gm) + cfg.kappa * np.abs(gs))
        rest = rnd * rest
    return np.where(np.isnan(bound), np.inf, bound), np.where(np.isnan(rest), np.inf, rest)


def reference(c, cfg):
    """{quantity: (want, bound, rest)} of one call, long double wants and float64 bounds without C"""
    key = cfg.key()
    if key not in c.a.cache:
        score, grad = gradient_mp(cfg, c.mu, c.dv, c.dmu, c.dd)
        b = c.bound
        bs, rs = A.score_bounds(cfg, c.mu, c.dv, cfg.sgn * cfg.best, b["mean"], b["var"])
        bg, rg = gradient_bounds(cfg, c.mu, c.dv, c.dmu, c.dd, b["mean"], b["var"], b["grad_mean"], b["grad_var"])
        c.a.cache[key] = dict(score=(score, bs, rs), grad=(grad, bg, rg), mean=(c.mu, b["mean"], 0.0),
                              grad_mean=(c.dmu, b["grad_mean"], 0.0), var=(c.dv, b["var"], 0.0),
                              grad_var=(c.dd, b["grad_var"], 0.0))
    return c.a.cache[key]


# ---- the float64 restatement in the device's operation order -----------------------------------------
def restatement64(c, cfg=None, mutate=None):
    """the six outputs (cfg None: var and grad_var only) in NumPy float64 on the float64 oracle's B and dB: explicit
    S = Linv^T Linv as the device forms X X^T, Y = S B^T stored, then d = sum_k Y_k B_k and dd = 2 sum_k Y_k dB_kl, mu
    and dmu with theta, and the epilogue of gradient64.  mutate: one of MUTATIONS."""
    if "Linv64" not in c.a.cache:
        c.a.cache["Linv64"] = np.linalg.solve(np.linalg.cholesky(c.H), np.eye(c.p))
    Linv = c.a.cache["Linv64"]
    B, dB = c.Bo64, c.dB64
    if mutate == "rho term dropped":
        # dB_kl = s (rho_l P_k + E_kl r'): without the first part.  rho_l is dimension l's gradient factor at level 0
        rho = np.stack([_f64(c.ref.g[l][:, 0]) for l in range(c.d)], axis=1)
        dB = dB - B[:, :, None] * rho[:, None, :]
    S = Linv.T @ Linv
    if mutate == "S replaced by diag(c)":
        S = np.diag(np.diag(S))
    Y = B @ S                                                       # row i: S b_i
    var = np.einsum("ik,ik->i", Y, B)
    gvar = (1.0 if mutate == "factor 2 of dd dropped" else 2.0) * np.einsum("ikl,ik->il", dB, Y)
    out = dict(var=var, grad_var=gvar)
    if cfg is not None:
        mean, gmean = B @ c.theta, np.einsum("ikl,k->il", dB, c.theta)
        score, grad = gradient64(cfg, mean, var, gmean, gvar, mutate)
        out.update(score=score, grad=grad, mean=mean, grad_mean=gmean)
    return out


# ---- measuring ----------------------------------------------------------------------------------------
def ratios(got, ref, C=1.0, sub_rest=False, rows=None):
    """{quantity: worst |got - want| / (C x bound + rest)} over EVERY row (rows: the first `rows`) and entry of what
    got holds.  sub_rest: (|got - want| - rest)+ / (C x bound), what C is measured with."""
    out = {}
    for q in QUANTITIES:
        if got.get(q) is None:
            continue
        want, bound, rest = ref[q]
        sl = slice(None) if rows is None else slice(0, rows)
        want, bound = want[sl], _f64(bound)[sl]
        rest = rest[sl] if np.ndim(rest) else rest
        g = np.asarray(got[q], dtype=ld)
        assert g.shape == want.shape, q
        err = _f64(np.abs(g - want))
        if sub_rest:
            err, den = np.maximum(err - rest, 0.0), C * bound
        else:
            den = C * bound + rest
        r = np.zeros(err.shape)
        np.divide(err, den, out=r, where=den > 0)
        r[(den <= 0) & (err > 0)] = np.inf
        r[~np.isfinite(err)] = np.inf                               # a NaN where a number is due is an error
        out[q] = float(np.max(r)) if r.size else 0.0
    return out


def allowance(ref, q, C):
    want, bound, rest = ref[q]
    return C * _f64(bound) + rest


def constant_of(c, cfg):
    """(C, r): r = the float64 restatement's own worst (err - rest) / bound on this case and call"""
    r = max(ratios(restatement64(c, cfg), reference(c, cfg), 1.0, sub_rest=True).values())
    return E.constant_from_oracle_ratio(r), r


def conditions(c, cfg, C):
    """the conditions of a case, from the reference alone: -> (smallest d_i / allowance, smallest |mu~ - level| /
    allowance of mu; inf unless the criterion is the straddle)"""
    ref = reference(c, cfg)
    dmin = float(np.min(_f64(c.dv) / allowance(ref, "var", C)))
    lmin = np.inf
    if cfg.criterion == A.STRADDLE:
        lmin = float(np.min(np.abs(_f64(c.mu) - cfg.level) / allowance(ref, "mean", C)))
    return dmin, lmin


# ---- the cases both test files share ------------------------------------------------------------------
def _wide():
    from test_acquire_host import wide_model
    om_o, om_d, terms = wide_model()
    return om_o, om_d, terms


def _pg(name, p, kind="select"):
    import test_gpu_predict_grad as G
    m = G.model(name)
    terms = G.terms_of(name, p) if kind == "select" else G.case(name, p, kind)["terms"]
    return m["om_o"], m["om_d"], np.ascontiguousarray(terms)


def _acq(name, p):
    from test_acquire_host import model
    return model(name, p)


MIX8 = ["mat25", "mat25pow", "mat25ang", "mat25", "mat25pow", "mat25ang", "mat25", "mat25"]


@functools.lru_cache(maxsize=None)
def _mixed8(p):
    """eight dimensions of all three families, twenty knots each, hyper-parameters a few tenths off their defaults"""
    from conftest import knots_for, make_pair
    rng = np.random.default_rng(88)
    nh = sum(E.NUMHYP[k] for k in MIX8)
    om_o, om_d = make_pair(MIX8, knots_for(MIX8, 20), hyp=rng.uniform(0.1, 0.4, nh) * rng.choice([-1.0, 1.0], nh))
    terms = np.ascontiguousarray(om_o.selectterms(p))
    assert len(terms) == p
    return om_o, om_d, terms


def _const(name):
    om_o, om_d, _ = _acq(name, 5)
    return om_o, om_d, np.zeros((1, om_o.d), dtype=np.int64)


# name: (model and terms, rows, seed); see test_gpu_acquire_grad.py for why each is there
CASES = {
    "d3 p=5": (lambda: _acq("d3", 5), 129, 301),
    "d3 p=1": (lambda: _const("d3"), 65, 302),
    "d8 p=67": (lambda: _mixed8(67), 65, 303),
    "d5 p=130": (lambda: _acq("d5", 130), 300, 304),
    "d4 knots130 p=65": (lambda: _pg("d4 knots130", 65), 65, 305),
    "d11 9-11 factors": (lambda: _pg("d11", 40, "long"), 65, 316),
    "wide d=40 p=357": (_wide, 65, 307),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """the case, its eight calls -- computed once, shared, left unchanged"""
    make, n, seed = CASES[name]
    om_o, om_d, terms = make()
    c = make_case(om_o, terms, n, seed)
    c.om_d = om_d
    return c, configs_of(c)


@functools.lru_cache(maxsize=None)
def built(name, ci):
    """case, call, reference and the C of the two"""
    c, cfgs = case(name)
    cfg = cfgs[ci]
    Cc, r = constant_of(c, cfg)
    return dict(c=c, cfg=cfg, ref=reference(c, cfg), C=Cc, r=r)


def scores_at(c, cfg, x):
    """the long-double scores of the call cfg at other rows x of the same posterior: what the central differences of
    test_acquire_grad_host.py are taken from"""
    knots = [np.asarray(c.om_o.knots_of(k), dtype=np.float64) for k in range(c.om_o.d)]
    B, _ = E.ExtendedRef(c.om_o.kinds, knots, c.om_o.hyp, c.om_o.rotmat, x).getmat(c.terms)
    Z = c.W @ B.T
    return A.score_mp(cfg, B @ np.array(c.theta, dtype=ld), (Z * Z).sum(axis=0), ld(cfg.sgn * cfg.best))
