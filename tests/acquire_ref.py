"""Extended-precision host restatement of the acquisition picks (csrc/acquire.cpp, kernels_acquire.hip): the
instrument test_gpu_acquire.py measures the device with, and test_acquire_host.py proves against mpmath's own
Cholesky and against the recurrences, and shows which failures it can see.

np.longdouble, NumPy and mpmath, in the style of design_ref.py; B and its conditioning bB come from
extended_ref.ExtendedRef.  NO recurrence: at every step t, with the picks j_1 .. j_t and the values y*_1 .. y*_t
the runs were given,

    H_t = H + sum_s b_js b_js^T / nu,      theta_t = inv(H_t) (H theta + sum_s b_js y*_s / nu),      nu = e^{2 sigma},

is factored afresh (posterior_ref.cholesky_ld, forward_ld) and mu = B theta_t, d = diag(B inv(H_t) B^T) are taken
from Z = L_t^-1 B^T.  The four scores are evaluated from those with mpmath at 50 digits.  It FOLLOWS the picks it is
given (states(c, cfg, picks)), so that one disagreement does not cascade, or its own argmax, first among equals
(states(c, cfg, None, k)); the value a run is given is always the reference's own (believer: its mu_j).

At steps t >= 1 of a case with more than SCREEN rows only the rows whose float64 score lies within 1e-6 (relative
to the spread of the scores) of the float64 maximum are evaluated with mpmath -- the argmax and the runner-up are
among them; the others carry their float64 score.  Step 0 is always evaluated in full (score0 is compared in full).

Allowances.  mu and d reach the device as float64 sums of at most K = p + t summands, so they are held to

    |got - want|  <=  C x K x (sum of the magnitudes of everything added and subtracted to reach it):

for mu_i: (|b_i| + bB_i) . |theta| (the terms of the dot product and the magnitudes inside the knot sums of b_i),
and per step |a_is delta_s| / gamma_s plus |delta_s| / gamma_s times the magnitudes inside a_is = b_i^T S b_j, which
are (|b_i| + bB_i)^T |W|^T |W| (|b_j| + bB_j), W = inv(L_s): the factorisation's backward term; for d_i: d_i(0),
2 |z_i|^T |W| bB_i (posterior_ref.ref_var's bound), and per step a_is^2 / gamma_s plus 2 |a_is| / gamma_s times the
same magnitudes of a_is.  Each score carries those through its exact partial derivatives, with
tol_sd = tol_d / (2 sd):

    EI   Phi(u) tol_mu + phi(u) tol_sd        PI   phi(u) / sd (tol_mu + |u| tol_sd)        LCB, straddle   tol_mu + kappa tol_sd

plus an evaluation term (`rest`, not multiplied by C) for forming the score in float64, the roundings counted from
the formula.  t = best - xi - mu has 2 roundings of magnitude |best| + |xi| + |mu|, sd 1 (sqrt) and u = t / sd 1 more,
-u / sqrt 2 two (the product and the constant): they move the ARGUMENT, so they go through the same partials as
perturbations 2 (|best| + |xi| + |mu|) of mu and 3 sd of sd, plus 2 |u| phi(u) on Phi and (-u^2 / 2: 2 roundings) 2 u^2
on phi relatively.  Then the values: erfc counts 16 and the halving is exact, exp counts 3 and its constant 1, the two
products 1 each and the sum 1 --

    EI   U [Phi 2(|best| + |xi| + |mu|) + phi 3 sd + 2 |t| |u| phi + 2 u^2 sd phi + 18 |t| Phi + 6 sd phi]
    PI   U [phi / sd (2(|best| + |xi| + |mu|) + 3 |u| sd) + 2 |u| phi + 16 Phi]
    LCB  U 4 (|mu| + kappa sd)        straddle   U 4 (|mu| + |level| + kappa sd)

erfc = 16 and exp = 3 are OpenCL's full-profile bounds, which the device math library is built to: that rests on the
specification, not on a measurement.  The unit roundoff of the sums is carried by C, as in design_ref.py: C is never a
constant of this module and never measured from the device -- every test measures the float64 restatement of the
device's recurrences (recurrence64, NumPy on the float64 oracle's B) on the same case and takes
extended_ref.constant_from_oracle_ratio of its worst (err - rest) / bound: eight times it, at most extended_ref.C_CAP.
"""
import math

import numpy as np

import extended_ref as E
import posterior_ref as P
from extended_ref import ld

EI, PI, LCB, STRADDLE = "ei", "pi", "lcb", "straddle"
CRITERIA = [EI, PI, LCB, STRADDLE]
BELIEVER, CONSTANT = "believer", "constant"
LIES = [BELIEVER, CONSTANT]
SCREEN = 300
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def to_mp(x):
    """a long double exactly, as the sum of two floats"""
    mp = _mp()
    x = ld(x)
    hi = float(x)
    if not math.isfinite(hi):
        return mp.mpf(hi)
    return mp.mpf(hi) + mp.mpf(float(x - ld(hi)))


def from_mp(v):
    hi = float(v)
    if not math.isfinite(hi) or hi == 0.0:
        return ld(hi)
    return ld(hi) + ld(float(v - _mp().mpf(hi)))


class Case:
    pass


class Config:
    """one call's arguments, in the caller's sign: best, xi, kappa, level, maximize, lie, lie_value"""

    def __init__(self, criterion, best=0.0, xi=0.0, kappa=1.96, level=0.0, maximize=False, lie=BELIEVER, lie_value=0.0):
        self.criterion, self.best, self.xi, self.kappa, self.level = criterion, float(best), float(xi), float(kappa), float(level)
        self.maximize, self.lie, self.lie_value = bool(maximize), lie, float(lie_value)
        self.sgn = -1.0 if maximize else 1.0

    def key(self):
        return (self.criterion, self.best, self.xi, self.kappa, self.level, self.maximize)

    def __repr__(self):
        return "%s %s %s" % (self.criterion, self.lie, "max" if self.maximize else "min")


def make_case(om_o, terms, H, sigma, theta, xcand, skip=None):
    """everything both routes need of one problem; H and theta float64 (taken as exact)"""
    import ob_oracle as O
    E.require_extended()
    c = Case()
    knots = [np.asarray(om_o.knots_of(k), dtype=np.float64) for k in range(om_o.d)]
    c.terms, c.H, c.sigma, c.theta, c.xcand = terms, _f64(H), float(sigma), _f64(theta), xcand
    c.m, c.p = len(xcand), len(terms)
    c.nu = np.exp(2 * ld(sigma))
    c.skip = np.zeros(c.m, dtype=bool) if skip is None else np.asarray(skip) != 0
    c.finite = np.all(np.isfinite(xcand), axis=1)
    xs = np.where(np.isfinite(xcand), xcand, 0.5)                  # a row that is not finite: masked, never used
    c.B, c.bB = E.ExtendedRef(om_o.kinds, knots, om_o.hyp, om_o.rotmat, xs).getmat(terms)
    c.Bo = O.ob_getmat(O.OuterBase(om_o, xs), terms)
    c.aB = np.abs(_f64(c.B)) + _f64(c.bB)
    c.rhs0 = np.array(c.H, dtype=ld) @ np.array(c.theta, dtype=ld)
    c.cache = {}
    return c


# ---- the explicit states ------------------------------------------------------------------------------
def _state(c, picks, ystar, cholesky=P.cholesky_ld):
    key = (tuple(picks), tuple(float(y) for y in ystar))
    if cholesky is P.cholesky_ld and key in c.cache:
        return c.cache[key]
    Ht = np.array(c.H, dtype=ld)
    rhs = c.rhs0.copy()
    for j, y in zip(picks, ystar):
        Ht = Ht + np.outer(c.B[j], c.B[j]) / c.nu
        rhs = rhs + c.B[j] * (ld(y) / c.nu)
    L = cholesky(Ht)
    Z = P.forward_ld(L, c.B.T)                                     # p x m
    w = P.forward_ld(L, rhs[:, None])[:, 0]
    s = dict(L=L, Z=Z, mu=Z.T @ w, d=(Z * Z).sum(axis=0))
    if cholesky is P.cholesky_ld and len(picks) == 0:
        c.cache[key] = s
    return s


def parts64(cfg, mu, d, best):
    """float64 (t, sd, u, Phi, phi) of the signed problem; best: the signed incumbent"""
    ms = cfg.sgn * _f64(mu)
    sd = np.sqrt(np.maximum(_f64(d), 0.0))
    t = best - cfg.xi - ms
    with np.errstate(all="ignore"):
        u = t / sd
        Phi = 0.5 * _erfc(-u / math.sqrt(2.0))
        phi = np.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    return ms, t, sd, u, Phi, phi


def score64(cfg, mu, d, best, mutate=None):
    """the device's formulas in float64"""
    ms, t, sd, u, Phi, phi = parts64(cfg, mu, d, best)
    if mutate == "Phi(-u)":
        Phi = 1.0 - Phi
    with np.errstate(all="ignore"):
        if cfg.criterion == LCB:
            return cfg.kappa * sd - ms
        if cfg.criterion == STRADDLE:
            return cfg.kappa * sd - np.abs(ms - cfg.sgn * cfg.level)
        if cfg.criterion == PI:
            return np.where(sd > 0, Phi, np.where(t > 0, 1.0, 0.0))
        return np.where(sd > 0, t * Phi + sd * phi, np.maximum(t, 0.0))


def score_mp(cfg, mu, d, best, rows=None):
    """the scores from the long-double mu and d with mpmath at 50 digits -> long double (rows: only those)"""
    mp = _mp()
    out = np.full(len(mu), -np.inf, dtype=ld)
    sgn, xi, kap = mp.mpf(cfg.sgn), mp.mpf(cfg.xi), mp.mpf(cfg.kappa)
    bst, lev = to_mp(best), mp.mpf(cfg.sgn * cfg.level)
    half, r2, c2 = mp.mpf(1) / 2, mp.sqrt(2), mp.sqrt(2 * mp.pi)
    for i in (range(len(mu)) if rows is None else rows):
        ms, di = sgn * to_mp(mu[i]), to_mp(d[i])
        sd = mp.sqrt(di) if di > 0 else mp.mpf(0)
        if cfg.criterion == LCB:
            v = kap * sd - ms
        elif cfg.criterion == STRADDLE:
            v = kap * sd - abs(ms - lev)
        else:
            t = bst - xi - ms
            if sd == 0:
                v = (mp.mpf(1 if t > 0 else 0)) if cfg.criterion == PI else max(t, mp.mpf(0))
            else:
                u = t / sd
                Phi = half * mp.erfc(-u / r2)
                v = Phi if cfg.criterion == PI else t * Phi + sd * mp.exp(-u * u / 2) / c2
        out[i] = from_mp(v)
    return out


def score_bounds(cfg, mu, d, best, bmu, bd, rnd=E.U):
    """(bound, rest) of a score: the allowances of mu and d through the partial derivatives, and the evaluation term"""
    ms, t, sd, u, Phi, phi = parts64(cfg, mu, d, best)
    with np.errstate(all="ignore"):
        bsd = bd / (2 * sd)
        au, amu = np.abs(u), np.abs(ms)
        mag = abs(best) + abs(cfg.xi) + amu
        if cfg.criterion == EI:
            bound = Phi * bmu + phi * bsd
            rest = rnd * (Phi * 2 * mag + phi * 3 * sd + 2 * np.abs(t) * au * phi + 2 * u * u * sd * phi
                          + 18 * np.abs(t) * Phi + 6 * sd * phi)
        elif cfg.criterion == PI:
            bound = phi / sd * (bmu + au * bsd)
            rest = rnd * (phi / sd * (2 * mag + 3 * au * sd) + 2 * au * phi + 16 * Phi)
        elif cfg.criterion == LCB:
            bound = bmu + cfg.kappa * bsd
            rest = rnd * 4 * (amu + cfg.kappa * sd)
        else:
            bound = bmu + cfg.kappa * bsd
            rest = rnd * 4 * (amu + abs(cfg.level) + cfg.kappa * sd)
    return np.where(np.isnan(bound), np.inf, bound), np.where(np.isnan(rest), np.inf, rest)


def incumbent(cfg, ystar):
    """the signed incumbent after the given values"""
    best = ld(cfg.sgn * cfg.best)
    if cfg.criterion in (EI, PI):
        for y in ystar:
            best = min(best, ld(cfg.sgn) * ld(y))
    return best


def states(c, cfg, picks=None, k=None, cholesky=P.cholesky_ld, rnd=E.U):
    """The reference along the picks it is given (picks=None: along its own argmax, for at most k picks): for
    t = 0 .. the number of picks the state BEFORE pick t -- mu, d, the masked scores, its own argmax (`best`; -1:
    nothing eligible), the incumbent -- and the float64 bounds (without C) of mu, d and the score with the score's
    evaluation term.  -> (picks, ystar, states)"""
    own = picks is None
    picks = [] if own else [int(j) for j in picks][:k]
    ystar, out, t = [], [], 0
    mag_mu = mag_d = None
    full = cholesky is not P.cholesky_ld
    while True:
        s = _state(c, picks[:t], ystar[:t], cholesky)
        K = c.p + t
        aW = np.abs(P.inverse64(_f64(s["L"])))
        if t == 0:
            mag_mu = c.aB @ np.abs(c.theta)
            mag_d = _f64(s["d"]) + 2 * np.einsum("ki,ki->i", np.abs(_f64(s["Z"])), aW @ _f64(c.bB).T)
        bmu, bd = K * mag_mu, K * mag_d
        inc = incumbent(cfg, ystar[:t])
        last = t == len(picks) and not (own and t < k)
        st = dict(t=t, mu=s["mu"], d=s["d"], finite=c.finite, bound_mu=bmu, bound_d=bd, incumbent=inc, best=-1)
        if not last:
            s64 = score64(cfg, s["mu"], s["d"], float(inc))
            ok = c.finite & ~c.skip & np.isfinite(s64)
            if len(picks[:t]):
                ok[np.asarray(picks[:t], dtype=np.int64)] = False
            skey = ("score",) + cfg.key()
            if t == 0 and not full and skey in c.cache:
                sc = c.cache[skey]
            elif t == 0 or c.m <= SCREEN or full:
                sc = score_mp(cfg, s["mu"], s["d"], inc)
                if t == 0 and not full:
                    c.cache[skey] = sc
            else:
                live = s64[ok]
                spread = float(live.max() - live.min()) + abs(float(live.max())) if len(live) else 0.0
                near = np.nonzero(ok & (s64 >= live.max() - 1e-6 * spread))[0] if len(live) else []
                sc = np.array(s64, dtype=ld)
                if len(near):
                    sc[near] = score_mp(cfg, s["mu"], s["d"], inc, near)[near]
            bs, rs = score_bounds(cfg, s["mu"], s["d"], float(inc), bmu, bd, rnd)
            masked = np.where(ok, sc, -np.inf)
            st.update(raw=sc, score=masked, ok=ok, bound_score=bs, rest_score=rs,
                      best=int(np.argmax(masked)) if np.any(ok) else -1)
        out.append(st)
        if own and t < k and st["best"] >= 0:
            picks.append(st["best"])
        if t == len(picks):
            return picks, ystar, out
        # what conditioning on picks[t] with its value adds to the magnitudes
        j = picks[t]
        y = s["mu"][j] if cfg.lie == BELIEVER else ld(cfg.lie_value)
        ystar.append(y)
        a = _f64(s["Z"].T @ s["Z"][:, j])
        gam = float(c.nu + s["d"][j])
        delta = abs(float(y - s["mu"][j]))
        mag_a = c.aB @ ((aW.T @ aW) @ c.aB[j])
        mag_mu = mag_mu + (np.abs(a) + mag_a) * delta / gam
        mag_d = mag_d + (a * a + 2 * np.abs(a) * mag_a) / gam
        t += 1


def allowance(st, C):
    return C * st["bound_score"] + st["rest_score"]


def gap_ratio(sts, C, exempt=()):
    """smallest (top score - runner-up) / (the larger of their allowances) over the steps with a pick; rows in
    `exempt` (a deliberate twin) are left out; inf when a step has one eligible candidate"""
    worst = np.inf
    for s in sts:
        if "ok" not in s:
            continue
        okk = s["ok"].copy()
        if len(exempt):
            okk[np.asarray(exempt, dtype=np.int64)] = False
        idx = np.nonzero(okk)[0]
        if len(idx) < 2:
            continue
        o = np.argsort(-_f64(s["score"][idx]), kind="stable")[:2]
        i0, i1 = idx[o[0]], idx[o[1]]
        gap = float(s["score"][i0] - s["score"][i1])
        al = allowance(s, C)
        worst = min(worst, gap / max(al[i0], al[i1], 1e-300))
    return worst


# ---- the float64 restatement of the recurrences -------------------------------------------------------
MUTATIONS = ["mean update dropped", "incumbent not updated", "Phi(-u)", "maximize ignored", "sd with the noise",
             "picked row not masked"]


def recurrence64(c, cfg, k, force=None, mutate=None, extended=False, bounds=False):
    """The device's algorithm in NumPy float64 on the float64 oracle's B: explicit S, one downdate of mu and d and
    one scoring per step; mu_j is the value the pick was scored with, no coefficient vector is updated.  force: the
    picks to follow (its own argmax is still reported in `own`).  mutate: one of MUTATIONS.  extended: the same
    recurrences in long double on the long-double B with mpmath scores (what test_acquire_host.py compares with the
    explicit refits).  bounds (float64 only): `states` in the result holds, per step and for the end, this
    restatement's own mu, d and scores with the bounds of states() formed in float64 along its own path -- the
    magnitudes inside a_is taken as the device forms S_t, |W_0|^T |W_0| + sum |s| |s|^T / gamma -- for a case whose long-double
    factorisation is out of reach.  -> dict(index, own, score, score0, mean, var, n_picked)"""
    if extended:
        B, nu, th = c.B, c.nu, np.array(c.theta, dtype=ld)
        Linv = P.inverse_ld(P.cholesky_ld(c.H))
    else:
        B, nu, th = c.Bo, float(np.exp(2.0 * c.sigma)), c.theta
        if "Linv64" not in c.cache:
            c.cache["Linv64"] = np.linalg.solve(np.linalg.cholesky(c.H), np.eye(c.p))
        Linv = c.cache["Linv64"]
    one = B.dtype.type(1)
    S = Linv.T @ Linv
    d = ((Linv @ B.T) ** 2).sum(axis=0)
    mu = B @ th
    ecfg = cfg
    if mutate == "maximize ignored":
        ecfg = Config(cfg.criterion, cfg.best, cfg.xi, cfg.kappa, cfg.level, False, cfg.lie, cfg.lie_value)
    sgn = B.dtype.type(ecfg.sgn)
    best = sgn * B.dtype.type(cfg.best)
    picked = np.zeros(c.m, dtype=bool)
    s, gamma, delta = np.zeros(c.p, dtype=B.dtype), one, 0 * one
    index, own, score, score0 = [], [], [], None
    sts = []
    if bounds:
        assert not extended and mutate is None
        if "aG64" not in c.cache:
            c.cache["aG64"] = np.abs(Linv).T @ np.abs(Linv)
            c.cache["cond64"] = 2 * np.einsum("ki,ki->i", np.abs(Linv @ B.T), np.abs(Linv) @ _f64(c.bB).T)
        aG = c.cache["aG64"].copy()
        mag_mu, mag_d = c.aB @ np.abs(c.theta), d + c.cache["cond64"]

    def record(t, raw=None):
        if not bounds:
            return
        K = c.p + t
        st = dict(t=t, mu=np.array(mu, dtype=ld), d=np.array(d, dtype=ld), finite=c.finite, bound_mu=K * mag_mu, bound_d=K * mag_d)
        if raw is not None:
            bs, rs = score_bounds(ecfg, mu, d, float(best), K * mag_mu, K * mag_d)
            st.update(raw=np.array(raw, dtype=ld), bound_score=bs, rest_score=rs)
        sts.append(st)

    def downdate_and_score():
        nonlocal mu, d
        a = B @ s
        ag = a / gamma
        if mutate != "mean update dropped":
            mu = mu + ag * delta
        d = d - a * ag
        dd = nu + d if mutate == "sd with the noise" else d
        if extended:
            sc = score_mp(ecfg, mu, dd, best)
        else:
            sc = score64(ecfg, mu, dd, float(best), mutate)
        bad = ~c.finite | c.skip | ~np.isfinite(_f64(sc))
        if mutate != "picked row not masked":
            bad |= picked
        return sc, np.where(bad, -np.inf, sc)
    for t in range(k):
        raw, sc = downdate_and_score()
        if t == 0:
            score0 = np.where(c.finite, raw, np.nan)
        record(t, raw)
        j = int(np.argmax(sc))
        if not sc[j] > -np.inf:
            break
        own.append(j)
        if force is not None:
            if t >= len(force):
                break
            j = int(force[t])
        index.append(j)
        score.append(sc[j])
        picked[j] = True
        b = B[j]
        s = S @ b
        gamma = nu + b @ s
        y = mu[j] if cfg.lie == BELIEVER else B.dtype.type(cfg.lie_value)
        delta = y - mu[j]
        if cfg.criterion in (EI, PI) and mutate != "incumbent not updated":
            best = min(best, sgn * y)
        S = S - np.outer(s, s) / gamma
        if bounds:
            a, g = B @ s, float(gamma)
            mag_a = c.aB @ (aG @ c.aB[j])
            mag_mu = mag_mu + (np.abs(a) + mag_a) * abs(float(delta)) / g
            mag_d = mag_d + (a * a + 2 * np.abs(a) * mag_a) / g
            aG += np.outer(np.abs(s), np.abs(s)) / g
    else:
        downdate_and_score()
    record(len(index))
    return dict(states=sts, index=np.asarray(index, dtype=np.int64), own=np.asarray(own, dtype=np.int64),
                score=np.asarray(score, dtype=B.dtype), score0=score0, mean=np.where(c.finite, mu, np.nan),
                var=np.where(c.finite, d, np.nan), n_picked=len(index))


# ---- measuring ----------------------------------------------------------------------------------------
def ratios(got, sts, C=1.0, sub_rest=False):
    """{quantity: worst |got - want| / (C x bound + rest)} of a result (recurrence64's dict, or the device's outputs
    under the same names) against the states along got["index"]; rows that are not finite are left out (NaN on
    both sides by construction).  sub_rest: (|got - want| - rest)+ / (C x bound), what C is measured with."""
    n = int(got["n_picked"])
    assert len(sts) >= n + 1
    last, fin = sts[n], sts[n]["finite"]
    out = {}

    def worst(g, want, bound, rest):
        if sub_rest:
            err = np.maximum(_f64(np.abs(np.asarray(g, dtype=ld) - want)) - rest, 0.0)
            den = C * _f64(bound)
            r = np.zeros(err.shape)
            np.divide(err, den, out=r, where=den > 0)
            r[(den <= 0) & (err > 0)] = np.inf
            return float(np.max(r)) if r.size else 0.0
        return E.worst_ratio(g, want, C * _f64(bound) + rest)
    if n:
        idx = [int(i) for i in got["index"][:n]]
        out["score"] = worst(got["score"][:n], np.array([sts[t]["raw"][idx[t]] for t in range(n)], dtype=ld),
                             np.array([sts[t]["bound_score"][idx[t]] for t in range(n)]),
                             np.array([sts[t]["rest_score"][idx[t]] for t in range(n)]))
    if got.get("score0") is not None and "raw" in sts[0]:
        f0 = sts[0]["finite"]
        out["score0"] = worst(_f64(got["score0"])[f0], sts[0]["raw"][f0], sts[0]["bound_score"][f0], sts[0]["rest_score"][f0])
    out["mean"] = worst(_f64(got["mean"])[fin], last["mu"][fin], last["bound_mu"][fin], 0.0)
    out["var"] = worst(_f64(got["var"])[fin], last["d"][fin], last["bound_d"][fin], 0.0)
    return out


def constant_of(c, cfg, sts, picks):
    """(C, r): r = the float64 restatement's own worst (err - rest) / bound along the same picks"""
    got = recurrence64(c, cfg, max(len(picks), 1), force=picks)
    r = max(ratios(got, sts, 1.0, sub_rest=True).values())
    return E.constant_from_oracle_ratio(r), r


# ---- the cases both test files share ------------------------------------------------------------------
def seeded_case(om_o, terms, m, seed, xcand=None, skip=None):
    """H of design_ref.hessian_of; the rows and theta from np.random.default_rng(seed).  theta is a draw scaled so that
    the latent mean varies over the candidates by twice their median latent standard deviation: the criteria then
    trade the mean against the variance."""
    import design_ref as D
    from conftest import sample_x
    rng = np.random.default_rng(seed)
    H, _ = D.hessian_of(om_o, terms, seed + 1)
    xc = sample_x(rng, m, om_o.kinds) if xcand is None else xcand
    z = rng.standard_normal(len(terms))
    c = make_case(om_o, terms, H, D.SIGMA, z, xc, skip)
    fin = c.finite
    Z = np.linalg.solve(np.linalg.cholesky(c.H), c.Bo[fin].T)
    sd = float(np.median(np.sqrt((Z * Z).sum(axis=0))))
    spread = float(np.std(c.Bo[fin] @ z)) if fin.sum() > 1 else float(np.abs(c.Bo[fin] @ z).max())
    c.theta = z * float(np.float32(2 * sd / spread))
    c.rhs0 = np.array(c.H, dtype=ld) @ np.array(c.theta, dtype=ld)
    return c


def configs_of(c):
    """the sixteen calls of a case: four criteria x two lies x two directions.  best is the lower (maximize: upper)
    decile of the latent means, xi a hundredth of their spread, level their median, the constant lie the incumbent:
    float32-rounded values taken from the float64 oracle's means"""
    mu = (c.Bo @ c.theta)[c.finite]
    f = lambda v: float(np.float32(v))
    out = []
    for crit in CRITERIA:
        for lie in LIES:
            for mx in (False, True):
                best = f(np.quantile(mu, 0.9 if mx else 0.1))
                out.append(Config(crit, best=best, xi=f(0.01 * (mu.max() - mu.min())), kappa=1.96, level=f(np.median(mu)),
                                  maximize=mx, lie=lie, lie_value=best))
    return out


# (model, p, m, k asked for, seed): see test_gpu_acquire.py for why each is there
SHAPES = [("d3", 5, 1, 1, 81), ("d3", 5, 63, 12, 82), ("d3", 5, 64, 12, 83), ("d3", 5, 65, 12, 84),
          ("d3", 5, 255, 3, 85), ("d3", 5, 256, 3, 86), ("d3", 5, 257, 3, 87), ("d3", 5, 66000, 2, 88),
          ("d8", 67, 65, 65, 89), ("d8", 67, 65, 70, 89), ("d5", 130, 129, 12, 90), ("d5", 130, 1000, 12, 91)]
WIDE = ("wide", 0, 65, 3, 92)
SEMANTICS = ("d5", 130, 129, 3, 93)
