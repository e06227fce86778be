"""Extended-precision host restatement of the sequential design (csrc/design.cpp, kernels_design.hip): the
instrument test_gpu_design.py measures the step kernels and the p-space downdates with, and
test_design_host.py proves against explicit refits and shows which failures it can see.

np.longdouble and NumPy only, in the style of posterior_ref.py; B and its conditioning bB come from
extended_ref.ExtendedRef.  NO recurrence: at every step t the reference forms

    H_t = H + sum_{j picked so far} b_j b_j^T / nu,      nu = e^{2 sigma},

factors it (posterior_ref.cholesky_ld) and solves (forward_ld); from Z = L_t^-1 B^T, W = L_t^-1,
S_t = W^T W, Y = S_t B^T and M = sum_r u_r b_r b_r^T / sum u it takes

    d_i = || z_i ||^2        num_i = y_i^T M y_i        tr(M S_t) = sum_kl M_kl S_kl      log det H_t
    score_i = w_i d_i  (maxvar)   |   w_i num_i / (nu + d_i)  (imse)

and masks as the device does (picked rows without replacement, w_i = 0, scores that are not finite).
It FOLLOWS the picks it is given: states(case, picks) conditions step t + 1 on picks[t], whoever made it,
so that one disagreement does not cascade.  states(case, None, k) follows its own argmax (first among equals).

Tolerances.  Every quantity the device reaches by the recurrences is a float64 sum of at most p + t
summands (p terms of a dot product, t downdates; with a reference measure of r rows the r summands of M as
well), so it is held to

    |got - want|  <=  C x (number of summands) x (sum of the magnitudes of everything added and subtracted
                                                   to reach it),

the magnitudes being: for d_i, d_i(0) and every a_is^2 / gamma_s taken off it, plus 2 |z_i|^T |W| bB_i, the
magnitudes inside the knot sums of b_i carried to d_i (posterior_ref.ref_var's bound); for num_i, num_i(0),
every 2 |a c| / gamma and a^2 tau / gamma^2, plus bB carried through |S| |M| |S| and through the rows of the
reference measure; scores and traces carry those of the d and num they are formed from plus four
roundings of their own value.  The unit roundoff is carried by C, as in posterior_ref.py: C is never a
constant of this module and never measured from the device -- every test measures the float64
restatement of the same recurrences (recurrence64, NumPy on the float64 oracle's B) on the same case and
takes extended_ref.constant_from_oracle_ratio of its worst err / bound: eight times it, at most
extended_ref.C_CAP = 2e-13, which is 1800 unit roundoffs per summand and magnitude.
"""
import numpy as np

import extended_ref as E
import posterior_ref as P
from extended_ref import ld

MAXVAR, IMSE = "maxvar", "imse"


def _f64(a):
    return np.asarray(a, dtype=np.float64)


class Case:
    pass


def make_case(om_o, terms, H, sigma, xcand, criterion, xref=None, u=None, weights=None, replace=False):
    """everything both routes need of one selection problem; H float64 (taken as exact)"""
    import ob_oracle as O
    E.require_extended()
    c = Case()
    knots = [np.asarray(om_o.knots_of(k), dtype=np.float64) for k in range(om_o.d)]

    def ext(x):
        return E.ExtendedRef(om_o.kinds, knots, om_o.hyp, om_o.rotmat, x).getmat(terms)
    c.terms, c.H, c.sigma, c.xcand, c.criterion, c.replace = terms, _f64(H), float(sigma), xcand, criterion, bool(replace)
    c.m, c.p = len(xcand), len(terms)
    c.nu = np.exp(2 * ld(sigma))
    c.w = np.ones(c.m) if weights is None else _f64(weights)
    c.finite = np.all(np.isfinite(xcand), axis=1)
    xs = np.where(np.isfinite(xcand), xcand, 0.5)                  # a row that is not finite: masked, never used
    c.B, c.bB = ext(xs)
    c.Bo = O.ob_getmat(O.OuterBase(om_o, xs), terms)
    c.r = 0
    if criterion == IMSE:
        c.xref, c.r = xref, len(xref)
        c.u = np.ones(c.r) if u is None else _f64(u)
        c.un = np.asarray(c.u, dtype=ld) / np.asarray(c.u, dtype=ld).sum()
        c.Br, c.bBr = ext(xref)
        c.Bro = O.ob_getmat(O.OuterBase(om_o, xref), terms)
        c.M = (c.Br * c.un[:, None]).T @ c.Br
    c.K = c.p + c.r                                                # summands before the first downdate
    return c


# ---- the explicit states ------------------------------------------------------------------------------
def _state(c, picks):
    Ht = np.array(c.H, dtype=ld)
    for j in picks:
        Ht = Ht + np.outer(c.B[j], c.B[j]) / c.nu
    L = P.cholesky_ld(Ht)
    Z = P.forward_ld(L, c.B.T)                                     # p x m
    s = dict(L=L, Z=Z, d=(Z * Z).sum(axis=0), logdet=2 * np.log(np.diagonal(L)).sum())
    if c.criterion == IMSE:
        W = P.inverse_ld(L)
        S = W.T @ W
        Y = W.T @ Z                                                # S B^T
        MY = c.M @ Y
        s.update(W=W, S=S, Y=Y, MY=MY, num=(Y * MY).sum(axis=0), tr=(c.M * S).sum())
    return s


def _scores(c, s, picks):
    """(masked long-double scores, the eligible rows)"""
    with np.errstate(all="ignore"):
        sc = c.w * s["d"] if c.criterion == MAXVAR else c.w * s["num"] / (c.nu + s["d"])
    ok = c.finite & (c.w > 0) & np.isfinite(_f64(sc))
    if not c.replace and len(picks):
        ok[np.asarray(picks, dtype=np.int64)] = False
    return np.where(ok, sc, -np.inf), ok


def states(c, picks=None, k=None):
    """The reference along the picks it is given (picks=None: along its own argmax, for at most k picks): for
    t = 0 .. the number of picks the state BEFORE pick t, with its scores, its own argmax (`best`; -1: nothing
    eligible), the trace, and the float64 bounds (without C) of d, num, score and trace at that step.
    -> (picks, states)"""
    own = picks is None
    picks = [] if own else [int(j) for j in picks][:k]
    out, mag_d, mag_n, tb, cum, t = [], None, None, 0.0, ld(0), 0
    while True:
        s = _state(c, picks[:t])
        K = c.K + t
        if t == 0:
            Zf = np.abs(_f64(s["Z"]))
            aW = np.abs(P.inverse64(_f64(s["L"])))
            cond_d = 2 * np.einsum("ki,ki->i", Zf, aW @ _f64(c.bB).T)
            mag_d = _f64(s["d"]).copy()
            cond_n = 0.0
            if c.criterion == IMSE:
                Yf, aS, aBr = np.abs(_f64(s["Y"])), np.abs(_f64(s["S"])), np.abs(_f64(c.Br))
                unf = _f64(c.un)
                aM = (aBr * unf[:, None]).T @ aBr
                cond_n = 2 * np.einsum("ki,ik->i", aS @ (aM @ Yf), _f64(c.bB)) \
                    + 2 * np.einsum("ir,ir,r->i", Yf.T @ aBr.T, Yf.T @ _f64(c.bBr).T, unf)
                mag_n = _f64(s["num"]).copy()
                tb = K * float(np.sum(aM * (aW.T @ aW))) + 2 * float(np.einsum("rk,rk,r->", aBr @ aS, _f64(c.bBr), unf))
        sc, ok = _scores(c, s, picks[:t])
        df, nuf = _f64(s["d"]), float(c.nu)
        bd = K * (mag_d + cond_d)
        if c.criterion == IMSE:
            nf = _f64(s["num"])
            bn = K * (mag_n + cond_n)
            bs = c.w * (bn / (nuf + df) + np.abs(nf) * bd / (nuf + df) ** 2) + 4 * np.abs(_f64(np.where(ok, sc, 0)))
            trace = s["tr"]
        else:
            bn = None
            bs = c.w * bd + 4 * np.abs(_f64(np.where(ok, sc, 0)))
            trace = cum
        best = int(np.argmax(sc)) if np.any(ok) else -1
        out.append(dict(t=t, d=s["d"], num=s.get("num"), score=sc, ok=ok, best=best, trace=trace, logdet=s["logdet"],
                        finite=c.finite, bound_d=bd, bound_num=bn, bound_score=bs,
                        bound_trace=tb + t * abs(float(trace))))
        if own and t < k and best >= 0:
            picks.append(best)
        if t == len(picks):
            return picks, out
        # what conditioning on picks[t] takes off d and num, and the trace after it
        j = picks[t]
        a = s["Z"].T @ s["Z"][:, j]
        gamma = c.nu + s["d"][j]
        af, gf = _f64(a), float(gamma)
        mag_d = mag_d + af * af / gf
        if c.criterion == IMSE:
            cc = s["Y"].T @ s["MY"][:, j]
            tau = float(s["num"][j])
            mag_n = mag_n + 2 * np.abs(af * _f64(cc)) / gf + af * af * abs(tau) / gf ** 2
            tb += bn[j] / gf + abs(tau) * bd[j] / gf ** 2 + 4 * abs(tau) / gf
        else:
            gain = np.log1p(s["d"][j] / c.nu)
            cum = cum + gain
            tb += bd[j] / gf + 4 * float(gain)
        t += 1


def gap_ratio(st, C):
    """smallest (top score - runner-up) / (C x the larger of their score bounds) over the steps with a pick;
    inf when a step has one eligible candidate"""
    worst = np.inf
    for s in st:
        idx = np.nonzero(s["ok"])[0]
        if len(idx) < 2:
            continue
        sc = _f64(s["score"][idx])
        o = np.argsort(-sc, kind="stable")[:2]
        gap = float(s["score"][idx[o[0]]] - s["score"][idx[o[1]]])
        worst = min(worst, gap / (C * max(s["bound_score"][idx[o[0]]], s["bound_score"][idx[o[1]]])))
    return worst


# ---- the float64 restatement of the recurrences -------------------------------------------------------
def recurrence64(c, k, force=None, mutate=None, extended=False):
    """The device's algorithm in NumPy float64 on the float64 oracle's B: explicit S and T, one downdate and
    one scoring per step.  force: the picks to follow (its own argmax is still reported in `own`).
    mutate: "gamma without nu", "tau term dropped", "picked row not masked" -- the failures
    test_design_host.py stages.  extended: the same recurrences in long double on the long-double B (what
    test_design_host.py compares with the explicit refits).  -> dict(index, own, score, var, num, trace, n_picked)"""
    imse = c.criterion == IMSE
    if extended:
        B, nu = c.B, c.nu
        Linv = P.inverse_ld(P.cholesky_ld(c.H))
    else:
        B, nu = c.Bo, float(np.exp(2.0 * c.sigma))
        Linv = np.linalg.solve(np.linalg.cholesky(c.H), np.eye(c.p))
    S = Linv.T @ Linv
    d = ((Linv @ B.T) ** 2).sum(axis=0)
    T = num = None
    trace = [B.dtype.type(0)]
    if imse:
        un = c.un if extended else c.u / c.u.sum()
        Br = c.Br if extended else c.Bro
        M = (Br * un[:, None]).T @ Br
        T = S @ M @ S
        num = ((B @ T) * B).sum(axis=1)
        trace = [np.sum(M * S)]
    picked = np.zeros(c.m, dtype=bool)
    s, h, gamma, tau = np.zeros(c.p, dtype=B.dtype), np.zeros(c.p, dtype=B.dtype), 1.0, 0.0
    index, own, score = [], [], []

    def downdate_and_score():
        nonlocal d, num
        a = B @ s
        ag = a / gamma
        d = d - a * ag
        with np.errstate(all="ignore"):
            if imse:
                cc = B @ h
                num = num + (ag * (-2.0 * cc) if mutate == "tau term dropped" else ag * (ag * tau - 2.0 * cc))
                sc = c.w * num / (nu + d)
            else:
                sc = c.w * d
        bad = ~c.finite | ~(c.w > 0) | ~np.isfinite(_f64(sc))
        if not c.replace and mutate != "picked row not masked":
            bad |= picked
        return np.where(bad, -np.inf, sc)
    for t in range(k):
        sc = downdate_and_score()
        j = int(np.argmax(sc))
        if not sc[j] > -np.inf:
            break
        own.append(j)
        if force is not None:
            j = int(force[t])
        index.append(j)
        score.append(sc[j])
        picked[j] = True
        b = B[j]
        s = S @ b
        dj = b @ s
        gamma = dj if mutate == "gamma without nu" else nu + dj
        if imse:
            h = T @ b
            tau = b @ h
            trace.append(trace[-1] - tau / gamma)
            T = T - (np.outer(s, h) + np.outer(h, s)) / gamma + np.outer(s, s) * (tau / gamma ** 2)
        else:
            trace.append(trace[-1] + np.log1p(dj / nu))
        S = S - np.outer(s, s) / gamma
    else:
        downdate_and_score()
    return dict(index=np.asarray(index, dtype=np.int64), own=np.asarray(own, dtype=np.int64),
                score=np.asarray(score, dtype=B.dtype), var=d, num=num, trace=np.asarray(trace, dtype=B.dtype),
                n_picked=len(index))


# ---- measuring ----------------------------------------------------------------------------------------
def ratios(got, st, C=1.0):
    """{quantity: worst |got - want| / (C x bound)} of a result (recurrence64's dict, or the device's outputs
    under the same names) against the states along got["index"]; rows that are not finite are left out of var
    and num (their values are NaN on both sides by construction)"""
    n = int(got["n_picked"])
    assert len(st) >= n + 1
    last = st[n]
    fin = last["finite"]
    out = {}
    if n:
        want = np.array([st[t]["score"][int(got["index"][t])] for t in range(n)], dtype=ld)
        tol = np.array([st[t]["bound_score"][int(got["index"][t])] for t in range(n)])
        out["score"] = E.worst_ratio(got["score"][:n], want, C * tol)
    out["var"] = E.worst_ratio(_f64(got["var"])[fin], last["d"][fin], C * last["bound_d"][fin])
    out["trace"] = E.worst_ratio(got["trace"][:n + 1], np.array([s["trace"] for s in st[:n + 1]], dtype=ld),
                                 C * np.array([max(s["bound_trace"], 1e-300) for s in st[:n + 1]]))
    if got.get("num") is not None and last["num"] is not None:
        out["num"] = E.worst_ratio(_f64(got["num"])[fin], last["num"][fin], C * last["bound_num"][fin])
    return out


def constant_of(c, st, picks):
    """(C, r): r = the float64 restatement's own worst err / bound along the same picks"""
    got = recurrence64(c, len(picks), force=picks)
    r = max(ratios(got, st).values())
    return E.constant_from_oracle_ratio(r), r


# ---- the cases both test files share ------------------------------------------------------------------
SIGMA = float(np.log(0.1))
RHO = 0.0        # prior precisions of order one and more: H is well conditioned with few fitted rows
NFIT = 40


def hessian_of(om_o, terms, seed):
    """float64 total Hessian e^{-2 sigma} B^T B + diag(prec) of NFIT seeded rows, exactly symmetric"""
    import ob_oracle as O
    from conftest import sample_x
    x = sample_x(np.random.default_rng(seed), NFIT, om_o.kinds)
    Bo = O.ob_getmat(O.OuterBase(om_o, x), terms)
    H = np.exp(-2.0 * SIGMA) * (Bo.T @ Bo) + np.diag(O.prior_prec(om_o, terms, RHO))
    return (H + H.T) / 2, x


def seeded_case(om_o, terms, m, criterion, seed, r=50, weights=None, replace=False, xcand=None):
    """candidates and (imse) a weighted reference measure drawn from the seed, a fifth of its weights zero"""
    from conftest import sample_x
    rng = np.random.default_rng(seed)
    H, _ = hessian_of(om_o, terms, seed + 1)
    xc = sample_x(rng, m, om_o.kinds) if xcand is None else xcand
    xref = u = None
    if criterion == IMSE:
        xref = sample_x(rng, r, om_o.kinds)
        u = rng.uniform(0.2, 1.0, r)
        u[rng.random(r) < 0.2] = 0.0
        u[0] = 0.5
    return make_case(om_o, terms, H, SIGMA, xc, criterion, xref, u, weights, replace)
