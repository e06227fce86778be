"""Extended-precision host restatement of the acquisition picks over several responses (csrc/acquire_multi.cpp,
kernels_acquire_multi.hip): the instrument test_gpu_acquire_multi.py measures the device with, and
test_acquire_multi_host.py proves against the definition of the hypervolume improvement and against the recurrences,
and shows which failures it can see.  It builds on acquire_ref.py (A), posterior_ref.py (P) and extended_ref.py (E).

NO recurrence: at every step t, with the picks j_1 .. j_t and the values y*_s,r the runs were given,

    H_t = H + sum_s b_js b_js^T / nu,      theta_t,r = inv(H_t) (H theta_r + sum_s b_js y*_s,r / nu),      nu = e^{2 sigma},

is factored afresh in long double (posterior_ref.cholesky_ld, forward_ld), mu = B Theta_t (m x q) and
d = diag(B inv(H_t) B^T) are taken from Z = L_t^-1 B^T.  The scores are evaluated from those with mpmath at 50 digits:
the constraint product, the strip sum of the expected hypervolume improvement, the front as the set of undominated
points inside the box (pareto(), brute force over all points so far).  It FOLLOWS the picks it is given, so that one
disagreement does not cascade, and reports its own argmax; the values the runs are given are the reference's own.
At steps t >= 1 only the rows whose float64 score lies within 1e-6 (relative to the spread) of the float64 maximum,
and the pick itself, are evaluated with mpmath; step 0 is evaluated in full.

Allowances.  mu_r and d carry acquire_ref's bounds, per response: K = p + t summands times the magnitudes of everything
added and subtracted (mu_r with |theta_r| and |delta_s,r|).  Psi(c; ms, d) and P(c; ms, d) carry them through
acquire_ref.score_bounds (EI and PI at best = c, xi = 0), which also gives their evaluation terms (erfc 16 ulp, exp 3
ulp).  Then, with (v, b, r) = (value, bound, evaluation term) of a factor and U the unit roundoff:

    product  prod_f v_f:   b = sum_f b_f prod_{l != f} |v_l|,   r = sum_f r_f prod_{l != f} |v_l| + (factors) U |prod|
    strip    D_s = Psi(u_s) - Psi(u_{s-1}) counts with M_s = Psi(u_s) + Psi(u_{s-1}):
             b_D = b(u_s) + b(u_{s-1}),  r_D = r(u_s) + r(u_{s-1}) + U M_s
             T_s = D_s Psi(c_s):  b = b_D Psi(c_s) + M_s b(c_s),  r = r_D Psi(c_s) + M_s r(c_s) + U M_s Psi(c_s)
    sum      b = sum_s b_T,   r = sum_s r_T + (F + 1) U sum_s M_s Psi(c_s)
    score    base x pof as a product of two factors.

The bound is multiplied by C, the evaluation term is not.  C is never measured from the device: every test takes
extended_ref.constant_from_oracle_ratio (eight times, capped at C_CAP) of the worst (err - r) / b of the float64 NumPy
restatement of the device's recurrences (recurrence64) on the same case.
"""
import math

import numpy as np

import acquire_ref as A
import extended_ref as E
import posterior_ref as P
from extended_ref import ld

CEI, CPI, POF, EHVI = "cei", "cpi", "pof", "ehvi"
CRITERIA = [CEI, CPI, POF, EHVI]
OBJ, CON, NONE = 0, 1, 2
_f64 = A._f64


class MConfig:
    """one call's arguments in the caller's sign: objs (response indices, ascending), maximize (per objective),
    constraints (j, "<=" | ">=", limit), best (None: no feasible run yet), ref and front (F0 x 2), xi, lie, lie_value (q)"""

    def __init__(self, criterion, q, objs=(), maximize=(), constraints=(), best=None, ref=None, front=(), xi=0.0,
                 lie=A.BELIEVER, lie_value=None):
        self.criterion, self.q, self.objs, self.maximize = criterion, int(q), [int(j) for j in objs], [bool(v) for v in maximize]
        self.constraints = [(int(j), op, float(lim)) for j, op, lim in constraints]
        self.best, self.ref, self.xi, self.lie = best, ref, float(xi), lie
        self.front = np.asarray(front, dtype=np.float64).reshape(-1, 2)
        self.lie_value = np.zeros(q) if lie_value is None else np.asarray(lie_value, dtype=np.float64)
        assert len(self.objs) == {CEI: 1, CPI: 1, POF: 0, EHVI: 2}[criterion] == len(self.maximize)
        self.role, self.g, self.cs = np.full(q, NONE), np.ones(q), np.zeros(q)
        for j, mx in zip(self.objs, self.maximize):
            self.role[j], self.g[j] = OBJ, -1.0 if mx else 1.0
        for j, op, lim in self.constraints:
            assert self.role[j] == NONE and op in ("<=", ">=")
            self.role[j], self.g[j] = CON, 1.0 if op == "<=" else -1.0
            self.cs[j] = self.g[j] * lim
        self.cons = [j for j in range(q) if self.role[j] == CON]
        self.best0 = math.inf
        if criterion in (CEI, CPI) and best is not None:
            self.best0 = self.g[self.objs[0]] * float(best)
        self.r = None
        if criterion == EHVI:
            self.r = (self.g[self.objs[0]] * float(ref[0]), self.g[self.objs[1]] * float(ref[1]))
            self.cs[self.objs[0]], self.cs[self.objs[1]] = self.r
        self.points0 = [(ld(self.g[self.objs[0]] * a), ld(self.g[self.objs[1]] * b), 0.0, 0.0) for a, b in self.front] \
            if criterion == EHVI else []

    def limits(self):
        """the C ABI's limits array, in the caller's sign"""
        out = self.g * self.cs
        if self.criterion in (CEI, CPI):
            out[self.objs[0]] = self.g[self.objs[0]] * self.best0
        return out

    def __repr__(self):
        return "%s q=%d %s obj%s con%s F0=%d" % (self.criterion, self.q, self.lie, self.objs, [(j, op) for j, op, _ in self.constraints],
                                                len(self.front))


# ---- the front ------------------------------------------------------------------------------------------
def pareto(points, r):
    """the undominated points strictly inside the box, ascending in the first coordinate; equal points count once.
    points: (y1, y2, tol1, tol2) signed; brute force over all pairs"""
    inside = [p for p in points if p[0] < r[0] and p[1] < r[1]]
    out = []
    for i, p in enumerate(inside):
        dominated = any((o[0] <= p[0] and o[1] <= p[1]) and ((o[0], o[1]) != (p[0], p[1]) or l < i) for l, o in enumerate(inside) if l != i)
        if not dominated:
            out.append(p)
    return sorted(out, key=lambda p: p[0])


def insert(front, y, r, keep_dominated=False):
    """the device's rule, one point after the other (the float64 restatement's; keep_dominated: the staged fault)"""
    if not (y[0] < r[0] and y[1] < r[1]):
        return front
    if any(p[0] <= y[0] and p[1] <= y[1] for p in front):
        return front
    rest = front if keep_dominated else [p for p in front if not (p[0] >= y[0] and p[1] >= y[1])]
    return sorted(rest + [y], key=lambda p: p[0])


def hvi(front, r, y):
    """the area of {z : y <= z < r, no front point <= z}, from the definition: the box [y, r) minus the union of the
    boxes [max(p, y), r) of the front points, the union summed over slabs of z1 between neighbouring corners"""
    if not (y[0] < r[0] and y[1] < r[1]):
        return 0 * y[0]
    corners = sorted((max(p[0], y[0]), max(p[1], y[1])) for p in front if p[0] < r[0] and p[1] < r[1])
    area = (r[0] - y[0]) * (r[1] - y[1])
    low = None
    for i, (x, c) in enumerate(corners):                          # the slab from this corner to the next one is covered
        low = c if low is None else min(low, c)                   # from the lowest corner so far up to r2
        area -= ((corners[i + 1][0] if i + 1 < len(corners) else r[0]) - x) * (r[1] - low)
    return area


# ---- mpmath -------------------------------------------------------------------------------------------------
def psi_mp(c, ms, d, xi=0):
    mp = A._mp()
    sd = mp.sqrt(d) if d > 0 else mp.mpf(0)
    t = c - xi - ms
    if sd == 0:
        return max(t, mp.mpf(0))
    u = t / sd
    return t * mp.erfc(-u / mp.sqrt(2)) / 2 + sd * mp.exp(-u * u / 2) / mp.sqrt(2 * mp.pi)


def p_mp(c, ms, d, xi=0):
    mp = A._mp()
    sd = mp.sqrt(d) if d > 0 else mp.mpf(0)
    t = c - xi - ms
    if sd == 0:
        return mp.mpf(1 if t > 0 else 0)
    return mp.erfc(-t / sd / mp.sqrt(2)) / 2


def ehvi_mp(front, r, ms1, ms2, d):
    """the strip sum: front = [(u, c), ..] ascending in u, all mpmath numbers"""
    mp = A._mp()
    U = [p[0] for p in front] + [r[0]]
    Cc = [r[1]] + [p[1] for p in front]
    prev, tot = mp.mpf(0), mp.mpf(0)
    for u, c in zip(U, Cc):
        pu = psi_mp(u, ms1, d)
        tot += (pu - prev) * psi_mp(c, ms2, d)
        prev = pu
    return tot


def score_mp(cfg, mu, d, best, front, rows=None):
    """(score, pof) of the rows from the long-double mu (m x q) and d with mpmath -> long double"""
    mp = A._mp()
    m = len(d)
    sc, pf = np.full(m, -np.inf, dtype=ld), np.full(m, np.nan, dtype=ld)
    g = [mp.mpf(float(v)) for v in cfg.g]
    cs = [mp.mpf(float(v)) for v in cfg.cs]
    fr = [(A.to_mp(p[0]), A.to_mp(p[1])) for p in front]
    r = None if cfg.r is None else (mp.mpf(cfg.r[0]), mp.mpf(cfg.r[1]))
    bst = None if not math.isfinite(float(best)) else A.to_mp(best)
    xi = mp.mpf(cfg.xi)
    for i in (range(m) if rows is None else rows):
        di = A.to_mp(d[i])
        ms = [g[j] * A.to_mp(mu[i, j]) for j in range(cfg.q)]
        pof = mp.mpf(1)
        for j in cfg.cons:
            pof *= p_mp(cs[j], ms[j], di)
        if cfg.criterion == POF or (cfg.criterion in (CEI, CPI) and bst is None):
            base = mp.mpf(1)
        elif cfg.criterion == CEI:
            base = psi_mp(bst, ms[cfg.objs[0]], di, xi)
        elif cfg.criterion == CPI:
            base = p_mp(bst, ms[cfg.objs[0]], di, xi)
        else:
            base = ehvi_mp(fr, r, ms[cfg.objs[0]], ms[cfg.objs[1]], di)
        sc[i], pf[i] = A.from_mp(base * pof), A.from_mp(pof)
    return sc, pf


# ---- float64: the device's formulas and the allowances ------------------------------------------------------
def _factor(kind, ms, d, c, bmu, bd, rnd, xi=0.0):
    """(value, bound, evaluation term) of Psi (kind EI) or P (PI) at best = c in float64"""
    cfg = A.Config(kind, xi=xi)
    v = A.score64(cfg, ms, d, c)
    b, r = A.score_bounds(cfg, ms, d, c, bmu, bd, rnd)
    return v, b, r


def _times(x, y, rnd):
    """the product of two (v, b, r) factors with one rounding"""
    with np.errstate(all="ignore"):
        v = x[0] * y[0]
        b = x[1] * np.abs(y[0]) + np.abs(x[0]) * y[1]
        r = x[2] * np.abs(y[0]) + np.abs(x[0]) * y[2] + rnd * np.abs(v)
    return v, np.where(np.isnan(b), np.inf, b), np.where(np.isnan(r), np.inf, r)


def score_parts(cfg, mu, d, best, front, bmu, bd, rnd=E.U, mutate=None):
    """float64 (score, pof) as the device forms them, with (bound, rest) of the score and of pof.  front: [(u, c, ..)]"""
    mu, d = _f64(mu), _f64(d)
    m = len(d)
    one = (np.ones(m), np.zeros(m), np.zeros(m))
    pof = one
    cons = cfg.cons[1:] if mutate == "constraint factor missing" else cfg.cons
    for j in cons:
        g, cs = cfg.g[j], cfg.cs[j]
        if mutate == ">= scored as <=" and g < 0:
            g, cs = 1.0, -cs
        pof = _times(pof, _factor(A.PI, g * mu[:, j], d, float(cs), bmu[:, j], bd, rnd), rnd)
    if cfg.criterion == POF or (cfg.criterion in (CEI, CPI) and not math.isfinite(float(best))):
        base = one
    elif cfg.criterion in (CEI, CPI):
        j = cfg.objs[0]
        base = _factor(A.EI if cfg.criterion == CEI else A.PI, cfg.g[j] * mu[:, j], d, float(best), bmu[:, j], bd, rnd, cfg.xi)
    else:
        j1, j2 = cfg.objs
        ms1, ms2 = cfg.g[j1] * mu[:, j1], cfg.g[j2] * mu[:, j2]
        U = [float(p[0]) for p in front] + [cfg.r[0]]
        Cc = [cfg.r[1]] + [float(p[1]) for p in front]
        if mutate == "c_s from front point s" and front:
            Cc = [float(p[1]) for p in front] + [float(front[-1][1])]
        prev = (np.zeros(m), np.zeros(m), np.zeros(m))
        v, b, r, mag = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
        for s, (u, c) in enumerate(zip(U, Cc)):
            pu = _factor(A.EI, ms1, d, u, bmu[:, j1], bd, rnd)
            if mutate == "strip left out" and s == len(U) - 1:
                continue
            pc = _factor(A.EI, ms2, d, c, bmu[:, j2], bd, rnd)
            with np.errstate(all="ignore"):
                M = pu[0] + prev[0]
                bD, rD = pu[1] + prev[1], pu[2] + prev[2] + rnd * M
                v = v + (pu[0] - prev[0]) * pc[0]
                b = b + bD * pc[0] + M * pc[1]
                r = r + rD * pc[0] + M * pc[2] + rnd * M * pc[0]
                mag = mag + M * pc[0]
            prev = pu
        r = r + len(U) * rnd * mag
        base = (v, np.where(np.isnan(b), np.inf, b), np.where(np.isnan(r), np.inf, r))
    sc = _times(base, pof, rnd)
    return sc, pof


# ---- the explicit states ------------------------------------------------------------------------------------
class MCase:
    pass


def make_case(c, Theta):
    """c: an acquire_ref case (B, bB, Bo, H, nu, finite, skip ..); Theta p x q float64 (taken as exact)"""
    mc = MCase()
    mc.c, mc.Theta, mc.q, mc.m, mc.p = c, _f64(Theta), Theta.shape[1], c.m, c.p
    mc.rhs0 = np.array(c.H, dtype=ld) @ np.array(Theta, dtype=ld)
    mc.cache = {}
    return mc


def _state(mc, picks, ystar):
    c = mc.c
    key = (tuple(picks), tuple(tuple(float(v) for v in y) for y in ystar))
    if key in mc.cache:
        return mc.cache[key]
    Ht = np.array(c.H, dtype=ld)
    rhs = mc.rhs0.copy()
    for j, y in zip(picks, ystar):
        Ht = Ht + np.outer(c.B[j], c.B[j]) / c.nu
        rhs = rhs + np.outer(c.B[j], np.asarray(y, dtype=ld) / c.nu)
    L = P.cholesky_ld(Ht)
    Z = P.forward_ld(L, c.B.T)
    W = P.forward_ld(L, rhs)
    s = dict(L=L, Z=Z, mu=Z.T @ W, d=(Z * Z).sum(axis=0))
    if len(picks) == 0:
        mc.cache[key] = s
    return s


def believed_feasible(cfg, y):
    return all(ld(cfg.g[j]) * y[j] <= ld(cfg.cs[j]) for j in cfg.cons)


def states(mc, cfg, picks=None, k=None, rnd=E.U, full0=True):
    """The reference along the picks it is given (None: its own argmax, at most k): per t the state BEFORE pick t -- mu
    (m x q), d, the incumbent, the front [(u, c, tol_u, tol_c)], raw scores and pof, the masked scores, its own argmax
    `best` -- with the float64 bounds (without C) of mu, d, the score and pof and the evaluation terms.  full0=False
    (a front too long to evaluate every row with mpmath): step 0 is screened like the later steps.
    -> (picks, ystar, states)"""
    c = mc.c
    own = picks is None
    picks = [] if own else [int(j) for j in picks][:k]
    ystar, out, t = [], [], 0
    inc, inc_tol, pts = ld(cfg.best0), 0.0, list(cfg.points0)
    while True:
        s = _state(mc, picks[:t], ystar[:t])
        K = c.p + t
        aW = np.abs(P.inverse64(_f64(s["L"])))
        if t == 0:
            mag_mu = c.aB @ np.abs(mc.Theta)
            mag_d = _f64(s["d"]) + 2 * np.einsum("ki,ki->i", np.abs(_f64(s["Z"])), aW @ _f64(c.bB).T)
        bmu, bd = K * mag_mu, K * mag_d
        front = pareto(pts, cfg.r) if cfg.criterion == EHVI else []
        last = t == len(picks) and not (own and t < k)
        st = dict(t=t, mu=s["mu"], d=s["d"], finite=c.finite, bound_mu=bmu, bound_d=bd, incumbent=inc, incumbent_tol=inc_tol,
                  front=front, best=-1)
        if not last:
            (s64, bs, rs), (p64, bp, rp) = score_parts(cfg, s["mu"], s["d"], inc, front, bmu, bd, rnd)
            ok = c.finite & ~c.skip & np.isfinite(s64)
            if len(picks[:t]):
                ok[np.asarray(picks[:t], dtype=np.int64)] = False
            if t == 0 and full0:
                sc, pf = score_mp(cfg, s["mu"], s["d"], inc, front)
            else:
                live = s64[ok]
                spread = float(live.max() - live.min()) + abs(float(live.max())) if len(live) else 0.0
                near = set(np.nonzero(ok & (s64 >= live.max() - 1e-6 * spread))[0]) if len(live) else set()
                if t < len(picks):
                    near.add(picks[t])
                sc, pf = np.array(s64, dtype=ld), np.array(p64, dtype=ld)
                if near:
                    near = sorted(near)
                    a, b = score_mp(cfg, s["mu"], s["d"], inc, front, near)
                    sc[near], pf[near] = a[near], b[near]
            masked = np.where(ok, sc, -np.inf)
            st.update(raw=sc, pof=pf, score=masked, ok=ok, bound_score=bs, rest_score=rs, bound_pof=bp, rest_pof=rp,
                      best=int(np.argmax(masked)) if np.any(ok) else -1)
        out.append(st)
        if own and t < k and st["best"] >= 0:
            picks.append(st["best"])
        if t == len(picks):
            return picks, ystar, out
        j = picks[t]
        y = s["mu"][j].copy() if cfg.lie == A.BELIEVER else np.asarray(cfg.lie_value, dtype=ld)
        ystar.append(y)
        tol = bmu[j] if cfg.lie == A.BELIEVER else np.zeros(mc.q)     # what the device's y* may be off by, without C
        st["feasible"] = believed_feasible(cfg, y)
        # (a constant lie is compared with its limit exactly on both sides: no margin to keep)
        st["margin"] = min([abs(float(ld(cfg.g[r]) * y[r] - ld(cfg.cs[r]))) / tol[r] for r in cfg.cons if tol[r] > 0] + [np.inf])
        if st["feasible"]:
            if cfg.criterion in (CEI, CPI):
                o = cfg.objs[0]
                v = ld(cfg.g[o]) * y[o]
                if v < inc:
                    inc, inc_tol = v, tol[o]
            if cfg.criterion == EHVI:
                o1, o2 = cfg.objs
                pts.append((ld(cfg.g[o1]) * y[o1], ld(cfg.g[o2]) * y[o2], tol[o1], tol[o2]))
        a = _f64(s["Z"].T @ s["Z"][:, j])
        gam = float(c.nu + s["d"][j])
        delta = np.abs(_f64(y - s["mu"][j]))
        mag_a = c.aB @ ((aW.T @ aW) @ c.aB[j])
        mag_mu = mag_mu + np.outer(np.abs(a) + mag_a, delta) / gam
        mag_d = mag_d + (a * a + 2 * np.abs(a) * mag_a) / gam
        t += 1


def allowance(st, C):
    return C * st["bound_score"] + st["rest_score"]


gap_ratio = A.gap_ratio          # it reads score, ok, bound_score, rest_score of the states: the same names


# ---- the float64 restatement of the recurrences ---------------------------------------------------------
MUTATIONS = ["strip left out", "c_s from front point s", "constraint factor missing", ">= scored as <=",
             "d downdated per response", "infeasible pick moves the incumbent", "dominated point left in the front"]


def recurrence64(mc, cfg, k, force=None, mutate=None, extended=False):
    """The device's algorithm in NumPy float64 on the float64 oracle's B: explicit S, one a, one downdate of d and q of
    mu per step, one scoring; the front by the device's insertion rule.  force: the picks to follow (`own`: its own
    argmax).  extended: the same recurrences in long double on the long-double B with mpmath scores.
    -> dict(index, own, score, score0, pof0, mean, var, front, best, n_picked)"""
    c = mc.c
    if extended:
        B, nu, Th = c.B, c.nu, np.array(mc.Theta, dtype=ld)
        Linv = P.inverse_ld(P.cholesky_ld(c.H))
    else:
        B, nu, Th = c.Bo, float(np.exp(2.0 * c.sigma)), mc.Theta
        Linv = np.linalg.solve(np.linalg.cholesky(c.H), np.eye(c.p))
    ty = B.dtype.type
    S = Linv.T @ Linv
    d = ((Linv @ B.T) ** 2).sum(axis=0)
    mu = B @ Th
    best = ty(cfg.best0)
    front = []
    for p in cfg.points0:
        front = insert(front, (ty(p[0]), ty(p[1])), cfg.r)
    picked = np.zeros(c.m, dtype=bool)
    s, gamma, delta = np.zeros(c.p, dtype=B.dtype), ty(1), np.zeros(mc.q, dtype=B.dtype)
    index, own, score, score0, pof0 = [], [], [], None, None
    zero = np.zeros((c.m, mc.q))

    def downdate_and_score():
        nonlocal mu, d
        a = B @ s
        ag = a / gamma
        mu = mu + np.outer(ag, delta)
        for _ in range(mc.q if mutate == "d downdated per response" else 1):
            d = d - a * ag
        if extended:
            sc, pf = score_mp(cfg, mu, d, best, front)
        else:
            (sc, _, _), (pf, _, _) = score_parts(cfg, mu, d, best, front, zero, np.zeros(c.m), mutate=mutate)
        bad = ~c.finite | c.skip | ~np.isfinite(_f64(sc)) | picked
        return sc, pf, np.where(bad, -np.inf, sc)
    for t in range(k):
        raw, pf, sc = downdate_and_score()
        if t == 0:
            score0, pof0 = np.where(c.finite, raw, np.nan), np.where(c.finite, pf, np.nan)
        j = int(np.argmax(sc))
        if not sc[j] > -np.inf:
            break
        own.append(j)
        if force is not None:
            if t >= len(force):
                break
            j = int(force[t])
        index.append(j)
        score.append(raw[j])
        picked[j] = True
        b = B[j]
        s = S @ b
        gamma = nu + b @ s
        y = mu[j].copy() if cfg.lie == A.BELIEVER else np.asarray(cfg.lie_value, dtype=B.dtype)
        delta = y - mu[j]
        feasible = all(ty(cfg.g[r]) * y[r] <= ty(cfg.cs[r]) for r in cfg.cons)
        if feasible or mutate == "infeasible pick moves the incumbent":
            if cfg.criterion in (CEI, CPI):
                best = min(best, ty(cfg.g[cfg.objs[0]]) * y[cfg.objs[0]])
            if cfg.criterion == EHVI:
                o1, o2 = cfg.objs
                front = insert(front, (ty(cfg.g[o1]) * y[o1], ty(cfg.g[o2]) * y[o2]), cfg.r,
                               keep_dominated=mutate == "dominated point left in the front")
        S = S - np.outer(s, s) / gamma
    else:
        downdate_and_score()
    return dict(index=np.asarray(index, dtype=np.int64), own=np.asarray(own, dtype=np.int64),
                score=np.asarray(score, dtype=B.dtype), score0=score0, pof0=pof0,
                mean=np.where(c.finite[:, None], mu, np.nan), var=np.where(c.finite, d, np.nan),
                front=np.array([[p[0], p[1]] for p in front], dtype=B.dtype).reshape(-1, 2), best=best, n_picked=len(index))


# ---- measuring ----------------------------------------------------------------------------------------------
def ratios(got, sts, cfg, C=1.0, sub_rest=False):
    """{quantity: worst |got - want| / (C x bound + rest)} of a result (recurrence64's dict, or the device's outputs
    under the same names, front and best SIGNED) against the states along got["index"].  sub_rest: (|got - want| -
    rest)+ / (C x bound), what C is measured with.  A front of another length, or an incumbent that is infinite on one
    side only, counts as inf."""
    n = int(got["n_picked"])
    assert len(sts) >= n + 1
    last, fin = sts[n], sts[n]["finite"]
    out = {}

    def worst(g, want, bound, rest):
        g, want = np.asarray(g, dtype=ld), np.asarray(want, dtype=ld)
        bound, rest = np.broadcast_to(_f64(bound), g.shape), np.broadcast_to(_f64(rest), g.shape)
        if sub_rest:
            err = np.maximum(_f64(np.abs(g - want)) - rest, 0.0)
            den = C * bound
            r = np.zeros(err.shape)
            np.divide(err, den, out=r, where=den > 0)
            r[(den <= 0) & (err > 0)] = np.inf
            return float(np.max(r)) if r.size else 0.0
        return E.worst_ratio(g, want, C * bound + rest)
    if n:
        idx = [int(i) for i in got["index"][:n]]
        out["score"] = worst(got["score"][:n], [sts[t]["raw"][idx[t]] for t in range(n)],
                             [sts[t]["bound_score"][idx[t]] for t in range(n)], [sts[t]["rest_score"][idx[t]] for t in range(n)])
    if got.get("score0") is not None and "raw" in sts[0]:
        f0 = sts[0]["finite"]
        out["score0"] = worst(_f64(got["score0"])[f0], sts[0]["raw"][f0], sts[0]["bound_score"][f0], sts[0]["rest_score"][f0])
        out["pof0"] = worst(_f64(got["pof0"])[f0], sts[0]["pof"][f0], sts[0]["bound_pof"][f0], sts[0]["rest_pof"][f0])
    out["mean"] = worst(np.asarray(got["mean"])[fin], last["mu"][fin], last["bound_mu"][fin], 0.0)
    out["var"] = worst(np.asarray(got["var"])[fin], last["d"][fin], last["bound_d"][fin], 0.0)
    if cfg.criterion == EHVI:
        fr, want = np.asarray(got["front"]).reshape(-1, 2), last["front"]
        if len(fr) != len(want):
            out["front"] = np.inf
        elif len(fr):
            w = np.array([[p[0], p[1]] for p in want], dtype=ld)
            tol = np.array([[p[2], p[3]] for p in want], dtype=np.float64)
            err = _f64(np.abs(np.asarray(fr, dtype=ld) - w))
            out["front"] = float(np.max(np.where(err > 0, err / np.maximum(C * tol, 1e-300), 0.0)))
    if cfg.criterion in (CEI, CPI):
        b, w = float(got["best"]), float(last["incumbent"])
        if math.isinf(b) or math.isinf(w):
            out["best"] = 0.0 if b == w else np.inf
        else:
            err = abs(float(ld(got["best"]) - last["incumbent"]))
            out["best"] = err / max(C * last["incumbent_tol"], 1e-300) if err > 0 else 0.0
    return out


def constant_of(mc, cfg, sts, picks):
    """(C, r): r = the float64 restatement's own worst (err - rest) / bound along the same picks"""
    got = recurrence64(mc, cfg, max(len(picks), 1), force=picks)
    r = max(ratios(got, sts, cfg, 1.0, sub_rest=True).values())
    return E.constant_from_oracle_ratio(r), r


# ---- the cases both test files share ------------------------------------------------------------------------
SHAPE = ("d5", 130, 300, 5)      # acquire_ref.SHAPES' d = 5, p = 130 term set; two 256-row workgroups, k = 5
SEED = 140


def seeded_case(om_o, terms, m, seed, q, xcand=None, skip=None):
    """acquire_ref.seeded_case for response 0; the other columns of Theta are further draws on the same scale"""
    c = A.seeded_case(om_o, terms, m, seed, xcand, skip)
    Th = np.zeros((len(terms), q))
    Th[:, 0] = c.theta
    fin = c.finite
    Z = np.linalg.solve(np.linalg.cholesky(c.H), c.Bo[fin].T)
    sd = float(np.median(np.sqrt((Z * Z).sum(axis=0))))
    for r in range(1, q):
        z = np.random.default_rng(seed + 1000 * r).standard_normal(len(terms))
        spread = float(np.std(c.Bo[fin] @ z)) if fin.sum() > 1 else float(np.abs(c.Bo[fin] @ z).max())
        Th[:, r] = z * float(np.float32(2 * sd / spread))
    return make_case(c, Th)


def config_of(mc, criterion, lie, F0=3, best=True):
    """the call of a case: float32-rounded quantiles of the float64 oracle's means.  The first objective is maximised;
    the constraints alternate "<=" (at the 0.7 quantile; pof: 0.02) and ">=" (0.3; pof: 0.98); the incumbent is the 0.8 quantile of the
    maximised objective, the reference point lies at the poor 0.1 / 0.9 quantiles, the initial front holds the means of
    F0 fixed rows, the constant lie is each response's 0.6 quantile.  None when q has too few responses."""
    q = mc.q
    mu = (mc.c.Bo @ mc.Theta)[mc.c.finite]
    f = lambda v: float(np.float32(v))
    qt = lambda j, a: f(np.quantile(mu[:, j], a))
    if criterion == EHVI:
        if q < 2:
            return None
        objs, mx = ([0, 1], [True, False]) if q == 2 else ([0, 2], [True, False])
    elif criterion == POF:
        objs, mx = [], []
    else:
        objs, mx = [0], [True]
    free = [j for j in range(q) if j not in objs]
    lo, hi = (0.02, 0.98) if criterion == POF else (0.3, 0.7)      # pof alone: limits few rows meet, or its top scores tie at 1
    cons = [(j, "<=" if i % 2 == 0 else ">=", qt(j, lo if (i % 2 == 0) == (criterion == POF) else hi)) for i, j in enumerate(free)]
    if criterion == POF and not cons:
        return None
    kw = dict(objs=objs, maximize=mx, constraints=cons, lie=lie, lie_value=[qt(j, 0.6) for j in range(q)])
    if criterion in (CEI, CPI):
        kw.update(best=qt(0, 0.8) if best else None, xi=f(0.01 * (mu[:, 0].max() - mu[:, 0].min())))
    if criterion == EHVI:
        rows = [3, 11, 40, 77, 5, 123, 200][:F0]
        rows = [i % len(mu) for i in rows]
        kw.update(ref=[qt(objs[0], 0.1), qt(objs[1], 0.9)], front=[[f(mu[i, objs[0]]), f(mu[i, objs[1]])] for i in rows])
    return MConfig(criterion, q, **kw)
