"""Extended-precision reference of the Shapley effects of the fitted mean -- the instrument of
test_shapley_host.py (which proves its three routes against each other) and test_gpu_shapley.py (which uses it).
np.longdouble and NumPy only; sobol_ref and extended_ref are imported unchanged and nothing here comes from the
code under test.

Notation as sobol_ref: m_l, C_l, t = t_kl, t' = t_k'l; per term pair c_i = C_i[t,t'], mm_i = m_i[t] m_i[t'],
A_i = c_i + mm_i.  The dimensions are partitioned into P players; player g has mm_g = prod_{i in g} mm_i and
c_g = prod_{i in g} A_i - prod_{i in g} mm_i.  With V_u = sum_{k,k'} theta theta' prod_{g in u} c_g prod_{g not in u}
mm_g the variance of the ANOVA term of the set u of players, the Shapley effect is Sh_g = sum_{u contains g} V_u / |u|.

Three routes:
  (a) quadrature    Sh_g = sum_{k,k'} theta theta' c_g int_0^1 prod_{h != g} (mm_h + s c_h) ds, the integrand of degree
                    P - 1 in s, by the Gauss-Legendre rule of G = ceil(P / 2) nodes on [0,1] (gauss_legendre01: long
                    double, Newton-converged); with it sum |summands|, the same sum with |theta|, |c|, |mm|
  (b) symmetric     the coefficients e_r of prod_{h != g} (mm_h + s c_h) by convolution, then sum_r e_r / (r + 1)
  (c) brute force   conditional expectations over the full tensor grid of nodes for all 2^P subsets of players, V_u
                    by inclusion-exclusion, then the definition

Tolerance of a float64 evaluation of (a) on the same float64 tables, sobol_ref's rule gamma_K . sum |summands|:
K = p^2 + 3 d + 2 G + 4 (a summand is theta theta' w_n times P factors, each one fused multiply-add of values that
cost the 3 d roundings of the player recursion, summed over G nodes and p^2 pairs), and (P - 1) eps sum |summands|
for nodes one ulp off (eps = 2^-52): a node enters the P - 1 factors mm_h + s c_h, each |mm_h| + s |c_h| at most in
sum |summands|.
"""
import itertools

import numpy as np

import extended_ref as E
import sobol_ref as S

ld = np.longdouble
ULP = 2.0 ** -52


def gauss_legendre01(G):
    """(nodes, weights) of the G-point Gauss-Legendre rule on [0,1] in long double, nodes ascending.
    Newton on Q_G(s) = (-1)^G P_G(2 s - 1) below 1/2, the upper half by symmetry; the recurrence runs on the
    differences D_k = Q_k - Q_{k-1}, (k + 1) D_{k+1} = k D_k - 2 (2 k + 1) s Q_k, so that 2 s - 1 is never formed
    and a node near 0 keeps its relative accuracy.  w = 1 / (s (1 - s) Q_G'(s)^2)."""
    G = int(G)
    nodes, weights = np.zeros(G, dtype=ld), np.zeros(G, dtype=ld)

    def q_dq(s):
        q, dq, dk, ddk = ld(1), ld(0), ld(0), ld(0)
        for k in range(G):
            dn = (k * dk - 2 * (2 * k + 1) * s * q) / (k + 1)
            ddn = (k * ddk - 2 * (2 * k + 1) * (q + s * dq)) / (k + 1)
            q, dq, dk, ddk = q + dn, dq + ddn, dn, ddn
        return q, dq
    for i in range((G + 1) // 2):
        s = np.sin(ld(0.5) * np.pi * (ld(i) + ld(0.75)) / (ld(G) + ld(0.5))) ** 2
        if 2 * i + 1 == G:
            s = ld(0.5)
        else:
            for _ in range(100):
                q, dq = q_dq(s)
                step = q / dq
                s = s - step
                if abs(step) <= 4 * E.EPS * s:
                    break
        _, dq = q_dq(s)
        w = 1 / (s * (1 - s) * dq * dq)
        nodes[i], weights[i] = s, w
        nodes[G - 1 - i], weights[G - 1 - i] = 1 - s, w
    return nodes, weights


def players_of(d, groups=None):
    """the list of dimension lists; None: every dimension its own player"""
    if groups is None:
        return [[l] for l in range(d)]
    players = [[int(l) for l in g] for g in groups]
    assert sorted(l for g in players for l in g) == list(range(d))
    return players


def _pair_tables(terms, m, Cv, dtype):
    """(c, mm): per dimension the p x p arrays C_l[t_kl, t_k'l] and m_l[t_kl] m_l[t_k'l]"""
    c, mm = [], []
    for l in range(terms.shape[1]):
        t = terms[:, l]
        c.append(np.asarray(Cv[l], dtype=dtype)[t[:, None], t[None, :]])
        mk = np.asarray(m[l], dtype=dtype)[t]
        mm.append(np.outer(mk, mk))
    return c, mm


def _player_tables(c, mm, players, dtype):
    """(c_g, mm_g, |c_g|, |mm_g|) per player, by D <- c PA + mm D, PA <- PA (c + mm); the absolute ones from
    |c| and |mm| in place of the values"""
    p = c[0].shape[0]
    cg, mg, acg, amg = [], [], [], []
    for dims in players:
        one, zero = np.ones((p, p), dtype=dtype), np.zeros((p, p), dtype=dtype)
        pa, dd, mmm, apa, add, ammm = one, zero, one, one, zero, one
        for i in dims:
            dd, pa, mmm = c[i] * pa + mm[i] * dd, pa * (c[i] + mm[i]), mmm * mm[i]
            ac, am = np.abs(c[i]), np.abs(mm[i])
            add, apa, ammm = ac * apa + am * add, apa * (ac + am), ammm * am
        cg.append(dd), mg.append(mmm), acg.append(add), amg.append(ammm)
    return cg, mg, acg, amg


def _theta(Theta, dtype):
    Th = np.asarray(Theta, dtype=dtype)
    return Th[:, None] if Th.ndim == 1 else Th


def shapley(terms, Theta, m, Cv, groups=None, dtype=ld, pair_weights=None, rule=None, ignore_groups=False):
    """Route (a).  dict(players, Sh (P x q) in `dtype`, abs_Sh (P x q, float64): sum |summands|, tol_Sh: the
    tolerance of a float64 evaluation on the same tables).
    pair_weights (p x p): the weight every pair (k, k') of terms enters with -- None: 1 (the full double sum).
    rule: (nodes, weights) in place of gauss_legendre01(ceil(P / 2)) -- mutations: a node dropped, nodes left on
    [-1,1].  ignore_groups: a mutation -- every dimension swept as a player of its own, a player's effect read
    from the slot of its last dimension."""
    terms = np.asarray(terms, dtype=np.int64)
    p, d = terms.shape
    Th = _theta(Theta, dtype)
    aTh = np.abs(Th)
    players = players_of(d, groups)
    P = len(players)
    G = (P + 1) // 2
    nodes, weights = gauss_legendre01(G) if rule is None else rule
    nodes, weights = np.asarray(nodes, dtype=dtype), np.asarray(weights, dtype=dtype)
    c, mm = _pair_tables(terms, m, Cv, dtype)
    swept = [[l] for l in range(d)] if ignore_groups else players
    cg, mg, acg, amg = _player_tables(c, mm, swept, dtype)
    n = len(swept)
    one = np.ones((p, p), dtype=dtype)
    F = [np.zeros((p, p), dtype=dtype) for _ in range(n)]
    aF = [np.zeros((p, p), dtype=dtype) for _ in range(n)]
    for s, w in zip(nodes, weights):
        for cs, ms, sn, wn, out in ((cg, mg, s, w, F), (acg, amg, np.abs(s), np.abs(w), aF)):
            v = [ms[g] + sn * cs[g] for g in range(n)]
            suf = [one] * (n + 1)
            for g in range(n - 1, -1, -1):
                suf[g] = suf[g + 1] * v[g]
            pre = one * wn
            for g in range(n):
                out[g] = out[g] + cs[g] * (pre * suf[g + 1])
                pre = pre * v[g]
    if ignore_groups:
        F, aF = [F[dims[-1]] for dims in players], [aF[dims[-1]] for dims in players]
    W = one if pair_weights is None else np.asarray(pair_weights, dtype=dtype)
    Sh = np.stack([np.einsum("kj,kl,lj->j", Th, F[g] * W, Th) for g in range(P)])
    aSh = E._f64(np.stack([np.einsum("kj,kl,lj->j", aTh, aF[g] * W, aTh) for g in range(P)]))
    K = p * p + 3 * d + 2 * G + 4
    return dict(players=players, Sh=Sh, abs_Sh=aSh, tol_Sh=(E.gamma(K) + (P - 1) * ULP) * aSh, G=G)


def shapley_symmetric(terms, Theta, m, Cv, groups=None):
    """Route (b), long double: Sh (P x q) without quadrature"""
    terms = np.asarray(terms, dtype=np.int64)
    p, d = terms.shape
    Th = _theta(Theta, ld)
    players = players_of(d, groups)
    P = len(players)
    c, mm = _pair_tables(terms, m, Cv, ld)
    cg, mg, _, _ = _player_tables(c, mm, players, ld)
    Sh = []
    for g in range(P):
        e = [np.ones((p, p), dtype=ld)]                                   # coefficients of s^r, ascending
        for h in range(P):
            if h == g:
                continue
            nxt = [np.zeros((p, p), dtype=ld) for _ in range(len(e) + 1)]
            for r, er in enumerate(e):
                nxt[r] = nxt[r] + er * mg[h]
                nxt[r + 1] = nxt[r + 1] + er * cg[h]
            e = nxt
        integral = sum(er / ld(r + 1) for r, er in enumerate(e))
        Sh.append(np.einsum("kj,kl,lj->j", Th, cg[g] * integral, Th))
    return np.stack(Sh)


def shapley_brute(ref_grid, n, terms, Theta, weights, groups=None):
    """Route (c): Sh (P x q) from f on the whole tensor grid (ref_grid: ExtendedRef on sobol_ref.grid_rows(nodes)),
    as sobol_ref.brute_force forms its conditional means: Var E[f | x_u] for every subset u of players, V_u by
    inclusion-exclusion, Sh_g = sum_{u contains g} V_u / |u|.  Independent of the pair formulas."""
    d = ref_grid.d
    Th = _theta(Theta, ld)
    q = Th.shape[1]
    players = players_of(d, groups)
    P = len(players)
    B, _ = ref_grid.getmat(terms)
    f = (B @ Th).reshape((n,) * d + (q,))
    wn = S.normalised_weights(weights, n, d)

    def shaped(l):
        return wn[:, l].reshape((1,) * l + (n,) + (1,) * (d - l))
    axes = tuple(range(d))
    Wfull = np.ones((1,) * (d + 1), dtype=ld)
    for l in range(d):
        Wfull = Wfull * shaped(l)
    mu = (Wfull * f).sum(axis=axes)
    closed = {}
    for u in itertools.chain.from_iterable(itertools.combinations(range(P), r) for r in range(P + 1)):
        inside = [l for g in u for l in players[g]]
        others = tuple(l for l in range(d) if l not in inside)
        Wo, Wi = np.ones((1,) * (d + 1), dtype=ld), np.ones((1,) * (d + 1), dtype=ld)
        for l in range(d):
            if l in inside:
                Wi = Wi * shaped(l)
            else:
                Wo = Wo * shaped(l)
        cond = (Wo * f).sum(axis=others, keepdims=True) if others else f           # E[f | x_u]
        closed[u] = (Wi * (cond - mu) ** 2).sum(axis=axes)
    Sh = [np.zeros(q, dtype=ld) for _ in range(P)]
    for u in closed:
        if not u:
            continue
        Vu = sum((-1) ** (len(u) - len(v)) * closed[v]
                 for r in range(len(u) + 1) for v in itertools.combinations(u, r))
        for g in u:
            Sh[g] = Sh[g] + Vu / len(u)
    return np.stack(Sh)
