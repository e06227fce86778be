"""Extended-precision reference of C = E[grad f grad f^T] and gbar = E[grad f] of the fitted mean -- the instrument
of test_active_host.py (which proves it against a brute-force sum over the tensor grid of nodes) and
test_gpu_active.py (which uses it).  np.longdouble and NumPy only; sobol_ref, extended_ref and extended_dx_ref are
imported unchanged and nothing here comes from the code under test.

Notation as sobol_ref: m_l, C_l, A_l = C_l + m_l m_l^T over a product of discrete measures with normalised weights
w^.  psi = R = cov(x, knots) . rot, psi' = R' = (dcov/dx) . rot in raw input units (extended_dx_ref's g_l . s).  Three
more tables per dimension, all raw moments (nothing centred, nothing subtracted):

    dm_l[t]   = sum_i w^_i R'_t(z_il)
    X_l[a,b]  = sum_i w^_i R'_a(z_il) R_b(z_il)              not symmetric
    D_l[a,b]  = sum_i w^_i R'_a(z_il) R'_b(z_il)             symmetric

and per response, t = t_kl, t' = t_k'l, s = t_km, s' = t_k'm:

    gbar_l = sum_k theta_k dm_l[t] prod_{i != l} m_i[t_ki]
    C_ll   = sum_{k,k'} theta_k theta_k' D_l[t,t'] prod_{i != l} A_i[t_ki,t_k'i]
    C_lm   = sum_{k,k'} theta_k theta_k' X_l[t,t'] X_m[s',s] prod_{i != l,m} A_i[t_ki,t_k'i]          l != m

Tolerances for a float64 result, extended_ref's rule C . bound + gamma_k . sum |summands|, derived and not fitted.

Stage 1, with (R, bR) and (R', bR') the long-double value and derivative and the bounds of their knot sums
(bR = |K| |rot|, bR' = |K'| |rot|):

    tol_dm[t]  = Cc sum w^ bR'_t + gamma_{n+2} sum w^ |R'_t|
    tol_X[a,b] = Cc sum w^ (bR'_a |R_b| + |R'_a| bR_b) + gamma_{n+3} sum w^ |R'_a| |R_b|
    tol_D[a,b] = Cc sum w^ (bR'_a |R'_b| + |R'_a| bR'_b) + gamma_{n+3} sum w^ |R'_a| |R'_b|

Cc is eight times the float64 restatement's own max(err / bound) of R and R' on the same nodes (the rule of
sobol_ref.ref_tables; the float64 side is extended_dx_ref._cov_f64 times the rotation).  gamma_{n+2}: n summands, one
product by the weight each and the division by the weight sum; gamma_{n+3}: one more product, that of the two
factors.  Nothing is centred, so no tol_m term enters.

Stage 2, on the same float64 tables on both sides:

    gbar    gamma_{p+d+1} sum_k |theta_k dm_l[t] prod m_i|
    C       gamma_{p^2+3d+4} sum_{k,k'} |theta_k theta_k'| |X_l| |X_m| prod |A_i|     (|D_l| on the diagonal)

The gamma indices against the summation lengths a float64 evaluation builds: a summand of gbar is theta times dm
times d - 1 means, d roundings, summed over p terms -- p + d - 1, within p + d + 1.  A summand of C is theta theta'
(one product) times d factors, every A_i one product and one addition from the tables and one product into the
running product (3 d at most), summed over p^2 ordered pairs; a tiled sum that visits the unordered pairs and adds
the two orientations spends one addition on that and a weight of 1 or 1/2, which is exact -- within p^2 + 3 d + 4.
"""
import numpy as np

import extended_dx_ref as X
import extended_ref as E
import sobol_ref as S

ld = np.longdouble


# ---- stage 1: the raw basis and its derivative ----------------------------------------------------------------
def raw_dx(om_o, x, dtype=ld):
    """per dimension (R, bR, R', bR'), n x m_l each, of an oracle model on the rows x; dtype = float64: the plain
    NumPy restatement (no bounds: None)"""
    x = np.asarray(x, dtype=np.float64)
    hyp = np.asarray(om_o.hyp, dtype=np.float64)
    kinds = list(om_o.kinds)
    knots = [np.asarray(om_o.knots_of(k), dtype=np.float64) for k in range(om_o.d)]
    kst = np.concatenate([[0], np.cumsum([len(k) for k in knots])]).astype(np.int64)
    hst = np.concatenate([[0], np.cumsum([E.NUMHYP[k] for k in kinds])]).astype(np.int64)
    out = []
    for k in range(om_o.d):
        mk = len(knots[k])
        rk = np.asarray(om_o.rotmat[:mk, kst[k]:kst[k] + mk], dtype=dtype)
        h = hyp[hst[k]:hst[k + 1]]
        if dtype is ld:
            K, _ = E.cov_ld(kinds[k], x[:, k], knots[k], h)
            dK = X.dcov_dx_ld(kinds[k], x[:, k], knots[k], h)
            out.append((K @ rk, np.abs(K) @ np.abs(rk), dK @ rk, np.abs(dK) @ np.abs(rk)))
        else:
            K, dK = X._cov_f64(kinds[k], x[:, k], knots[k], h)
            out.append((K @ rk, None, dK @ rk, None))
    return out


def f64_raw_ratio(om_o, x, levels, raw=None):
    """max(err / bound) of the float64 restatement of R and R' on the nodes x: what constant_from_oracle_ratio is
    given"""
    raw = raw_dx(om_o, x) if raw is None else raw
    r64 = raw_dx(om_o, x, dtype=np.float64)
    worst = 0.0
    for l in range(om_o.d):
        L = levels[l]
        worst = max(worst, E.worst_ratio(r64[l][0][:, :L], raw[l][0][:, :L], raw[l][1][:, :L]),
                    E.worst_ratio(r64[l][2][:, :L], raw[l][2][:, :L], raw[l][3][:, :L]))
    return worst


def grad_tables_from_bases(R, Rp, levels, weights, dtype=ld):
    """(dm, Xc, Dd): lists per dimension, from the raw 1-D bases R[l] and their derivatives Rp[l] (n x >= L_l)"""
    n, d = R[0].shape[0], len(R)
    wn = S.normalised_weights(weights, n, d, dtype)
    dm, Xc, Dd = [], [], []
    for l in range(d):
        r = np.asarray(R[l][:, :levels[l]], dtype=dtype)
        rp = np.asarray(Rp[l][:, :levels[l]], dtype=dtype)
        w = wn[:, l]
        dm.append(w @ rp)
        Xc.append((rp * w[:, None]).T @ r)
        Dd.append((rp * w[:, None]).T @ rp)
    return dm, Xc, Dd


def ref_grad_tables(raw, levels, weights, Cc):
    """((dm, Xc, Dd), (tol_dm, tol_X, tol_D)) in long double from raw_dx's output; Cc: constant_from_oracle_ratio"""
    n, d = raw[0][0].shape[0], len(raw)
    wn = E._f64(S.normalised_weights(weights, n, d))
    tabs = grad_tables_from_bases([r[0] for r in raw], [r[2] for r in raw], levels, weights)
    tol_dm, tol_X, tol_D = [], [], []
    for l in range(d):
        L = levels[l]
        aR, bR, aP, bP = (E._f64(np.abs(a[:, :L])) for a in raw[l])
        w = wn[:, l]
        tol_dm.append(Cc * (w @ bP) + E.gamma(n + 2) * (w @ aP))
        wP, wbP = aP * w[:, None], bP * w[:, None]
        tol_X.append(Cc * (wbP.T @ aR + wP.T @ bR) + E.gamma(n + 3) * (wP.T @ aR))
        tol_D.append(Cc * (wbP.T @ aP + wP.T @ bP) + E.gamma(n + 3) * (wP.T @ aP))
    return tabs, (tol_dm, tol_X, tol_D)


# ---- stage 2: the closed form on given tables ----------------------------------------------------------------------
def ordered_weights(p, tile):
    """(U, W): U the weights of the device's sum -- the upper triangle of pairs of `tile`-wide term tiles, 1 off the
    diagonal, 1/2 on it, every visited pair adding both orientations -- and W = U + U^T, the weight every ORDERED
    pair (k, k') enters with: 1 throughout."""
    U = S.tile_weights(p, tile, diag=0.5, off=1.0)
    return U, U + U.T


def formulas_active(terms, Theta, m, Cv, dm, Xc, Dd, dtype=ld, pair_weights=None, untransposed=False, d_is_x=False):
    """dict(gbar (d x q), C (d x d x q, both triangles evaluated), abs_gbar, abs_C, tol_gbar, tol_C) in `dtype`; the
    tolerances are those of a float64 evaluation on the same tables.
    pair_weights (p x p): the weight every ORDERED pair (k, k') of terms enters C with -- None: 1.
    Mutations: untransposed -- X_m read as X_m[s,s']; d_is_x -- X_l in the place of D_l."""
    terms = np.asarray(terms, dtype=np.int64)
    p, d = terms.shape
    Th = np.asarray(Theta, dtype=dtype)
    if Th.ndim == 1:
        Th = Th[:, None]
    aTh = np.abs(Th)
    q = Th.shape[1]
    m, Cv, dm, Xc, Dd = ([np.asarray(a, dtype=dtype) for a in tab] for tab in (m, Cv, dm, Xc, Dd))
    # gbar: exclusion products by prefix and suffix
    mk = [m[l][terms[:, l]] for l in range(d)]
    pre, suf = [np.ones(p, dtype=dtype)], [np.ones(p, dtype=dtype)]
    for l in range(d):
        pre.append(pre[-1] * mk[l])
        suf.append(suf[-1] * mk[d - 1 - l])
    gbar, agbar = [], []
    for l in range(d):
        h = dm[l][terms[:, l]] * pre[l] * suf[d - 1 - l]
        gbar.append(Th.T @ h), agbar.append(aTh.T @ np.abs(h))
    out = dict(gbar=np.stack(gbar), abs_gbar=E._f64(np.stack(agbar)))
    out["tol_gbar"] = E.gamma(p + d + 1) * out["abs_gbar"]
    # the pair sums over the terms
    a, xf, dg = [], [], []
    for l in range(d):
        t = terms[:, l]
        A = Cv[l] + np.outer(m[l], m[l])
        a.append(A[t[:, None], t[None, :]])
        xf.append(Xc[l][t[:, None], t[None, :]])                                       # X_l[t_k, t_k']
        dg.append((Xc[l] if d_is_x else Dd[l])[t[:, None], t[None, :]])
    onepp = np.ones((p, p), dtype=dtype)
    W = onepp if pair_weights is None else np.asarray(pair_weights, dtype=dtype)
    sufp = [onepp] * (d + 1)                                                           # products over i >= l
    for l in range(d - 1, -1, -1):
        sufp[l] = sufp[l + 1] * a[l]
    asufp = [np.abs(s) for s in sufp]
    Cm, aC = np.zeros((d, d, q), dtype=dtype), np.zeros((d, d, q), dtype=dtype)

    def quad(F, aF):
        return np.einsum("kj,kl,lj->j", Th, F * W, Th), np.einsum("kj,kl,lj->j", aTh, aF * W, aTh)
    prep, aprep = onepp, onepp
    for l in range(d):
        Cm[l, l], aC[l, l] = quad(prep * dg[l] * sufp[l + 1], aprep * np.abs(dg[l]) * asufp[l + 1])
        rowf, arow = prep * xf[l], aprep * np.abs(xf[l])                                # X_l[t,t'] prod_{i<l} A_i
        rowb = prep * xf[l].T                                                          # X_l[t',t]
        for j in range(l + 1, d):
            xbj = xf[j] if untransposed else xf[j].T                                   # X_j[s',s]
            xfj = xf[j].T if untransposed else xf[j]
            Cm[l, j], aC[l, j] = quad(rowf * xbj * sufp[j + 1], arow * np.abs(xbj) * asufp[j + 1])
            Cm[j, l], _ = quad(rowb * xfj * sufp[j + 1], arow * np.abs(xbj) * asufp[j + 1])
            aC[j, l] = aC[l, j]
            rowf, rowb, arow = rowf * a[j], rowb * a[j], arow * np.abs(a[j])
        prep, aprep = prep * a[l], aprep * np.abs(a[l])
    out.update(C=Cm, abs_C=E._f64(aC))
    out["tol_C"] = E.gamma(p * p + 3 * d + 4) * out["abs_C"]
    return out


def pack_out(f):
    """what obhip_active_dev writes, q x (d + d (d + 1) / 2): gbar, then the upper triangle of C row-major -- and the
    tolerances packed alike: (want (long double), tol (float64))"""
    d = f["gbar"].shape[0]
    iu = np.triu_indices(d)
    want = np.concatenate([f["gbar"], f["C"][iu[0], iu[1]]], axis=0).T
    tol = np.concatenate([f["tol_gbar"], f["tol_C"][iu[0], iu[1]]], axis=0).T
    return want, tol


# ---- brute force: the weighted sum of grad f grad f^T over the full tensor grid of nodes ------------------------
def brute_active(refdx_grid, idx, n, terms, Theta, weights):
    """dict(gbar (d x q), C (d x d x q), abs_C (d x d x q): sum w |J_l| |J_m| with |J| from absolute summands) from
    grad f on the whole grid (refdx_grid: ExtendedRefDx on sobol_ref.grid_rows(nodes)).  Independent of the tables."""
    d = refdx_grid.d
    Th = np.asarray(Theta, dtype=ld)
    if Th.ndim == 1:
        Th = Th[:, None]
    wn = S.normalised_weights(weights, n, d)
    Wrow = np.prod(wn[idx, np.arange(d)[None, :]], axis=1)
    J, aJ = [], []
    for l in range(d):
        dB, _ = refdx_grid.getmat_dx(terms, l)
        J.append(dB @ Th), aJ.append(np.abs(dB) @ np.abs(Th))
    J, aJ = np.stack(J), np.stack(aJ)                                                  # d x rows x q
    return dict(gbar=np.einsum("i,lij->lj", Wrow, J), C=np.einsum("i,lij,mij->lmj", Wrow, J, J),
                abs_C=E._f64(np.einsum("i,lij,mij->lmj", Wrow, aJ, aJ)), abs_gbar=E._f64(np.einsum("i,lij->lj", Wrow, aJ)))


# ---- random CONSISTENT tables: the five tables of one synthetic discrete measure ---------------------------------
def consistent_tables(rng, levels, nodes=6):
    """(m, Cv, dm, Xc, Dd) float64 of a synthetic measure of `nodes` points per dimension: psi_0 near 1, the higher
    levels falling off like 0.5^t, psi' of the same fall-off around a mean slope of 2 (a derivative of mean zero
    makes E[d f / d x_l d f / d x_m] of random terms a near-cancellation, which the host test rules out); all five
    tables formed from these psi and psi' (in long double, rounded once; Cv and Dd symmetrised bit for bit).
    Independent random matrices would not be the moments of any measure, and C would not be positive
    semi-definite."""
    m, Cv, dm, Xc, Dd = [], [], [], [], []
    for L in levels:
        fall = 0.5 ** np.arange(L)
        psi = 0.6 * rng.standard_normal((nodes, L)) * fall[None, :]
        psi[:, 0] = 1.0 + 0.1 * rng.standard_normal(nodes)
        dpsi = (2.0 + rng.standard_normal((nodes, L))) * fall[None, :]
        w = rng.uniform(0.5, 1.5, nodes)
        (ml,), (cl,) = S.tables_from_bases([psi], [L], w[:, None])
        (a,), (b,), (c,) = grad_tables_from_bases([psi], [dpsi], [L], w[:, None])
        cl, c = E._f64(cl), E._f64(c)
        m.append(E._f64(ml)), Cv.append(0.5 * (cl + cl.T)), dm.append(E._f64(a)), Xc.append(E._f64(b))
        Dd.append(0.5 * (c + c.T))
    return m, Cv, dm, Xc, Dd


def pack_grad_tables(dm, Xc, Dd):
    f = np.float64
    return (np.concatenate([np.asarray(a, dtype=f) for a in dm]), np.concatenate([np.asarray(a, dtype=f).ravel() for a in Xc]),
            np.concatenate([np.asarray(a, dtype=f).ravel() for a in Dd]))


def unpack_grad_tables(pdm, px, pd, levels):
    dm, Xc = S.unpack_tables(pdm, px, levels)
    return dm, Xc, S.unpack_tables(pdm, pd, levels)[1]
