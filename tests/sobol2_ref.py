"""Extended-precision reference of the pairwise part of the variance decomposition -- the instrument of
test_sobol2_host.py (which proves it against a brute-force ANOVA) and test_gpu_sobol2.py (which uses it).
np.longdouble and NumPy only; sobol_ref and extended_ref are imported unchanged and nothing here comes from
the code under test.

Notation as sobol_ref: m_l, C_l, A_l = C_l + m_l m_l^T, t = t_kl, t' = t_k'l.  For a pair i < j of dimensions
(order (0,1), (0,2), .. (0,d-1), (1,2), ..):

    G_ij[t,s] = sum_{k: t_ki = t, t_kj = s} theta_k prod_{l != i,j} m_l[t_kl]                 L_i x L_j
    V2_ij     = sum_{t,t',s,s'} C_i[t,t'] C_j[s,s'] G_ij[t,s] G_ij[t',s']                   = tr(C_i G C_j G^T)
              = Var E[f | x_i, x_j] - V1_i - V1_j
    VT2_ij    = sum_{k,k'} theta_k theta_k' C_i[t,t'] C_j[t,t'] prod_{l != i,j} A_l[t_kl, t_k'l]
              = the variances of all subsets of dimensions that hold both i and j

Tolerances for a float64 result on the same float64 tables, extended_ref's rule gamma_k . sum |summands|:

    tol_G    gamma_{p+d+1} |G|,  |G| summed from absolute values
    tol_V2   gamma_{p+d+2 L_i L_j+6} sum |C_i| |C_j| |G| |G|
    tol_VT2  gamma_{p^2+3d+4} sum |theta theta'| |C_i| |C_j| prod |A_l|

The gamma indices against the summation lengths a float64 evaluation builds: an entry of G is one product of
d - 1 factors (theta and d - 2 means) summed over at most p terms, p + d - 2 roundings, within p + d + 1.  V2 as
(C_i G) then <., G C_j>: L_i and L_j products and sums, one product of the two, a sum over L_i L_j cells -- L_i +
L_j + L_i L_j + 1 <= 2 L_i L_j + 2 roundings (L >= 2; L = 1 gives C = 0 and V2 = 0 exactly) beside those of one
entry of G; the index p + d + 2 L_i L_j + 6 counts G's roundings once, as sobol_ref's V1 does, which is
the tighter choice.  A summand of VT2 is theta theta' times d factors, each A_l one addition and one product
from the tables (3 d + 2), summed over p^2 pairs; a tiled sum adds its weight and no more.  The indices are
those lengths, not fitted to any result.
"""
import numpy as np

import extended_ref as E
import sobol_ref as S

ld = np.longdouble


def pairs_of(d):
    return [(i, j) for i in range(d) for j in range(i + 1, d)]


def formulas2(terms, Theta, m, Cv, dtype=ld, pair_weights=None, drop_middle=False):
    """dict(pairs, G (list of L_i x L_j x q), V2 (n_pairs x q), VT2 (n_pairs x q)) in `dtype`, and the
    tolerances tol_G (list), tol_V2, tol_VT2 (float64) of a float64 evaluation on the same tables, with the
    absolute sums abs_V2, abs_VT2 they are made of.
    pair_weights (p x p): the weight every pair (k, k') of terms enters VT2 with -- None: 1.
    drop_middle: a mutation -- the factors A_l, i < l < j, left out of VT2."""
    terms = np.asarray(terms, dtype=np.int64)
    p, d = terms.shape
    Th = np.asarray(Theta, dtype=dtype)
    if Th.ndim == 1:
        Th = Th[:, None]
    aTh = np.abs(Th)
    q = Th.shape[1]
    m = [np.asarray(a, dtype=dtype) for a in m]
    Cv = [np.asarray(a, dtype=dtype) for a in Cv]
    L = [len(a) for a in m]
    pairs = pairs_of(d)
    mk = [m[l][terms[:, l]] for l in range(d)]
    one = np.ones(p, dtype=dtype)
    G, tG, V2, aV2 = [], [], [], []
    for i, j in pairs:
        hole = one.copy()
        for l in range(d):
            if l != i and l != j:
                hole = hole * mk[l]
        cell = terms[:, i] * L[j] + terms[:, j]
        sel = (cell[None, :] == np.arange(L[i] * L[j])[:, None]).astype(dtype)          # cells x p
        g = (sel @ (Th * hole[:, None])).reshape(L[i], L[j], q)
        ag = (sel @ (aTh * np.abs(hole)[:, None])).reshape(L[i], L[j], q)
        G.append(g), tG.append(E.gamma(p + d + 1) * E._f64(ag))
        V2.append(np.einsum("tu,sv,tsj,uvj->j", Cv[i], Cv[j], g, g))
        aV2.append(np.einsum("tu,sv,tsj,uvj->j", np.abs(Cv[i]), np.abs(Cv[j]), ag, ag))
    out = dict(pairs=np.array(pairs, dtype=np.int64).reshape(-1, 2), G=G, tol_G=tG)
    if pairs:
        gam = np.array([E.gamma(p + d + 2 * L[i] * L[j] + 6) for i, j in pairs])
        out.update(V2=np.stack(V2), abs_V2=E._f64(np.stack(aV2)))
        out["tol_V2"] = gam[:, None] * out["abs_V2"]
    else:
        out.update(V2=np.zeros((0, q), dtype=dtype), abs_V2=np.zeros((0, q)), tol_V2=np.zeros((0, q)))
    # the pair sums over the terms
    a, c = [], []
    for l in range(d):
        t = terms[:, l]
        A = Cv[l] + np.outer(m[l], m[l])
        a.append(A[t[:, None], t[None, :]])
        c.append(Cv[l][t[:, None], t[None, :]])
    onepp = np.ones((p, p), dtype=dtype)
    W = onepp if pair_weights is None else np.asarray(pair_weights, dtype=dtype)
    suf = [onepp] * (d + 1)                                                            # products over l > j
    for l in range(d - 1, 0, -1):
        suf[l - 1] = suf[l] * a[l]
    asuf = [np.abs(x) for x in suf]
    VT2, aVT2 = [], []
    pre, apre = onepp, onepp
    for i in range(d):
        row, arow = pre * c[i], apre * np.abs(c[i])
        for j in range(i + 1, d):
            F, aF = row * c[j] * suf[j], arow * np.abs(c[j]) * asuf[j]
            VT2.append(np.einsum("kj,kl,lj->j", Th, F * W, Th))
            aVT2.append(np.einsum("kj,kl,lj->j", aTh, aF * W, aTh))
            if not drop_middle:
                row, arow = row * a[j], arow * np.abs(a[j])
        pre, apre = pre * a[i], apre * np.abs(a[i])
    if pairs:
        out.update(VT2=np.stack(VT2), abs_VT2=E._f64(np.stack(aVT2)))
    else:
        out.update(VT2=np.zeros((0, q), dtype=dtype), abs_VT2=np.zeros((0, q)))
    out["tol_VT2"] = E.gamma(p * p + 3 * d + 4) * out["abs_VT2"]
    return out


def brute_force2(ref_grid, n, terms, Theta, weights):
    """dict(Vc (n_pairs x q): Var E[f | x_i, x_j]; VT2 (n_pairs x q): E[h^2], h = f - E_i f - E_j f + E_ij f with
    the means over the axes i and j at fixed other coordinates) from f on the whole tensor grid
    (ref_grid: ExtendedRef on sobol_ref.grid_rows(nodes)).  Independent of the pair formulas."""
    d = ref_grid.d
    Th = np.asarray(Theta, dtype=ld)
    if Th.ndim == 1:
        Th = Th[:, None]
    q = Th.shape[1]
    B, _ = ref_grid.getmat(terms)
    f = (B @ Th).reshape((n,) * d + (q,))
    wn = S.normalised_weights(weights, n, d)

    def shaped(l):
        return wn[:, l].reshape((1,) * l + (n,) + (1,) * (d - l))
    Wfull = np.ones((1,) * (d + 1), dtype=ld)
    for l in range(d):
        Wfull = Wfull * shaped(l)
    axes = tuple(range(d))
    mu = (Wfull * f).sum(axis=axes)
    Vc, VT2 = [], []
    for i, j in pairs_of(d):
        others = tuple(l for l in range(d) if l not in (i, j))
        Wo = np.ones((1,) * (d + 1), dtype=ld)
        for l in others:
            Wo = Wo * shaped(l)
        cond = (Wo * f).sum(axis=others, keepdims=True) if others else f           # E[f | x_i, x_j]
        Vc.append((shaped(i) * shaped(j) * (cond - mu) ** 2).sum(axis=axes))
        Ei = (shaped(i) * f).sum(axis=i, keepdims=True)
        Ej = (shaped(j) * f).sum(axis=j, keepdims=True)
        Eij = (shaped(j) * Ei).sum(axis=j, keepdims=True)
        h = f - Ei - Ej + Eij
        VT2.append((Wfull * h * h).sum(axis=axes))
    return dict(Vc=np.stack(Vc), VT2=np.stack(VT2))


def pack_G(G):
    """the packed G of obhip_sobol2_dev: q x n_G float64, G_ij row-major in pair order"""
    q = G[0].shape[2]
    return np.concatenate([E._f64(g).reshape(-1, q) for g in G], axis=0).T.copy()
