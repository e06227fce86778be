"""Extended-precision reference of the variance decomposition of the fitted mean -- the instrument of
test_sobol_host.py (which proves it against a brute-force ANOVA) and test_gpu_sobol.py (which uses it).
np.longdouble and NumPy only; extended_ref is imported unchanged and nothing here comes from the code
under test.

The fitted mean is f(x) = sum_k theta_k prod_l psi_{l, t_kl}(x_l), psi_l = ExtendedRef.getbase(l).  Under a
product of discrete measures (nodes z_il, weights w_il >= 0 normalised by their sum per dimension), with
L_l = 1 + the highest level of dimension l:

    m_l[t]    = sum_i w^_i psi_t(z_il)                          C_l = centred second moments (two passes)
    A_l       = C_l + m_l m_l^T
    mu        = sum_k theta_k prod_l m_l[t_kl]
    V1_l      = g_l^T C_l g_l,  g_l[t] = sum_{k: t_kl = t} theta_k prod_{i != l} m_i[t_ki]
    VT_l      = sum_{k,k'} theta_k theta_k' C_l[t,t'] prod_{i != l} A_i[t_ki, t_k'i]
    V         = sum_{k,k'} theta_k theta_k' sum_l (prod_{i<l} A_i) C_l (prod_{i>l} m_i m_i)

Tolerances for a float64 result follow extended_ref's rule C . bound + gamma_k . sum |summands|:

    stage 1   tol_m[t]    = C sum w^ bR_t + gamma_{n+2} sum w^ |R_t|
              tol_C[t,t'] = C sum w^ (bR_t |D_t'| + |D_t| bR_t') + gamma_{n+4} sum w^ |D_t| |D_t'|
                            + tol_m[t] sum w^ |D_t'| + tol_m[t'] sum w^ |D_t|             (D = R - m)
    stage 2   (the same float64 tables on both sides)
              mu    gamma_{p+d+1} sum |theta_k u_k|
              V1_l  gamma_{p+d+2 L_l+4} |g|^T |C_l| |g|,  |g| summed from absolute values
              VT_l  gamma_{p^2+3d+4} sum |theta_k theta_k'| |C_l| prod |A_i|;  V: the telescoped analogue
"""
import numpy as np

import extended_ref as E

ld = np.longdouble


def levels_of(terms):
    return np.asarray(terms, dtype=np.int64).max(axis=0) + 1


def normalised_weights(weights, n, d, dtype=ld):
    """w^ (n x d): the weights of every dimension divided by their sum; None: 1 / n"""
    if weights is None:
        return np.full((n, d), 1.0, dtype=dtype) / dtype(n)
    w = np.asarray(weights, dtype=dtype)
    return w / w.sum(axis=0)[None, :]


# ---- stage 1: the tables ---------------------------------------------------------------------------
def tables_from_bases(bases, levels, weights, dtype=ld):
    """(m, Cv): lists per dimension, from the raw 1-D bases `bases[l]` (n x >= L_l) in `dtype`"""
    n, d = bases[0].shape[0], len(bases)
    wn = normalised_weights(weights, n, d, dtype)
    m, Cv = [], []
    for l in range(d):
        R = np.asarray(bases[l][:, :levels[l]], dtype=dtype)
        ml = wn[:, l] @ R
        D = R - ml[None, :]
        m.append(ml)
        Cv.append((D * wn[:, l][:, None]).T @ D)
    return m, Cv


def ref_tables(ref, levels, weights, C):
    """((m, Cv), (tol_m, tol_C)) of an ExtendedRef built on the nodes; C: constant_from_oracle_ratio"""
    n, d = ref.n, ref.d
    wn = normalised_weights(weights, n, d)
    m, Cv = tables_from_bases([ref.getbase(l)[0] for l in range(d)], levels, weights)
    tol_m, tol_C = [], []
    for l in range(d):
        R, bR = (a[:, :levels[l]] for a in ref.getbase(l))
        w = E._f64(wn[:, l])
        aR, bRf, aD = np.abs(E._f64(R)), E._f64(bR), np.abs(E._f64(R - m[l][None, :]))
        tm = C * (w @ bRf) + E.gamma(n + 2) * (w @ aR)
        wD = w @ aD
        cross = (bRf * w[:, None]).T @ aD
        tc = (C * (cross + cross.T) + E.gamma(n + 4) * ((aD * w[:, None]).T @ aD)
              + tm[:, None] * wD[None, :] + wD[:, None] * tm[None, :])
        tol_m.append(tm), tol_C.append(tc)
    return (m, Cv), (tol_m, tol_C)


def oracle_getbase_ratio(ref, om_o, x, levels):
    """max(err / bound) of the float64 oracle's getbase on the nodes x: what constant_from_oracle_ratio is given"""
    import ob_oracle as O
    b = O.OuterBase(om_o, x)
    return max(E.worst_ratio(b.getbase(l + 1)[:, :levels[l]], *(a[:, :levels[l]] for a in ref.getbase(l)))
               for l in range(ref.d))


class RowSlice:
    """the first n rows of an ExtendedRef, as far as ref_tables reads one"""

    def __init__(self, ref, n):
        self.ref, self.n, self.d = ref, n, ref.d

    def getbase(self, l):
        R, bR = self.ref.getbase(l)
        return R[:self.n], bR[:self.n]


# ---- stage 2: the formulas on given tables ------------------------------------------------------------
def tile_weights(p, tile, diag=1.0, off=2.0):
    """p x p weights of a sum over the upper triangle of pairs of `tile`-wide term tiles"""
    I = np.arange(p) // tile
    return np.where(I[:, None] == I[None, :], diag, np.where(I[:, None] < I[None, :], off, 0.0))


def formulas(terms, Theta, m, Cv, dtype=ld, pair_weights=None):
    """dict(mu (q), V (q), V1 (d x q), VT (d x q), g (list of L_l x q)) in `dtype`, and with dtype = long double
    the tolerances tol_mu, tol_V, tol_V1, tol_VT (and tol_g: gamma_{p+d+1} |g|) of a float64 evaluation on the
    same tables.
    pair_weights (p x p): the weight every pair (k, k') enters VT and V with -- None: 1 (the full double sum)."""
    terms = np.asarray(terms, dtype=np.int64)
    p, d = terms.shape
    Th = np.asarray(Theta, dtype=dtype)
    if Th.ndim == 1:
        Th = Th[:, None]
    aTh = np.abs(Th)
    m = [np.asarray(a, dtype=dtype) for a in m]
    Cv = [np.asarray(a, dtype=dtype) for a in Cv]
    L = [len(a) for a in m]
    # mu and the first-order part
    mk = [m[l][terms[:, l]] for l in range(d)]                       # p each
    pre, suf = [np.ones(p, dtype=dtype)], [np.ones(p, dtype=dtype)]
    for l in range(d):
        pre.append(pre[-1] * mk[l])
        suf.append(suf[-1] * mk[d - 1 - l])
    u = pre[d]
    out = dict(mu=Th.T @ u, tol_mu=E.gamma(p + d + 1) * E._f64(aTh.T @ np.abs(u)))
    V1, tV1, g, tg = [], [], [], []
    for l in range(d):
        excl = pre[l] * suf[d - 1 - l]
        sel = (terms[:, l][None, :] == np.arange(L[l])[:, None]).astype(dtype)      # L x p
        gl, agl = sel @ (Th * excl[:, None]), sel @ (aTh * np.abs(excl)[:, None])   # L x q
        g.append(gl), tg.append(E.gamma(p + d + 1) * E._f64(agl))
        V1.append(np.einsum("tj,tu,uj->j", gl, Cv[l], gl))
        tV1.append(E.gamma(p + d + 2 * L[l] + 4) * E._f64(np.einsum("tj,tu,uj->j", agl, np.abs(Cv[l]), agl)))
    out.update(V1=np.stack(V1), tol_V1=np.stack(tV1), g=g, tol_g=tg)
    # the pair sums
    a, c, mm = [], [], []
    for l in range(d):
        t = terms[:, l]
        A = Cv[l] + np.outer(m[l], m[l])
        a.append(A[t[:, None], t[None, :]])
        c.append(Cv[l][t[:, None], t[None, :]])
        mm.append(np.outer(mk[l], mk[l]))
    one = np.ones((p, p), dtype=dtype)
    sa, sm = [one] * (d + 1), [one] * (d + 1)                          # products over i >= l
    for l in range(d - 1, -1, -1):
        sa[l], sm[l] = sa[l + 1] * a[l], sm[l + 1] * mm[l]
    W = one if pair_weights is None else np.asarray(pair_weights, dtype=dtype)

    def quad(F):
        return np.einsum("kj,kl,lj->j", Th, F * W, Th), np.einsum("kj,kl,lj->j", aTh, np.abs(F) * W, aTh)
    VT, tVT = [], []
    Vm, aVm, pa = np.zeros((p, p), dtype=dtype), np.zeros((p, p), dtype=dtype), one
    gq = E.gamma(p * p + 3 * d + 4)
    for l in range(d):
        pc = pa * c[l]
        v, av = quad(pc * sa[l + 1])
        VT.append(v), tVT.append(gq * E._f64(av))
        Vm, aVm = Vm + pc * sm[l + 1], aVm + np.abs(pc * sm[l + 1])
        pa = pa * a[l]
    out.update(VT=np.stack(VT), tol_VT=np.stack(tVT))
    out["V"] = np.einsum("kj,kl,lj->j", Th, Vm * W, Th)
    out["tol_V"] = gq * E._f64(np.einsum("kj,kl,lj->j", aTh, aVm * W, aTh))
    return out


# ---- brute force: ANOVA over the full tensor grid of nodes ----------------------------------------------
def grid_rows(nodes):
    """the n^d rows of the tensor grid of nodes (n x d), first dimension slowest"""
    n, d = nodes.shape
    idx = np.stack(np.meshgrid(*[np.arange(n)] * d, indexing="ij"), axis=-1).reshape(-1, d)
    return nodes[idx, np.arange(d)[None, :]], idx


def brute_force(ref_grid, idx, n, terms, Theta, weights):
    """dict(mu, V, V1, VT) from f on the whole grid (ref_grid: ExtendedRef on grid_rows(nodes)): conditional
    means by summing axes, every variance centred.  Independent of the pair formulas."""
    d = ref_grid.d
    Th = np.asarray(Theta, dtype=ld)
    if Th.ndim == 1:
        Th = Th[:, None]
    q = Th.shape[1]
    B, _ = ref_grid.getmat(terms)
    f = (B @ Th).reshape((n,) * d + (q,))
    wn = normalised_weights(weights, n, d)

    def shaped(l):
        return wn[:, l].reshape((1,) * l + (n,) + (1,) * (d - l))
    Wfull = np.ones((1,) * (d + 1), dtype=ld)
    for l in range(d):
        Wfull = Wfull * shaped(l)
    axes = tuple(range(d))
    mu = (Wfull * f).sum(axis=axes)
    V = (Wfull * (f - mu) ** 2).sum(axis=axes)
    V1, VT = [], []
    for l in range(d):
        others = tuple(i for i in range(d) if i != l)
        Wo = np.ones((1,) * (d + 1), dtype=ld)
        for i in others:
            Wo = Wo * shaped(i)
        cond = (Wo * f).sum(axis=others, keepdims=True)                  # E[f | x_l]
        V1.append((shaped(l) * (cond - mu) ** 2).sum(axis=axes))
        inner = (shaped(l) * f).sum(axis=l, keepdims=True)               # E[f | x_~l]
        VT.append((Wfull * (f - inner) ** 2).sum(axis=axes))             # E Var(f | x_~l) = V - Var E[f | x_~l]
    return dict(mu=mu, V=V, V1=np.stack(V1), VT=np.stack(VT))


# ---- random tables (any float64 tables are inputs of the pair kernel) -------------------------------------
def random_tables(rng, levels):
    """(m, Cv) float64: m_l[0] near 1, the others small; C_l symmetric positive semi-definite"""
    m, Cv = [], []
    for L in levels:
        ml = 0.3 * rng.standard_normal(L)
        ml[0] = 1.0 + 0.1 * rng.standard_normal()
        X = rng.standard_normal((L, L + 2)) * (0.5 ** np.arange(L))[:, None]
        G = 0.2 * (X @ X.T) / (L + 2)
        m.append(ml), Cv.append(0.5 * (G + G.T))
    return m, Cv


def pack_tables(m, Cv):
    return (np.concatenate([np.asarray(a, dtype=np.float64) for a in m]),
            np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in Cv]))


def unpack_tables(pm, pc, levels):
    om_ = np.concatenate([[0], np.cumsum(levels)])
    oc_ = np.concatenate([[0], np.cumsum(np.asarray(levels) ** 2)])
    return ([pm[om_[l]:om_[l + 1]] for l in range(len(levels))],
            [pc[oc_[l]:oc_[l + 1]].reshape(levels[l], levels[l]) for l in range(len(levels))])
