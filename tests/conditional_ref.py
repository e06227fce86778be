"""Extended-precision reference of the conditional moments of the fitted mean -- the instrument of
test_conditional_host.py (which proves it against a brute-force mean and variance over the tensor grid of the
noise nodes) and of test_gpu_conditional.py (which uses it).  np.longdouble and NumPy only; extended_ref,
extended_dx_ref and sobol_ref are imported unchanged and nothing here comes from the code under test.

With E the noise dimensions, S the others and the tables m_l, C_l, A_l = C_l + m_l m_l^T of sobol_ref:

    P_ik = prod_{l in S} R_{l,t_kl}(x_il)                         (side_products: the factors of ExtendedRefDx)
    M_ij = sum_k theta_kj P_ik mE_k,         mE_k = prod_{l in E} m_l[t_kl]
    W_ij = sum_{k,k'} theta_kj theta_k'j P_ik P_ik' Kp[k,k'],
    Kp[k,k'] = sum_{l in E} (prod_{i in E, i<l} A_i) C_l (prod_{i in E, i>l} m_i m_i)  at [t_kl, t_k'l]

-- the plain double sum over pairs of TERMS, no grouping.  The gradients replace P_ik by dP_ik / dx_l once
(twice the symmetric bilinear form for W).  Tolerances for a float64 result on the same float64 tables
follow the project's rule C . bound + gamma_k . sum |summands| (sobol_ref stage 2, extended_ref):

    M, dM    k = p + d + 4       bound: the first-order bound of P (or dP) carried through the sum
    W, dW    k = p^2 + 3 d + 4   over pairs, |Kp| summed from the magnitudes of its |E| summands
"""
import numpy as np

import extended_ref as E

ld = np.longdouble
CM, CW = 4, 4           # the constants c of gamma_{p+d+c} and gamma_{p^2+3d+c}: those of sobol_ref's V


def control_dims(d, noise):
    return np.setdiff1d(np.arange(d), np.asarray(noise, dtype=np.int64))


def side_products(ref, terms, S, replace=None):
    """(P, bP), n x p each: prod_{l in S} R_{l,t_kl}(x_il) and its first-order bound; replace: the dimension of S
    whose factor is its derivative by the input (ref: an ExtendedRefDx on full-width rows)"""
    terms = np.asarray(terms, dtype=np.int64)
    p = terms.shape[0]
    P0, S0 = np.ones(ref.n, dtype=ld), np.zeros(ref.n, dtype=ld)
    for l in S:
        P0, S0 = ref._times(P0, S0, ref.s[l], ref.bs[l])
    P, B = np.repeat(P0[:, None], p, axis=1), np.repeat(S0[:, None], p, axis=1)
    for l in S:
        if replace is not None and l == replace:
            lev = terms[:, l]
            P, B = ref._times(P, B, ref.g[l][:, lev], ref.bg[l][:, lev])
            continue
        idx = np.nonzero(terms[:, l] > 0)[0]
        if len(idx):
            lev = terms[idx, l]
            P[:, idx], B[:, idx] = ref._times(P[:, idx], B[:, idx], ref.r[l][:, lev], ref.br[l][:, lev])
    return P, B


def pair_tables(terms, noise, m, Cv, dtype=ld):
    """(mE (p), Kp (p x p), aKp (p x p)) on the TERMS: the product of the means, the telescoped bracket and the sum
    of the magnitudes of its summands"""
    terms = np.asarray(terms, dtype=np.int64)
    p = terms.shape[0]
    m = [np.asarray(a, dtype=dtype) for a in m]
    Cv = [np.asarray(a, dtype=dtype) for a in Cv]
    one = np.ones((p, p), dtype=dtype)
    mE = np.ones(p, dtype=dtype)
    a, c, mm = [], [], []
    for l in noise:
        t = terms[:, l]
        mE = mE * m[l][t]
        A = Cv[l] + np.outer(m[l], m[l])
        a.append(A[t[:, None], t[None, :]])
        c.append(Cv[l][t[:, None], t[None, :]])
        mm.append(np.outer(m[l][t], m[l][t]))
    ne = len(noise)
    sm = [one] * (ne + 1)
    for e in range(ne - 1, -1, -1):
        sm[e] = sm[e + 1] * mm[e]
    Kp, aKp, pa = np.zeros((p, p), dtype=dtype), np.zeros((p, p), dtype=dtype), one
    for e in range(ne):
        s = pa * c[e] * sm[e + 1]
        Kp, aKp = Kp + s, aKp + np.abs(s)
        pa = pa * a[e]
    return mE, Kp, aKp


def group_tables(tuples, m, Cv):
    """(mE (G), K (G x G)) and their tolerances for a float64 result, on the groups' level tuples (G x |E|; m, Cv:
    the tables of the noise dimensions alone, in the order of the tuples' columns)"""
    tuples = np.asarray(tuples, dtype=np.int64)
    ne = tuples.shape[1]
    mE, K, aK = pair_tables(tuples, list(range(ne)), m, Cv)
    return mE, K, E.gamma(ne + 1) * E._f64(np.abs(mE)), E.gamma(3 * ne + 4) * E._f64(aK)


def groups_of(terms, noise):
    """(group_of (p), tuples (G x |E|)): groups numbered in the order of their first term"""
    key, gof, tuples = {}, [], []
    for row in np.asarray(terms, dtype=np.int64)[:, list(noise)]:
        k = tuple(int(v) for v in row)
        if k not in key:
            key[k] = len(tuples)
            tuples.append(k)
        gof.append(key[k])
    return np.array(gof, dtype=np.int64), np.array(tuples, dtype=np.int64).reshape(len(tuples), len(noise))


def moments(ref, terms, Theta, noise, m, Cv, C, grad=False):
    """dict(M, W (n x q), tol_M, tol_W and, with grad, dM, dW, tol_dM, tol_dW (n x |S| x q)) in long double with the
    tolerances of a float64 evaluation on the same tables; C: constant_from_oracle_ratio"""
    terms = np.asarray(terms, dtype=np.int64)
    p, d = terms.shape
    S = list(control_dims(d, noise))
    Th = np.asarray(Theta, dtype=ld)
    if Th.ndim == 1:
        Th = Th[:, None]
    aTh = np.abs(E._f64(Th))
    mE, Kp, aKp = pair_tables(terms, list(noise), m, Cv)
    amE, Kf, aKf = np.abs(E._f64(mE)), E._f64(Kp), E._f64(aKp)
    P, bP = side_products(ref, terms, S)
    Pf, bPf = np.abs(E._f64(P)), E._f64(bP)
    gM, gW = E.gamma(p + d + CM), E.gamma(p * p + 3 * d + CW)
    out = {}
    out["M"] = (P * mE[None, :]) @ Th
    out["bnd_M"], out["abs_M"] = (bPf * amE[None, :]) @ aTh, (Pf * amE[None, :]) @ aTh
    out["tol_M"] = C * out["bnd_M"] + gM * out["abs_M"]
    q = Th.shape[1]
    W, tW = [], []
    for j in range(q):
        Z, aZ, bZ = P * Th[None, :, j], Pf * aTh[None, :, j], bPf * aTh[None, :, j]
        W.append(np.sum((Z @ Kp) * Z, axis=1))
        tW.append(C * 2 * np.sum((bZ @ aKf) * aZ, axis=1) + gW * np.sum((aZ @ aKf) * aZ, axis=1))
    out["W"], out["tol_W"] = np.stack(W, axis=1), np.stack(tW, axis=1)
    if grad:
        dM, tdM, dW, tdW = [], [], [], []
        for l in S:
            dP, bdP = side_products(ref, terms, S, replace=l)
            dPf, bdPf = np.abs(E._f64(dP)), E._f64(bdP)
            dM.append((dP * mE[None, :]) @ Th)
            tdM.append(C * ((bdPf * amE[None, :]) @ aTh) + gM * ((dPf * amE[None, :]) @ aTh))
            w, tw = [], []
            for j in range(q):
                Z, aZ, bZ = P * Th[None, :, j], Pf * aTh[None, :, j], bPf * aTh[None, :, j]
                Zd, aZd, bZd = dP * Th[None, :, j], dPf * aTh[None, :, j], bdPf * aTh[None, :, j]
                w.append(2 * np.sum((Zd @ Kp) * Z, axis=1))
                tw.append(2 * (C * (np.sum((bZd @ aKf) * aZ, axis=1) + np.sum((aZd @ aKf) * bZ, axis=1))
                               + gW * np.sum((aZd @ aKf) * aZ, axis=1)))
            dW.append(np.stack(w, axis=1)), tdW.append(np.stack(tw, axis=1))
        out["dM"], out["tol_dM"] = np.stack(dM, axis=1), np.stack(tdM, axis=1)
        out["dW"], out["tol_dW"] = np.stack(dW, axis=1), np.stack(tdW, axis=1)
    out["Kf"] = Kf
    return out


def grouped_moments(P, Theta, terms, noise, m, Cv, twice=None, c_for_a=None, skip_block=None):
    """(M, W) by the grouped form c^T mE and c^T K c in long double, for ONE response column Theta (p); the
    mutants of test_conditional_host.py: twice -- a group whose coefficient counts twice; c_for_a -- a noise
    dimension whose C is replaced by A; skip_block -- a 16-wide block of groups left out of Y = K c"""
    gof, tuples = groups_of(terms, noise)
    G = len(tuples)
    mt = [np.asarray(m[l], dtype=ld) for l in noise]
    Ct = [np.asarray(Cv[l], dtype=ld) for l in noise]
    if c_for_a is not None:
        e = list(noise).index(c_for_a)
        Ct[e] = Ct[e] + np.outer(mt[e], mt[e])
    mE, K, _ = pair_tables(tuples, list(range(len(noise))), mt, Ct)
    sel = (gof[None, :] == np.arange(G)[:, None]).astype(ld)                     # G x p
    c = (P * np.asarray(Theta, dtype=ld)[None, :]) @ sel.T                       # n x G
    if twice is not None:
        c[:, twice] = 2 * c[:, twice]
    Y = c @ K
    if skip_block is not None:
        Y[:, 16 * skip_block:16 * skip_block + 16] = 0
    return c @ mE, np.sum(c * Y, axis=1)
