"""Extended-precision reference of the multi-response predictor's Jacobian and vector-Jacobian
product -- the instrument of test_predict_jac_host.py (which proves it) and test_gpu_predict_jac.py
(which uses it).  extended_ref and extended_dx_ref are imported unchanged; the rules are theirs, and
nothing here comes from the code under test.

    jac[i, l, j] = sum_k dB[i, k, l] Theta[k, j]         ExtendedRefDx.ref_grad_mean's rule, column by
                                                          column: C . (bdB @ |Theta|) + gamma_p (|dB| @ |Theta|)
    vjp[i, l]    = sum_j W[i, j] jac[i, l, j]             sum_j |W_ij| tol_ilj + gamma_q sum_j |W_ij jac_ilj|

The VJP's tolerance covers both ways a kernel may contract: over the responses of a finished Jacobian
(every entry within its own tolerance, then q rounded products summed), or through phi = W Theta^T
(the same products in another order).  One getmat_dx per dimension serves all responses.
"""
import numpy as np

import extended_ref as E

ld = np.longdouble


def ref_mean(ref, terms, Theta, C):
    """(B Theta, tolerance), n x q each: E.ref_matmul for every column at once"""
    B, bB = ref.getmat(terms)
    Th = np.asarray(Theta, dtype=ld)
    aT = np.abs(E._f64(Th))
    return B @ Th, E._sum_tol(C, E._f64(bB) @ aT, B.shape[1], np.abs(E._f64(B)) @ aT)


def ref_jac(ref, terms, Theta, C):
    """(jac, tolerance), n x d x q each"""
    Th = np.asarray(Theta, dtype=ld)
    aT = np.abs(E._f64(Th))
    want, tol = [], []
    for l in range(ref.d):
        dB, bdB = ref.getmat_dx(terms, l)
        want.append(dB @ Th)
        tol.append(E._sum_tol(C, E._f64(bdB) @ aT, dB.shape[1], np.abs(E._f64(dB)) @ aT))
    return np.stack(want, axis=1), np.stack(tol, axis=1)


def ref_vjp(jac, tol, W):
    """(vjp, tolerance), n x d each, from ref_jac's (jac, tolerance) and the float64 weights W (n x q)"""
    Wl = np.asarray(W, dtype=ld)[:, None, :]
    prod = Wl * jac
    aW = np.abs(np.asarray(W, dtype=np.float64))[:, None, :]
    q = jac.shape[2]
    return prod.sum(axis=2), (aW * tol).sum(axis=2) + E.gamma(q) * np.abs(E._f64(prod)).sum(axis=2)


def response_scales(q):
    """10^-3 .. 10^3 in a pattern of period 7: every prefix of two or more responses holds both ends,
    and responses 16 apart (the same lane of neighbouring blocks) never share a scale"""
    return 10.0 ** np.array([-3, 3, -1, 1, 0, -2, 2], dtype=np.float64)[np.arange(q) % 7]
