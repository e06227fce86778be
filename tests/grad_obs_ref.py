"""Host reference of the Newton fit with observed input gradients (include/obhip.h, "observed input
gradients"): the augmented normal equations

    (e^{-2 sigma} (B^T B + sum_l w_l D_l^T D_l) + diag(prec)) theta = e^{-2 sigma} (B^T y~ + sum_l w_l D_l^T g~_l)

formed in float64 from extended_dx_ref.dB_f64_of and in np.longdouble from ExtendedRefDx.getmat_dx, solved in
float64 and refined in long double.  Shared by test_grad_obs_host.py (which proves it) and
test_gpu_grad_obs.py (which holds the device to it)."""
import functools
import math

import numpy as np

import extended_dx_ref as X
import extended_ref as E
from conftest import knots_for, make_pair
from test_predict_grad_host import HYP, KINDS, special_rows

ld = np.longdouble
# sigma: the fit's default.  rho: NOT the default 6.  With two value rows and eight gradient equations for 129
# terms (the last of CPU_CASES) the prior carries the fit, and at rho = 6 its precisions go down to 7e-6 beside
# e^{-2 sigma} = 1e4: cond(H) = 1.5e14, where no float64 factorisation has six digits to offer, the reference's
# own float64 solve included.  At rho = 0 cond(H) is 3.6e5 .. 9.3e8 over the three cases, inside the range
# (5e5 .. 2.4e9) for which the 1.6e-11 of test_grad_obs_host.py and the 1e-6 of the GPU fit were stated.
SIGMA, RHO = math.log(0.01), 0.0
WEIGHTS = np.array([1.0, 0.25, 2.0, 0.5])
CPU_CASES = [(129, 128), (65, 300), (2, 129)]          # (rows, terms): d = 4 mixed kinds, 20 knots


def response(x, q=1):
    """(Y n x q, dY n x d x q): smooth responses on different scales and offsets with their analytic gradients"""
    n, d = x.shape
    Y, dY = np.empty((n, q)), np.empty((n, d, q))
    for j in range(q):
        a = 0.7 + 0.3 * np.arange(d) + 0.2 * j
        ph = 0.4 * j + 0.1 * np.arange(d)
        s, c = np.sin(a * x + ph), np.cos(a * x + ph)
        tot = s.sum(axis=1)
        Y[:, j] = (1.0 + j) * (tot + 0.25 * tot * tot) - 3.0 * j
        dY[:, :, j] = (1.0 + j) * (1 + 0.5 * tot)[:, None] * (a * c)
    return Y, dY


def stacked(ref, terms, dims, weights):
    """the rows the device stages: the blocks sqrt(w_j) dB / dx_dims[j] one under the other, long double, with
    their bounds; sqrt(w_j) is the float64 square root the library takes"""
    sq = np.ones(len(dims)) if weights is None else np.sqrt(np.asarray(weights, dtype=np.float64))
    S, bS = [], []
    for j, l in enumerate(dims):
        D, bD = ref.getmat_dx(terms, int(l))
        S.append(ld(sq[j]) * D)
        bS.append(ld(sq[j]) * bD)
    return np.concatenate(S, axis=0), np.concatenate(bS, axis=0), sq


def stacked_g(dY, sq):
    """sqrt(w_j) g_j under one another as the device forms them (one float64 product per entry): (n L) x q"""
    n, L, q = dY.shape
    return (dY * sq[None, :, None]).transpose(1, 0, 2).reshape(L * n, q)


def normal_equations(B, Y, prec, sigma, S=None, Gs=None, dtype=np.float64):
    """(H, R, cent, sd) in dtype: B n x p the value rows' design matrix, Y n x q raw; S, Gs the stacked gradient
    rows and observations (None: value rows only).  cent and sd (n - 1 denominator) from the value rows."""
    B, Y = np.asarray(B, dtype=dtype), np.asarray(Y, dtype=dtype)
    cent = Y.mean(axis=0)
    sd = np.sqrt(((Y - cent) ** 2).sum(axis=0) / dtype(Y.shape[0] - 1))
    e2 = np.exp(-2 * dtype(sigma))
    G, R = B.T @ B, B.T @ ((Y - cent) / sd)
    if S is not None:
        S = np.asarray(S, dtype=dtype)
        G = G + S.T @ S
        R = R + S.T @ (np.asarray(Gs, dtype=dtype) / sd)
    return e2 * G + np.diag(np.asarray(prec, dtype=dtype)), e2 * R, cent, sd


def solve_refined(H, R, steps=4):
    """(float64 solution, long double solution): LAPACK in float64, then iterative refinement with long double
    residuals of the long double system"""
    H64, Hl, Rl = np.asarray(H, dtype=np.float64), np.asarray(H, dtype=ld), np.asarray(R, dtype=ld)
    t64 = np.linalg.solve(H64, np.asarray(R, dtype=np.float64))
    t = np.asarray(t64, dtype=ld)
    for _ in range(steps):
        t = t + np.asarray(np.linalg.solve(H64, np.asarray(Rl - Hl @ t, dtype=np.float64)), dtype=ld)
    return t64, t


def relerr(got, want):
    """worst column of max |got - want| / max |want|"""
    got, want = np.asarray(got, dtype=ld), np.asarray(want, dtype=ld)
    got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
    return float(max(np.max(np.abs(got[:, j] - want[:, j])) / np.max(np.abs(want[:, j])) for j in range(want.shape[1])))


@functools.lru_cache(maxsize=None)
def pair():
    """(oracle model, device-side model handle) of the d = 4 mixed model on 20 knots"""
    return make_pair(KINDS, knots_for(KINDS, 20), hyp=HYP)


@functools.lru_cache(maxsize=None)
def cpu_case(n, p, q=1):
    """one of CPU_CASES with everything the tests compare against, computed once"""
    import ob_oracle as O
    om_o, _ = pair()
    knots = knots_for(KINDS, 20)
    terms = om_o.selectterms(p)
    x = special_rows(np.random.default_rng(100 + n), n, KINDS, knots)
    Y, dY = response(x, q)
    dims = np.arange(4)
    ref = X.reference_dx_of(om_o, x)
    prec = O.prior_prec(om_o, terms, RHO)
    B64, dB64 = X.dB_f64_of(om_o, x, terms)
    sq = np.sqrt(WEIGHTS)
    S64 = np.concatenate([sq[j] * dB64[:, :, l] for j, l in enumerate(dims)], axis=0)
    Gs = stacked_g(dY, sq)
    Bl, bBl = ref.getmat(terms)
    Sl, bSl, _ = stacked(ref, terms, dims, WEIGHTS)
    H64, R64, _, _ = normal_equations(B64, Y, prec, SIGMA, S64, Gs)
    Hl, Rl, cent, sd = normal_equations(Bl, Y, prec, SIGMA, Sl, Gs, dtype=ld)
    t64, _ = solve_refined(H64, R64)
    _, tl = solve_refined(Hl, Rl)
    return dict(om_o=om_o, terms=terms, x=x, Y=Y, dY=dY, dims=dims, ref=ref, prec=prec, B64=B64, S64=S64, Gs=Gs,
                Bl=Bl, bBl=bBl, Sl=Sl, bSl=bSl, H64=H64, R64=R64, Hl=Hl, Rl=Rl, cent=cent, sd=sd, theta64=t64, theta=tl)
