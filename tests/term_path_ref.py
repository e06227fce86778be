"""Extended-precision host restatement of the term-count path (csrc/term_path.cpp, csrc/kernels_term_path.hip;
include/obhip.h, "term-count path"): for the model of the first k terms, at every checkpoint k, the coefficients
theta_k, the log evidence and the row scores (sse, spe, lpd, sumv) in hold-out and leave-one-out form.  The
instrument test_gpu_term_path.py measures k_term_path, k_term_path_fold / _final, k_term_path_coef / _theta, the
stored fixed-order product of the two-operand Gram kernel with its triangular cut, and the host arithmetic of
obhip_posterior_path_evidence with (test_term_path_host.py holds it against direct fits and stages the failures it
must see).

np.longdouble and NumPy only, in the style of posterior_ref.py, whose cholesky_ld, forward_ld, dyadic_hessian,
extended, inside_rows and spread_terms it reuses.  NESTING IS THE CLAIM UNDER TEST, NOT AN INPUT: for a real Hessian
every checkpoint factors H[:k,:k] on its own (cholesky_ld) and substitutes on its own.  For the dyadic Hessian
L[:k,:k] is the exact factor of H[:k,:k] by construction (a leading block of an integer triangle), so one
substitution serves all k there.

Inputs taken as exact: the float64 H, the right-hand sides G (p x q), the responses Y (n x q, standardised) and the
prior precisions; B and its bound bB come from extended_ref.ExtendedRef.

Tolerances follow the project's rule  |got - want| <= C x bound + rest,  bound = what the design matrix's own bound
bB allows, propagated to first order, rest = gamma_k x sum |summands| of every sum on the way, with k the number of
roundings a summand can collect in ANY order of summation.  Per row i and checkpoint k, with W = |inv(L_k)|,
z = inv(L_k) b, u = inv(L_k) G:

  z      bound  W bB_i                                (first-order propagation through the substitution)
         rest   gamma(2k + 4) W |L_k| W |b_i|         (an explicitly formed inverse, |dX| <= gamma_k |inv L| |L|
                                                      |inv L| -- Higham, Accuracy and Stability, section 14.2 --
                                                      and the product's own gamma_k |X| |b| <= gamma_k W |L| W |b|,
                                                      because |L| W >= I entry by entry)
  u      rest   gamma(2k + 4) W |L_k| W |G|           (the same; G is exact, so no bound part)
  mean   sum_t z_t u_t: (bound z) . |u|;  rest (rest z) . |u| + |z| . (rest u) + gamma(k + 2) sum |z_t u_t|
  v      sum_t z_t^2:   2 |z| . (bound z);  rest 2 |z| . (rest z) + gamma(k + 2) v
  real H the float64 factorisation of either side is backward stable, L^ L^^T = H_k + dH with
         |dH| <= gamma(k + 1) |L| |L|^T (theorem 10.3), and a float64 factor of H nests that of H_k, so this holds
         per prefix: mean moves by at most gamma(k + 1) (|L|^T |y|) . (|L|^T |theta|), v by gamma(k + 1)
         || |L|^T |y| ||^2, y = inv(H_k) b (`backward`, as in posterior_ref)
  r = y - mean, then with nu = e^{2 sigma} to first order
     hold-out  s2 = nu + v:  ds2 = dv
     loo       h = v / nu, om = 1 - h, e = r / om, s2 = nu / om:  de = dr / om + |r| dv / (nu om^2),
               ds2 = dv / om^2
     sse_i = r^2: 2 |r| dr;   spe_i = e^2: 2 |e| de;
     lpd_i = -1/2 log(2 pi s2) - 1/2 e^2 / s2:  |e| de / s2 + (1 + e^2 / s2) ds2 / (2 s2)
     each with 8 u of its own magnitude for the handful of operations and libm calls that form it
  sums over the n rows: the parts add, plus gamma(n + 8) sum_i |summand_i| (any tree over n summands).
  The leave-one-out cases keep max h <= 0.9 (asserted), so that 1 / om^2 <= 100 and first order is what matters.
  evidence  -(n/2) log 2 pi - n sigma - 1/2 e^{-2 sigma} yty + 1/2 sum u_t^2 - sum log L_tt + 1/2 sum log prec_t:
            no design matrix in it, so rest only: |u| . (rest u) + gamma(k + 2) 1/2 sum u^2 + (gamma(k) + 2 u)
            (sum |log L_tt| + 1/2 sum |log prec_t|) + 8 u |head|, and for a real H the backward error of the factor,
            gamma(k + 1) / 2 (sum_ab |inv(H_k)|_ab (|L| |L|^T)_ab + || |L|^T |theta| ||^2)

C is never a constant of this module and never measured from the device: path_case measures the float64 LAPACK
route's own max(err / bound) over mean_k and v_k of every row and checkpoint of the case (and of a 130-row probe of
the same model when the case has fewer than 65 rows) and takes extended_ref.constant_from_oracle_ratio of it.
"""
import functools
import math

import numpy as np

import extended_ref as E
import posterior_ref as P
from extended_ref import U, gamma, ld

TILE = 128       # rows of a tile of k_term_path
GROUP = 64       # tiles of a group of the second stage
LOG2PI = np.log(8 * np.arctan(ld(1)))


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def checkpoints(p, step):
    """k_c = min((c + 1) step, p), c < K = ceil(p / step)"""
    K = 1 if step >= p else (p + step - 1) // step
    return [min((c + 1) * step, p) for c in range(K)]


# ---- the factors: one per checkpoint ------------------------------------------------------------------------------
def prefix_factors(H, L, ks, nested):
    """{k: long-double factor of H[:k,:k]}.  nested (the dyadic H): the leading block of the exact L; else every
    prefix is factored on its own"""
    if nested:
        Ll = np.asarray(L, dtype=ld)
        return {k: Ll[:k, :k] for k in ks}
    return {k: P.cholesky_ld(_f64(H)[:k, :k]) for k in ks}


def _row_parts(Lk, Bk, bBk, Gk, backward):
    """per row and response of one checkpoint: z-sums and their (bound, rest) pairs.
    -> mean (n x q), v (n), (bm, rm) (n x q), (bv, rv) (n), u (k x q), ru (k x q), theta (k x q)"""
    k = Lk.shape[0]
    Z = P.forward_ld(Lk, Bk.T)                                   # k x n
    u = P.forward_ld(Lk, Gk)                                     # k x q
    L64 = _f64(Lk)
    W = np.abs(P.inverse64(L64))
    aL = np.abs(L64)
    Zf, uf = np.abs(_f64(Z)), np.abs(_f64(u))
    bz = W @ _f64(bBk).T                                         # k x n
    rz = gamma(2 * k + 4) * (W @ (aL @ (W @ np.abs(_f64(Bk)).T)))
    ru = gamma(2 * k + 4) * (W @ (aL @ (W @ np.abs(_f64(Gk)))))
    mean = Z.T @ u
    v = (Z * Z).sum(axis=0)
    bm = bz.T @ uf
    rm = rz.T @ uf + Zf.T @ ru + gamma(k + 2) * (Zf.T @ uf)
    bv = 2 * np.einsum("ti,ti->i", Zf, bz)
    rv = 2 * np.einsum("ti,ti->i", Zf, rz) + gamma(k + 2) * _f64(v)
    W64 = P.inverse64(L64)
    theta = W64.T @ _f64(u)                                      # (float64: for the backward terms only)
    if backward:
        LY = aL.T @ np.abs(W64.T @ _f64(Z))                      # |L|^T |y_i|, k x n
        LT = aL.T @ np.abs(theta)                                # |L|^T |theta|, k x q
        rm = rm + gamma(k + 1) * (LY.T @ LT)
        rv = rv + gamma(k + 1) * np.sum(LY ** 2, axis=0)
    return mean, v, (bm, rm), (bv, rv), u, ru, theta


def ref_path(H, L, nested, B, bB, G, Y, sigma, step, loo, backward=False):
    """The row scores and sums of every checkpoint in long double.
    -> dict: ks; mean (K, n, q), v (K, n) with their (bound, rest) pairs mean_tol, v_tol; scores (K, q, 3) and
    sumv (K) with scores_tol, sumv_tol = (bound, rest); hmax (the largest leverage, loo only)"""
    E.require_extended()
    n, p = B.shape
    G, Y = np.asarray(G, dtype=ld), np.asarray(Y, dtype=ld)
    q = G.shape[1]
    ks = checkpoints(p, step)
    Ls = prefix_factors(H, L, ks, nested)
    nu = np.exp(2 * ld(sigma))
    nuf = float(nu)
    out = dict(ks=ks, mean=[], v=[], mean_tol=[], v_tol=[], hmax=0.0)
    S = np.zeros((len(ks), q, 3), dtype=ld)
    Sb, Sr = np.zeros((len(ks), q, 3)), np.zeros((len(ks), q, 3))
    V, Vb, Vr = np.zeros(len(ks), dtype=ld), np.zeros(len(ks)), np.zeros(len(ks))
    for c, k in enumerate(ks):
        mean, v, (bm, rm), (bv, rv), _, _, _ = _row_parts(Ls[k], B[:, :k], bB[:, :k], G[:k], backward)
        out["mean"].append(mean), out["v"].append(v), out["mean_tol"].append((bm, rm)), out["v_tol"].append((bv, rv))
        r = Y - mean                                             # n x q
        rf = np.abs(_f64(r))
        if loo:
            om = 1 - v / nu
            omf = _f64(om)
            out["hmax"] = max(out["hmax"], float(np.max(1 - omf)))
            e, s2 = r / om[:, None], nu / om
            de = lambda dm, dv: dm / omf[:, None] + rf * (dv / (nuf * omf ** 2))[:, None]
            ds2 = lambda dv: dv / omf ** 2
        else:
            e, s2 = r, nu + v
            de = lambda dm, dv: dm
            ds2 = lambda dv: dv
        ef, s2f = np.abs(_f64(e)), _f64(s2)
        sse_i, spe_i = r * r, e * e
        lpd_i = -(LOG2PI + np.log(s2))[:, None] / 2 - spe_i / s2[:, None] / 2
        mags = [_f64(sse_i), _f64(spe_i), np.abs(_f64((LOG2PI + np.log(s2)))[:, None] / 2) + _f64(spe_i / s2[:, None]) / 2]
        for which, (dm, dv) in enumerate(((bm, bv), (rm, rv))):
            dsse = 2 * rf * dm
            dspe = 2 * ef * de(dm, dv)
            dlpd = ef * de(dm, dv) / s2f[:, None] + ((1 + _f64(spe_i) / s2f[:, None]) * (ds2(dv) / (2 * s2f))[:, None])
            tgt = Sb if which == 0 else Sr
            for s, d in enumerate((dsse, dspe, dlpd)):
                tgt[c, :, s] = d.sum(axis=0)
        for s, (val, mag) in enumerate(zip((sse_i, spe_i, lpd_i), mags)):
            S[c, :, s] = val.sum(axis=0)
            Sr[c, :, s] += (gamma(n + 8) + 8 * U) * mag.sum(axis=0)
        V[c], Vb[c], Vr[c] = v.sum(), bv.sum(), rv.sum() + gamma(n + 8) * float(v.sum())
    out.update(scores=S, scores_tol=(Sb, Sr), sumv=V, sumv_tol=(Vb, Vr))
    return out


def ref_coef(H, L, nested, G, step, ks_theta=(), backward=False):
    """U = inv(L) G and Theta_k = inv(H_k) G[:k] (zeros behind k) in long double with their rest (no design matrix:
    no bound part).  U row t is taken from the factor of the first checkpoint that holds it (nested: from L).
    -> (U, rest_U, {k: (Theta_k, rest)})"""
    E.require_extended()
    G = np.asarray(G, dtype=ld)
    p, q = G.shape
    Ls = prefix_factors(H, L, sorted(set(list(ks_theta) + [p])), nested)
    u = P.forward_ld(Ls[p], G)
    L64 = _f64(Ls[p])
    W, aL = np.abs(P.inverse64(L64)), np.abs(L64)
    ru = gamma(2 * p + 4) * (W @ (aL @ (W @ np.abs(_f64(G)))))
    if backward:       # u = L^T theta: L moves by the factorisation's backward error, relative gamma(p + 1) per entry
        ru = ru + gamma(p + 1) * (aL.T @ np.abs(P.inverse64(L64).T @ _f64(u))) + gamma(p + 1) * np.abs(_f64(u))
    thetas = {}
    for k in ks_theta:
        Lk = Ls[k]
        uk = P.forward_ld(Lk, G[:k])
        Lk64 = _f64(Lk)
        Wk = P.inverse64(Lk64)
        th = np.zeros((p, q), dtype=ld)
        # back substitution L_k^T theta = u_k
        th[:k] = P.forward_ld(Lk.T[::-1, ::-1], uk[::-1])[::-1]
        rest = np.zeros((p, q))
        aW, aLk = np.abs(Wk), np.abs(Lk64)
        ruk = gamma(2 * k + 4) * (aW @ (aLk @ (aW @ np.abs(_f64(G[:k])))))
        rest[:k] = aW.T @ ruk + gamma(2 * k + 4) * (aW.T @ (aLk.T @ (aW.T @ np.abs(_f64(uk)))))
        if backward:
            Hinv = np.abs(Wk.T @ Wk)
            rest[:k] += gamma(k + 1) * (Hinv @ ((aLk @ aLk.T) @ np.abs(_f64(th[:k]))))
        thetas[k] = (th, rest)
    return u, ru, thetas


def ref_evidence(H, L, nested, G, prec, yty, n_rows, sigma, step, backward=False):
    """(want, rest): log p(y | first k terms) per checkpoint and response (K x q), long double"""
    E.require_extended()
    G = np.asarray(G, dtype=ld)
    p, q = G.shape
    ks = checkpoints(p, step)
    Ls = prefix_factors(H, L, ks, nested)
    prec = np.asarray(prec, dtype=ld)
    s = ld(sigma)
    head = -(ld(n_rows) / 2) * LOG2PI - ld(n_rows) * s - np.exp(-2 * s) * np.asarray(yty, dtype=ld) / 2   # (q)
    headmag = float(n_rows) / 2 * float(LOG2PI) + float(n_rows) * abs(float(sigma)) + math.exp(-2 * sigma) * np.abs(_f64(yty)) / 2
    want, rest = np.zeros((len(ks), q), dtype=ld), np.zeros((len(ks), q))
    for c, k in enumerate(ks):
        Lk = Ls[k]
        u = P.forward_ld(Lk, G[:k])
        L64 = _f64(Lk)
        W64 = P.inverse64(L64)
        W, aL = np.abs(W64), np.abs(L64)
        ru = gamma(2 * k + 4) * (W @ (aL @ (W @ np.abs(_f64(G[:k])))))
        logd, logp = np.log(np.diagonal(Lk)), np.log(prec[:k])
        want[c] = head + (u * u).sum(axis=0) / 2 - logd.sum() + logp.sum() / 2
        uf = np.abs(_f64(u))
        rest[c] = (uf * ru).sum(axis=0) + gamma(k + 2) * _f64((u * u).sum(axis=0)) / 2 \
            + (gamma(k) + 2 * U) * (float(np.abs(logd).sum()) + float(np.abs(logp).sum()) / 2) + 8 * U * headmag
        if backward:
            LLt = aL @ aL.T
            LT = aL.T @ np.abs(W64.T @ _f64(u))
            rest[c] += 0.5 * gamma(k + 1) * (float(np.sum(np.abs(W64.T @ W64) * LLt)) + np.sum(LT ** 2, axis=0))
    return want, rest


def tolerance(C, pair):
    return C * _f64(pair[0]) + _f64(pair[1])


# ---- the float64 host route C is measured from ------------------------------------------------------------------
def host_path64(H, Bo, G, Y, sigma, step, loo):
    """LAPACK Cholesky and triangular solves per checkpoint, NumPy sums, all float64.
    -> dict: mean (K, n, q), v (K, n), scores (K, q, 3), sumv (K)"""
    H, Bo, G, Y = _f64(H), _f64(Bo), _f64(G), _f64(Y)
    n, p = Bo.shape
    nu = math.exp(2.0 * sigma)
    out = dict(mean=[], v=[], scores=[], sumv=[])
    for k in checkpoints(p, step):
        Lk = np.linalg.cholesky(H[:k, :k])
        Z = np.linalg.solve(Lk, Bo[:, :k].T)
        u = np.linalg.solve(Lk, G[:k])
        mean, v = Z.T @ u, (Z * Z).sum(axis=0)
        out["mean"].append(mean), out["v"].append(v)
        out["scores"].append(row_scores64(mean, v, Y, nu, loo).sum(axis=0))
        out["sumv"].append(v.sum())
    return {a: np.array(b) for a, b in out.items()}


def row_scores64(mean, v, Y, nu, loo, h_with_nu=False):
    """(n, q, 3) = (r^2, e^2, lpd) of every row as k_term_path forms them.  h_with_nu: the staged fault h = v nu"""
    r = Y - mean
    if loo:
        om = 1.0 - (v * nu if h_with_nu else v / nu)
        e, s2 = r / om[:, None], nu / om
    else:
        e, s2 = r, nu + v
    lpd = (-0.5 * (math.log(2 * math.pi) + np.log(s2)))[:, None] - 0.5 * (e * e) / s2[:, None]
    return np.stack([r * r, e * e, lpd], axis=2)


def host_evidence64(H, G, prec, yty, n_rows, sigma, step):
    H, G = _f64(H), _f64(G)
    p = H.shape[0]
    out = []
    head = -0.5 * n_rows * math.log(2 * math.pi) - n_rows * sigma - 0.5 * math.exp(-2 * sigma) * _f64(yty)
    for k in checkpoints(p, step):
        Lk = np.linalg.cholesky(H[:k, :k])
        u = np.linalg.solve(Lk, G[:k])
        out.append(head + 0.5 * (u * u).sum(axis=0) - np.log(np.diagonal(Lk)).sum() + 0.5 * np.log(_f64(prec)[:k]).sum())
    return np.array(out)


# ---- the kernel's scheme restated in float64, so that its failures can be staged on the CPU ----------------------
def scheme64(H, Bo, G, Y, sigma, step, loo, fault=None):
    """The device's route in float64: ONE factor of the whole H, Z = B L^-T and U = L^-1 G once, every row walked
    over its columns in ascending order with v and m accumulated, the scores formed at the checkpoint columns,
    rows summed per 128-row tile, tiles in groups of 64 in ascending order, groups in ascending order.
    -> (scores (K, q, 3), sumv (K)).  fault, one of
      ("tile", c, T)   tile T left out of the sums of checkpoint c
      "early"          every checkpoint taken one column early (the last: at p - 1)
      "u_short"        u truncated one short: the mean at checkpoint k misses term k
      "restart"        the running sums restarted at every 128-column tile edge
      "h_nu"           h formed with nu in place of 1 / nu (leave-one-out only)"""
    H, Bo, G, Y = _f64(H), _f64(Bo), _f64(G), _f64(Y)
    n, p = Bo.shape
    q = G.shape[1]
    nu = math.exp(2.0 * sigma)
    Lf = np.linalg.cholesky(H)
    Z = np.linalg.solve(Lf, Bo.T).T                              # n x p
    u = np.linalg.solve(Lf, G)                                   # p x q
    ks = checkpoints(p, step)
    ntiles = (n + TILE - 1) // TILE
    scores, sumv = np.zeros((len(ks), q, 3)), np.zeros(len(ks))
    ZZ, ZU = Z * Z, Z[:, :, None] * u[None, :, :]                # n x p (x q)
    for c, k in enumerate(ks):
        kk = max(1, k - 1) if fault == "early" else k
        lo = (kk - 1) // TILE * TILE if fault == "restart" else 0
        v = ZZ[:, lo:kk].sum(axis=1)
        mean = ZU[:, lo:(kk - 1 if fault == "u_short" else kk)].sum(axis=1)
        rows = row_scores64(mean, v, Y, nu, loo, h_with_nu=fault == "h_nu")
        groups, gv = {}, {}
        for T in range(ntiles):
            if isinstance(fault, tuple) and fault[0] == "tile" and (c, T) == fault[1:]:
                continue
            sl = slice(T * TILE, min(n, (T + 1) * TILE))
            groups[T // GROUP] = groups.get(T // GROUP, 0.0) + rows[sl].sum(axis=0)
            gv[T // GROUP] = gv.get(T // GROUP, 0.0) + v[sl].sum()
        for g in sorted(groups):
            scores[c] += groups[g]
            sumv[c] += gv[g]
    return scores, sumv


# ---- the cases both test files share ---------------------------------------------------------------------------
def rhs_and_responses(H, Bo, q, seed, noise=0.5):
    """G (p x q) and Y (n x q), float64, taken as exact inputs: G = H theta0 for seeded coefficients of unit size
    over all terms, Y = Bo theta0 plus seeded noise, so that every term carries weight in the mean, the residuals
    are of the size of the response and no score cancels to nothing"""
    rng = np.random.default_rng(seed)
    p = H.shape[0]
    theta0 = rng.standard_normal((p, q)) / math.sqrt(p)
    return _f64(H) @ theta0, _f64(Bo) @ theta0 + noise * rng.standard_normal((Bo.shape[0], q))


def path_case(om, terms, H, L, nested, x, G, Y, sigma, step, loo, backward=False, probe_seed=9):
    """reference, tolerances and the float64 host route of one case, and the case's C (module docstring)"""
    import ob_oracle as O
    B, bB = P.extended(om, x).getmat(terms)
    Bo = O.ob_getmat(O.OuterBase(om, x), terms)
    ref = ref_path(H, L, nested, B, bB, G, Y, sigma, step, loo, backward)
    h64 = host_path64(H, Bo, G, Y, sigma, step, loo)
    r = 0.0
    for c in range(len(ref["ks"])):
        r = max(r, E.worst_ratio(h64["mean"][c], ref["mean"][c], ref["mean_tol"][c][0]),
                E.worst_ratio(h64["v"][c], ref["v"][c], ref["v_tol"][c][0]))
    rp = r
    if len(x) < 65:
        xp = P.inside_rows(P.PROBE_ROWS, probe_seed)
        Yp = np.zeros((len(xp), G.shape[1]))
        rp = path_case(om, terms, H, L, nested, xp, G, Yp, sigma, step, loo, backward)["r"]
    C = E.constant_from_oracle_ratio(max(r, rp))
    return dict(x=x, Bo=Bo, ref=ref, h64=h64, r=r, r_probe=rp, C=C,
                tol_scores=tolerance(C, ref["scores_tol"]), tol_sumv=tolerance(C, ref["sumv_tol"]))


def score_ratios(scores, sumv, case):
    """worst |got - want| / tolerance of (sse, spe, lpd, sumv)"""
    ref = case["ref"]
    out = {}
    for s, name in enumerate(("sse", "spe", "lpd")):
        out[name] = E.worst_ratio(scores[:, :, s], ref["scores"][:, :, s], case["tol_scores"][:, :, s])
    out["sumv"] = E.worst_ratio(sumv, ref["sumv"], case["tol_sumv"])
    return out


@functools.lru_cache(maxsize=None)
def short_model():
    return P.oracle_model(P.HYP_SHORT)


@functools.lru_cache(maxsize=None)
def dyadic(p):
    """the dyadic Hessian and the shuffled term set of posterior_ref's cases"""
    om = short_model()
    H, L = P.dyadic_hessian(p, 100 + p)
    return dict(om=om, terms=P.spread_terms(om, p, 5), H=H, L=L)


@functools.lru_cache(maxsize=None)
def hold_case(p, n, step, q=1):
    """hold-out mode on the dyadic Hessian, sigma = 0 (nu = 1): the rows are not rows of any fit"""
    import ob_oracle as O
    c = dyadic(p)
    x = P.inside_rows(n, 9)
    G, Y = rhs_and_responses(c["H"], O.ob_getmat(O.OuterBase(c["om"], x), c["terms"]), q, 1000 + p)
    case = path_case(c["om"], c["terms"], c["H"], c["L"], True, x, G, Y, 0.0, step, False)
    case.update(G=G, Y=Y, sigma=0.0, step=step, loo=False, H=c["H"], terms=c["terms"], p=p, q=q)
    return case


@functools.lru_cache(maxsize=None)
def real(p):
    """test_gpu_posterior.real's recipe: the oracle's total Hessian of a fit on 1500 rows at the default
    hyper-parameters, sigma = log 0.1, and three standardised responses of those rows (the first the fit's own)"""
    import ob_oracle as O
    om = P.oracle_model()
    x, y = O.synth_xy(42, 0, 1500, P.KINDS)
    y = (y - y.mean()) / y.std(ddof=1)
    terms = np.asarray(om.selectterms(p), dtype=np.int64)
    sigma = math.log(0.1)
    ob_ = O.OuterBase(om, x)
    _, H = O.fit_newton(ob_, terms, y, sigma=sigma)
    H = 0.5 * (H + H.T)
    rng = np.random.default_rng(77)
    Y = np.stack([y, y + 0.3 * rng.standard_normal(len(y)), np.sin(3 * y)], axis=1)
    Y[:, 1:] = (Y[:, 1:] - Y[:, 1:].mean(axis=0)) / Y[:, 1:].std(axis=0, ddof=1)
    Bo = O.ob_getmat(ob_, terms)
    G = math.exp(-2 * sigma) * (Bo.T @ Y)
    return dict(om=om, terms=terms, H=H, x=x, Y=Y, G=G, sigma=sigma, rho=O.DEFAULT_RHO)


@functools.lru_cache(maxsize=None)
def loo_case(p, step, q=1):
    """leave-one-out mode on the Hessian formed from 1500 data rows, scored on the first 300 of them"""
    c = real(p)
    x, Y, G = c["x"][:LOO_ROWS], c["Y"][:LOO_ROWS, :q].copy(), c["G"][:, :q].copy()
    case = path_case(c["om"], c["terms"], c["H"], None, False, x, G, Y, c["sigma"], step, True, backward=True)
    case.update(G=G, Y=Y, sigma=c["sigma"], step=step, loo=True, H=c["H"], terms=c["terms"], p=p, q=q)
    return case


# the shapes of test_gpu_term_path.py (the host test holds the float64 route to the same tolerance at every one)
HOLD_P = [(p, 130, 16) for p in (1, 15, 16, 17, 127, 128, 129, 385)]
HOLD_N = [(129, n, 16) for n in (1, 127, 128, 129, 300)]
HOLD_STEP = [(129, 130, s) for s in (1, 7, 129, 1000)]
HOLD_CASES = HOLD_P + HOLD_N + HOLD_STEP
HOLD_Q = (3, 6)                    # at p = 129, n = 130, step 16: one response block and more than one (block = 4)
LOO_CASES = [(64, 16), (385, 64)]  # (p, step) on the first 300 of the 1500 rows of the fit; q in (1, 3)
LOO_ROWS = 300
LOO_Q = (1, 3)
