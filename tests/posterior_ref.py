"""Extended-precision host restatement of the posterior-covariance path (csrc/posterior.cpp): the
variance of predr_std, var_i = || L^-1 b_i ||^2 + e^{2 sigma} with H = L L^T, and the full-Hessian
marginal adjustment.  The instrument test_gpu_posterior.py measures k_trtri_diag / k_trtri_cols, the
two-operand Gram kernel (row norms and stored products), k_transpose, k_dot_cols and the host
arithmetic of obhip_margadj_full with (test_posterior_ref_host.py proves it against 50-digit
arithmetic and shows which failures it can see).

np.longdouble and NumPy only, in the style of extended_ref.py; nothing of the float64 oracle takes
part in the arithmetic.  B, dB / dhyp and their bounds bB, bdB come from extended_ref.ExtendedRef.

Two Hessians:

  dyadic   L = an integer lower triangle / 1024 (strict part |k| <= 32, diagonal 1024 .. 2048),
           H = L L^T by an integer product scaled by 2^-20.  H is exact in float64 and L is its
           EXACT Cholesky factor, so the reference needs no factorisation and no O(p^3) long-double
           work: Z = L^-1 B^T by forward substitution costs O(p^2 n).  cond(H) is about 10.
  real     any float64 H: a long-double Cholesky of it, then the same substitution.  The float64
           factorisation of either side is backward stable, L^ L^^T = H + dH with
           |dH| <= gamma(p + 1) |L| |L|^T in any order of summation (Higham, Accuracy and Stability
           of Numerical Algorithms, theorem 10.3); that moves b^T inv(H) b by y^T dH y, y = inv(H) b,
           at most gamma(p + 1) || |L|^T |y| ||^2, which the bound then carries (`backward`).

Tolerances follow extended_ref's rule, |got - want| <= C x bound + gamma_k x sum |summands|:

  var_i       bound = 2 |z_i|^T |L^-1| bB_i (first-order propagation of bB through the substitution),
              summands z_ik^2 (k = p of them), the noise term with its exponential (2 more) and
              four roundings inside every summand (its factor z_ik twice, each with the division
              by L_kk -- or the rounding of (L^-1)_kk -- and one product; they are all there is at
              p = 1): gamma(p + 6).  The inner sums z_ik = sum_j (L^-1)_kj b_ij and the rounding of
              the rest of an explicitly formed L^-1 get no term of their own: the criterion is
              stricter than a worst-case analysis, and test_posterior_ref_host.py makes it a
              CONDITION that the float64 LAPACK route stays within it on every row of every case.
  traces      tr(inv(H) B^T B) = sum_ik z_ik^2 and tr(inv(H) B^T Bge_l) = sum_ik z_ik g_ik with
              g_i = L^-1 dB_i: bound = sum_i (|g_i|^T |L^-1| bB_i + |z_i|^T |L^-1| bdB_i); the
              n p summands z_ik g_ik are taken as nested sums (rows within terms, or any blocked or
              pairwise scheme) over inner sums of p: gamma(n + 2 p).  Only one strictly sequential
              sum over all n p summands would need gamma(n p).
  diag inv(H) inv(H)_kk = || (L^-1)[:, k] ||^2, p summands; the prior sums sum_k inv(H)_kk prec_k (..)
              another p, prec_k = 1 / (exp(sum_l basisvar) exp(2 rho)) taken good to
              gamma(d) sum |basisvar| + 4 u relative (a float64 sum of d entries, two libm
              exponentials, a product and a division).
  val         -sum_k log L_kk: gamma(p) sum |log L_kk|, 2 u per libm logarithm, and the backward
              error of the factorisation through d log det H = tr(inv(H) dH):
              gamma(p + 1) / 2 sum_ab |inv(H)|_ab (|L| |L|^T)_ab -- on the dyadic H too, whose
              float64 factor need not come out exact from a blocked factorisation.

C is never a constant of this module and never measured from the device: every test measures the
float64 host route's own max(err / bound) on the same case and takes
extended_ref.constant_from_oracle_ratio of it.
"""
import numpy as np

import extended_ref as E
from extended_ref import U, gamma, ld

TB = 64          # block of the triangular inversion (csrc/kernels_trtri.hip)
TILE = 128       # tile of the two-operand Gram kernel


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- the Hessians ------------------------------------------------------------------------------------
def dyadic_hessian(p, seed):
    """(H, L) float64, H = L L^T exactly and L its exact Cholesky factor"""
    E.require_extended()
    rng = np.random.default_rng(seed)
    Li = np.tril(rng.integers(-32, 33, size=(p, p)), -1).astype(np.int64)
    Li[np.arange(p), np.arange(p)] = rng.integers(1024, 2049, size=p)
    Hi = Li @ Li.T
    assert int(np.max(np.abs(Hi))) < 2 ** 53, "the integer H is not exact in float64"
    H, L = Hi.astype(np.float64) * 2.0 ** -20, Li.astype(np.float64) * 2.0 ** -10
    # the scale-back round-trips: nothing was rounded on the way to float64
    assert np.array_equal((H * 2.0 ** 20).astype(np.int64), Hi)
    assert np.array_equal((L * 2.0 ** 10).astype(np.int64), Li)
    assert np.array_equal(H, H.T)
    return H, L


def cholesky_ld(H):
    """long-double Cholesky factor of the float64 H (taken as exact)"""
    E.require_extended()
    A = np.array(H, dtype=ld)
    p = A.shape[0]
    L = np.zeros((p, p), dtype=ld)
    for j in range(p):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        assert v[0] > 0, "H is not positive definite"
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def forward_ld(L, R):
    """inv(L) R by forward substitution, long double; R is p x m"""
    E.require_extended()
    L, R = np.asarray(L, dtype=ld), np.asarray(R, dtype=ld)
    p = L.shape[0]
    assert L.shape == (p, p) and R.shape[0] == p
    Z = np.empty(R.shape, dtype=ld)
    for k in range(p):
        Z[k] = (R[k] - L[k, :k] @ Z[:k]) / L[k, k]
    return Z


def inverse_ld(L):
    """inv(L), long double, the zeros above the diagonal never touched: p^3 / 3"""
    E.require_extended()
    L = np.asarray(L, dtype=ld)
    p = L.shape[0]
    W = np.zeros((p, p), dtype=ld)
    for k in range(p):
        W[k, :k] = -(L[k, :k] @ W[:k, :k]) / L[k, k]
        W[k, k] = 1 / L[k, k]
    return W


def inverse64(L):
    """float64 inv(L) of the lower triangle L (LU of a triangle with a dominant diagonal = the
    triangle: LAPACK does a forward substitution); for bounds and for the float64 host route"""
    L = _f64(L)
    return np.tril(np.linalg.solve(L, np.eye(L.shape[0])))


# ---- the variance -------------------------------------------------------------------------------------
def ref_var(L, B, bB, sigma, backward=False):
    """(want, bound, rest, Z): var_i = || inv(L) b_i ||^2 + e^{2 sigma} at the n rows of the long-double
    B (n x p, bound bB), held to C x bound + rest (tolerance()).  L: the exact factor (float64 dyadic,
    or cholesky_ld's)."""
    n, p = B.shape
    Z = forward_ld(L, B.T)                                       # p x n
    post = (Z * Z).sum(axis=0)
    noise = np.exp(2 * ld(sigma))
    W64, Zf = inverse64(L), np.abs(_f64(Z))
    bound = 2 * np.einsum("ki,ki->i", Zf, np.abs(W64) @ _f64(bB).T)
    rest = gamma(p + 6) * (_f64(post) + float(noise))
    if backward:
        Y = W64.T @ _f64(Z)                                      # inv(H) b_i
        rest = rest + gamma(p + 1) * np.sum((np.abs(_f64(L)).T @ np.abs(Y)) ** 2, axis=0)
    return post + noise, bound, rest, Z


def tolerance(C, bound, rest):
    return C * _f64(bound) + _f64(rest)


def host_var64(H, Bo, sigma):
    """the float64 host route C is measured from: LAPACK Cholesky, triangular solve, row norms"""
    Z = np.linalg.solve(np.linalg.cholesky(_f64(H)), _f64(Bo).T)
    return (Z * Z).sum(axis=0) + np.exp(2.0 * sigma)


def constant_of(got64, want, bound):
    """(C, r): r = the float64 host route's own max(err / bound) on the case, C eight times that, at
    most extended_ref.C_CAP"""
    r = E.worst_ratio(got64, want, bound)
    return E.constant_from_oracle_ratio(r), r


# ---- the marginal adjustment ------------------------------------------------------------------------
def prior_ld(basisvar, knotptst, lbv_gradhyp, gest, hypmatch, terms, rho):
    """(prec, relative bound of a float64 prec, lv) of logpr_gauss: prec_k = 1 / (exp(sum_l basisvar[
    knotptst[l] + t_kl]) exp(2 rho)), lv[k, h] = logbasisvar_gradhyp[gest[h] + t_k,hypmatch[h]] -- model
    data both sides hold in float64, taken as exact"""
    E.require_extended()
    terms = np.asarray(terms, dtype=np.int64)
    d = terms.shape[1]
    bv = np.asarray(basisvar, dtype=ld)[np.asarray(knotptst, dtype=np.int64)[:d][None, :] + terms]
    prec = 1 / (np.exp(bv.sum(axis=1)) * np.exp(2 * ld(rho)))
    rel = gamma(d) * _f64(np.abs(bv).sum(axis=1)) + 4 * U
    lv = np.stack([np.asarray(lbv_gradhyp, dtype=ld)[int(gest[h]) + terms[:, int(hypmatch[h])]]
                   for h in range(len(hypmatch))], axis=1)
    return prec, rel, lv


def ref_margadj(L, B, bB, dB, bdB, sigma, rho, prec, prec_rel, lv, backward=False):
    """obhip_margadj_full written out independently: {name: (want, bound, rest)} for val, gradhyp (nhyp)
    and gradpara (2), each held to C x bound + rest.  dH / dhyp_l = e^{-2 sigma} (B^T Bge_l + Bge_l^T B)
    - diag(lv_l prec), so

        val         = -sum_k log L_kk
        gradhyp[l]  = -e^{-2 sigma} tr(inv(H) B^T Bge_l) + 1/2 sum_k inv(H)_kk prec_k lv_kl
        gradpara[0] = e^{-2 sigma} tr(inv(H) B^T B),   gradpara[1] = sum_k inv(H)_kk prec_k

    with tr(inv(H) B^T Bge_l) = sum_i (L^-1 b_i) . (L^-1 g_l,i): one forward substitution for B and
    one per hyper-parameter (all right-hand sides in one sweep).  dB may be None: val only."""
    n, p = B.shape
    Ll = np.asarray(L, dtype=ld)
    L64, W64 = _f64(L), inverse64(L)
    Hinv64 = W64.T @ W64
    LLt = np.abs(L64) @ np.abs(L64).T
    logd = np.log(np.diagonal(Ll))
    out = {"val": (-logd.sum(), 0.0, gamma(p) * float(np.abs(logd).sum()) + 2 * U * p
                   + 0.5 * gamma(p + 1) * float(np.sum(np.abs(Hinv64) * LLt)))}
    if dB is None:
        return out
    nh = dB.shape[2]
    Zall = forward_ld(Ll, np.concatenate([B.T] + [dB[:, :, h].T for h in range(nh)], axis=1))
    Z, Zg = Zall[:, :n], [Zall[:, (h + 1) * n:(h + 2) * n] for h in range(nh)]
    Zf, aW = np.abs(_f64(Z)), np.abs(W64)
    WbB = aW @ _f64(bB).T
    e2 = np.exp(-2 * ld(sigma))
    e2f = float(e2)
    kq = n + 2 * p

    def trace(G, bG):
        """sum_ik z_ik g_ik for g = inv(L) (the matrix bG bounds)^T, p x n"""
        Gf = np.abs(_f64(G))
        bound = float(np.sum(Gf * WbB) + np.sum(Zf * (aW @ _f64(bG).T)))
        rest = gamma(kq) * float(np.sum(Zf * Gf))
        if backward:       # tr(inv(H) dH inv(H) M) with inv(H) M inv(H) = (inv(H) B^T) (G inv(H))
            rest += gamma(p + 1) * float(np.sum(np.abs((W64.T @ _f64(Z)) @ (W64.T @ _f64(G)).T) * LLt))
        return (Z * G).sum(), bound, rest

    # diag inv(H) and the prior sums
    Wl = inverse_ld(Ll)
    hinv = (Wl * Wl).sum(axis=0)
    thinv = gamma(p) * _f64(hinv)
    if backward:
        aH = np.abs(Hinv64)
        thinv = thinv + gamma(p + 1) * np.sum((aH @ LLt) * aH.T, axis=1)
    precf, hf = _f64(prec), _f64(hinv)

    def prior(w):
        """sum_k inv(H)_kk prec_k w_k and its allowance (no design matrix in it)"""
        wf = np.abs(_f64(w))
        return (hinv * prec * w).sum(), float(np.sum(precf * wf * thinv) + np.sum((gamma(p) + prec_rel) * hf * precf * wf))

    qB, bqB, rqB = trace(Z, bB)
    pr1, tp1 = prior(np.ones(p, dtype=ld))
    gh, bgh, rgh = np.empty(nh, dtype=ld), np.empty(nh), np.empty(nh)
    for h in range(nh):
        q, bq, rq = trace(Zg[h], bdB[:, :, h])
        pr, tp = prior(lv[:, h])
        gh[h], bgh[h] = -e2 * q + pr / 2, e2f * bq
        # e^{-2 sigma} in float64 (libm, 1 u), the products and the final sum: 4 u of the magnitudes
        rgh[h] = e2f * rq + tp / 2 + 4 * U * (e2f * abs(float(q)) + abs(float(pr)) / 2)
    out["gradhyp"] = (gh, bgh, rgh)
    out["gradpara"] = (np.array([e2 * qB, pr1], dtype=ld), np.array([e2f * bqB, 0.0]),
                       np.array([e2f * (rqB + 4 * U * abs(float(qB))), tp1]))
    return out


def margadj_constant(got64, ref):
    """(C, r) of a marginal-adjustment case from the float64 host route's entries that depend on B"""
    r = max(E.worst_ratio(got64["gradhyp"], ref["gradhyp"][0], ref["gradhyp"][1]),
            E.worst_ratio(got64["gradpara"][:1], ref["gradpara"][0][:1], ref["gradpara"][1][:1]))
    return E.constant_from_oracle_ratio(r), r


def host_margadj64(H, Bo, dBo, sigma, rho, prec64, lv64):
    """the float64 host route of the same quantities: LAPACK Cholesky, inv(H) formed, NumPy sums"""
    L = np.linalg.cholesky(_f64(H))
    Hinv = np.linalg.inv(_f64(H))
    e2 = np.exp(-2.0 * sigma)
    Y = Hinv @ Bo.T
    hd = np.diagonal(Hinv)
    gh = np.array([-e2 * np.sum(Y * dBo[:, :, h].T) + 0.5 * np.sum(hd * prec64 * lv64[:, h])
                   for h in range(dBo.shape[2])])
    return {"val": -np.sum(np.log(np.diagonal(L))), "gradhyp": gh,
            "gradpara": np.array([e2 * np.sum(Y * Bo.T), np.sum(hd * prec64)])}


# ---- the blocked inversion, restated so that its failures can be staged on the CPU -------------------
def blocked_inverse64(L, skip=None):
    """float64 W = inv(L) by the recursion the inversion kernels use, in blocks of TB:
    W_jj = inv(L_jj), W_ij = -inv(L_ii) sum_{k = j .. i - 1} L_ik W_kj.  skip(i, j, k) -> True leaves
    block k out of the sum of W_ij (and what is built on W_ij inherits it, as it would on the device)."""
    L = _f64(L)
    p = L.shape[0]
    nb = (p + TB - 1) // TB
    s = [slice(b * TB, min(p, (b + 1) * TB)) for b in range(nb)]
    W = np.zeros((p, p))
    D = [np.linalg.solve(L[s[b], s[b]], np.eye(s[b].stop - s[b].start)) for b in range(nb)]
    for j in range(nb):
        W[s[j], s[j]] = np.tril(D[j])
        for i in range(j + 1, nb):
            T = np.zeros((s[i].stop - s[i].start, s[j].stop - s[j].start))
            for k in range(j, i):
                if skip is None or not skip(i, j, k):
                    T += L[s[i], s[k]] @ W[s[k], s[j]]
            W[s[i], s[j]] = -D[i] @ T
    return W


def var_from_inverse64(W, Bo, sigma, drop_tile=None):
    """row norms of Z = B W^T plus the noise, float64; drop_tile = (I, J) leaves the TILE x TILE tile
    (rows I, terms J) of Z out of the norms"""
    Z2 = (_f64(Bo) @ _f64(W).T) ** 2
    if drop_tile is not None:
        I, J = drop_tile
        Z2[I * TILE:(I + 1) * TILE, J * TILE:(J + 1) * TILE] = 0.0
    return Z2.sum(axis=1) + np.exp(2.0 * sigma)


# ---- the cases both test files share -----------------------------------------------------------------
KINDS = ["mat25", "mat25pow", "mat25ang", "mat25"]      # all three families: 1 + 2 + 2 + 1 hyper-parameters
NKNOTS = 40
# The dyadic cases use short length scales (every scale hyper-parameter at -2, inside its bounds): at the
# default scales a level-2 factor already cancels three digits and a level-5 one six (bR / |R| = 1e3,
# 1e6), so that bB alone would allow 1e-9 of var at p = 1100 and no 1e-12 failure could show.  At -2 every
# level factor is conditioned like the scale factor (bound / |value| = 2 ... 3 up to level 9) and the
# prior variance falls slowly with the level, so that p = 1100 terms of d = 4 all carry weight.
HYP_SHORT = np.array([-2.0, -2.0, 0.0, -2.0, -2.0, -2.0])


def spread_terms(om, p, seed):
    """selectterms(p) in a seeded random order: selectterms sorts by prior variance, and the design
    matrix's weight falls with it -- shuffled, every 64-block of terms carries its share"""
    terms = np.asarray(om.selectterms(p), dtype=np.int64)
    return terms[np.random.default_rng(seed).permutation(p)]


def inside_rows(n, seed, kinds=KINDS):
    """n rows inside the knot range (conftest.sample_x's box)"""
    x = 0.02 + 0.96 * np.random.default_rng(seed).random((n, len(kinds)))
    for j, k in enumerate(kinds):
        if k == "mat25ang":
            x[:, j] *= 6.283185
    return x


def tile_edge_rows(n):
    """the fixed subset of a large case that goes through long double: first and last row of every
    64-row tile"""
    r = sorted(set(list(range(0, n, 64)) + [min(n, a + 64) - 1 for a in range(0, n, 64)]))
    return np.asarray(r, dtype=np.int64)


def oracle_model(hyp=None):
    """the float64 oracle's model of the cases: KINDS on NKNOTS knots"""
    import ob_oracle as O
    om = O.OuterMod()
    om.setcovfs(KINDS)
    if hyp is not None:
        om.hyp_set(np.asarray(hyp, dtype=np.float64))
    om.setknot(O.bench_knots(KINDS, NKNOTS))
    return om


def extended(om, x, grad=False):
    knots = [np.asarray(om.knots_of(k), dtype=np.float64) for k in range(om.d)]
    return E.ExtendedRef(KINDS, knots, om.hyp, om.rotmat, x, om.rotmat_gradhyp if grad else None)


PROBE_ROWS = 130


def var_case(om, terms, H, L, x, sigma, backward=False, probe_seed=9):
    """reference, bound and the float64 host route (v64, its err / bound r) of one variance case, and the
    case's C.  C belongs to the case (model, term set, Hessian), not to a handful of rows -- the maximum of
    err / bound over one row is noise -- so fewer than 65 rows also take the 130-row probe of the case."""
    import ob_oracle as O
    B, bB = extended(om, x).getmat(terms)
    Bo = O.ob_getmat(O.OuterBase(om, x), terms)
    want, bound, rest, Z = ref_var(L, B, bB, sigma, backward)
    v64 = host_var64(H, Bo, sigma)
    r = E.worst_ratio(v64, want, bound)
    rp = r if len(x) >= 65 else var_case(om, terms, H, L, inside_rows(PROBE_ROWS, probe_seed), sigma, backward)["r"]
    return dict(x=x, Bo=Bo, bB=bB, want=want, bound=bound, rest=rest, v64=v64, r=r, r_probe=rp,
                C=E.constant_from_oracle_ratio(max(r, rp)), post=want - np.exp(2 * ld(sigma)))


def var_bound64(L, Bo, bB, sigma):
    """(bound, rest) of ref_var for rows that do not go through long double, from the float64 substitution"""
    p = Bo.shape[1]
    Z = np.linalg.solve(_f64(L), _f64(Bo).T)
    bound = 2 * np.einsum("ki,ki->i", np.abs(Z), np.abs(inverse64(L)) @ _f64(bB).T)
    return bound, gamma(p + 6) * ((Z * Z).sum(axis=0) + np.exp(2.0 * sigma))


def margadj_case(om, terms, H, L, x, sigma, rho, backward=False):
    """reference {name: (want, bound, rest)}, the float64 host route and (C, r) of one marginal-adjustment case"""
    import ob_oracle as O
    ref = extended(om, x, grad=True)
    B, bB = ref.getmat(terms)
    dB, bdB = ref.getmat_gradhyp(terms)
    prec, prel, lv = prior_ld(om.basisvar, om.knotptst, om.logbasisvar_gradhyp, om.gest, om.hypmatch, terms, rho)
    want = ref_margadj(L, B, bB, dB, bdB, sigma, rho, prec, prel, lv, backward)
    bo = O.OuterBase(om, x, dograd=True)
    got64 = host_margadj64(H, O.ob_getmat(bo, terms), O.ob_getmat_gradhyp(bo, terms), sigma, rho,
                           O.prior_prec(om, terms, rho), om.getlvar_gradhyp(terms))
    C, r = margadj_constant(got64, want)
    return dict(x=x, ref=want, got64=got64, C=C, r=r)


def margadj_ratios(got, case):
    """{name: worst |got - want| / (C x bound + rest)}"""
    out = {}
    for name, (want, bound, rest) in case["ref"].items():
        out[name] = E.worst_ratio(np.atleast_1d(got[name]), np.atleast_1d(want),
                                  tolerance(case["C"], np.atleast_1d(bound), np.atleast_1d(rest)))
    return out


# the shapes of test_gpu_posterior.py, each the smallest at which a piece can still go wrong (the host test
# holds the float64 route to the same tolerance at every one of them)
VAR_SIZES = [(p, 130) for p in (1, 63, 64, 65, 128, 129, 320, 321, 385, 641, 1024, 1025, 1100)] + \
            [(385, n) for n in (1, 127, 128, 129)] + [(130, 1100)]
MARGADJ_SIZES = [(64, 200), (129, 130), (385, 257), (700, 300)]
