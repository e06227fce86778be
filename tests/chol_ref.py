"""Host reference of the dense SPD solve (csrc/kernels_chol.hip, launch_newton_solve): the instrument
test_gpu_chol.py holds the device's factor L^ and solution theta^ to, per entry
(test_chol_ref_host.py proves it against 50-digit arithmetic and shows which failures it can see).

NumPy and np.longdouble only, in the style of posterior_ref.py.  Two cases:

  exact    posterior_ref.dyadic_hessian's construction: L0 = an integer lower triangle / 1024 (strict
           part |k| <= 32, diagonal 1024 .. 2048), H = L0 L0^T by a float64 BLAS product of the integer
           matrices (every partial sum is an integer below 2^53 in any order, so the product is exact;
           the int64 product of NumPy takes 50 s at p = 3200, this one half a second).  L0 is the EXACT
           factor: no factorisation is needed, and L^ is compared with L0 entry by entry against the
           first-order perturbation bound of the factor under the backward error of Higham, Accuracy
           and Stability of Numerical Algorithms, theorem 10.3 (L^ L^^T = H + dH,
           |dH| <= gamma(p + 1) |L^| |L^|^T in any order of summation):

               dL = L0 Phi(L0^-1 dH L0^-T)          Phi = lower triangle, diagonal halved
               |L^ - L0| <= C gamma(p + 1) |L0| Phi(|L0^-1| (|L0| |L0|^T) |L0^-T|)

  real     a float64 Hessian e^{-2 sigma} B^T B + diag(prec) of the oracle's design matrix B
           (posterior_ref.KINDS at the default length scales, sigma = log 0.01).  No reference factor:
           L^ is held to the componentwise backward error of the same theorem,
           |L^ L^^T - H| <= C gamma(p + 1) (|L^| |L^|^T), the left side formed in long double.

  solution (both cases, every size, every column of the batched solve)
           |H theta^ - r| <= C_s gamma(3 p + 1) |L^| (|L^|^T |theta^|)  (theorem 10.4), in long double.

C and C_s are no constants of this module and are never measured from the device: eight times
(extended_ref's margin) the larger err / bound of two float64 host routes on the same matrix --
np.linalg.cholesky with a dot-product substitution, and blocked_cholesky64 / blocked_solve64, a NumPy
restatement of the device's scheme (right-looking, 64-column panels, the panel solve a product with
explicitly inverted 16 x 16 diagonal sub-blocks, the substitutions with the same inverses) -- capped at
1, the theorems' own constant.  The device sums in another order and rounds its pivots' reciprocals
differently; it shares no arithmetic with either route.
"""
import functools
import math

import numpy as np

import extended_ref as E
from extended_ref import gamma, ld

NB = 64       # panel width of the factorisation
SB = 16       # explicitly inverted diagonal sub-blocks
C_CAP = 1.0   # the theorems' own constant


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def constant_from_ratio(ratio):
    """eight times the float64 routes' own max(err / bound), at most the theorem's constant"""
    return min(8.0 * float(ratio), C_CAP)


# ---- the exact case ------------------------------------------------------------------------------------
def dyadic_hessian(p, seed):
    """(H, L0) float64, H = L0 L0^T exactly and L0 its exact Cholesky factor: the draws of
    posterior_ref.dyadic_hessian, the integer product by float64 BLAS"""
    E.require_extended()
    rng = np.random.default_rng(seed)
    Li = np.tril(rng.integers(-32, 33, size=(p, p)), -1).astype(np.float64)
    Li[np.arange(p), np.arange(p)] = rng.integers(1024, 2049, size=p)
    Hi = Li @ Li.T
    # sum_k |l_ik| |l_jk| <= max_i sum_k l_ik^2 (Cauchy-Schwarz): every partial sum of every entry, in any
    # order and under fused multiply-adds, is an integer below 2^53 and therefore exact
    assert float(np.max(np.diagonal(Hi))) < 2.0 ** 53, "the integer H is not exact in float64"
    assert np.array_equal(Hi, np.round(Hi)) and np.array_equal(Hi, Hi.T)
    return Hi * 2.0 ** -20, Li * 2.0 ** -10


def inverse64(L):
    """float64 inv(L) of a lower triangle (for bounds)"""
    L = _f64(L)
    return np.tril(np.linalg.solve(L, np.eye(L.shape[0])))


def factor_bound(L0, W=None):
    """gamma(p + 1) |L0| Phi(|L0^-1| (|L0| |L0|^T) |L0^-T|), lower triangle: the first-order bound of
    |L^ - L0| under theorem 10.3's backward error (W: inverse64(L0) if the caller has it)"""
    aL = np.abs(_f64(L0))
    p = aL.shape[0]
    W = np.abs(inverse64(L0) if W is None else W)
    S = W @ (aL @ aL.T) @ W.T
    Phi = np.tril(S)
    Phi[np.arange(p), np.arange(p)] *= 0.5
    return gamma(p + 1) * np.tril(aL @ Phi)


def cond_spd(L0, W, iters=100):
    """cond_2(L0 L0^T) by power iteration on H and on inv(H) = W^T W, W = inv(L0): O(p^2) per step, good
    to a few per cent (it is only reported)"""
    v = np.random.default_rng(1).standard_normal(L0.shape[0])
    u = v.copy()
    for _ in range(iters):
        v = L0 @ (L0.T @ v)
        hi = float(np.linalg.norm(v))
        v /= hi
        u = W.T @ (W @ u)
        lo = float(np.linalg.norm(u))
        u /= lo
    return hi * lo


def factor_ratio_exact(Lhat, L0, bound):
    """worst |L^ - L0| / bound over the lower triangle (the strict upper triangle of the device's H is
    scratch and not looked at)"""
    err = np.abs(np.tril(_f64(Lhat)) - L0)
    return _worst(err, bound)


def _worst(err, den):
    """max err / den; inf where something is wrong at a zero denominator; nan if err is not finite"""
    if err.size == 0:
        return 0.0
    if not np.all(np.isfinite(err)):
        return float("nan")
    out = np.zeros(err.shape)
    np.divide(err, den, out=out, where=den > 0)
    out[(den <= 0) & (err > 0)] = np.inf
    return float(out.max())


# ---- the real case -------------------------------------------------------------------------------------
REAL_SIGMA = math.log(0.01)
REAL_RHO = 6.0
REAL_ROWS = 1500


@functools.lru_cache(maxsize=None)
def real_parts(p):
    """the oracle's pieces of the real case: terms, G = e^{-2 sigma} B^T B (symmetric float64, scaled on the
    host so that the device is called with sigma = 0), the right-hand side e^{-2 sigma} B^T y and the
    float64 prior precision diag(prec) the host test adds (the device test takes the diagonal the device
    formed instead)"""
    import ob_oracle as O
    import posterior_ref as P
    om = P.oracle_model()
    x, y = O.synth_xy(42, 0, REAL_ROWS, P.KINDS)
    y = (y - y.mean()) / y.std(ddof=1)
    terms = np.asarray(om.selectterms(p), dtype=np.int64)
    B = O.ob_getmat(O.OuterBase(om, x), terms)
    e2 = math.exp(-2.0 * REAL_SIGMA)
    G = e2 * (B.T @ B)
    G = 0.5 * (G + G.T)
    return dict(terms=terms, G=G, r=e2 * (B.T @ y), prec=_f64(O.prior_prec(om, terms, REAL_RHO)))


def real_hessian(G, diag):
    """G with its diagonal replaced by the one that was factorised"""
    H = np.array(G, dtype=np.float64)
    H[np.diag_indices(H.shape[0])] = diag
    return H


def factor_residual_ratio(Lhat, H):
    """worst |L^ L^^T - H| / (gamma(p + 1) |L^| |L^|^T) over the lower triangle, the residual in long
    double (p^3 long-double operations: 2 s at p = 705)"""
    E.require_extended()
    L = np.tril(_f64(Lhat))
    p = L.shape[0]
    if not np.all(np.isfinite(L)):
        return float("nan")
    Ll = np.asarray(L, dtype=ld)
    res = np.tril(_f64(np.abs(Ll @ Ll.T - np.asarray(H, dtype=ld))))
    aL = np.abs(L)
    return _worst(res, gamma(p + 1) * np.tril(aL @ aL.T))


# ---- the solution ----------------------------------------------------------------------------------------
def solve_residual(H, theta, r):
    """|H theta - r| in long double, by row blocks (O(p^2))"""
    E.require_extended()
    p = H.shape[0]
    tl, rl = np.asarray(theta, dtype=ld), np.asarray(r, dtype=ld)
    out = np.empty(p)
    for a in range(0, p, 512):
        out[a:a + 512] = _f64(np.abs(np.asarray(H[a:a + 512], dtype=ld) @ tl - rl[a:a + 512]))
    return out


def solve_bound(Lhat, theta):
    """gamma(3 p + 1) |L^| (|L^|^T |theta^|)"""
    aL = np.abs(np.tril(_f64(Lhat)))
    return gamma(3 * aL.shape[0] + 1) * (aL @ (aL.T @ np.abs(_f64(theta))))


def solve_ratio(H, r, Lhat, theta):
    """worst |H theta^ - r| / (gamma(3 p + 1) |L^| |L^|^T |theta^|) with the side's OWN factor and solution"""
    theta = _f64(theta)
    if not (np.all(np.isfinite(theta)) and np.all(np.isfinite(np.tril(_f64(Lhat))))):
        return float("nan")
    return _worst(solve_residual(H, theta, r), solve_bound(Lhat, theta))


# ---- the two float64 host routes -----------------------------------------------------------------------
def substitute64(L, r):
    """theta = L^-T (L^-1 r), float64, dot-product form (row-oriented forward, column-oriented backward)"""
    L, z = _f64(L), np.array(r, dtype=np.float64)
    p = L.shape[0]
    for k in range(p):
        z[k] = (z[k] - L[k, :k] @ z[:k]) / L[k, k]
    for k in range(p - 1, -1, -1):
        z[k] = (z[k] - L[k + 1:, k] @ z[k + 1:]) / L[k, k]
    return z


def lapack_route(H, r):
    L = np.linalg.cholesky(_f64(H))
    return L, substitute64(L, r)


def _potrf16(D):
    """unblocked right-looking float64 Cholesky of a block of at most 16 columns"""
    D = np.array(D, dtype=np.float64)
    m = D.shape[0]
    for k in range(m):
        D[k, k] = math.sqrt(D[k, k]) if D[k, k] > 0 else float("nan")
        D[k + 1:, k] /= D[k, k]
        D[k + 1:, k + 1:] -= np.outer(D[k + 1:, k], D[k + 1:, k])
    return np.tril(D)


def blocked_cholesky64(H, hook=None):
    """(L, inv): the float64 factor by the device's scheme -- right-looking over 64-column panels; inside
    a panel the 16-column sub-blocks in turn: L_bb unblocked, inv(L_bb) formed explicitly, every row below
    solved as X_b = (A_b - sum_{c < b} X_c L_bc^T) inv(L_bb)^T, a PRODUCT with the inverse; then the
    trailing matrix A22 -= X X^T.  inv: the inverses of the 16 x 16 diagonal sub-blocks, one per 16 columns
    (the last one ragged).  hook(j0, A, X) runs after panel j0's trailing update (X: the solved rows
    j0 + 64 .. p of the panel) and may undo part of it: that is how the failures are staged."""
    A = np.array(H, dtype=np.float64)
    p = A.shape[0]
    inv = []
    for j0 in range(0, p, NB):
        j1 = min(p, j0 + NB)
        for b0 in range(j0, j1, SB):
            b1 = min(j1, b0 + SB)
            Lbb = _potrf16(A[b0:b1, b0:b1])
            ok = np.all(np.isfinite(Lbb))
            Ib = np.tril(np.linalg.solve(Lbb, np.eye(b1 - b0))) if ok else np.full_like(Lbb, np.nan)
            inv.append(Ib)
            A[b0:b1, b0:b1] = Lbb
            if b1 < p:
                X = A[b1:, b0:b1] @ Ib.T
                A[b1:, b0:b1] = X
                # inside the panel: the columns to the right, all rows below; the rest waits for the panel
                if b1 < j1:
                    A[b1:, b1:j1] -= X @ X[:j1 - b1].T
        if j1 < p:
            X = A[j1:, j0:j1]
            A[j1:, j1:] -= X @ X.T
            if hook is not None:
                hook(j0, A, X)
    return np.tril(A), inv


def blocked_solve64(L, inv, r, swap=None):
    """theta by the device's substitutions: forward with the right-hand side carried through the panel solve
    (z_b = inv(L_bb) (r_b - sum_{c < b} L_bc z_c)), backward theta_b = inv(L_bb)^T z_b,
    z[0:b) -= L[b, 0:b)^T theta_b.  swap = (b, b2): the backward step of sub-block b takes sub-block b2's
    inverse (a staged failure)."""
    L, z = _f64(L), np.array(r, dtype=np.float64)
    p = L.shape[0]
    nb = len(inv)
    for b in range(nb):
        b0, b1 = b * SB, min(p, (b + 1) * SB)
        z[b0:b1] = inv[b] @ z[b0:b1]
        z[b1:] -= L[b1:, b0:b1] @ z[b0:b1]
    for b in range(nb - 1, -1, -1):
        b0, b1 = b * SB, min(p, (b + 1) * SB)
        Ib = inv[b] if swap is None or swap[0] != b else inv[swap[1]]
        z[b0:b1] = Ib.T @ z[b0:b1]
        z[:b0] -= L[b0:b1, :b0].T @ z[b0:b1]
    return z


def blocked_route(H, r):
    L, inv = blocked_cholesky64(H)
    return L, blocked_solve64(L, inv, r)


# ---- the launch loop of launch_newton_solve, restated --------------------------------------------------
def panels_at(p, m, forced=0, m8=8192, m4=4096):
    """chol_panels_at: panels of the pass that starts with m rows left"""
    if forced:
        return forced
    if p < 3072:
        return 1
    return 8 if m >= m8 else (4 if m >= m4 else 2)


def launch_plan(p, forced=0, m8=8192, m4=4096):
    """[(first panel column, panels taken, [(t0, rows m = p - t0, strip)])] per pass: the update launches of
    launch_newton_solve in order"""
    plan = []
    j0, done = 0, False
    while not done and j0 < p:
        npan = panels_at(p, p - j0, forced, m8, m4)
        ups, taken = [], 0
        for i in range(npan):
            jp = j0 + i * NB
            taken += 1
            if p - (jp + NB) <= 0:
                done = True
                break
            ups.append((jp + NB, p - (jp + NB), i + 1 < npan))
        plan.append((j0, taken, ups))
        j0 += npan * NB
    return plan


# ---- the cases both test files share -------------------------------------------------------------------
SCHEDULE_SIZES = [64, 65, 129, 200, 257, 449, 513, 640, 1000, 1217]
# With OBHIP_CHOL_T64=0 every update runs on 128 x 128 tiles.  Rows left (m = p - t0) when an update of the
# 128-tile kernel starts, per panels per pass (pass width w = 64 x panels; the last trailing update of a run
# starts at the last multiple of w below p):
#   2 panels (w = 128): 129 -> m = 1, 255 -> 127, 256 -> 128; a trailing update never has more than w rows
#                       left after the last pass, so 129 rows come from the strip at t0 = 192 of p = 321
#   4 panels (w = 256): 257 -> 1, 383 -> 127, 384 -> 128, 385 -> 129
#   8 panels (w = 512): 513 -> 1, 639 -> 127, 640 -> 128, 641 -> 129
# (129, 257, 513 and 640 are schedule sizes already.)
RAGGED_SIZES = {2: [255, 256, 321], 4: [383, 384, 385], 8: [639, 641]}
BY_ROWS_LEFT = dict(OBHIP_CHOL_M8="2048", OBHIP_CHOL_M4="1024")

# name -> (environment, exact sizes, real sizes, batched solves (case, p, q), not-positive-definite columns at
# p = 700, seconds allowed to the child process)
ENVIRONMENTS = {"default": ({}, [1, 63, 64, 65, 129, 449, 1217, 4160], [257, 705], [], [], 120)}
for _n in (2, 4, 8):
    ENVIRONMENTS["panels%d" % _n] = (dict(OBHIP_CHOL_PANELS=str(_n)), SCHEDULE_SIZES, [705] if _n == 8 else [], [],
                                     [5, 200, 699] if _n == 8 else [], 60)
    ENVIRONMENTS["panels%d_t128" % _n] = (dict(OBHIP_CHOL_PANELS=str(_n), OBHIP_CHOL_T64="0"),
                                          sorted(SCHEDULE_SIZES + RAGGED_SIZES[_n]), [705] if _n == 8 else [],
                                          [("exact", 1217, 3)] if _n == 8 else [], [], 60)
ENVIRONMENTS["t128"] = (dict(OBHIP_CHOL_T64="0"), [], [], [], [5, 200, 699], 60)
ENVIRONMENTS["by_rows_left"] = (dict(BY_ROWS_LEFT), [3072, 3137], [], [("exact", 3137, 3)], [], 120)
ENVIRONMENTS["by_rows_left_t128"] = (dict(BY_ROWS_LEFT, OBHIP_CHOL_T64="0"), [3137], [], [], [], 90)
NPD_P = 700
EXACT_RHO = 100.0    # every prior precision is absorbed by the diagonal of the dyadic H (asserted bit for bit)


def all_exact_sizes():
    return sorted({p for e in ENVIRONMENTS.values() for p in e[1]})


def all_real_sizes():
    return sorted({p for e in ENVIRONMENTS.values() for p in e[2]})


def rhs_of(p, q=1, seed=0):
    """q right-hand sides, q x p (the columns of the batched solve contiguous)"""
    return np.random.default_rng(7000 + 13 * p + seed).standard_normal((q, p))


def route_constants(H, r, L0=None, bound=None):
    """C, C_s and the two routes' ratios of one matrix.  Exact case (L0, bound given): the factor's ratio is
    |L - L0| / bound; real case: the long-double residual rule."""
    out = {}
    for name, route in (("lapack", lapack_route), ("blocked", blocked_route)):
        L, th = route(H, r)
        rf = factor_ratio_exact(L, L0, bound) if L0 is not None else factor_residual_ratio(L, H)
        out[name] = (rf, solve_ratio(H, r, L, th))
    out["C"] = constant_from_ratio(max(out["lapack"][0], out["blocked"][0]))
    out["Cs"] = constant_from_ratio(max(out["lapack"][1], out["blocked"][1]))
    return out


@functools.lru_cache(maxsize=None)
def exact_case(p):
    """L0, the bound of |L^ - L0|, the right-hand side, cond(H) and the constants of the exact case at p; H
    itself is L0 L0^T again (exact_hessian) and is not kept"""
    H, L0 = dyadic_hessian(p, 100 + p)
    W = inverse64(L0)
    bound = factor_bound(L0, W)
    r = rhs_of(p)[0]
    k = route_constants(H, r, L0, bound)
    return dict(p=p, L0=L0, bound=bound, r=r, cond=cond_spd(L0, W), **k)


def exact_hessian(c):
    """H of an exact case: the float64 product of L0 with itself is exact (dyadic_hessian)"""
    return c["L0"] @ c["L0"].T


def multi_rhs(p, q):
    """the q right-hand sides of a batched solve (q x p): the case's own, then q - 1 more"""
    return np.concatenate([exact_case(p)["r"][None, :], rhs_of(p, q - 1, seed=1)])


@functools.lru_cache(maxsize=None)
def multi_constants(p, q):
    """C_s per column of the batched solve on the exact case: both routes' substitutions on that column, each
    route's factor taken once"""
    H = exact_hessian(exact_case(p))
    L1 = np.linalg.cholesky(H)
    L2, inv = blocked_cholesky64(H)
    return [constant_from_ratio(max(solve_ratio(H, r, L1, substitute64(L1, r)),
                                    solve_ratio(H, r, L2, blocked_solve64(L2, inv, r)))) for r in multi_rhs(p, q)]


_REAL = {}


def real_case(p, diag=None):
    """H (G with the diagonal that was factorised: `diag` from the device, or G's own plus the float64 prior
    precision), r, cond(H) and the constants of the real case at p"""
    parts = real_parts(p)
    if diag is None:
        diag = np.diagonal(parts["G"]) + parts["prec"]
    key = (p, _f64(diag).tobytes())
    if key not in _REAL:
        H = real_hessian(parts["G"], diag)
        k = route_constants(H, parts["r"])
        _REAL[key] = dict(p=p, H=H, r=parts["r"], terms=parts["terms"], cond=float(np.linalg.cond(H)), **k)
    return _REAL[key]


def describe(c):
    return ("C %.3g C_s %.3g cond %.3g; float64 routes err/bound L lapack %.3g blocked %.3g, theta lapack %.3g "
            "blocked %.3g" % (c["C"], c["Cs"], c["cond"], c["lapack"][0], c["blocked"][0], c["lapack"][1],
                              c["blocked"][1]))
