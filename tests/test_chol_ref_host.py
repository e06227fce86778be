"""The Cholesky instrument of tests/chol_ref.py itself (no GPU): its exact case exact, its residuals and
bounds right against 50-digit arithmetic, both float64 host routes within an eighth of the theorems' constants
on every case test_gpu_chol.py runs on the device (the condition under which C and C_s mean anything), its
restatement of the launch loop giving the passes and row counts the cases were chosen for, and the failures
the kernel could plausibly have, staged on the float64 factor, at least ten times above the tolerance."""
import numpy as np
import pytest

import chol_ref as R
import posterior_ref as P

ld = np.longdouble


def teardown_module():
    """the cached cases hold L0 and its bound at every size (0.7 GB): not for the rest of the session"""
    R.exact_case.cache_clear()
    R.multi_constants.cache_clear()


# ---- the construction ----------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 64, 449, 1217])
def test_float64_product_gives_the_integer_hessian(p):
    """chol_ref.dyadic_hessian (float64 BLAS product) = posterior_ref.dyadic_hessian (int64 product) bit for
    bit, both scale back to integers, and at p <= 449 L0 L0^T = H exactly in long double and the long-double
    Cholesky of H is L0: the factor the device must find is known without a factorisation."""
    H, L0 = R.dyadic_hessian(p, 100 + p)
    Hi, Li = P.dyadic_hessian(p, 100 + p)
    assert np.array_equal(H, Hi) and np.array_equal(L0, Li)
    assert np.array_equal(H * 2.0 ** 20, np.round(H * 2.0 ** 20)) and np.array_equal(L0 * 1024, np.round(L0 * 1024))
    assert np.array_equal(L0 @ L0.T, H)                                   # what exact_hessian relies on
    if p <= 449:
        Ll = np.asarray(L0, dtype=ld)
        assert np.array_equal(Ll @ Ll.T, np.asarray(H, dtype=ld))
        assert np.array_equal(P.cholesky_ld(H), Ll)


def test_float64_product_at_the_largest_sizes_on_sampled_rows():
    """p = 3137 and 4160: the int64 product of all rows takes a minute; 24 seeded rows of it (and the last)
    against the float64 product, every entry an integer below 2^53 (asserted inside the helper too)"""
    for p in (3137, 4160):
        H, L0 = R.dyadic_hessian(p, 100 + p)
        Li = np.round(L0 * 1024).astype(np.int64)
        rows = np.unique(np.concatenate([np.random.default_rng(p).integers(0, p, 24), [p - 1]]))
        assert np.array_equal((Li[rows] @ Li.T).astype(np.float64) * 2.0 ** -20, H[rows])
        assert float(np.max(np.abs(H))) * 2.0 ** 20 < 2.0 ** 53


# ---- against 50-digit arithmetic -----------------------------------------------------------------------
def _mp_matrix(A):
    import mpmath
    A = np.asarray(A, dtype=np.float64)
    return mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in A])


def _mp_abs(M):
    import mpmath
    return mpmath.matrix([[abs(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


@pytest.mark.parametrize("kind,p", [("exact", 40), ("exact", 17), ("real", 33)])
def test_residuals_and_bounds_against_50_digit_arithmetic(kind, p):
    """The first-order bound of the factor, the factor's residual ratio and the solution's residual ratio of
    the LAPACK route's float64 L and theta, recomputed by mpmath at 50 digits.  The float64 bounds are right
    to 1e-12 relative (sums of p positive products).  A long-double residual is wrong by at most
    (p + 1) eps_ld (|L| |L|^T)_ij, eps_ld = 2^-63, against a denominator gamma(p + 1) (|L| |L|^T)_ij of
    (p + 1) 2^-53: 2^-10 of the bound, and no more for the solution's (gamma(3 p + 1) below it)."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    if kind == "exact":
        H, L0 = R.dyadic_hessian(p, 3)
    else:
        parts = R.real_parts(p)
        H = R.real_hessian(parts["G"], np.diagonal(parts["G"]) + parts["prec"])
    r = R.rhs_of(p)[0]
    L, th = R.lapack_route(H, r)
    u = mpmath.mpf(2) ** -53
    g = lambda k: k * u / (1 - k * u)
    Hm, Lm, aL = _mp_matrix(H), _mp_matrix(L), _mp_abs(_mp_matrix(L))
    den = aL * aL.T
    res = _mp_abs(Lm * Lm.T - Hm)
    # (an entry of the dyadic L0 may vanish with its whole denominator: nothing is allowed there)
    assert all(res[i, j] == 0 for i in range(p) for j in range(i + 1) if den[i, j] == 0)
    want = max(res[i, j] / (g(p + 1) * den[i, j]) for i in range(p) for j in range(i + 1) if den[i, j] != 0)
    got = R.factor_residual_ratio(L, H)
    assert abs(got - float(want)) <= 2.0 ** -10, (got, float(want))
    thm = mpmath.matrix([mpmath.mpf(float(v)) for v in th])
    rm = mpmath.matrix([mpmath.mpf(float(v)) for v in r])
    sres = Hm * thm - rm
    sden = aL * (aL.T * mpmath.matrix([abs(v) for v in thm]))
    swant = max(abs(sres[i]) / (g(3 * p + 1) * sden[i]) for i in range(p))
    sgot = R.solve_ratio(H, r, L, th)
    assert abs(sgot - float(swant)) <= 2.0 ** -10, (sgot, float(swant))
    bnd = R.solve_bound(L, th)
    assert all(abs(bnd[i] - float(g(3 * p + 1) * sden[i])) <= 1e-12 * bnd[i] for i in range(p))
    if kind == "exact":
        L0m = _mp_matrix(L0)
        aL0, W = _mp_abs(L0m), _mp_abs(L0m ** -1)
        S = W * (aL0 * aL0.T) * W.T
        for i in range(p):
            for j in range(p):
                S[i, j] = 0 if j > i else (S[i, j] / 2 if j == i else S[i, j])
        B = aL0 * S
        bound = R.factor_bound(L0)
        assert np.array_equal(bound, np.tril(bound))
        assert all(abs(bound[i, j] - float(g(p + 1) * B[i, j])) <= 1e-12 * bound[i, j]
                   for i in range(p) for j in range(i + 1))
        assert all(B[i, j] > 0 for i in range(p) for j in range(i + 1))
        # and the exact factor is mpmath's own
        Lc = mpmath.cholesky(Hm)
        assert all(Lc[i, j] == L0m[i, j] for i in range(p) for j in range(i + 1))
        ewant = max(abs(Lm[i, j] - L0m[i, j]) / (g(p + 1) * B[i, j]) for i in range(p) for j in range(i + 1))
        assert abs(R.factor_ratio_exact(L, L0, bound) - float(ewant)) <= 1e-9


# ---- the condition of every device case ----------------------------------------------------------------
@pytest.mark.parametrize("p", R.all_exact_sizes())
def test_both_float64_routes_are_within_an_eighth_on_the_exact_case(p):
    """|L - L0| / bound and the solution's residual ratio of np.linalg.cholesky + dot-product substitution and of
    the blocked restatement: 8 x ratio < 1, so that C and C_s are measured, not the cap"""
    c = R.exact_case(p)
    print("exact p = %d: %s" % (p, R.describe(c)))
    for route in ("lapack", "blocked"):
        assert 8 * c[route][0] < 1 and 8 * c[route][1] < 1, (route, c[route])
    assert c["C"] < 1 and c["Cs"] < 1 and c["cond"] < 100


@pytest.mark.parametrize("p", R.all_real_sizes())
def test_both_float64_routes_are_within_an_eighth_on_the_real_case(p):
    c = R.real_case(p)
    print("real p = %d: %s" % (p, R.describe(c)))
    for route in ("lapack", "blocked"):
        assert 8 * c[route][0] < 1 and 8 * c[route][1] < 1, (route, c[route])
    assert np.array_equal(c["H"], c["H"].T)


def test_both_float64_routes_are_within_an_eighth_on_every_column_of_the_batched_solves():
    for name, e in R.ENVIRONMENTS.items():
        for case, p, q in e[3]:
            Cs = R.multi_constants(p, q)
            print("%s batched %s p = %d q = %d: C_s per column %s" % (name, case, p, q, " ".join("%.3g" % v for v in Cs)))
            assert len(Cs) == q and all(0 < v < 1 for v in Cs)


# ---- the launch loop -----------------------------------------------------------------------------------
def test_launch_plan_gives_the_passes_and_row_counts_the_cases_were_chosen_for():
    """The restated launch loop of launch_newton_solve: the by-rows-left schedule at p = 3137 under
    OBHIP_CHOL_M8=2048 OBHIP_CHOL_M4=1024 takes three passes of 8 panels, three of 4, then passes of 2 down to
    a one-row last panel; p = 4160 at the shipped thresholds goes from 4 to 2; and the sizes added for the
    128 x 128 tiles leave 1, 127, 128 and 129 rows to an update."""
    plan = R.launch_plan(3137, 0, 2048, 1024)
    assert [t for _, t, _ in plan] == [8, 8, 8, 4, 4, 4] + [2] * 7
    assert plan[-1][0] == 3072 and plan[-1][2] == [(3136, 1, True)]
    assert [t for _, t, _ in R.launch_plan(3072, 0, 2048, 1024)] == [8, 8, 8, 4, 4, 4] + [2] * 6
    assert [R.panels_at(4160, 4160 - j0) for j0, _, _ in R.launch_plan(4160)][:3] == [4, 2, 2]
    assert all(t == 1 for _, t, _ in R.launch_plan(1217))
    for n, want in ((2, {1, 127, 128}), (4, {1, 127, 128, 129}), (8, {1, 127, 128, 129})):
        sizes = R.ENVIRONMENTS["panels%d_t128" % n][1]
        trailing = {m for p in sizes for _, _, ups in R.launch_plan(p, n) for _, m, strip in ups if not strip}
        strips = {m for p in sizes for _, _, ups in R.launch_plan(p, n) for _, m, strip in ups if strip}
        assert want <= trailing, (n, sorted(trailing))
        assert 129 in trailing | strips
    # every pass of p = 700 at 8 panels: the first takes eight panels, the second the three that are left
    assert [(j0, t) for j0, t, _ in R.launch_plan(700, 8)] == [(0, 8), (512, 3)]


# ---- the failures the cases must be able to see ----------------------------------------------------------
def _stages(p):
    """name -> (hook of blocked_cholesky64 | None, change of the finished L | None, swap of blocked_solve64 | None)"""
    last_full = p // 64 - 1 if p % 64 else (p + 63) // 64 - 1

    def slice_scaled(L):
        L[64 * last_full:64 * last_full + 64, 16:32] *= 1 + 1e-9

    def kpart(j0, A, X):           # panel 1, tile (2, 1) of its trailing update: k = 32 .. 63 left out
        if j0 == 64:
            A[256:320, 192:256] += X[128:192, 32:64] @ X[64:128, 32:64].T

    def strip_panel(j0, A, X):     # pass of 8 panels from column 0: panel 2 left out of the strip of panel 5
        if j0 == 128:
            A[320:, 320:384] += X[128:] @ X[128:192].T

    def ragged(j0, A, X):          # panel 0, 128-tile (last tile row, tile column 0): its ragged rows
        if j0 == 0:
            m = p - 64
            first = 64 + (m - 1) // 128 * 128
            assert 0 < p - first < 128
            A[first:, 64:192] += X[first - 64:] @ X[:128].T

    return {"slice x (1 + 1e-9)": (None, slice_scaled, None), "32-column k part": (kpart, None, None),
            "panel left out of a strip": (strip_panel, None, None), "neighbour's 16 x 16 inverse": (None, None, (5, 6)),
            "ragged rows of a 128-tile": (ragged, None, None)}


@pytest.mark.parametrize("p", [449, 3137])
def test_staged_failures_land_ten_times_above_the_tolerance(p):
    """Five failures staged on the float64 factor of the blocked route (exact case): a 64 x 16 slice of L in
    the last full block row scaled by 1 + 1e-9; one 32-column k part left out of one 64 x 64 trailing tile's
    update; one panel left out of one strip update of an 8-panel pass; the 16 x 16 inverse of one diagonal
    sub-block replaced by its neighbour's in the back-substitution (seen by the theta rule, the factor being
    untouched); one 128 x 128 tile's ragged last rows not updated.  Each must exceed its tolerance by 10 x;
    printed beside it: the normwise figures the older tests look at (||L - L0|| / ||L0|| and
    ||theta - theta_lapack|| / ||theta_lapack||; they allow 1e-13 cond(H) on a randn(p, p + 3) family whose
    cond(H) is about 8 p: 1e-9 at p = 1217, the largest size at which they look at L)."""
    c = R.exact_case(p)
    H = R.exact_hessian(c)
    L0, r = c["L0"], c["r"]
    th_ref = R.substitute64(np.linalg.cholesky(H), r)
    Lc, inv = R.blocked_cholesky64(H)
    clean = (R.factor_ratio_exact(Lc, L0, c["bound"]) / c["C"],
             R.solve_ratio(H, r, Lc, R.blocked_solve64(Lc, inv, r)) / c["Cs"])
    assert max(clean) <= 1.0 / 8 + 1e-12
    for name, (hook, change, swap) in _stages(p).items():
        L, iv = (R.blocked_cholesky64(H, hook) if hook else (Lc.copy(), inv))
        if change:
            change(L)
        th = R.blocked_solve64(L, iv, r, swap)
        over_l = R.factor_ratio_exact(L, L0, c["bound"]) / c["C"]
        over_s = R.solve_ratio(H, r, L, th) / c["Cs"]
        print("p = %d %s: err/tolerance L %.3g theta %.3g (unstaged %.3g, %.3g); normwise L %.3g theta %.3g"
              % (p, name, over_l, over_s, clean[0], clean[1], np.linalg.norm(L - L0) / np.linalg.norm(L0),
                 np.linalg.norm(th - th_ref) / np.linalg.norm(th_ref)))
        assert (over_s if swap else over_l) >= 10.0, name
