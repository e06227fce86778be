"""The posterior-covariance path per entry against the long-double instrument of tests/posterior_ref.py:
obhip_predict_std (k_trtri_diag / k_trtri_cols, the row-norm form of the two-operand Gram kernel) and
obhip_margadj_full (its stored-product form, k_transpose, k_dot_cols and the host arithmetic), through the
C ABI on Hessians the test designs, at the sizes where each piece takes another path: up to 18 block rows
of the inversion (three trips of its k loop), 9 x 9 tiles (two squares of the task table each way), more
shapes than the task-table cache holds; and once through the model layer, one factor serving two shapes.

Every entry is held to  C x (bound propagated from the design matrix's) + gamma_k x sum |summands|  with C
eight times the float64 LAPACK route's own err / bound on the same case (posterior_ref's docstring;
test_posterior_ref_host.py holds that route to the same tolerance at every shape used here and stages the
failures these shapes must be able to see).  Each check prints one line -- C, err / bound and err /
tolerance of the device and of the float64 route -- the rows of the table in DESIGN.md section 6.

The row-chunk frame that post_var_dev, row_forms_dev and the acquisition gradients share (csrc/row_chunks.h) runs
with more than one chunk on a GPU through test_gpu_acquire_grad.py (chunk_rows = 128); its arithmetic is walked on
the host by test_row_chunks_host.py.  Still not run on a GPU: post_var_dev's and row_forms_dev's own epilogues at
r0 != 0 (the partial sums and row sums written at d_var + r0), because their caps -- 8 GiB and 1 GiB per term-major
block -- cannot be reached at test sizes and no switch is added for it."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import extended_ref as E
import posterior_ref as P
from conftest import knots_for, make_pair

pytestmark = pytest.mark.gpu
ld = np.longdouble


@functools.lru_cache(maxsize=None)
def models(short):
    """(oracle model, device model) on the oracle's rotation: short length scales for the dyadic cases,
    the default hyper-parameters for the real Hessians"""
    om_o, om_d = make_pair(P.KINDS, knots_for(P.KINDS, P.NKNOTS), hyp=P.HYP_SHORT if short else None)
    rot, _, _ = om_d.rotation()
    assert np.array_equal(rot, om_o.rotmat)
    return om_o, om_d


@functools.lru_cache(maxsize=None)
def dyadic(p):
    import outerbase_amd as ob
    om_o, om_d = models(True)
    H, L = P.dyadic_hessian(p, 100 + p)
    terms = P.spread_terms(om_o, p, 5)
    return dict(om=om_o, om_d=om_d, terms=terms, t=ob.obmod._Terms(om_d, terms), H=H, L=L)


@functools.lru_cache(maxsize=None)
def real(p):
    """the oracle's total Hessian of a fit on 1500 rows at the default hyper-parameters, sigma = log 0.1"""
    import ob_oracle as O
    import outerbase_amd as ob
    om_o, om_d = models(False)
    x, y = O.synth_xy(42, 0, 1500, P.KINDS)
    y = (y - y.mean()) / y.std(ddof=1)
    terms = np.asarray(om_o.selectterms(p), dtype=np.int64)
    sigma = math.log(0.1)
    _, H = O.fit_newton(O.OuterBase(om_o, x), terms, y, sigma=sigma)
    H = 0.5 * (H + H.T)
    return dict(om=om_o, om_d=om_d, terms=terms, t=ob.obmod._Terms(om_d, terms), H=H, L=P.cholesky_ld(H), x=x, y=y,
                sigma=sigma)


def device_var(c, x, sigma, ldx=None):
    """obhip_predict_std on host buffers; ldx > n: NaN in the padding rows of x"""
    from outerbase_amd._lib import call, ptr
    n = x.shape[0]
    ldx = n if ldx is None else ldx
    xpad = np.full((ldx, x.shape[1]), np.nan, order="F")
    xpad[:n] = x
    mean, var = np.empty(n), np.full(n, np.nan)
    H, theta = np.asfortranarray(c["H"]), np.zeros(len(c["terms"]))
    call("obhip_predict_std", c["om_d"]._h, c["t"]._h, ptr(theta), ptr(H), ptr(xpad), n, ldx, ptr(mean), sigma,
         ptr(var))
    assert np.all(mean == 0.0)
    return var


def check_var(label, got, v):
    """the device's var against the long-double reference of the case v (posterior_ref.var_case)"""
    assert np.all(np.isfinite(got)), label
    tol = P.tolerance(v["C"], v["bound"], v["rest"])
    rmap = E.ratio_map(got, v["want"], tol)
    print("posterior | %s: C %.3g; device max-norm %.3g err/bound %.3g err/tol %.3g; float64 route max-norm %.3g "
          "err/bound %.3g err/tol %.3g" % (label, v["C"], E.maxnorm_relerr(got, v["want"]),
                                           E.worst_ratio(got, v["want"], v["bound"]), rmap.max(),
                                           E.maxnorm_relerr(v["v64"], v["want"]), v["r"],
                                           E.worst_ratio(v["v64"], v["want"], tol)))
    assert rmap.max() <= 1.0, "%s: row %d, %d of %d rows above tolerance" % (
        label, int(np.argmax(rmap)), int((rmap > 1).sum()), rmap.size)


# ---- obhip_predict_std, dyadic H -----------------------------------------------------------------------------
@pytest.mark.parametrize("p,n", P.VAR_SIZES)
def test_predict_std_on_the_dyadic_hessian(p, n):
    """sigma = -40: the floor e^{2 sigma} = 1.8e-35 is below rounding, so the posterior term is compared at
    full sensitivity.  p: one block row (1, 63, 64), ragged and edge-full block rows (65, 128, 129), five
    block rows -- the last shape with single-trip k loops (320) --, six and seven, where the second trip
    starts (321, 385), eleven, where the third starts (641), and 8 against 9 column tiles, the square
    boundary of the task table, with the tri cut at every J (1024, 1025, 1100); n = 1, 127, 128, 129 at
    p = 385 and 9 row tiles against 2 column tiles (p = 130, n = 1100)."""
    c = dyadic(p)
    v = P.var_case(c["om"], c["terms"], c["H"], c["L"], P.inside_rows(n, 9), -40.0)
    check_var("dyadic p=%d n=%d" % (p, n), device_var(c, v["x"], -40.0), v)


def test_predict_std_nine_tiles_on_both_sides():
    """p = 1100, n = 1100: two squares of the task table each way.  A fixed subset of rows, stated here and
    not derived from any result -- the first and the last row of every 64-row tile (posterior_ref.
    tile_edge_rows: 0, 63, 64, 127, ..., 1088, 1099) -- goes through the long-double reference, and C is
    measured on them; EVERY row is compared with the float64 LAPACK route, each side allowed its own
    tolerance: the device C x bound + rest, the route the (C / 8) x bound + rest it was measured at."""
    import ob_oracle as O
    p = n = 1100
    c = dyadic(p)
    x = P.inside_rows(n, 9)
    got = device_var(c, x, -40.0)
    sub = P.tile_edge_rows(n)
    assert len(sub) == 36 and sub[0] == 0 and sub[-1] == n - 1
    v = P.var_case(c["om"], c["terms"], c["H"], c["L"], x[sub], -40.0)
    check_var("dyadic p=1100 n=1100, 36 tile-edge rows", got[sub], v)
    Bo = O.ob_getmat(O.OuterBase(c["om"], x), c["terms"])
    _, bB = P.extended(c["om"], x).getmat(c["terms"])
    bound, rest = P.var_bound64(c["L"], Bo, bB, -40.0)
    v64 = P.host_var64(c["H"], Bo, -40.0)
    assert np.all(np.isfinite(got))
    ratio = np.abs(got - v64) / (P.tolerance(v["C"], bound, rest) + P.tolerance(v["C"] / 8, bound, rest))
    print("posterior | dyadic p=1100 n=1100, all rows against the float64 route: max-norm %.3g, worst |device - route| "
          "/ (both tolerances) %.3g" % (E.maxnorm_relerr(got, v64), ratio.max()))
    assert ratio.max() <= 1.0, "row %d, %d rows above" % (int(np.argmax(ratio)), int((ratio > 1).sum()))


def test_predict_std_leading_dimension_and_the_noise_floor():
    """x with ldx > n and NaN in its padding rows (the padding must never reach a result), and sigma = log 0.1:
    var is the reference's posterior term plus e^{2 sigma}, and above the floor everywhere."""
    c = dyadic(385)
    v = P.var_case(c["om"], c["terms"], c["H"], c["L"], P.inside_rows(130, 9), -40.0)
    got = device_var(c, v["x"], -40.0, ldx=200)
    check_var("dyadic p=385 n=130 ldx=200, NaN padding", got, v)
    assert np.array_equal(got, device_var(c, v["x"], -40.0))
    s = math.log(0.1)
    v = P.var_case(c["om"], c["terms"], c["H"], c["L"], P.inside_rows(130, 9), s)
    got = device_var(c, v["x"], s)
    check_var("dyadic p=385 n=130 sigma=log 0.1", got, v)
    assert np.all(got > math.exp(2 * s))


# ---- obhip_predict_std, real H ---------------------------------------------------------------------------------
def test_predict_std_on_the_oracles_hessian():
    """p = 450, the total Hessian of a mixed-covariance d = 4 fit (cond about 100) at the default length
    scales: accuracy under the conditioning of a real prior, where the design matrix's own bound and the
    backward error of the factorisation (gamma(p + 1) || |L|^T |inv(H) b_i| ||^2) make the tolerance."""
    c = real(450)
    v = P.var_case(c["om"], c["terms"], c["H"], c["L"], P.inside_rows(257, 11), -40.0, backward=True)
    check_var("real H p=450 n=257", device_var(c, v["x"], -40.0), v)


# ---- the task-table cache ------------------------------------------------------------------------------------
def test_task_table_cache_evicts_and_rebuilds_bit_for_bit():
    """launch_atb keeps the task tables of the 8 most recently used (row tiles, column tiles) shapes.  Ten
    distinct shapes in one process, then the first again -- evicted twice over by then, so its table is built
    anew: the result must equal its first run bit for bit, which also pins the run-to-run determinism of the
    row-norm epilogue.  Every run is also held to the reference."""
    shapes = [(64, n) for n in (100, 200, 300, 400, 600)] + [(129, n) for n in (100, 200, 300, 400, 600)]
    assert len({((n + 127) // 128, (p + 127) // 128) for p, n in shapes}) == 10

    def run(p, n):
        c = dyadic(p)
        x = P.inside_rows(n, 9)
        return c, x, device_var(c, x, -40.0)

    c0, x0, first = run(*shapes[0])
    v = P.var_case(c0["om"], c0["terms"], c0["H"], c0["L"], x0, -40.0)
    check_var("cache, first shape p=64 n=100", first, v)
    for p, n in shapes[1:]:
        c, x, got = run(p, n)
        assert np.all(np.isfinite(got)) and np.all(got > 0)
    c, x, got = run(*shapes[-1])                                  # the last shape is still cached
    v = P.var_case(c["om"], c["terms"], c["H"], c["L"], x, -40.0)
    check_var("cache, tenth shape p=129 n=600", got, v)
    _, _, again = run(*shapes[0])
    assert np.array_equal(first, again)


# ---- obhip_margadj_full ----------------------------------------------------------------------------------------
def device_margadj(c, x, sigma, rho, grads=True):
    import outerbase_amd as ob
    from outerbase_amd._lib import call, ptr
    om_d = c["om_d"]
    basis = ob.outerbase(om_d, x)
    nh = len(c["om"].hypmatch)
    val = C.c_double(float("nan"))
    gh, gp = np.full(nh, np.nan), np.full(2, np.nan)
    H = np.asfortranarray(c["H"])
    call("obhip_margadj_full", basis._h, c["t"]._h, om_d._h, ptr(H), sigma, rho, C.byref(val),
         ptr(gh) if grads else None, ptr(gp) if grads else None)
    return {"val": val.value, "gradhyp": gh, "gradpara": gp}


def check_margadj(label, got, m):
    assert np.isfinite(got["val"]) and np.all(np.isfinite(got["gradhyp"])) and np.all(np.isfinite(got["gradpara"]))
    dev, host = P.margadj_ratios(got, m), P.margadj_ratios(m["got64"], m)
    bnd = lambda g: max(E.worst_ratio(g["gradhyp"], m["ref"]["gradhyp"][0], m["ref"]["gradhyp"][1]),
                        E.worst_ratio(g["gradpara"][:1], m["ref"]["gradpara"][0][:1], m["ref"]["gradpara"][1][:1]))
    rel = lambda g: max(E.maxnorm_relerr(np.atleast_1d(g[k]), np.atleast_1d(m["ref"][k][0])) for k in m["ref"])
    print("posterior | %s: C %.3g; device max-norm %.3g err/bound %.3g err/tol val %.3g gradhyp %.3g gradpara %.3g; "
          "float64 route max-norm %.3g err/bound %.3g err/tol val %.3g gradhyp %.3g gradpara %.3g"
          % (label, m["C"], rel(got), bnd(got), dev["val"], dev["gradhyp"], dev["gradpara"],
             rel(m["got64"]), m["r"], host["val"], host["gradhyp"], host["gradpara"]))
    assert max(dev.values()) <= 1.0, (label, dev)


@pytest.mark.parametrize("p,n", P.MARGADJ_SIZES)
def test_margadj_full_on_the_dyadic_hessian(p, n):
    """val, every gradhyp (one- and two-hyper-parameter dimensions: 1 + 2 + 2 + 1) and both gradpara, sigma =
    log 0.1, rho = 2: one tile of terms (64), ragged second tile (129), four tiles against three row tiles
    (385, 257), six against three (700, 300) -- the stored products inv(H) = Linv^T Linv (pp x pp) and
    Y = inv(H) B^T (pp x npad), k_transpose over more than one 64-tile, k_dot_cols over more than one."""
    c = dyadic(p)
    sigma, rho = math.log(0.1), 2.0
    m = P.margadj_case(c["om"], c["terms"], c["H"], c["L"], P.inside_rows(n, 9), sigma, rho)
    check_margadj("margadj dyadic p=%d n=%d" % (p, n), device_margadj(c, m["x"], sigma, rho), m)


def test_margadj_full_on_the_oracles_hessian_and_val_only():
    """p = 385 on 257 of the rows of the fit whose total Hessian it is (sigma = log 0.1, rho = 6, the prior's
    default), with the factorisation's backward-error terms; and one call with gradhyp = gradpara = NULL, the
    want_inverse = false branch: the same val, bit for bit, and nothing else written."""
    c = real(385)
    m = P.margadj_case(c["om"], c["terms"], c["H"], c["L"], c["x"][:257], c["sigma"], 6.0, backward=True)
    got = device_margadj(c, m["x"], c["sigma"], 6.0)
    check_margadj("margadj real H p=385 n=257", got, m)
    only = device_margadj(c, m["x"], c["sigma"], 6.0, grads=False)
    assert only["val"] == got["val"]
    assert np.all(np.isnan(only["gradhyp"])) and np.all(np.isnan(only["gradpara"]))


# ---- through the model layer -----------------------------------------------------------------------------------
def test_model_layer_one_factor_two_shapes_and_the_marginal_adjustment():
    """lpdfvec(loglik_std, logpr_gauss).optnewton() at p = 450 on 1500 rows, then predictor.update with 130 and
    with 1030 rows: one PostFactor serves two shapes (2 and 9 row tiles).  var() against long double on the H
    the library reports (lp.hess(), symmetrised; the factorisation's backward error in the tolerance).
    lp.val / gradhyp / gradpara = the oracle's likelihood and prior parts plus the marginal adjustment, the
    latter in long double on the same H; the oracle's float64 parts are allowed the flat tolerances
    test_full_hessian_marginal_adjustment_after_optnewton gives the whole (1e-9, 1e-7, 1e-8 of their own
    magnitude), the adjustment its per-entry one."""
    import ob_oracle as O
    import outerbase_amd as ob
    om_o, om_d = models(False)
    c0 = real(450)
    x, y, terms = c0["x"], c0["y"], c0["terms"]
    lik = ob.loglik_std(om_d, terms, y, x)
    pr = ob.logpr_gauss(om_d, terms)
    lp = ob.lpdfvec(lik, pr)
    assert lp.domarg
    lp.optnewton()
    sigma, rho = float(lik.para[0]), float(pr.para[0])
    H = lp.hess()
    H = 0.5 * (H + H.T)
    L = P.cholesky_ld(H)
    pred = ob.predictor(lp)
    for n in (130, 1030):
        pred.update(P.inside_rows(n, 21))
        v = P.var_case(om_o, terms, H, L, P.inside_rows(n, 21), sigma, backward=True)
        got = pred.var()
        check_var("model layer p=450 n=%d" % n, got, v)
        assert np.all(got > math.exp(2 * sigma))
    # the marginal adjustment on the training rows
    m = P.margadj_case(om_o, terms, H, L, x, sigma, rho, backward=True)
    bo = O.OuterBase(om_o, x, dograd=True)
    theta, _ = O.fit_newton(bo, terms, y, sigma=sigma, rho=rho)
    ov, _, ogh, ogp = O.loglik_update(bo, terms, y, sigma, theta)
    pv, _, pgh, pgp = O.logpr_update(om_o, terms, rho, theta)
    ref = m["ref"]
    tol = lambda k: P.tolerance(m["C"], np.atleast_1d(ref[k][1]), np.atleast_1d(ref[k][2]))
    e_val = abs(float(ld(lp.val) - (ld(ov + pv) + ref["val"][0])))
    e_gh = np.abs(E._f64(np.asarray(lp.gradhyp, dtype=ld) - (np.asarray(ogh + pgh, dtype=ld) + ref["gradhyp"][0])))
    base_gp = np.array([ogp[0], pgp[0]])
    e_gp = np.abs(E._f64(np.asarray(lp.gradpara, dtype=ld) - (np.asarray(base_gp, dtype=ld) + ref["gradpara"][0])))
    t_val = tol("val")[0] + 1e-9 * abs(ov + pv)
    t_gh = tol("gradhyp") + 1e-7 * np.max(np.abs(ogh + pgh))
    t_gp = tol("gradpara") + 1e-8 * np.max(np.abs(base_gp))
    print("posterior | model layer p=450 n=1500 marginal adjustment: C %.3g; err/tol val %.3g gradhyp %.3g gradpara "
          "%.3g (share of the adjustment's own tolerance in each: %.3g, %.3g, %.3g)"
          % (m["C"], e_val / t_val, np.max(e_gh / t_gh), np.max(e_gp / t_gp), tol("val")[0] / t_val,
             np.max(tol("gradhyp") / t_gh), np.max(tol("gradpara") / t_gp)))
    assert e_val <= t_val and np.all(e_gh <= t_gh) and np.all(e_gp <= t_gp)
