"""Host-side checks of the fit with observed input gradients (no GPU): the reference of
tests/grad_obs_ref.py proved against the value-only equations and against central differences, its float64
solve against its refined long-double solve on the cases the GPU tests use, and the library's host side --
symbols, Python names, argument errors in the documented order before any device call."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import extended_dx_ref as X
import extended_ref as E
import grad_obs_ref as R
from conftest import knots_for
from test_predict_grad_host import KINDS, special_rows

ld = np.longdouble
NEW = ["obhip_design_dx_dev", "obhip_normal_acc_add_grad_dev", "obhip_normal_acc_grad_info"]


# ---- the instrument -------------------------------------------------------------------------------
def test_equations_without_gradients_are_the_value_only_equations():
    """what test_gpu_stream.py holds the accumulator to: the oracle's total Hessian and
    e^{-2 sigma} B^T ((Y - mean) / sd)"""
    import ob_oracle as O
    c = R.cpu_case(129, 128)
    obo = O.OuterBase(c["om_o"], c["x"])
    H = O.total_hess(obo, c["terms"], R.SIGMA, R.RHO)
    Bo = O.ob_getmat(obo, c["terms"])
    Ys = (c["Y"] - c["Y"].mean(axis=0)) / c["Y"].std(axis=0, ddof=1)
    Rv = math.exp(-2 * R.SIGMA) * (Bo.T @ Ys)
    Hh, Rh, cent, sd = R.normal_equations(Bo, c["Y"], c["prec"], R.SIGMA)
    eh, er = E.maxnorm_relerr(Hh, H), E.maxnorm_relerr(Rh, Rv)
    print("value-only equations against the oracle's: H %.3g, right-hand side %.3g" % (eh, er))
    assert eh < 1e-14 and er < 1e-13
    assert np.allclose(cent, c["Y"].mean(axis=0), rtol=1e-14) and np.allclose(sd, c["Y"].std(axis=0, ddof=1), rtol=1e-14)
    # and with gradient rows of weight ~ 0 nothing else comes in: S = 0 adds exact zeros
    H0, R0, _, _ = R.normal_equations(Bo, c["Y"], c["prec"], R.SIGMA, np.zeros_like(c["S64"]), c["Gs"])
    assert np.array_equal(H0, Hh) and np.array_equal(R0, Rh)


def test_stacked_rows_are_the_weighted_derivative_blocks():
    c = R.cpu_case(65, 300)
    n, p = 65, 300
    S, bS, sq = R.stacked(c["ref"], c["terms"], [2, 0], [4.0, 0.25])
    assert S.shape == bS.shape == (2 * n, p) and np.array_equal(sq, [2.0, 0.5])
    D2, _ = c["ref"].getmat_dx(c["terms"], 2)
    D0, b0 = c["ref"].getmat_dx(c["terms"], 0)
    assert np.array_equal(S[:n], 2 * D2) and np.array_equal(S[n:], D0 / 2) and np.array_equal(bS[n:], b0 / 2)
    g = R.stacked_g(c["dY"][:, [2, 0], :], sq)
    assert g.shape == (2 * n, 1) and np.array_equal(g[:n, 0], 2 * c["dY"][:, 2, 0]) and np.array_equal(g[n:, 0], c["dY"][:, 0, 0] / 2)


def test_analytic_gradient_of_the_test_response():
    rng = np.random.default_rng(1)
    x = 0.1 + 0.8 * rng.random((7, 4))
    _, dY = R.response(x, 3)
    for l in range(4):
        xp, xm = x.copy(), x.copy()
        xp[:, l] += 1e-6
        xm[:, l] -= 1e-6
        fd = (R.response(xp, 3)[0] - R.response(xm, 3)[0]) / (xp[:, l] - xm[:, l])[:, None]
        assert np.max(np.abs(fd - dY[:, l, :])) < 1e-8 * np.max(np.abs(dY))


def test_float64_derivative_basis_against_central_differences():
    """the float64 dB the helper forms its equations from against a central difference of B (long double, as
    test_predict_grad_host.py takes it: short length scales, the terms whose difference quotient is known to
    half the allowance), 1e-10 in the max-norm"""
    import ob_oracle as O
    knots = knots_for(KINDS, 20)
    om = O.OuterMod()
    om.setcovfs(KINDS)
    om.hyp_set(np.array([-0.6, -0.5, 0.4, -0.5, -0.6, -0.5]))
    om.setknot(knots)
    terms = om.selectterms(40)
    x = special_rows(np.random.default_rng(7), 40, KINDS, knots)
    _, dB64 = X.dB_f64_of(om, x, terms)
    for l in range(om.d):
        step = 1e-7 * float(np.max(knots[l]) - np.min(knots[l]))
        xp, xm = x.copy(), x.copy()
        xp[:, l] += step
        xm[:, l] -= step
        Bp, bBp = E.ExtendedRef(om.kinds, knots, om.hyp, om.rotmat, xp).getmat(terms)
        Bm, _ = E.ExtendedRef(om.kinds, knots, om.hyp, om.rotmat, xm).getmat(terms)
        den = (np.asarray(xp[:, l], dtype=ld) - np.asarray(xm[:, l], dtype=ld))[:, None]
        fd = (Bp - Bm) / den
        noise = np.max(E._f64(2 * E.EPS * bBp / np.abs(den)), axis=0)
        keep = noise <= 0.5e-10 * float(np.max(np.abs(dB64[:, :, l])))
        assert keep.sum() >= 25, (l, int(keep.sum()))
        rel = float(np.max(np.abs(fd - dB64[:, :, l])[:, keep]) / np.max(np.abs(dB64[:, :, l][:, keep])))
        print("dimension %d: central difference against the float64 dB/dx on %d terms, max-norm %.3g" % (l, keep.sum(), rel))
        assert rel < 1e-10


@pytest.mark.parametrize("n,p", R.CPU_CASES)
def test_float64_solve_is_within_the_refined_long_double_solve(n, p):
    c = R.cpu_case(n, p)
    cond = np.linalg.cond(c["H64"])
    rel = R.relerr(c["theta64"], c["theta"])
    res = float(np.max(np.abs(c["Hl"] @ c["theta"] - c["Rl"])) / np.max(np.abs(c["Rl"])))
    print("n=%d p=%d: cond(H) %.3g, float64 solve against the refined long double solve %.3g (1.6e-11), "
          "residual of the refined solve %.3g" % (n, p, cond, rel, res))
    assert rel <= 1.6e-11


def test_gradient_rows_change_the_solution():
    c = R.cpu_case(129, 128)
    Hv, Rv, _, _ = R.normal_equations(c["B64"], c["Y"], c["prec"], R.SIGMA)
    tv = np.linalg.solve(Hv, Rv)
    assert R.relerr(tv, c["theta"]) > 1e-3


# ---- the library's host side ------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_by_both_libraries():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    testing = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"))
    for name in NEW:
        assert name in protos, name
        assert hasattr(_lib.lib, name), name
        assert hasattr(testing, name), name
    assert len(protos["obhip_design_dx_dev"][1]) == 9
    assert len(protos["obhip_normal_acc_add_grad_dev"][1]) == 9
    assert len(protos["obhip_normal_acc_grad_info"][1]) == 3
    assert _lib.lib.obhip_abi_version() == 5 and testing.obhip_abi_version() == 5    # purely additive


def test_python_names_are_exported():
    import outerbase_amd as ob
    for name in ("design_dx", "fit_newton_grad"):
        assert name in ob.__all__ and hasattr(ob, name)
    for name in ("add_grad", "remove_grad", "grad_rows"):
        assert hasattr(ob.NewtonAccumulator, name)


def _model():
    import outerbase_amd as ob
    kinds = ["mat25", "mat25pow", "mat25ang"]
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    return om, om.selectterms(40)


def test_design_dx_argument_errors_in_the_documented_order_before_any_device_call():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    om, terms = _model()
    t = ob.obmod._Terms(om, terms)
    buf = (C.c_double * 4096)()
    a = C.cast(buf, C.c_void_p)

    def u32(*v):
        return (C.c_uint32 * len(v))(*v)

    def f64(*v):
        return (C.c_double * len(v))(*v)

    dev = lib.obhip_design_dx_dev
    ok = u32(2, 0)
    # null arguments first, whatever else is wrong
    assert dev(None, t._h, a, 4, ok, 2, None, a, 40) == 1
    assert dev(om._h, None, a, 4, ok, 2, None, a, 40) == 1
    assert dev(om._h, t._h, None, 4, ok, 2, None, a, 40) == 1
    assert dev(om._h, t._h, a, 4, None, 0, None, a, 1) == 1 and b"null" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, 4, ok, 2, None, None, 40) == 1
    # ndims = 0 before a repeated dimension, that before a dimension >= d, that before a bad weight, that before ldo
    assert dev(om._h, t._h, a, 4, u32(1, 1), 0, f64(-1.0), a, 1) == 1 and b"ndims" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, 4, u32(0, 1, 2, 0), 4, None, a, 40) == 1 and b"ndims" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, 4, u32(7, 7), 2, f64(-1.0, 1.0), a, 1) == 1 and b"twice" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, 4, u32(1, 3), 2, f64(-1.0, 1.0), a, 1) == 1 and b"dimension 3" in lib.obhip_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert dev(om._h, t._h, a, 4, u32(1, 2), 2, f64(1.0, bad), a, 1) == 1 and b"weights" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, 4, u32(1, 2), 2, f64(1.0, 2.0), a, 39) == 1 and b"ldo" in lib.obhip_last_error()
    # terms of another model's dimension count
    other = ob.outermod()
    ob.setcovfs(other, ["mat25"])
    ob.setknot(other, knots_for(["mat25"], 20))
    assert dev(other._h, t._h, a, 4, u32(0), 1, None, a, 40) == 1
    # n = 0: a no-op; a well-formed call without a GPU: OBHIP_ERR_NO_DEVICE
    assert dev(om._h, t._h, None, 0, ok, 2, None, a, 40) == 0
    if ob.device_count() == 0:
        assert dev(om._h, t._h, a, 4, ok, 2, f64(1.0, 0.5), a, 40) == 2          # OBHIP_ERR_NO_DEVICE
    # the accumulator's entry: null arguments and the sign (an accumulator needs a device to exist: the rest of
    # its order is checked in test_gpu_grad_obs.py)
    add = lib.obhip_normal_acc_add_grad_dev
    assert add(None, a, 4, ok, 2, None, a, 4, 1) == 1
    assert lib.obhip_normal_acc_grad_info(None, None, None) == 1


def test_python_argument_errors():
    import outerbase_amd as ob
    om, terms = _model()
    x = np.full((3, 3), 0.5)
    for kw in (dict(dims=[0, 0]), dict(dims=[3]), dict(dims=[]), dict(dims=[0.5]), dict(weights=[1.0, 1.0]),
               dict(dims=[1], weights=[0.0]), dict(dims=[1], weights=[float("nan")])):
        with pytest.raises(ValueError):
            ob.design_dx(om, terms, x, **kw)
    with pytest.raises(ValueError):
        ob.design_dx(om, terms, np.full((3, 2), 0.5))
    acc = ob.NewtonAccumulator(om, terms, 2)           # (no device touched before the arguments are checked)
    with pytest.raises(ValueError):
        acc.add_grad(x, np.zeros((3, 3)))              # q = 2: n x L x 2
    with pytest.raises(ValueError):
        acc.add_grad(x, np.zeros((3, 2, 2)))           # L = d = 3
    with pytest.raises(ValueError):
        acc.add_grad(x, np.full((3, 3, 2), np.inf))
    acc._closed = True


def test_new_sources_are_in_the_makefile():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mk = open(os.path.join(root, "outerbase_amd", "csrc", "Makefile")).read()
    assert "kernels_materialize_dx.hip" in mk and "grad_obs.cpp" in mk

