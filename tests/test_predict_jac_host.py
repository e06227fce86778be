"""Host-side checks of the multi-response Jacobian / VJP (no GPU): the batched reference of
tests/extended_jac_ref.py against ExtendedRefDx.ref_grad_mean column by column, a cross-talk mutation
the flat tolerance lets through, and the library's host side -- symbols, Python names, the Makefile,
argument errors that return before any device call, shape errors of the Python functions."""
import ctypes as C
import os

import numpy as np
import pytest

import extended_dx_ref as X
import extended_jac_ref as J
import extended_ref as E
from conftest import knots_for
from test_predict_grad_host import case

NEW = {"obhip_predict_jac_multi_dev": 8, "obhip_predict_vjp_multi_dev": 10, "obhip_predict_jac_multi": 9}
Q = 9


def _theta(p, q, seed=21):
    return np.random.default_rng(seed).standard_normal((p, q)) * J.response_scales(q)[None, :]


# ---- the instrument -------------------------------------------------------------------------------
def test_batched_reference_equals_ref_grad_mean_column_by_column():
    c = case()
    ref, terms = c["ref"], c["terms"]
    Theta = _theta(len(terms), Q)
    Cc = 1e-15
    jac, tol = J.ref_jac(ref, terms, Theta, Cc)
    mean, mtol = J.ref_mean(ref, terms, Theta, Cc)
    n = c["x"].shape[0]
    assert jac.shape == tol.shape == (n, 4, Q) and mean.shape == mtol.shape == (n, Q)
    assert jac.dtype == ld_dtype() and np.all(tol > 0) and np.all(mtol > 0)
    B, bB = ref.getmat(terms)
    worst = 0.0
    for j in range(Q):
        gw, gt = ref.ref_grad_mean(terms, Theta[:, j], Cc)
        assert np.array_equal(jac[:, :, j], gw)
        worst = max(worst, float(np.max(np.abs(tol[:, :, j] - gt) / gt)))
        mw, mt = E.ref_matmul(B, bB, Theta[:, j], Cc)
        assert np.array_equal(mean[:, j], mw)
        worst = max(worst, float(np.max(np.abs(mtol[:, j] - mt) / mt)))
    print("batched tolerances against the column rule: %.3g relative" % worst)
    # the float64 sums |dB| @ |Theta| of p = 150 non-negative summands differ by their order only:
    # at most 2 gamma_150 = 3.4e-14 relative
    assert worst < 2 * E.gamma(len(terms))


def ld_dtype():
    return np.dtype(np.longdouble)


def test_vjp_reference_is_the_weighted_sum_and_covers_both_contraction_orders():
    c = case()
    ref, terms, om, x = c["ref"], c["terms"], c["om"], c["x"]
    Theta = _theta(len(terms), Q)
    Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, om, x, terms))
    jac, tol = J.ref_jac(ref, terms, Theta, Cc)
    W = np.random.default_rng(4).standard_normal((x.shape[0], Q))
    want, vtol = J.ref_vjp(jac, tol, W)
    # the definition, summed in another order: the two agree to the long-double rounding of q summands
    Wl = np.asarray(W, dtype=np.longdouble)
    other = np.einsum("ij,ilj->il", Wl, jac)
    absum = np.einsum("ij,ilj->il", np.abs(Wl), np.abs(jac))
    assert np.all(np.abs(other - want) <= 2 * Q * E.EPS * absum)
    assert np.all(vtol > 0) and want.shape == vtol.shape == (x.shape[0], 4)
    # the float64 restatement, contracted over the responses and through phi = W Theta^T
    _, dB64 = X.dB_f64_of(om, x, terms)
    jac64 = np.einsum("ikl,kj->ilj", dB64, Theta)
    r_jac = E.worst_ratio(jac64, jac, tol)
    r_sum = E.worst_ratio(np.einsum("ij,ilj->il", W, jac64), want, vtol)
    r_phi = E.worst_ratio(np.einsum("ikl,ik->il", dB64, W @ Theta.T), want, vtol)
    print("float64 restatement: jac %.3g, vjp over responses %.3g, vjp through phi %.3g of the tolerance"
          % (r_jac, r_sum, r_phi))
    assert max(r_jac, r_sum, r_phi) < 1


def test_cross_talk_between_responses_passes_the_flat_tolerance_and_fails_the_per_entry_one():
    """1e-9 of the largest-scale response's Jacobian leaking into the smallest-scale one: what a kernel
    that mixes response blocks produces"""
    c = case()
    ref, terms, om, x = c["ref"], c["terms"], c["om"], c["x"]
    Theta = _theta(len(terms), Q)
    sc = J.response_scales(Q)
    lo, hi = int(np.argmin(sc)), int(np.argmax(sc))
    assert sc[lo] == 1e-3 and sc[hi] == 1e3
    Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, om, x, terms))
    jac, tol = J.ref_jac(ref, terms, Theta, Cc)
    _, dB64 = X.dB_f64_of(om, x, terms)
    jac64 = np.einsum("ikl,kj->ilj", dB64, Theta)
    assert E.worst_ratio(jac64, jac, tol) < 1
    mut = jac64.copy()
    mut[:, :, lo] += 1e-9 * jac64[:, :, hi]
    flat = E.maxnorm_relerr(mut, jac)
    r = E.ratio_map(mut, jac, tol)[:, :, lo]
    print("cross-talk 1e-9: flat error %.3g, per entry %.3g x tolerance" % (flat, r.max()))
    assert flat < 1e-6
    assert r.max() > 1


# ---- the library's host side ------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_by_both_libraries():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    testing = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"))
    for name, nargs in NEW.items():
        assert name in protos, name
        assert len(protos[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert hasattr(testing, name), name
    assert _lib.lib.obhip_abi_version() == 5 and testing.obhip_abi_version() == 5    # purely additive


def test_python_names_are_exported():
    import outerbase_amd as ob
    for name in ("predict_jac", "predict_vjp", "TorchEmulator"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert callable(ob.MultiFit.vjp) and callable(ob.MultiFit.torch)


def test_new_sources_are_in_the_makefile():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mk = open(os.path.join(root, "outerbase_amd", "csrc", "Makefile")).read()
    assert "kernels_predict_jac.hip" in mk and "predict_jac.cpp" in mk


def _model():
    import outerbase_amd as ob
    kinds = ["mat25", "mat25pow", "mat25ang"]
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    return om, om.selectterms(40)


def test_argument_errors_return_before_any_device_call():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    om, terms = _model()
    t = ob.obmod._Terms(om, terms)
    buf = (C.c_double * 512)()
    a = C.cast(buf, C.c_void_p)
    big = (1 << 40) + 1
    jac = lib.obhip_predict_jac_multi_dev
    assert jac(None, t._h, a, 2, a, 4, a, a) == 1
    assert jac(om._h, None, a, 2, a, 4, a, a) == 1
    assert jac(om._h, t._h, None, 2, a, 4, a, a) == 1
    assert jac(om._h, t._h, a, 2, None, 4, a, a) == 1
    assert jac(om._h, t._h, a, 2, a, 4, a, None) == 1              # no jac
    assert jac(om._h, t._h, a, 0, a, 4, a, a) == 1                 # q = 0
    assert jac(om._h, t._h, a, 2, a, big, a, a) == 1
    assert b"2^40" in lib.obhip_last_error()
    assert jac(om._h, t._h, a, 2, a, 0, None, a) == 0              # n = 0: a no-op
    vjp = lib.obhip_predict_vjp_multi_dev
    assert vjp(None, t._h, a, 2, a, 4, a, 4, a, a) == 1
    assert vjp(om._h, None, a, 2, a, 4, a, 4, a, a) == 1
    assert vjp(om._h, t._h, None, 2, a, 4, a, 4, a, a) == 1
    assert vjp(om._h, t._h, a, 2, None, 4, a, 4, a, a) == 1
    assert vjp(om._h, t._h, a, 2, a, 4, None, 4, a, a) == 1        # no W
    assert vjp(om._h, t._h, a, 2, a, 4, a, 4, a, None) == 1        # no out
    assert vjp(om._h, t._h, a, 0, a, 4, a, 4, a, a) == 1           # q = 0
    assert vjp(om._h, t._h, a, 2, a, 4, a, 3, a, a) == 1           # ldw below n
    assert b"leading dimension" in lib.obhip_last_error()
    assert vjp(om._h, t._h, a, 2, a, big, a, big, a, a) == 1
    assert b"2^40" in lib.obhip_last_error()
    assert vjp(om._h, t._h, a, 2, a, 0, a, 0, None, a) == 0        # n = 0: a no-op
    host = lib.obhip_predict_jac_multi
    assert host(None, t._h, a, 2, a, 4, 4, a, a) == 1
    assert host(om._h, None, a, 2, a, 4, 4, a, a) == 1
    assert host(om._h, t._h, None, 2, a, 4, 4, a, a) == 1
    assert host(om._h, t._h, a, 2, None, 4, 4, a, a) == 1
    assert host(om._h, t._h, a, 2, a, 4, 4, a, None) == 1
    assert host(om._h, t._h, a, 0, a, 4, 4, a, a) == 1
    assert host(om._h, t._h, a, 2, a, 4, 3, a, a) == 1             # ldx below n
    assert host(om._h, t._h, a, 2, a, big, big, a, a) == 1
    assert host(om._h, t._h, a, 2, a, 0, 0, None, a) == 0
    # terms of another model's dimension count
    other = ob.outermod()
    ob.setcovfs(other, ["mat25"])
    ob.setknot(other, knots_for(["mat25"], 20))
    assert jac(other._h, t._h, a, 2, a, 4, a, a) == 1
    assert vjp(other._h, t._h, a, 2, a, 4, a, 4, a, a) == 1
    assert host(other._h, t._h, a, 2, a, 4, 4, a, a) == 1


def test_shape_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    om, terms = _model()
    x = np.full((2, 3), 0.5)
    with pytest.raises(ValueError):
        ob.predict_jac(om, terms, np.zeros((3, 2)), x)               # Theta: not one row per term
    with pytest.raises(ValueError):
        ob.predict_jac(om, terms, np.zeros(40), x)                   # Theta: not a matrix
    with pytest.raises(ValueError):
        ob.predict_jac(om, terms, np.zeros((40, 0)), x)              # no response
    with pytest.raises(ValueError):
        ob.predict_jac(om, terms, np.zeros((40, 2)), np.full((2, 2), 0.5))
    with pytest.raises(ValueError):
        ob.predict_vjp(om, terms, np.zeros((40, 2)), np.full((2, 2), 0.5), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        ob.predict_vjp(om, terms, np.zeros((3, 2)), x, np.zeros((2, 2)))
    with pytest.raises(ValueError):
        ob.predict_vjp(om, terms, np.zeros((40, 2)), x, np.zeros((2, 3)))   # W: not n x q
    with pytest.raises(ValueError):
        ob.predict_vjp(om, terms, np.zeros((40, 2)), x, np.zeros((3, 2)))
    mf = ob.MultiFit(om, ob.obmod._Terms(om, terms), np.zeros((40, 2)), np.array([[0.0, 1.0, 5.0]] * 2),
                     np.ones(40), 0.0, 6.0)
    with pytest.raises(ValueError):
        mf.vjp(np.full((2, 2), 0.5), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        mf.vjp(x, np.zeros((2, 3)))
