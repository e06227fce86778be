"""Host-side checks of the streaming Newton fit (no GPU): declared and exported symbols, the state
size arithmetic, argument errors that return before any device call, the Python shape checks and
the fold assignment."""
import ctypes as C
import os

import numpy as np
import pytest

NEW = ["obhip_normal_acc_create", "obhip_normal_acc_destroy", "obhip_normal_acc_reset", "obhip_normal_acc_info",
       "obhip_normal_acc_bytes", "obhip_normal_acc_export_dev", "obhip_normal_acc_add_dev",
       "obhip_normal_acc_combine_dev", "obhip_normal_acc_solve_dev", "obhip_cv_score_dev"]


def test_new_symbols_are_declared_and_exported_by_both_libraries():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    testing = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"))
    for name in NEW:
        assert name in protos, name
        assert hasattr(_lib.lib, name), name
        assert hasattr(testing, name), name
    assert len(protos["obhip_normal_acc_add_dev"][1]) == 5
    assert len(protos["obhip_normal_acc_solve_dev"][1]) == 10
    assert len(protos["obhip_cv_score_dev"][1]) == 7
    assert _lib.lib.obhip_abi_version() == 5 and testing.obhip_abi_version() == 5    # purely additive


def test_python_names_are_exported():
    import outerbase_amd as ob
    for name in ("NewtonAccumulator", "cv_newton_multi", "cv_folds", "CVResult"):
        assert name in ob.__all__ and hasattr(ob, name)


@pytest.mark.parametrize("p", [1, 63, 300, 4096, 16384])
def test_state_bytes(p):
    """[packed upper triangle][B^T (Y - c): p q][B^T 1: p][c, mu, M2, n per response] doubles"""
    from outerbase_amd._lib import lib
    b = C.c_uint64(0)
    for q in (1, 3, 17, 40):
        assert lib.obhip_normal_acc_bytes(p, q, C.byref(b)) == 0
        assert b.value == 8 * (p * (p + 1) // 2 + p * q + p + 4 * q)
    assert lib.obhip_normal_acc_bytes(0, 3, C.byref(b)) == 1
    assert lib.obhip_normal_acc_bytes(p, 0, C.byref(b)) == 1
    assert lib.obhip_normal_acc_bytes(p, 3, None) == 1
    assert b"normal_acc_bytes" in lib.obhip_last_error()


def _model():
    import outerbase_amd as ob
    from conftest import knots_for
    kinds = ["mat25", "mat25pow"]
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    return om, om.selectterms(10)


def test_null_and_zero_arguments_are_invalid_before_any_device_call():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    om, terms = _model()
    t = ob.obmod._Terms(om, terms)
    h = C.c_void_p()
    assert lib.obhip_normal_acc_create(None, om._h, t._h, 2) == 1
    assert lib.obhip_normal_acc_create(C.byref(h), None, t._h, 2) == 1
    assert lib.obhip_normal_acc_create(C.byref(h), om._h, None, 2) == 1
    assert lib.obhip_normal_acc_create(C.byref(h), om._h, t._h, 0) == 1
    assert not h.value
    assert lib.obhip_normal_acc_destroy(None) == 0
    assert lib.obhip_normal_acc_reset(None) == 1
    assert lib.obhip_normal_acc_info(None, None, None, None, None) == 1
    assert lib.obhip_normal_acc_export_dev(None, None, 0) == 1
    assert lib.obhip_normal_acc_add_dev(None, None, None, 10, 1) == 1
    assert lib.obhip_normal_acc_combine_dev(None, None, 1) == 1
    assert lib.obhip_normal_acc_solve_dev(None, None, 0.0, 6.0, None, None, None, None, None, 0) == 1
    assert lib.obhip_cv_score_dev(None, None, 10, 2, 10, None, None) == 1
    one = (C.c_double * 4)()
    assert lib.obhip_cv_score_dev(one, one, 2, 0, 2, None, one) == 1       # no responses
    assert lib.obhip_cv_score_dev(one, one, 2, 1, 1, None, one) == 1       # ld below the rows
    assert b"cv_score_dev" in lib.obhip_last_error()


def test_shape_and_finiteness_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    om, terms = _model()
    x = np.full((50, 2), 0.5)
    Y = np.zeros((50, 3))
    with pytest.raises(ValueError):
        ob.NewtonAccumulator(om, terms, q=0)
    acc = ob.NewtonAccumulator(om, terms, q=3)          # no device call yet
    for f in (acc.add, acc.remove):
        with pytest.raises(ValueError, match="rows"):
            f(x, Y[:49])
        with pytest.raises(ValueError, match="responses"):
            f(x, Y[:, :2])
        with pytest.raises(ValueError, match="no columns"):
            f(x, Y[:, :0])
        with pytest.raises(ValueError, match="n x d"):
            f(x[:, :1], Y)
        for bad in (np.inf, np.nan):
            Yb = Y.copy()
            Yb[7, 1] = bad
            with pytest.raises(ValueError, match="finite"):
                f(x, Yb)
            xb = x.copy()
            xb[3, 0] = bad
            with pytest.raises(ValueError, match="finite"):
                f(xb, Y)
    with pytest.raises(TypeError):
        acc.merge(object())
    with pytest.raises(ValueError):
        acc.merge(acc, sign=2)
    acc.close()
    with pytest.raises(RuntimeError, match="closed"):
        acc.add(x, Y)
    with pytest.raises(ValueError, match="rows"):
        ob.cv_newton_multi(om, terms, x, Y[:49])
    with pytest.raises(ValueError, match="folds"):
        ob.cv_newton_multi(om, terms, x, Y, folds=1)
    with pytest.raises(ValueError, match="folds"):
        ob.cv_newton_multi(om, terms, x, Y, folds=51)
    with pytest.raises(ValueError, match="finite"):
        ob.cv_newton_multi(om, terms, x, Y, sigmas=(np.nan,))
    with pytest.raises(ValueError, match="non-empty"):
        ob.cv_newton_multi(om, terms, x, Y, rhos=())


def test_fold_assignment_is_deterministic_and_balanced():
    import outerbase_amd as ob
    a, b, c = ob.cv_folds(1003, 4, seed=5), ob.cv_folds(1003, 4, seed=5), ob.cv_folds(1003, 4, seed=6)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    counts = np.bincount(a, minlength=4)
    assert counts.sum() == 1003 and counts.max() - counts.min() <= 1 and set(a) == {0, 1, 2, 3}


def test_new_sources_are_in_the_makefile_and_name_no_new_switch():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "outerbase_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "kernels_acc.hip" in mk and "normal_acc.cpp" in mk
    for f in ("kernels_acc.hip", "normal_acc.cpp"):
        assert "getenv" not in open(os.path.join(csrc, f)).read()
