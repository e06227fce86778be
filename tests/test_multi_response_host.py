"""Host-side checks of the multi-response entries (no GPU): declared and exported symbols, the
count and workspace arithmetic, argument errors, and the Python shape checks."""
import ctypes as C

import numpy as np
import pytest

NEW = ["obhip_standardise_multi_dev", "obhip_destandardise_multi_dev", "obhip_fit_newton_multi_count",
       "obhip_newton_multi_workspace_bytes", "obhip_newton_multi_solve_dev", "obhip_fit_newton_multi_dev",
       "obhip_predict_multi_dev", "obhip_fit_newton_multi", "obhip_predict_multi"]


def test_new_symbols_are_declared_and_exported():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
        assert hasattr(_lib.lib, name), name
    assert len(protos["obhip_fit_newton_multi_dev"][1]) == 17
    assert len(protos["obhip_predict_multi_dev"][1]) == 10
    assert _lib.lib.obhip_abi_version() == 5          # purely additive


def test_python_names_are_exported():
    import outerbase_amd as ob
    from outerbase_amd.driver import HotPath
    for name in ("fit_newton_multi", "MultiFit", "MultiHotPath"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert issubclass(ob.MultiHotPath, HotPath)
    with pytest.raises(ValueError):
        ob.MultiHotPath(["mat25"], 20, 10, 100, responses=0)
    with pytest.raises(ValueError):
        ob.MultiHotPath(["mat25"], 20, 10, 100, responses=2, backend="cg")


@pytest.mark.parametrize("p", [1, 63, 300, 4096])
def test_exchange_count(p):
    from outerbase_amd._lib import lib
    tri = p * (p + 1) // 2
    c, c1 = C.c_uint64(0), C.c_uint64(0)
    for nranks in (1, 2, 3, 8):
        assert lib.obhip_fit_newton_multi_count(p, 1, nranks, C.byref(c)) == 0
        assert lib.obhip_fit_newton_count(p, nranks, C.byref(c1)) == 0
        assert c.value == c1.value                  # q = 1 is the single-response buffer
        for q in (3, 16, 17, 40):
            assert lib.obhip_fit_newton_multi_count(p, q, nranks, C.byref(c)) == 0
            raw = tri + p * q
            assert c.value >= raw and c.value - raw < 2 * nranks and c.value % (2 * nranks) == 0
    for bad in ((0, 3, 1), (p, 0, 1), (p, 3, 0)):
        assert lib.obhip_fit_newton_multi_count(*bad, C.byref(c)) == 1
    assert lib.obhip_fit_newton_multi_count(p, 3, 1, None) == 1
    assert b"fit_newton_multi_count" in lib.obhip_last_error()


@pytest.mark.parametrize("p", [1, 129, 260, 4096, 16384])
def test_workspace_bytes(p):
    from outerbase_amd._lib import lib
    w1, w = C.c_uint64(0), C.c_uint64(0)
    assert lib.obhip_newton_workspace_bytes(p, C.byref(w1)) == 0
    sizes = set()
    for q in (1, 3, 16, 17, 40, 1000):
        assert lib.obhip_newton_multi_workspace_bytes(p, q, C.byref(w)) == 0
        sizes.add(w.value)
    # the single workspace plus two copies of one 64-column chunk of right-hand sides over p
    # rounded up to whole 64-row blocks -- whatever q is
    assert sizes == {w1.value + 2 * ((p + 63) // 64 * 64) * 64 * 8}
    assert lib.obhip_newton_multi_workspace_bytes(p, 0, C.byref(w)) == 1
    assert lib.obhip_newton_multi_workspace_bytes(0, 2, C.byref(w)) == 1
    assert lib.obhip_newton_multi_workspace_bytes(p, 2, None) == 1


def test_null_arguments_are_invalid_before_any_device_call():
    from outerbase_amd._lib import lib
    assert lib.obhip_standardise_multi_dev(None, None, 10, 2, 10, None, None) == 1
    assert lib.obhip_destandardise_multi_dev(None, 10, 2, 10, None, 0) == 1
    assert lib.obhip_newton_multi_solve_dev(None, None, None, None, 2, 0.0, 6.0, None, None, None, 0) == 1
    assert lib.obhip_fit_newton_multi_dev(None, None, None, None, None, 2, 10, 0.0, 6.0, None, None, None, None,
                                          None, 0, None, 0) == 1
    assert lib.obhip_predict_multi_dev(None, None, None, 2, None, 10, None, None, 0.0, None) == 1
    assert lib.obhip_fit_newton_multi(None, None, None, None, 2, 10, 0.0, 6.0, None, None) == 1
    assert lib.obhip_predict_multi(None, None, None, 2, None, 10, 10, None, None, 0.0, None) == 1


def test_shape_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    from conftest import knots_for
    kinds = ["mat25", "mat25pow"]
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    terms = om.selectterms(10)
    x = np.full((50, 2), 0.5)
    Y = np.zeros((50, 3))
    with pytest.raises(ValueError, match="rows"):
        ob.fit_newton_multi(om, terms, x, Y[:49])
    with pytest.raises(ValueError, match="no columns"):
        ob.fit_newton_multi(om, terms, x, Y[:, :0])
    Ybad = Y.copy()
    Ybad[7, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        ob.fit_newton_multi(om, terms, x, Ybad)
    Ybad[7, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        ob.fit_newton_multi(om, terms, x, Ybad)
    with pytest.raises(ValueError, match="n x d"):
        ob.fit_newton_multi(om, terms, x[:, :1], Y)
    with pytest.raises(ValueError):
        ob.fit_newton_multi(om, terms, x, np.zeros((50, 3, 2)))
