"""Host-side checks of the gradient by xb on the product of two input blocks (no GPU): the reference
instrument of tests/product_dx_ref.py against central differences of its own long-double sums (second-order
convergence), obhip_product_grad_layout, the refusals that need no device, the ABI version and the Python names."""
import ctypes as C
import math

import numpy as np
import pytest

import product_dx_ref as D
import product_ref as P
from conftest import sample_x
from test_product_host import INVALID, SIGMA, coefficients, model

NEW = {"obhip_product_grad_layout": 7, "obhip_predict_product_grad_dev": 14, "obhip_product_loglik_grad_dev": 14,
       "obhip_predict_product_grad": 16, "obhip_product_loglik_grad": 16}
# (p, dims_b, seed of the rows): the B sides hold a mat25, a mat25pow and a mat25ang dimension between them.
# The seeds are ones for which no candidate sits so close to a knot of its dimension that the jump of the
# kernel's third derivative there enters the stencil of h = 2^-10 (checked below: at most 5 % left out, every
# other entry converging at second order).
CONVERGENCE = [(129, (0, 1, 2), 11), (129, (1, 3), 12), (700, (2,), 13)]


def central(m, seed, xa, xb, dims_b, l, h, theta, y, ov, cv):
    """central differences by column l of xb of the instrument's own two sums: (nb, nb) long doubles"""
    out = []
    for sgn in (1.0, -1.0):
        xs = xb.copy()
        xs[:, l] += sgn * h
        (c2, _), (lg, _) = P.ProductRef(m, xa, xs, dims_b, seed).sums(theta, y, ov, cv, SIGMA)
        out.append((c2, lg))
    return (out[0][0] - out[1][0]) / (2 * np.longdouble(h)), (out[0][1] - out[1][1]) / (2 * np.longdouble(h))


@pytest.mark.parametrize("p,dims_b,seed", CONVERGENCE)
def test_instrument_converges_at_second_order(p, dims_b, seed):
    """the analytic gradients of the instrument against central differences of ProductRef.sums with h = 2^-10
    and 2^-11: the disagreement falls by a factor in [3, 5] (4 = second order) in every entry whose first
    disagreement is not below 1e-14 of the gradient's scale, and those are at most 5 % of the entries"""
    m, mseed = model("mixed d4 p%d" % p)
    na, nb = 5, 14
    rng = np.random.default_rng(seed)
    x = sample_x(rng, na + nb, m["kinds"])
    xa, xb = P.split_x(x[:na], dims_b)[0], P.split_x(x[na:], dims_b)[1]
    Theta, cv = coefficients(m, 1, mseed)
    theta = Theta[:, 0]
    ref = D.ProductDxRef(m, xa, xb, dims_b, mseed)
    y = np.asarray(ref.mean(theta)[0][:, 0], dtype=np.float64) + 0.05 * rng.standard_normal(na)
    ov = 0.01 * (1.0 + rng.random(na))
    (dc, _), (dl, _) = ref.sums_grad(theta, y, ov, cv, SIGMA)
    ratios, left_out, total = [], 0, 0
    for l in range(len(dims_b)):
        e = [central(m, mseed, xa, xb, dims_b, l, h, theta, y, ov, cv) for h in (2.0 ** -10, 2.0 ** -11)]
        for w, want in enumerate((dc[:, l], dl[:, l])):
            scale = float(np.max(np.abs(want)))
            e1 = np.abs(np.asarray(e[0][w] - want, dtype=np.float64))
            e2 = np.abs(np.asarray(e[1][w] - want, dtype=np.float64))
            keep = e1 >= 1e-14 * scale
            total += keep.size
            left_out += int((~keep).sum())
            ratios.extend((e1[keep] / e2[keep]).tolist())
            print("p = %d, dims_b = %s, l = %d, %s: scale %.3g, disagreement %.3g -> %.3g" % (
                p, list(dims_b), l, ("chi2", "logdet")[w], scale, e1.max(), e2.max()))
    print("ratios: min %.4g max %.4g, %d of %d left out" % (min(ratios), max(ratios), left_out, total))
    assert left_out <= 0.05 * total
    assert min(ratios) >= 3.0 and max(ratios) <= 5.0


def test_mean_only_instrument_has_no_variance_gradient():
    m, mseed = model("mixed d4 p129")
    rng = np.random.default_rng(5)
    x = sample_x(rng, 7, m["kinds"])
    xa, xb = P.split_x(x[:3], (1, 3))[0], P.split_x(x[3:], (1, 3))[1]
    theta = coefficients(m, 1, mseed)[0][:, 0]
    ref = D.ProductDxRef(m, xa, xb, (1, 3), mseed)
    (dm, tm), (dv, tv) = ref.pair_grads(theta)
    assert dm.shape == (3, 4, 2) and np.all(tm > 0) and not np.any(dv) and not np.any(tv)
    (dc, tc), (dl, tl) = ref.sums_grad(theta, np.zeros(3), None, None, SIGMA)
    assert dc.shape == (4, 2) and np.all(tc > 0) and not np.any(dl) and not np.any(tl)


def test_grad_layout_on_the_host():
    from outerbase_amd import product_grad_layout, product_layout
    m, _ = model("mixed d4 p129")
    terms = np.asarray(m["terms"])
    for dims_b in ([0], [1, 3], [0, 1, 2], [3], [2, 3]):
        mu_a, mu_b, view_terms, fused = product_grad_layout(m["om_d"], terms, dims_b)
        assert (mu_a, mu_b) == product_layout(m["om_d"], terms, dims_b)[:2]
        assert view_terms == int((terms[:, dims_b] > 0).sum())
        assert fused
    # a dimension of B that no term has: an empty view
    assert product_grad_layout(m["om_d"], terms[:1], [2]) == (1, 1, 0, True)


def test_refusals_before_any_device_call():
    """as test_product_host's: OBHIP_ERR_INVALID where a call that reached the device would return
    OBHIP_ERR_NO_DEVICE, and nothing written"""
    from outerbase_amd import _lib, obmod
    lib = _lib.lib
    m, _ = model("mixed d4 p129")
    t = obmod._terms_of(m["om_d"], m["terms"])
    om, p = m["om_d"]._h, t.p
    for name, nargs in NEW.items():
        assert len(_lib.PROTOS[name][1]) == nargs and hasattr(lib, name)
    buf = np.zeros(4096)
    sentinel = np.full(64, np.nan)
    a, sn = buf.ctypes.data, sentinel.ctypes.data
    u32 = lambda v: np.asarray(v, dtype=np.uint32)
    vt = C.c_uint64(7)
    for db in ([4], [1, 1], [3, 1], [], [0, 1, 2, 3]):
        d = u32(db)
        assert lib.obhip_product_grad_layout(t._h, d.ctypes.data, d.size, None, None, C.byref(vt), None) == INVALID
        assert lib.obhip_predict_product_grad_dev(om, t._h, a, d.ctypes.data, d.size, a, 2, a, 2, sn, 2, None, SIGMA,
                                                  None) == INVALID
        assert lib.obhip_product_loglik_grad_dev(om, t._h, a, d.ctypes.data, d.size, a, 2, a, None, a, 2, None, SIGMA,
                                                 sn) == INVALID
    assert vt.value == 7
    assert lib.obhip_product_grad_layout(None, None, 1, None, None, None, None) == INVALID
    d = u32([1, 3])
    call = lambda lda, cv, dvar: lib.obhip_predict_product_grad_dev(om, t._h, a, d.ctypes.data, 2, a, 3, a, 2, sn, lda,
                                                                    cv, SIGMA, dvar)
    assert call(2, None, None) == INVALID          # lda < na
    assert call(3, None, sn) == INVALID            # d_dvar without d_coeffvar
    assert lib.obhip_predict_product_grad_dev(None, t._h, a, d.ctypes.data, 2, a, 3, a, 2, sn, 3, None, SIGMA, None) == INVALID
    assert lib.obhip_product_loglik_grad_dev(om, t._h, None, d.ctypes.data, 2, a, 3, a, None, a, 2, None, SIGMA, sn) == INVALID
    xa, xb, y, th = np.full((3, 2), 0.5), np.full((2, 2), 0.5), np.zeros(3), np.zeros(p)
    for bad in (-1e-300, np.nan, np.inf):
        ov = np.array([0.1, bad, 0.1])
        assert lib.obhip_product_loglik_grad(om, t._h, th.ctypes.data, d.ctypes.data, 2, xa.ctypes.data, 3, 3,
                                             y.ctypes.data, ov.ctypes.data, xb.ctypes.data, 2, 2, None, SIGMA, sn) == INVALID
    assert lib.obhip_product_loglik_grad(om, t._h, th.ctypes.data, d.ctypes.data, 2, xa.ctypes.data, 3, 2, y.ctypes.data,
                                         None, xb.ctypes.data, 2, 2, None, SIGMA, sn) == INVALID
    assert lib.obhip_predict_product_grad(om, t._h, th.ctypes.data, d.ctypes.data, 2, xa.ctypes.data, 3, 3,
                                          xb.ctypes.data, 2, 1, sn, 3, None, SIGMA, None) == INVALID
    assert lib.obhip_predict_product_grad(om, t._h, th.ctypes.data, d.ctypes.data, 2, xa.ctypes.data, 3, 3,
                                          xb.ctypes.data, 2, 2, sn, 3, None, SIGMA, sn) == INVALID
    assert np.all(np.isnan(sentinel))              # a refused call changes nothing
    # nothing to do: no device call either
    assert lib.obhip_predict_product_grad_dev(om, t._h, a, d.ctypes.data, 2, None, 0, a, 2, None, 0, None, SIGMA, None) == 0
    assert lib.obhip_product_loglik_grad_dev(om, t._h, a, d.ctypes.data, 2, a, 3, a, None, None, 0, None, SIGMA, None) == 0


def test_abi_version_and_python_names():
    import inspect

    import outerbase_amd as ob
    from outerbase_amd import _lib
    from outerbase_amd.multi import MultiFit
    assert _lib.lib.obhip_abi_version() == 5
    for name in ("predict_product_grad", "product_loglik_grad", "product_grad_layout", "TorchCalibration"):
        assert hasattr(ob, name) and name in ob.__all__
    assert inspect.signature(MultiFit.calibration_loglik).parameters["grad"].default is False
    m, _ = model("mixed d4 p129")
    om, terms = m["om_d"], np.asarray(m["terms"])
    p = len(terms)
    th, xa, xb = np.zeros(p), np.full((3, 2), 0.5), np.full((2, 2), 0.5)
    with pytest.raises(ValueError, match="dims_b"):
        ob.predict_product_grad(om, terms, th, xa, xb, [3, 1])
    with pytest.raises(ValueError, match="theta must"):
        ob.predict_product_grad(om, terms, np.zeros((p, 2)), xa, xb, [1, 3])
    with pytest.raises(ValueError, match="y must have"):
        ob.product_loglik_grad(om, terms, th, xa, np.zeros(2), xb, [1, 3])
    with pytest.raises(ValueError, match="obsvar must be finite"):
        ob.product_loglik_grad(om, terms, th, xa, np.zeros(3), xb, [1, 3], obsvar=np.array([0.1, -1.0, 0.1]))
    # empty blocks need no device
    assert ob.predict_product_grad(om, terms, th, xa[:0], xb, [1, 3]).shape == (0, 2, 2)
    out = ob.product_loglik_grad(om, terms, th, xa, np.zeros(3), xb[:0], [1, 3])
    assert [o.shape for o in out] == [(0,), (0,), (0, 2), (0, 2)]
    fit = MultiFit(om, ob.obmod._terms_of(om, terms), np.zeros((p, 2)), np.array([[0.0, 1.0, 1.0], [1.0, 2.0, 1.0]]),
                   np.ones(p), SIGMA, 6.0)
    with pytest.raises(ValueError, match="response must be"):
        fit.calibration_loglik(xa, np.zeros(3), xb, [1, 3], response=2, grad=True)
