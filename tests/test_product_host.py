"""Host-side checks of the predictor on the product of two input blocks (no GPU): the reference's row
expansion against a plain double loop, a float64 restatement of the product form inside the reference's
tolerances, obhip_product_layout, the refusals that need no device and the Python argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import extended_ref as E
import product_ref as P
from conftest import sample_x

INVALID = 1
NEW = {"obhip_product_layout": 6, "obhip_predict_product_dev": 15, "obhip_product_loglik_dev": 14,
       "obhip_predict_product": 17, "obhip_product_loglik": 16}
SPLITS = ([0], [1, 3], [0, 1, 2])
SIGMA = math.log(0.01)


def model(name):
    from test_gpu_extended import SEED, model as ext_model
    return ext_model(name), SEED[name]


def coefficients(m, q, seed):
    """N(0, 1) sqrt(getvar(terms)) coefficients and the coefficient variances 1 / (1 / getvar + 50)"""
    gv = m["om_o"].getvar(m["terms"])
    rng = np.random.default_rng(seed)
    return rng.standard_normal((len(gv), q)) * np.sqrt(gv)[:, None], 1.0 / (1.0 / gv + 50.0)


def test_expand_against_a_double_loop():
    rng = np.random.default_rng(3)
    for d, dims_b, na, nb in ((4, [0], 3, 5), (4, [1, 3], 4, 2), (5, [0, 1, 2, 4], 1, 3), (3, [2], 2, 1)):
        xa, xb = rng.random((na, d - len(dims_b))), rng.random((nb, len(dims_b)))
        X = P.expand(xa, xb, dims_b)
        assert X.shape == (na * nb, d)
        da = [l for l in range(d) if l not in dims_b]
        for i in range(na):
            for j in range(nb):
                for s, l in enumerate(da):
                    assert X[i * nb + j, l] == xa[i, s]
                for s, l in enumerate(dims_b):
                    assert X[i * nb + j, l] == xb[j, s]
        ra, rb = P.split_x(X, dims_b)
        assert np.array_equal(ra[::nb], xa) and np.array_equal(rb[:nb], xb)


def side_factors(m, xs, side, fill):
    """float64 (U, s) of one side from the oracle's basemat / basescalemat: xs holds the side's columns"""
    import ob_oracle as O
    om, terms = m["om_o"], np.asarray(m["terms"])
    x = np.full((len(xs), om.d), fill)
    x[:, side] = xs
    for l in range(om.d):
        if m["kinds"][l] == "mat25ang" and l not in side:
            x[:, l] = 3.0
    ob = O.OuterBase(om, x)
    U = np.ones((len(xs), len(terms)))
    for l in side:                                   # the factors in the order of the dimensions
        has = terms[:, l] > 0
        U[:, has] *= ob.basemat[:, om.knotptst[l] + terms[has, l]]
    s = np.ones(len(xs))
    for l in side:
        s = s * ob.basescalemat[:, l]
    return U, s


@pytest.mark.parametrize("p", [129, 700])
def test_float64_product_form_inside_the_tolerances(p):
    """sA sB (U o theta) V^T, sA^2 sB^2 (U^2 o c) (V^2)^T + e^{2 sigma} and the likelihood sums in float64
    NumPy against the long-double reference on the expanded rows: the separation the kernel rests on."""
    m, seed = model("mixed d4 p%d" % p)
    Theta, cv = coefficients(m, 1, seed)
    theta = Theta[:, 0]
    rng = np.random.default_rng(seed + 1)
    worst = 0.0
    for dims_b in SPLITS:
        na, nb = 17, 23
        x = sample_x(rng, na + nb, m["kinds"])
        xa, xb = P.split_x(x[:na], dims_b)[0], P.split_x(x[na:], dims_b)[1]
        ref = P.ProductRef(m, xa, xb, dims_b, seed)
        U, sa = side_factors(m, xa, P.dims_a_of(4, dims_b), 0.5)
        V, sb = side_factors(m, xb, list(dims_b), 0.5)
        mean = (sa[:, None] * sb[None, :]) * ((U * theta[None, :]) @ V.T)
        var = (sa[:, None] * sb[None, :]) ** 2 * (((U * U) * cv[None, :]) @ (V * V).T) + math.exp(2 * SIGMA)
        want, tol = ref.mean(theta)
        rm = E.worst_ratio(mean, want, tol)
        wantv, tolv = ref.var(cv, SIGMA)
        rv = E.worst_ratio(var, wantv, tolv)
        y = np.asarray(want[:, 0], dtype=np.float64) + 0.05 * rng.standard_normal(na)
        ov = 0.01 * (1.0 + rng.random(na))
        (c2, t2), (lg, tl) = ref.sums(theta, y, ov, cv, SIGMA)
        r, v = y[:, None] - mean, var + ov[:, None]
        rc = E.worst_ratio((r * r / v).sum(0), c2, t2)
        rl = E.worst_ratio(np.log(v).sum(0), lg, tl)
        print("p = %d, dims_b = %s: err / tol mean %.3g, var %.3g, chi2 %.3g, logdet %.3g; tol / |chi2| %.3g, "
              "tol / |logdet| %.3g" % (p, dims_b, rm, rv, rc, rl, float(np.max(t2 / np.abs(np.asarray(c2, dtype=float)))),
                                       float(np.max(tl / np.abs(np.asarray(lg, dtype=float))))))
        worst = max(worst, rm, rv, rc, rl)
    assert worst <= 1.0


def used_columns(terms, dims):
    return sum(len(set(terms[:, l]) - {0}) for l in dims)


def test_product_layout_on_the_host():
    from outerbase_amd import product_layout
    m, _ = model("mixed d4 p129")
    terms = np.asarray(m["terms"])
    for dims_b in SPLITS + ([3], [2, 3]):
        da = P.dims_a_of(4, dims_b)
        pure_a = np.any((terms[:, da] > 0).any(1) & ~(terms[:, dims_b] > 0).any(1))
        pure_b = np.any((terms[:, dims_b] > 0).any(1) & ~(terms[:, da] > 0).any(1))
        assert pure_a and pure_b                     # terms with no factor on one side: a 1 there
        mu_a, mu_b, fused = product_layout(m["om_d"], terms, dims_b)
        assert mu_a == 1 + used_columns(terms, da) and mu_b == 1 + used_columns(terms, dims_b)
        assert mu_a + mu_b == (1 + used_columns(terms, range(4))) + 1    # Mu + 1
        assert fused
    assert product_layout(m["om_d"], terms[:1], [2]) == (1, 1, True)    # the constant term alone


def test_refusals_before_any_device_call():
    """every refusal of the C entries that needs no device returns OBHIP_ERR_INVALID here, where a call
    that reached the device would return OBHIP_ERR_NO_DEVICE"""
    from outerbase_amd import _lib, obmod
    lib = _lib.lib
    m, _ = model("mixed d4 p129")
    t = obmod._terms_of(m["om_d"], m["terms"])
    om, p = m["om_d"]._h, t.p
    for name, nargs in NEW.items():
        assert len(_lib.PROTOS[name][1]) == nargs and hasattr(lib, name)
    buf = np.zeros(4096)
    sentinel = np.full(64, np.nan)
    a = buf.ctypes.data
    u32 = lambda v: np.asarray(v, dtype=np.uint32)
    mu = C.c_uint64(7)
    bad_splits = ([4], [1, 1], [3, 1], [], [0, 1, 2, 3])
    for db in bad_splits:
        d = u32(db)
        assert lib.obhip_product_layout(t._h, d.ctypes.data, d.size, C.byref(mu), None, None) == INVALID
        assert lib.obhip_predict_product_dev(om, t._h, a, 1, d.ctypes.data, d.size, a, 2, a, 2,
                                             sentinel.ctypes.data, 2, None, SIGMA, None) == INVALID
        assert lib.obhip_product_loglik_dev(om, t._h, a, d.ctypes.data, d.size, a, 2, a, None, a, 2, None, SIGMA,
                                            sentinel.ctypes.data) == INVALID
    assert mu.value == 7
    assert lib.obhip_product_layout(t._h, None, 1, None, None, None) == INVALID
    d = u32([1, 3])
    call = lambda lda, cv, var: lib.obhip_predict_product_dev(om, t._h, a, 1, d.ctypes.data, 2, a, 3, a, 2,
                                                              sentinel.ctypes.data, lda, cv, SIGMA, var)
    assert call(2, None, None) == INVALID                    # lda < na
    assert call(3, None, sentinel.ctypes.data) == INVALID    # d_var without d_coeffvar
    assert lib.obhip_predict_product_dev(om, t._h, a, 0, d.ctypes.data, 2, a, 3, a, 2, a, 3, None, SIGMA, None) == INVALID
    assert lib.obhip_predict_product_dev(None, t._h, a, 1, d.ctypes.data, 2, a, 3, a, 2, a, 3, None, SIGMA, None) == INVALID
    # the host-buffer forms: leading dimensions, and a negative or non-finite observation variance
    xa, xb, y, th = np.full((3, 2), 0.5), np.full((2, 2), 0.5), np.zeros(3), np.zeros(p)
    for bad in (-1e-300, np.nan, np.inf):
        ov = np.array([0.1, bad, 0.1])
        assert lib.obhip_product_loglik(om, t._h, th.ctypes.data, d.ctypes.data, 2, xa.ctypes.data, 3, 3,
                                        y.ctypes.data, ov.ctypes.data, xb.ctypes.data, 2, 2, None, SIGMA,
                                        sentinel.ctypes.data) == INVALID
    assert lib.obhip_product_loglik(om, t._h, th.ctypes.data, d.ctypes.data, 2, xa.ctypes.data, 3, 2, y.ctypes.data,
                                    None, xb.ctypes.data, 2, 2, None, SIGMA, sentinel.ctypes.data) == INVALID
    assert lib.obhip_predict_product(om, t._h, th.ctypes.data, 1, d.ctypes.data, 2, xa.ctypes.data, 3, 3,
                                     xb.ctypes.data, 2, 1, sentinel.ctypes.data, 3, None, SIGMA, None) == INVALID
    assert lib.obhip_predict_product(om, t._h, th.ctypes.data, 1, d.ctypes.data, 2, xa.ctypes.data, 3, 3,
                                     xb.ctypes.data, 2, 2, sentinel.ctypes.data, 3, None, SIGMA,
                                     sentinel.ctypes.data) == INVALID
    assert np.all(np.isnan(sentinel))                        # a refused call changes nothing
    # nothing to do: no device call either
    assert lib.obhip_predict_product_dev(om, t._h, a, 1, d.ctypes.data, 2, None, 0, a, 2, None, 0, None, SIGMA, None) == 0
    assert lib.obhip_product_loglik_dev(om, t._h, a, d.ctypes.data, 2, a, 3, a, None, None, 0, None, SIGMA, None) == 0


def test_python_argument_checks():
    import outerbase_amd as ob
    from outerbase_amd.multi import MultiFit
    m, _ = model("mixed d4 p129")
    om, terms = m["om_d"], np.asarray(m["terms"])
    p = len(terms)
    th, xa, xb = np.zeros((p, 2)), np.full((3, 2), 0.5), np.full((2, 2), 0.5)
    for db in ([4], [1, 1], [3, 1], [], [0, 1, 2, 3], [0.5], [[1]]):
        with pytest.raises(ValueError, match="dims_b"):
            ob.predict_product(om, terms, th, xa, xb, db)
    with pytest.raises(ValueError, match="xa must be"):
        ob.predict_product(om, terms, th, np.zeros((3, 3)), xb, [1, 3])
    with pytest.raises(ValueError, match="xb must be"):
        ob.predict_product(om, terms, th, xa, np.zeros((2, 1)), [1, 3])
    with pytest.raises(ValueError, match="Theta must be"):
        ob.predict_product(om, terms, np.zeros((p + 1, 2)), xa, xb, [1, 3])
    with pytest.raises(ValueError, match="coeffvar"):
        ob.predict_product(om, terms, th, xa, xb, [1, 3], coeffvar=np.zeros(p - 1))
    with pytest.raises(ValueError, match="theta must"):
        ob.product_loglik(om, terms, th, xa, np.zeros(3), xb, [1, 3])
    with pytest.raises(ValueError, match="y must have"):
        ob.product_loglik(om, terms, th[:, 0], xa, np.zeros(2), xb, [1, 3])
    with pytest.raises(ValueError, match="y must be finite"):
        ob.product_loglik(om, terms, th[:, 0], xa, np.array([0.0, np.nan, 0.0]), xb, [1, 3])
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="obsvar must be finite"):
            ob.product_loglik(om, terms, th[:, 0], xa, np.zeros(3), xb, [1, 3], obsvar=np.array([0.1, bad, 0.1]))
    # empty blocks need no device
    assert ob.predict_product(om, terms, th, xa[:0], xb, [1, 3]).shape == (0, 2, 2)
    mean, var = ob.predict_product(om, terms, th, xa, xb[:0], [1, 3], coeffvar=np.ones(p))
    assert mean.shape == (3, 0, 2) and var.shape == (3, 0)
    fit = MultiFit(om, ob.obmod._terms_of(om, terms), th, np.array([[0.0, 1.0, 1.0], [1.0, 2.0, 1.0]]), np.ones(p),
                   SIGMA, 6.0)
    assert fit.predict_product(xa[:0], xb, [1, 3]).shape == (0, 2, 2)
    with pytest.raises(ValueError, match="response must be"):
        fit.calibration_loglik(xa, np.zeros(3), xb, [1, 3], response=2)
    with pytest.raises(ValueError, match="y_field"):
        fit.calibration_loglik(xa, np.zeros(4), xb, [1, 3])
    with pytest.raises(ValueError, match="obs_var must be"):
        fit.calibration_loglik(xa, np.zeros(3), xb, [1, 3], obs_var=np.ones(2))
    with pytest.raises(ValueError, match="dims_b"):
        fit.calibration_loglik(xa, np.zeros(3), xb, [3, 1])
