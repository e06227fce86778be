"""Host-side checks of the Hessian-vector predictor (no GPU): the long-double second-derivative
reference of tests/extended_d2_ref.py against high-precision differentiation and against central
differences of the first-derivative reference, the normalised algebra of the kernel against the
direct products, the float64 restatement inside the instrument on every case of the GPU file,
mutations of the algebra that a flat tolerance lets through, and the library's host side -- symbols,
Python names, argument errors that return before any device call, the layout query."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import extended_d2_ref as D2
import extended_dx_ref as X
import extended_jac_ref as J
import extended_ref as E
from conftest import knots_for
from test_gpu_predict_hvp import HCASES, hparts
from test_predict_grad_host import KINDS, HYP, _mp_cov, special_rows

ld = np.longdouble
NEW = ["obhip_predict_hvp_multi_dev", "obhip_predict_hvp_multi", "obhip_predict_hvp_layout"]


@functools.lru_cache(maxsize=None)
def case():
    import ob_oracle as O
    knots = knots_for(KINDS, 20)
    om = O.OuterMod()
    om.setcovfs(KINDS)
    om.hyp_set(HYP)
    om.setknot(knots)
    terms = om.selectterms(150)
    x = special_rows(np.random.default_rng(7), 40, KINDS, knots)
    ref = D2.reference_d2_of(om, x)
    V = D2.direction_rows(len(x), om.d, 11)
    return dict(om=om, knots=knots, terms=terms, x=x, ref=ref, V=V, hvt=ref.hv_terms(terms, V),
                jvt=ref.jv_terms(terms, V))


# ---- the instrument -------------------------------------------------------------------------------
def test_d2cov_dx2_against_high_precision_differentiation():
    """80 digits: a second difference quotient at step 1e-25 keeps 30; on a knot it straddles |.|, which
    the Matern-5/2 kernel allows (its third derivative is continuous there), at a truncation of the
    order of the step"""
    mp = pytest.importorskip("mpmath")
    from test_extended_ref import _mp_of
    kn = knots_for(["mat25"], 20)[0]
    worst = 0.0
    with mp.workdps(80):
        for kind, hyp, xs in (("mat25", [0.3], [kn[4], 0.37, 0.911]),
                              ("mat25pow", [-0.2, 0.4], [0.02, kn[7], 0.55]),
                              ("mat25ang", [0.25, -0.3], [kn[3], 2.9, 5.7])):
            got = D2.d2cov_dx2_ld(kind, np.array(xs), kn, np.array(hyp))
            first = X.dcov_dx_ld(kind, np.array(xs), kn, np.array(hyp))
            assert np.array_equal(D2._cov012(kind, np.array(xs), kn, np.array(hyp), ld)[1], first)
            mh = [mp.mpf(float(h)) for h in hyp]
            for i, xv in enumerate(xs):
                for j in (0, 3, 4, 7, 12, 19):
                    kj = mp.mpf(float(kn[j]))
                    want = mp.diff(lambda z: _mp_cov(kind, z, kj, mh), mp.mpf(float(xv)), 2, h=mp.mpf(10) ** -25)
                    # the entry's own magnitude plus the conditioning of h, a difference of two rounded
                    # transforms, through |d3k/dh3| <= 1/3 and du/dx twice more; for mat25pow at small x
                    # the term k' d2t/dx2 besides
                    if kind == "mat25ang":
                        slope = 1.0 / min(np.exp(2 * hyp[0]), np.exp(2 * hyp[1]))
                        cond = 4.0 * slope ** 3
                    elif kind == "mat25":
                        els = np.exp(2 * hyp[0])
                        cond = (abs(float(xv)) + abs(float(kn[j]))) / els ** 3
                    else:
                        powv, els = np.exp(0.25 * hyp[1]), np.exp(2 * hyp[0] + 0.25 * hyp[1])
                        t1, t2 = float(xv) ** powv / els, float(kn[j]) ** powv / els
                        du = powv * t1 / float(xv)
                        cond = (t1 + t2) * (du * du + abs(powv * (powv - 1) * t1) / float(xv) ** 2)
                    bound = abs(float(want)) + cond
                    err = float(abs(_mp_of(got[i, j]) - want))
                    worst = max(worst, err / (E.EPS * bound))
                    assert err <= 64 * E.EPS * bound, (kind, xv, j, err, float(want))
    print("d2cov_dx2_ld against 80 digits: worst error %.3g eps_longdouble x bound" % worst)


def test_reference_second_derivative_against_central_differences_of_getmat_dx():
    """The model with short length scales and the terms of the first-derivative test
    (test_predict_grad_host.py), for the reason written there: the difference quotient of dB/dx_l in
    long double has its own round-off, 2 eps_ld bound / step."""
    import ob_oracle as O
    knots = knots_for(KINDS, 20)
    om = O.OuterMod()
    om.setcovfs(KINDS)
    om.hyp_set(np.array([-0.6, -0.5, 0.4, -0.5, -0.6, -0.5]))
    om.setknot(knots)
    terms = om.selectterms(40)
    x = special_rows(np.random.default_rng(7), 40, KINDS, knots)
    ref = D2.reference_d2_of(om, x)
    worst = 0.0
    for m in range(om.d):
        span = float(np.max(knots[m]) - np.min(knots[m]))
        step = 1e-7 * span
        xp, xm = x.copy(), x.copy()
        xp[:, m] += step
        xm[:, m] -= step
        rp, rm = X.reference_dx_of(om, xp), X.reference_dx_of(om, xm)
        den = (np.asarray(xp[:, m], dtype=ld) - np.asarray(xm[:, m], dtype=ld))[:, None]
        for l in range(om.d):
            Dp, bDp = rp.getmat_dx(terms, l)
            Dm, _ = rm.getmat_dx(terms, l)
            fd = (Dp - Dm) / den
            D, _ = ref.getmat_d2(terms, l, m)
            noise = np.max(E._f64(2 * E.EPS * bDp / np.abs(den)), axis=0)
            scale = float(np.max(np.abs(D)))
            keep = noise <= 0.5e-10 * scale
            assert keep.sum() >= 20, (l, m, int(keep.sum()))
            rel = float(np.max(np.abs(fd - D)[:, keep]) / np.max(np.abs(D[:, keep])))
            worst = max(worst, rel)
            assert rel < 1e-10, (l, m, rel)
    print("central differences of dB/dx_l by x_m against d2B: worst max-norm %.3g" % worst)


def test_normalised_algebra_in_long_double_equals_the_direct_sum():
    c = case()
    B, jv, hv = D2.hv_terms_norm(D2.norm_basis_of(c["om"], c["x"], ld), c["terms"], c["V"])
    w = {"B": E.worst_ratio(B, *c["ref"].getmat(c["terms"])), "jv": E.worst_ratio(jv, c["jvt"][0], c["jvt"][1]),
         "hv": E.worst_ratio(hv, c["hvt"][0], c["hvt"][1])}
    print("normalised algebra in long double: err/bound %s (eps_longdouble %.3g)" % (
        ", ".join("%s %.3g" % kv for kv in w.items()), E.EPS))
    assert max(w.values()) < 4 * E.EPS


def test_hessian_assembled_from_unit_directions_is_symmetric():
    c = case()
    om, x, terms, ref = c["om"], c["x"][:8], c["terms"], None
    ref = D2.reference_d2_of(om, x)
    nb = D2.norm_basis_of(om, x, np.float64)
    d = om.d
    H, bH = np.empty((8, len(terms), d, d)), np.empty((8, len(terms), d, d))
    for m in range(d):
        V = np.zeros((8, d))
        V[:, m] = 1.0
        H[:, :, :, m] = D2.hv_terms_norm(nb, terms, V)[2]
        T, bT, _ = ref.hv_terms(terms, V)
        bH[:, :, :, m] = bT
        for l in range(d):
            assert np.array_equal(T[:, :, l], ref.getmat_d2(terms, m, l)[0])      # the reference: exactly
    Cc = E.constant_from_oracle_ratio(D2.f64_ratio(ref, om, x, terms, np.ones((8, d))))
    asym = E.worst_ratio(H, H.transpose(0, 1, 3, 2), Cc * (bH + bH.transpose(0, 1, 3, 2)))
    print("float64 Hessian entries: asymmetry / (sum of the two tolerances) %.3g" % asym)
    assert asym < 1


def test_float64_restatement_sits_at_a_few_eps_of_the_bound():
    c = case()
    ratio = D2.f64_ratio(c["ref"], c["om"], c["x"], c["terms"], c["V"], (c["hvt"], c["jvt"]))
    print("float64 normalised restatement: err/bound %.3g" % ratio)
    assert ratio < 4e-15 and 8 * ratio < E.C_CAP


@pytest.mark.parametrize("name,p,kind", HCASES + [("wide", 0, "select")])
def test_constant_stays_below_the_cap_on_every_gpu_case(name, p, kind):
    """a condition of the GPU file: with C at the cap the instrument would no longer measure the
    reference's own form"""
    ratio = hparts(name, p, kind)["ratio"]
    print("%s p=%d %s: float64 normalised restatement err/bound %.3g, C = %.3g" % (name, p, kind, ratio, 8 * ratio))
    assert 8 * ratio < E.C_CAP


@pytest.mark.parametrize("mutate", ["kappa", "cross", "r2"])
def test_mutated_algebra_passes_a_flat_tolerance_and_fails_the_per_entry_one(mutate):
    """kappa_l - rho_l^2 replaced by kappa_l, the cross term r' dE dropped, r'' without 2 r' R'_0: each
    confined to the rows of V and the responses of scale 1e-3 (a fault of one block of rows and
    responses), where a max-norm test at 1e-6 cannot see it"""
    c = case()
    om, x, terms, V = c["om"], c["x"], c["terms"], c["V"]
    q = 7
    Theta = np.random.default_rng(3).standard_normal((len(terms), q)) * J.response_scales(q)[None, :]
    Cc = E.constant_from_oracle_ratio(D2.f64_ratio(c["ref"], om, x, terms, V, (c["hvt"], c["jvt"])))
    want, tol = D2.ref_hv(c["hvt"], Theta, Cc)
    good = D2.hv_terms_norm(D2.norm_basis_of(om, x, np.float64), terms, V)[2]
    bad = D2.hv_terms_norm(D2.norm_basis_of(om, x, np.float64, mutate if mutate == "r2" else None), terms, V,
                           mutate if mutate != "r2" else None)[2]
    hv_good = np.stack([good[:, :, l] @ Theta for l in range(om.d)], axis=1)
    hv_bad = hv_good.copy()
    rows = np.nonzero(J.response_scales(len(x)) == 1e-3)[0]
    rows = rows[np.any(V[rows], axis=1)]
    for l in range(om.d):
        hv_bad[rows, l, 0] = (bad[:, :, l] @ Theta)[rows, 0]
    assert E.worst_ratio(hv_good, want, tol) < 1
    assert E.maxnorm_relerr(hv_bad, want) < 1e-6
    r = E.ratio_map(hv_bad, want, tol)[rows][:, :, 0]
    print("mutation %s: %.3g x tolerance, %d of %d entries fail" % (mutate, r.max(), (r > 1).sum(), r.size))
    assert r.max() > 1e3


# ---- the library's host side ------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_by_both_libraries():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    testing = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"))
    for name in NEW:
        assert name in protos, name
        assert hasattr(_lib.lib, name), name
        assert hasattr(testing, name), name
    assert len(protos["obhip_predict_hvp_multi_dev"][1]) == 13
    assert len(protos["obhip_predict_hvp_multi"][1]) == 15
    assert len(protos["obhip_predict_hvp_layout"][1]) == 6
    assert _lib.lib.obhip_abi_version() == 5 and testing.obhip_abi_version() == 5    # purely additive


def test_python_names_are_exported():
    import outerbase_amd as ob
    for name in ("predict_hvp", "predict_hess"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert hasattr(ob.MultiFit, "hvp") and hasattr(ob.MultiFit, "predict_hess")


def _model():
    import outerbase_amd as ob
    kinds = ["mat25", "mat25pow", "mat25ang"]
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    return om, om.selectterms(40)


def test_argument_errors_return_before_any_device_call_and_write_nothing():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    om, terms = _model()
    t = ob.obmod._Terms(om, terms)
    inp = np.full(512, 0.5)
    outs = [np.full(512, -7.0) for _ in range(4)]
    a = inp.ctypes.data
    me, vj, jv, hv = (o.ctypes.data for o in outs)
    dev = lib.obhip_predict_hvp_multi_dev
    q, n = 2, 4
    assert dev(None, t._h, a, q, a, n, a, n, a, me, vj, jv, hv) == 1
    assert dev(om._h, None, a, q, a, n, a, n, a, me, vj, jv, hv) == 1
    assert dev(om._h, t._h, None, q, a, n, a, n, a, me, vj, jv, hv) == 1
    assert dev(om._h, t._h, a, q, None, n, a, n, a, me, vj, jv, hv) == 1           # no x
    assert dev(om._h, t._h, a, q, a, n, a, n, None, me, vj, jv, hv) == 1           # no V
    assert dev(om._h, t._h, a, 0, a, n, a, n, a, me, vj, jv, hv) == 1              # q = 0
    assert b"no response" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, q, a, n, a, n - 1, a, me, vj, jv, hv) == 1          # ldw below n
    assert b"leading dimension" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, q, a, (1 << 40) + 1, a, (1 << 40) + 1, a, me, vj, jv, hv) == 1
    assert b"2^40" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, q, a, n, a, n, a, me, vj, None, None) == 1          # neither jvp nor hvp
    assert b"neither" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, q, a, n, None, n, a, me, None, jv, hv) == 1         # hvp without W
    assert dev(om._h, t._h, a, q, a, n, None, n, a, me, vj, jv, None) == 1         # vjp without W
    assert b"need W" in lib.obhip_last_error()
    other = ob.outermod()                                                          # another dimension count
    ob.setcovfs(other, ["mat25"])
    ob.setknot(other, knots_for(["mat25"], 20))
    assert dev(other._h, t._h, a, q, a, n, a, n, a, me, vj, jv, hv) == 1
    assert dev(om._h, t._h, a, q, a, 0, a, 0, a, me, vj, jv, hv) == 0              # n = 0: a no-op
    host = lib.obhip_predict_hvp_multi
    assert host(None, t._h, a, q, a, n, n, a, n, a, n, me, vj, jv, hv) == 1
    assert host(om._h, t._h, a, q, a, n, n - 1, a, n, a, n, me, vj, jv, hv) == 1   # ldx below n
    assert host(om._h, t._h, a, q, a, n, n, a, n, a, n - 1, me, vj, jv, hv) == 1   # ldg below n
    assert host(om._h, t._h, a, q, a, n, n, a, n, a, n, me, vj, None, None) == 1
    assert host(om._h, t._h, a, q, a, 0, 0, a, 0, a, 0, me, vj, jv, hv) == 0
    assert lib.obhip_predict_hvp_layout(None, 1, None, None, None, None) == 1
    assert lib.obhip_predict_hvp_layout(t._h, 0, None, None, None, None) == 1
    assert all(np.all(o == -7.0) for o in outs)                                    # nothing was written
    with pytest.raises(ValueError):
        ob.predict_hvp(om, terms, np.zeros((40, 2)), np.full((2, 3), 0.5), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        ob.predict_hvp(om, terms, np.zeros((40, 2)), np.full((2, 3), 0.5), np.zeros((2, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        ob.predict_hess(om, terms, np.zeros((40, 2)), np.full((2, 3), 0.5))


def _layout(t, q):
    from outerbase_amd._lib import call
    mu, rows, lds, fused = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(-1)
    call("obhip_predict_hvp_layout", t._h, q, C.byref(mu), C.byref(rows), C.byref(lds), C.byref(fused))
    return mu.value, rows.value, lds.value, fused.value


def test_layout_of_the_headline_term_set_and_of_the_wide_one():
    import outerbase_amd as ob
    kinds = ["mat25"] * 20
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 40))
    terms = om.selectterms(4096)
    t = ob.obmod._Terms(om, terms)
    used = 1 + sum(len(np.unique(terms[:, l][terms[:, l] > 0])) for l in range(20))
    for q in (1, 16):
        mu, rows, lds, fused = _layout(t, q)
        print("headline d=20 p=4096 q=%d: Mu %d, tile rows %d, LDS %d bytes, fused %d" % (q, mu, rows, lds, fused))
        assert mu == used and rows == 32 and fused == 1 and lds <= 160 * 1024
        assert lds >= (3 * mu + 3 * 20) * 33 * 8
    from test_gpu_predict_grad import wide
    _, _, om_d, wterms, wused, _ = wide()
    mu, rows, lds, fused = _layout(ob.obmod._Terms(om_d, wterms), 1)
    print("wide d=40: Mu %d, LDS %d bytes, fused %d" % (mu, lds, fused))
    assert mu == wused == 198 and fused == 0 and lds <= 160 * 1024


def test_new_sources_are_in_the_makefile():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mk = open(os.path.join(root, "outerbase_amd", "csrc", "Makefile")).read()
    assert "kernels_predict_hvp.hip" in mk and "predict_hvp.cpp" in mk
    assert mk.count("device_d2.h") >= 2            # HDRS and the prerequisites of the .hip rule
