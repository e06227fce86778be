"""Host-side checks of the input-gradient predictor (no GPU): the long-double derivative reference of
tests/extended_dx_ref.py against 50-digit arithmetic and against central differences of the value
reference, the float64 restatement at a few eps64 of the bound, a mutation the flat tolerance lets
through, and the library's host side -- symbols, Python names, argument errors that return before
any device call, the dimension views of a term set."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import extended_dx_ref as X
import extended_ref as E
from conftest import knots_for, sample_x

ld = np.longdouble
NEW = ["obhip_predict_grad_dev", "obhip_predict_grad", "obhip_predictor_gradmean", "obhip_predictor_d",
       "obhip_terms_dimview"]
KINDS = ["mat25", "mat25pow", "mat25ang", "mat25"]
HYP = np.array([0.3, -0.2, 0.4, 0.25, -0.3, -0.15])


def special_rows(rng, n, kinds, knots):
    """sample_x rows; row 0 sits exactly on a knot in every dimension, row 1 has x = 0.02 in the
    mat25pow dimensions"""
    x = sample_x(rng, n, kinds)
    for k, kind in enumerate(kinds):
        x[0, k] = knots[k][len(knots[k]) // 3]
        if kind == "mat25pow" and n > 1:
            x[1, k] = 0.02
    return x


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
    ref = X.reference_dx_of(om, x)
    return dict(om=om, knots=knots, terms=terms, x=x, ref=ref)


# ---- the instrument -------------------------------------------------------------------------------
def _mp_cov(kind, xv, kj, hyp):
    import mpmath as mp
    if kind == "mat25ang":
        hs = (mp.sin(xv) - mp.sin(kj)) / mp.exp(2 * hyp[0])
        hc = (mp.cos(xv) - mp.cos(kj)) / mp.exp(2 * hyp[1])
        h = mp.sqrt(hs * hs + hc * hc)
    elif kind == "mat25":
        h = abs(xv - kj) / mp.exp(2 * hyp[0])
    else:
        powv = mp.exp(hyp[1] / 4)
        h = abs(mp.power(xv, powv) - mp.power(kj, powv)) / mp.exp(2 * hyp[0] + hyp[1] / 4)
    return (1 + h + h * h / 3) * mp.exp(-h)


def _conditioning(kind, xv, kj, hyp):
    if kind == "mat25ang":
        slope = 1.0 / min(np.exp(2 * hyp[0]), np.exp(2 * hyp[1]))
        return 2.0 * slope * slope / 3
    if kind == "mat25":
        els = np.exp(2 * hyp[0])
        return (abs(xv) + abs(kj)) / els / els / 3
    powv, els = np.exp(0.25 * hyp[1]), np.exp(2 * hyp[0] + 0.25 * hyp[1])
    t1, t2 = xv ** powv / els, kj ** powv / els
    return (t1 + t2) * (powv * t1 / xv) / 3


def test_dcov_dx_against_50_digit_differentiation():
    mp = pytest.importorskip("mpmath")
    from test_extended_ref import _mp_of
    kn = knots_for(["mat25"], 20)[0]
    worst = 0.0
    with mp.workdps(50):
        for kind, hyp, xs in (("mat25", [0.3], [kn[4], 0.37, 0.911]),
                              ("mat25pow", [-0.2, 0.4], [0.02, kn[7], 0.55]),
                              ("mat25ang", [0.25, -0.3], [kn[3], 2.9, 5.7])):
            got = X.dcov_dx_ld(kind, np.array(xs), kn, np.array(hyp))
            mh = [mp.mpf(float(h)) for h in hyp]
            for i, xv in enumerate(xs):
                for j in (0, 3, 4, 7, 12, 19):
                    kj = mp.mpf(float(kn[j]))
                    if float(xv) == float(kn[j]):
                        want = mp.mpf(0)         # the kernel's maximum (mp.diff would straddle |.|)
                    else:
                        want = mp.diff(lambda z: _mp_cov(kind, z, kj, mh), mp.mpf(float(xv)), h=mp.mpf(10) ** -20)
                    # first-order bound of one entry: its own magnitude plus the conditioning of h, a
                    # difference of two rounded transforms: |d2k/dh2| <= 1/3 times their magnitudes,
                    # times du/dx once more
                    bound = abs(float(want)) + _conditioning(kind, float(xv), float(kn[j]), hyp)
                    err = float(abs(_mp_of(got[i, j]) - want))
                    worst = max(worst, err / (E.EPS * bound))
                    assert err <= 64 * E.EPS * bound, (kind, xv, j, err, float(want))
    print("dcov_dx_ld against 50 digits: worst error %.3g eps_longdouble x bound" % worst)


def test_reference_derivative_against_central_differences_of_getmat():
    """A central difference of B in long double has its own round-off, 2 eps_ld bB / step per entry: at
    step 1e-7 that passes 1e-10 wherever a column cancels more than four digits (bB / |B| > 1e4: the
    higher levels, and every level once the length scales are long).  The comparison is therefore
    made on a model with short length scales and on the terms whose difference quotient is known to
    better than half the allowance; the other half is for the truncation term, step^2 / 6 times
    the third derivative."""
    import ob_oracle as O
    knots = knots_for(KINDS, 20)
    om = O.OuterMod()
    om.setcovfs(KINDS)
    om.hyp_set(np.array([-0.6, -0.5, 0.4, -0.5, -0.6, -0.5]))
    om.setknot(knots)
    terms = om.selectterms(40)
    x = special_rows(np.random.default_rng(7), 40, KINDS, knots)
    ref = X.reference_dx_of(om, x)
    worst = 0.0
    for l in range(om.d):
        span = float(np.max(knots[l]) - np.min(knots[l]))
        step = 1e-7 * span
        # exact float64 rows on both sides: the step actually taken is (x + step) - (x - step)
        xp, xm = x.copy(), x.copy()
        xp[:, l] += step
        xm[:, l] -= step
        Bp, bBp = E.ExtendedRef(om.kinds, knots, om.hyp, om.rotmat, xp).getmat(terms)
        Bm, _ = E.ExtendedRef(om.kinds, knots, om.hyp, om.rotmat, xm).getmat(terms)
        den = (np.asarray(xp[:, l], dtype=ld) - np.asarray(xm[:, l], dtype=ld))[:, None]
        fd = (Bp - Bm) / den
        dB, _ = ref.getmat_dx(terms, l)
        noise = np.max(E._f64(2 * E.EPS * bBp / np.abs(den)), axis=0)
        scale = float(np.max(np.abs(dB)))
        keep = noise <= 0.5e-10 * scale
        assert keep.sum() >= 25 and np.any(terms[keep, l] > 0), (l, int(keep.sum()))
        rel = float(np.max(np.abs(fd - dB)[:, keep]) / np.max(np.abs(dB[:, keep])))
        worst = max(worst, rel)
        print("dimension %d (%s): central difference against dB/dx on %d of %d terms, max-norm %.3g"
              % (l, om.kinds[l], keep.sum(), len(terms), rel))
        assert rel < 1e-10
    print("worst %.3g" % worst)


def test_float64_restatement_sits_at_a_few_eps_of_the_bound():
    c = case()
    ratio = X.f64_ratio(c["ref"], c["om"], c["x"], c["terms"])
    print("float64 restatement: err/bound %.3g" % ratio)
    assert ratio < 2e-15


def test_mutated_derivative_column_passes_the_flat_tolerance_and_fails_the_per_entry_one():
    c = case()
    om, x, terms, ref = c["om"], c["x"], c["terms"], c["ref"]
    C_ = E.constant_from_oracle_ratio(X.f64_ratio(ref, om, x, terms))
    _, dB64 = X.dB_f64_of(om, x, terms)
    dB, bdB = ref.getmat_dx(terms, 1)
    tol = C_ * np.asarray(bdB, dtype=np.float64)
    assert E.worst_ratio(dB64[:, :, 1], dB, tol) < 1
    dm = dB64[:, :, 1].copy()
    dm[:, 5] *= 1 + 1e-9
    assert E.maxnorm_relerr(dm, dB) < 1e-6
    r = E.ratio_map(dm, dB, tol)[:, 5]
    print("derivative column x (1 + 1e-9): %.3g x tolerance, %d of %d rows fail" % (r.max(), (r > 1).sum(), len(r)))
    assert r.max() > 1


def test_gradient_sums_agree_with_their_definition():
    """ref_grad_mean / ref_grad_var are the sums over the terms of dB and 2 B dB"""
    c = case()
    ref, terms = c["ref"], c["terms"]
    rng = np.random.default_rng(3)
    th, cv = rng.standard_normal(len(terms)), rng.random(len(terms))
    gm, tm = ref.ref_grad_mean(terms, th, 1e-15)
    gv, tv = ref.ref_grad_var(terms, cv, 1e-15)
    assert gm.shape == tm.shape == gv.shape == tv.shape == (c["x"].shape[0], 4)
    assert np.all(tm > 0) and np.all(tv > 0)
    B, _ = ref.getmat(terms)
    for l in range(4):
        dB, _ = ref.getmat_dx(terms, l)
        assert np.array_equal(gm[:, l], dB @ np.asarray(th, dtype=ld))
        assert np.array_equal(gv[:, l], 2 * ((B * dB) @ np.asarray(cv, dtype=ld)))


# ---- the library's host side ------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_by_both_libraries():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    testing = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"))
    for name in NEW:
        assert name in protos, name
        assert hasattr(_lib.lib, name), name
        assert hasattr(testing, name), name
    assert len(protos["obhip_predict_grad_dev"][1]) == 11
    assert len(protos["obhip_predict_grad"][1]) == 13
    assert len(protos["obhip_predictor_gradmean"][1]) == 2
    assert len(protos["obhip_terms_dimview"][1]) == 4
    assert _lib.lib.obhip_abi_version() == 5 and testing.obhip_abi_version() == 5    # purely additive


def test_python_names_are_exported():
    import outerbase_amd as ob
    for name in ("predict_grad", "obpred_grad", "term_dim_views"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert hasattr(ob.MultiFit, "predict_grad") and hasattr(ob.predictor, "gradmean")


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
    dev = lib.obhip_predict_grad_dev
    assert dev(None, t._h, a, a, 4, a, a, None, 0.0, None, None) == 1
    assert dev(om._h, None, a, a, 4, a, a, None, 0.0, None, None) == 1
    assert dev(om._h, t._h, None, a, 4, a, a, None, 0.0, None, None) == 1
    assert dev(om._h, t._h, a, a, 4, a, None, None, 0.0, None, None) == 1          # no grad
    assert dev(om._h, t._h, a, a, 4, a, a, None, 0.0, None, a) == 1                # gradvar without coeffvar
    assert b"gradvar needs coeffvar" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, a, (1 << 40) + 1, a, a, None, 0.0, None, None) == 1  # beyond the entry's rows
    assert b"2^40" in lib.obhip_last_error()
    assert dev(om._h, t._h, a, a, 0, None, a, None, 0.0, None, None) == 0          # n = 0: a no-op
    host = lib.obhip_predict_grad
    assert host(None, t._h, a, a, 4, 4, a, a, 4, None, 0.0, None, None) == 1
    assert host(om._h, t._h, a, a, 4, 4, a, None, 4, None, 0.0, None, None) == 1
    assert host(om._h, t._h, a, a, 4, 3, a, a, 4, None, 0.0, None, None) == 1      # ldx below n
    assert host(om._h, t._h, a, a, 4, 4, a, a, 3, None, 0.0, None, None) == 1      # ldg below n
    assert host(om._h, t._h, a, a, 4, 4, a, a, 4, None, 0.0, None, a) == 1
    assert host(om._h, t._h, a, a, 0, 0, None, a, 0, None, 0.0, None, None) == 0
    assert lib.obhip_predictor_gradmean(None, a) == 1
    assert lib.obhip_predictor_d(None, None) == 1
    cnt = C.c_uint64(0)
    assert lib.obhip_terms_dimview(None, 0, C.byref(cnt), None) == 1
    assert lib.obhip_terms_dimview(t._h, 3, C.byref(cnt), None) == 1               # d = 3: dimensions 0 .. 2
    assert lib.obhip_terms_dimview(t._h, 0, None, None) == 1
    # terms of another model's dimension count
    other = ob.outermod()
    ob.setcovfs(other, ["mat25"])
    ob.setknot(other, knots_for(["mat25"], 20))
    assert dev(other._h, t._h, a, a, 4, a, a, None, 0.0, None, None) == 1
    with pytest.raises(ValueError):
        ob.predict_grad(om, terms, np.zeros(3), np.full((2, 3), 0.5))
    with pytest.raises(ValueError):
        ob.predict_grad(om, terms, np.zeros(40), np.full((2, 2), 0.5))
    with pytest.raises(ValueError):
        ob.predict_grad(om, terms, np.zeros(40), np.full((2, 3), 0.5), coeffvar=np.ones(2))


def test_dimension_views_of_a_term_set():
    import outerbase_amd as ob
    om, terms = _model()
    terms = np.vstack([np.zeros((1, 3), dtype=terms.dtype), terms[terms.sum(1) > 0]])   # constant term first
    views = ob.term_dim_views(om, terms)
    assert len(views) == 3
    pairs = [(int(k), l) for l, v in enumerate(views) for k in v]
    want = [(int(k), int(l)) for k, l in zip(*np.nonzero(terms > 0))]
    assert len(pairs) == len(set(pairs)) and sorted(pairs) == sorted(want)      # every pair exactly once
    assert all(0 not in v for v in views)                                       # the constant term: nowhere
    assert all(np.all(np.diff(v) > 0) for v in views)                           # in term order
    again = ob.term_dim_views(om, terms)                                        # a second build: the same
    assert all(np.array_equal(a, b) for a, b in zip(views, again))
    only_constant = ob.term_dim_views(om, np.zeros((1, 3), dtype=np.int64))
    assert [len(v) for v in only_constant] == [0, 0, 0]


def test_new_sources_are_in_the_makefile():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mk = open(os.path.join(root, "outerbase_amd", "csrc", "Makefile")).read()
    assert "kernels_predict_dx.hip" in mk and "predict_dx.cpp" in mk and "device_dx.h" in mk
