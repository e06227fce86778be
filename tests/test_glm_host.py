"""Host-side checks of the GLM fit (no GPU): the reference of tests/glm_ref.py in float64 against its refined
long-double run on the six cases the GPU tests use -- iteration and halving counts, the distance of every
Newton decrement from its threshold -- and the library's host side: symbols, Python names, argument errors
before any device call, OBHIP_ERR_NO_DEVICE from the device entries."""
import ctypes as C
import os

import numpy as np
import pytest

import glm_ref as R
from conftest import knots_for

NEW = {"obhip_glm_workspace_bytes": 3, "obhip_glm_rows_dev": 15, "obhip_fit_glm_dev": 18, "obhip_predict_glm_dev": 12,
       "obhip_fit_glm": 15, "obhip_predict_glm": 13}


# ---- the instrument -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,rho", R.SIZES)
@pytest.mark.parametrize("family", [R.GAUSSIAN, R.BINOMIAL, R.POISSON])
def test_float64_reference_against_the_long_double_one(family, n, p, rho):
    """Both runs stop after the same iterations and halvings (Gaussian 2 / 0, binomial 5-6 / 0, Poisson
    6 / 2: its first step from theta = 0 overshoots), no decrement within a factor 100 of its threshold (the
    two arithmetics could otherwise stop an iteration apart, a gap of 1e-10 that is stopping, not rounding),
    and then eta and theta agree to a few 1e-15 of their largest entry."""
    c = R.cpu_case(family, n, p, rho)
    a, b = c["r64"], c["rl"]
    de, dt = R.relerr(a["eta"], b["eta"]), R.relerr(a["theta"], b["theta"])
    dist = min(R.threshold_distance(a), R.threshold_distance(b))
    print("%s n=%d p=%d rho=%g: iterations %d / %d, halvings %d / %d, converged %s / %s, dec float64 %s, long double "
          "%s, nearest dec / threshold factor %.3g, eta %.3g theta %.3g of the largest entry, F %.17g, deviance %.17g"
          % (R.FAMILY_NAMES[family], n, p, rho, a["iterations"], b["iterations"], a["halvings"], b["halvings"],
             a["converged"], b["converged"], ["%.3g" % d for d in a["decs"]], ["%.3g" % d for d in b["decs"]], dist,
             de, dt, b["F"], b["deviance"]))
    assert a["converged"] and b["converged"]
    assert (a["iterations"], a["halvings"]) == (b["iterations"], b["halvings"])
    if family == R.BINOMIAL:
        assert a["iterations"] in (5, 6) and a["halvings"] == 0
    else:
        assert (a["iterations"], a["halvings"]) == R.EXPECTED[family]
    assert dist >= 100.0
    assert de <= 1e-14 and dt <= 1e-14


def test_row_pass_formulas_at_the_edges():
    """the overflow-free forms at |eta| = 40, 745, 800: mu in [0, 1], w = 0 gives u = 0, the Poisson row at
    eta = 800 is counted and left out of the sums, and the float64 forms agree with the long-double ones"""
    eta = np.array([0.0, 40.0, -40.0, 745.0, -745.0, 709.0, 800.0, -800.0, 1.5])
    y = np.array([0.0, 1.0, 0.25, 1.0, 0.0, 0.5, 1.0, 0.0, 0.75])
    a = np.array([1.0, 2.0, 3.0, 1.0, 5.0, 1.0, 2.0, 1.0, 4.0])
    rb, rbl = R.rows(R.BINOMIAL, eta, y, a), R.rows(R.BINOMIAL, eta, y, a, dtype=R.ld)
    assert np.all((rb["mu"] >= 0) & (rb["mu"] <= 1)) and rb["sums"][2] == 0
    assert rb["w"][6] == 0.0 and rb["u"][6] == 0.0 and rb["w"][7] == 0.0 and rb["u"][7] == 0.0
    live = rb["w"] > 0
    # u = a (y - mu) / sqrt(w) against the magnitude of the terms it is the difference of (y = 1 at eta = 40
    # cancels every digit of y - mu in float64)
    # (|eta| <= 700: beyond that e = exp(-|eta|) is subnormal in float64 and w, u keep a digit or none)
    live &= np.abs(eta) <= 700
    den = (a * (np.abs(y) + rbl["mu"]))[live] / rbl["sw"][live]
    assert R.relerr(rb["mu"], rbl["mu"]) < 1e-15 and np.max(np.abs(rb["u"][live] - rbl["u"][live]) / den) < 1e-15
    rp = R.rows(R.POISSON, eta, np.round(10 * y), a)
    # (e^745 and e^800 overflow, e^709 does not)
    assert rp["sums"][2] == 2 and not rp["fin"][3] and not rp["fin"][6] and rp["fin"][5]
    assert np.isfinite(rp["sums"][0]) and rp["u"][3] == 0.0 and rp["u"][6] == 0.0 and rp["sw"][6] == 0.0
    assert rp["w"][7] == 0.0 and rp["u"][7] == 0.0
    rg = R.rows(R.GAUSSIAN, eta[:3], y[:3], a[:3], sigma=0.3)
    assert np.allclose(rg["sw"] * rg["u"], a[:3] * (y[:3] - eta[:3]) * np.exp(-0.6), rtol=1e-15)


@pytest.mark.parametrize("family", [R.GAUSSIAN, R.BINOMIAL, R.POISSON])
def test_the_kernels_row_arithmetic_on_the_host(family, tmp_path):
    """csrc/glm_row.h, the functions k_glm_rows and k_glm_response call per row, compiled with g++ under the
    address and undefined-behaviour sanitizers into a program of its own (tests/glm_rows_check.cpp) and compared
    with the long-double formulas on 4000 rows with the edge values among them: mu, sqrt(w) and a l relative to
    the entry, u and the log-likelihood relative to the magnitude of the terms they are the difference of --
    within eight times what the NumPy float64 restatement keeps on the rows with |eta| <= 700; the rows without
    weight and the rows left out of the sums are the same rows."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "glm_rows_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(root, "tests", "glm_rows_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(40 + family)
    n = 4000
    eta = 3.0 * rng.standard_normal(n)
    eta[:9] = [0.0, 40.0, -40.0, 745.0, -745.0, 709.0, 800.0, -800.0, 36.8]
    a = rng.uniform(0.5, 3.0, n)
    a[:9] = 1.0
    if family == R.BINOMIAL:
        m = rng.integers(1, 6, n)
        y = rng.integers(0, 6, n) % (m + 1) / m
    elif family == R.POISSON:
        y = rng.poisson(3.0, n).astype(np.float64)
    else:
        y = eta + rng.standard_normal(n)
    e2 = float(np.exp(-2 * R.SIGMA))
    text = "".join("%d %s %s %s %s\n" % (family, float(e).hex(), float(v).hex(), float(w).hex(), e2.hex())
                   for e, v, w in zip(eta, y, a))
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    got = np.array([[float.fromhex(v) for v in line.split()[:5]] + [float(line.split()[5])] for line in r.stdout.splitlines()])
    assert got.shape == (n, 6)
    r64, rl = R.rows(family, eta, y, a), R.rows(family, eta, y, a, dtype=R.ld)
    assert np.array_equal(got[:, 5] == 1.0, r64["fin"]) and np.array_equal(got[:, 1] == 0.0, r64["sw"] == 0.0)
    assert np.all(got[:, 2][r64["sw"] == 0.0] == 0.0) and np.all(np.isfinite(got[:, 1:3]))
    sel = (np.abs(eta) <= 700) & (r64["sw"] > 0)
    tiny = float(np.finfo(np.float64).tiny)
    uden = a * (np.abs(y) + np.abs(rl["mu"])) * (e2 if family == R.GAUSSIAN else 1.0) / np.where(sel, rl["sw"], 1)
    for j, key, den in ((0, "mu", np.abs(rl["mu"])), (1, "sw", rl["sw"]), (2, "u", uden), (3, "al", rl["mag"]),
                        (4, "mag", rl["mag"])):
        den = np.maximum(np.asarray(den, dtype=R.ld)[sel], tiny)
        e_c = float(np.max(np.abs(np.asarray(got[:, j][sel], dtype=R.ld) - rl[key][sel]) / den))
        e_np = float(np.max(np.abs(np.asarray(r64[key][sel], dtype=R.ld) - rl[key][sel]) / den))
        print("%s %s: error / entry glm_row.h %.3g, NumPy float64 %.3g" % (R.FAMILY_NAMES[family], key, e_c, e_np))
        assert e_c <= 8.0 * e_np


# ---- the library's host side ------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_by_both_libraries():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    testing = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"))
    for name, nargs in NEW.items():
        assert name in protos, name
        assert hasattr(_lib.lib, name) and hasattr(testing, name), name
        assert len(protos[name][1]) == nargs, name
    assert _lib.lib.obhip_abi_version() == 5 and testing.obhip_abi_version() == 5    # purely additive


def test_python_names_and_the_info_struct():
    import outerbase_amd as ob
    from outerbase_amd import glm
    for name in ("fit_glm", "GlmFit"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert hasattr(ob.GlmFit, "predict")
    # obhip_glm_info as the header lays it out: two ints, two uint64_t, three doubles
    assert C.sizeof(glm.GlmInfo) == 48 and glm.GlmInfo.iterations.offset == 8 and glm.GlmInfo.dec.offset == 24
    assert glm.FAMILIES == {"gaussian": 0, "binomial": 1, "poisson": 2}


def test_new_sources_are_in_the_makefile():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mk = open(os.path.join(root, "outerbase_amd", "csrc", "Makefile")).read()
    assert "kernels_glm.hip" in mk and "glm.cpp" in mk


def _model():
    import outerbase_amd as ob
    kinds = ["mat25", "mat25pow", "mat25ang"]
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    return om, om.selectterms(40)


def test_c_entries_refuse_bad_arguments_before_any_device_call():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    from outerbase_amd.glm import GlmInfo
    om, terms = _model()
    t = ob.obmod._Terms(om, terms)
    buf = (C.c_double * 4096)()
    a = C.cast(buf, C.c_void_p)
    nbytes = C.c_uint64(0)
    assert lib.obhip_glm_workspace_bytes(40, 1000, C.byref(nbytes)) == 0 and nbytes.value > 4 * 1024 * 8 + 3 * 40 * 8
    assert lib.obhip_glm_workspace_bytes(40, 1000, None) == 1 and lib.obhip_glm_workspace_bytes(0, 10, C.byref(nbytes)) == 1
    rows = lib.obhip_glm_rows_dev
    assert rows(7, 4, a, None, 0.0, a, None, None, 0.0, a, a, a, a, a, a) == 1 and b"family" in lib.obhip_last_error()
    assert rows(1, 4, a, None, 0.0, None, None, None, 0.0, a, a, a, a, a, a) == 1
    assert rows(1, 4, a, None, 0.0, a, None, None, 0.0, a, a, a, a, a, None) == 1
    assert rows(1, 0, a, None, 0.0, a, None, None, 0.0, a, a, a, a, a, a) == 1
    assert rows(1, 4, a, None, 0.0, a, None, None, 0.0, a, a, a, None, a, a) == 1 and b"go together" in lib.obhip_last_error()
    assert rows(1, 4, a, a, float("nan"), a, None, None, 0.0, a, None, None, None, None, a) == 1
    info = GlmInfo()
    fit = lib.obhip_fit_glm_dev
    assert fit(None, t._h, om._h, 1, a, None, None, 0.0, 6.0, 1e-8, 25, a, a, a, a, C.byref(info), a, 1 << 20) == 1
    assert lib.obhip_fit_glm(None, t._h, om._h, 1, a, None, None, 0.0, 6.0, 1e-8, 25, a, None, None, C.byref(info)) == 1
    pred = lib.obhip_predict_glm_dev
    assert pred(None, t._h, 1, a, a, 4, None, None, a, None, a, None) == 1
    assert pred(om._h, t._h, 3, a, a, 4, None, None, a, None, a, None) == 1 and b"family" in lib.obhip_last_error()
    assert pred(om._h, t._h, 1, a, a, 4, None, None, a, a, a, None) == 1 and b"coeffvar" in lib.obhip_last_error()
    assert pred(om._h, t._h, 1, a, None, 4, None, None, a, None, a, None) == 1
    hp = lib.obhip_predict_glm
    assert hp(om._h, t._h, 1, a, a, 0, 4, None, None, a, None, a, None) == 1
    assert hp(om._h, t._h, 1, a, a, 4, 3, None, None, a, None, a, None) == 1
    assert hp(om._h, t._h, 1, a, a, 4, 4, None, None, a, None, a, a) == 1 and b"coeffvar" in lib.obhip_last_error()
    if ob.device_count() == 0:
        # well-formed calls without a GPU: OBHIP_ERR_NO_DEVICE, nothing computed
        assert rows(1, 4, a, None, 0.0, a, None, None, 0.0, a, a, a, a, a, a) == 2
        assert rows(2, 4, a, a, 0.5, a, None, None, 0.0, None, None, None, None, None, a) == 2
        assert pred(om._h, t._h, 1, a, a, 4, None, None, a, None, a, None) == 2
        assert hp(om._h, t._h, 2, a, a, 4, 4, None, None, a, None, a, None) == 2


def test_python_argument_errors():
    import outerbase_amd as ob
    om, terms = _model()
    x = np.full((5, 3), 0.5)
    y = np.array([0.0, 1.0, 0.5, 0.25, 1.0])
    bad = [dict(family="probit"), dict(y=y[:4]), dict(y=np.array([0, 1, 0.5, 1.5, 1.0])), dict(y=-y, family="poisson"),
           dict(y=np.array([0, 1, np.nan, 0, 0.0]), family="gaussian"), dict(weights=np.ones(4)),
           dict(weights=np.array([1, 1, 0.0, 1, 1])), dict(weights=np.array([1, 1, np.inf, 1, 1])),
           dict(weights=-np.ones(5)), dict(offset=np.zeros(4)), dict(offset=np.full(5, np.nan)), dict(tol=-1.0),
           dict(tol=float("nan")), dict(maxit=0), dict(x=np.full((5, 2), 0.5)), dict(x=np.zeros((0, 3)), y=np.zeros(0))]
    for kw in bad:
        args = dict(x=x, y=y)
        args.update(kw)
        with pytest.raises(ValueError):
            ob.fit_glm(om, terms, **args)
    # a result object refuses bad prediction arguments before it touches the device, and n = 0 is empty
    from outerbase_amd.glm import GlmFit, GlmInfo
    fit = GlmFit(om, None, "binomial", np.zeros(40), np.ones(40), np.zeros(5), GlmInfo(), 0.0, 6.0)
    for kw in (dict(kind="mean"), dict(xnew=np.zeros((4, 2))), dict(offset=np.zeros(3)), dict(offset=np.full(4, np.inf))):
        args = dict(xnew=np.full((4, 3), 0.5))
        args.update(kw)
        with pytest.raises(ValueError):
            fit.predict(**args)
    assert fit.predict(np.zeros((0, 3))).shape == (0,)
    m, v = fit.predict(np.zeros((0, 3)), var=True, kind="link")
    assert m.shape == v.shape == (0,)
