"""Host-side checks of the Sobol indices (no GPU): the pair formulas of tests/sobol_ref.py against a
brute-force ANOVA over the full tensor grid of nodes, the float64 restatement inside every tolerance,
three mutations the instrument must fail, the identities of the decomposition, and the library's host
side -- symbols, Python names, the Makefile, argument errors that return before any device call."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import extended_jac_ref as J
import extended_ref as E
import sobol_ref as S
from conftest import knots_for, make_pair, sample_x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ld = np.longdouble
NEW = {"obhip_sobol_layout": 3, "obhip_dim_moments_dev": 9, "obhip_sobol_workspace_bytes": 4, "obhip_sobol_dev": 9,
       "obhip_main_effect_dev": 8, "obhip_dim_moments": 9, "obhip_sobol": 7}
Q = 4
MIX5 = ["mat25", "mat25pow", "mat25ang", "mat25", "mat25"]


def reference_of(om_o, x):
    return E.ExtendedRef(om_o.kinds, [om_o.knots_of(k) for k in range(om_o.d)], om_o.hyp, om_o.rotmat, x)


@functools.lru_cache(maxsize=None)
def golden_model(name):
    """the model of tests/golden/<name>.npz as (oracle, device) pair, with its terms and rows"""
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    kinds, st = [str(k) for k in g["kinds"]], g["knotptst"]
    knots = [g["knotpt"][st[l]:st[l + 1]] for l in range(len(kinds))]
    om_o, om_d = make_pair(kinds, knots, hyp=g["hyp"])
    return dict(kinds=kinds, om_o=om_o, om_d=om_d, terms=np.ascontiguousarray(g["terms"]), x=g["x"])


@functools.lru_cache(maxsize=None)
def d5_model():
    knots = knots_for(MIX5, 20)
    rng = np.random.default_rng(55)
    nh = sum(E.NUMHYP[k] for k in MIX5)
    om_o, om_d = make_pair(MIX5, knots, hyp=rng.uniform(0.1, 0.4, nh) * rng.choice([-1.0, 1.0], nh))
    return dict(kinds=MIX5, om_o=om_o, om_d=om_d, terms=np.ascontiguousarray(om_o.selectterms(30)), x=None)


def some_zero_weights(rng, n, d):
    w = rng.uniform(0.2, 1.0, (n, d))
    w[rng.random((n, d)) < 0.2] = 0.0
    w[0] = 0.5                                           # every column keeps some mass
    return w


def theta_of(terms, q, seed):
    """coefficients that fall with the order of the term, those of the one-factor terms kept away from zero (so
    that every dimension has a main effect worth the name), columns scaled 1e-3 .. 1e3"""
    rng = np.random.default_rng(seed)
    order = (np.asarray(terms) > 0).sum(axis=1)
    th = rng.standard_normal((len(terms), q))
    main = rng.uniform(0.5, 1.5, th.shape) * rng.choice([-1.0, 1.0], th.shape)
    th = np.where((order == 1)[:, None], main, th)
    return th * (0.5 ** order)[:, None] * J.response_scales(q)[None, :]


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """nodes, weights, Theta, the long-double tables on the nodes and the brute-force ANOVA on their tensor grid"""
    if name == "mixed_d3":
        mdl, n, weights = golden_model("mixed_d3"), 12, None
    elif name == "mixed_d3 weighted":
        mdl, n, weights = golden_model("mixed_d3"), 12, True
    else:
        mdl, n, weights = d5_model(), 6, None
    rng = np.random.default_rng(len(name))
    kinds, terms = mdl["kinds"], mdl["terms"]
    d = len(kinds)
    nodes = sample_x(rng, n, kinds)
    w = some_zero_weights(rng, n, d) if weights else None
    Theta = theta_of(terms, Q, 3 + len(name))
    levels = S.levels_of(terms)
    ref = reference_of(mdl["om_o"], nodes)
    m, Cv = S.tables_from_bases([ref.getbase(l)[0] for l in range(d)], levels, w)
    rows, idx = S.grid_rows(nodes)
    gref = reference_of(mdl["om_o"], rows)
    brute = S.brute_force(gref, idx, n, terms, Theta, w)
    # the absolute sums the agreement is measured against: E[sum_k |theta_k B_k|] and its second moment
    B, _ = gref.getmat(terms)
    wn = S.normalised_weights(w, n, d)
    Wrow = np.prod(wn[idx, np.arange(d)[None, :]], axis=1)
    aB = np.abs(B) @ np.abs(np.asarray(Theta, dtype=ld))
    return dict(mdl=mdl, nodes=nodes, weights=w, Theta=Theta, terms=terms, levels=levels, ref=ref, m=m, Cv=Cv,
                brute=brute, abs1=Wrow @ aB, abs2=Wrow @ (aB * aB), rows=len(rows))


GRID_CASES = ["mixed_d3", "mixed_d3 weighted", "d5"]


# ---- the instrument ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRID_CASES)
def test_pair_formulas_agree_with_the_brute_force_anova(name):
    """two algebraically different routes in long double: they differ by rounding only.  K = grid rows + p^2 +
    3 d + 4 summands at most on either route; the absolute sums are those of the brute force, which bound the
    formulas' (|C| <= 2 E|psi psi'|, |A| <= E|psi psi'|)."""
    c = grid_case(name)
    p, d = c["terms"].shape
    f = S.formulas(c["terms"], c["Theta"], c["m"], c["Cv"])
    K = c["rows"] + p * p + 3 * d + 4
    worst = {}
    for key, absum in (("mu", c["abs1"]), ("V", c["abs2"]), ("V1", c["abs2"]), ("VT", c["abs2"])):
        err = np.abs(f[key] - c["brute"][key])
        worst[key] = float(np.max(err / (2 * K * E.EPS * absum)))
    print("%s (%d grid rows, p=%d): err / (2 K EPS abs sum) %s" % (
        name, c["rows"], p, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) < 1


@pytest.mark.parametrize("name", GRID_CASES)
def test_no_index_under_test_is_pure_cancellation(name):
    c = grid_case(name)
    share = E._f64(c["brute"]["V1"] / c["brute"]["V"][None, :])
    print("%s: smallest V1_l / V %.3g" % (name, share.min()))
    assert share.min() >= 1e-3


@pytest.mark.parametrize("name", GRID_CASES)
def test_identities_of_the_decomposition(name):
    c = grid_case(name)
    f = S.formulas(c["terms"], c["Theta"], c["m"], c["Cv"])
    slack = 4 * E.EPS * (len(c["terms"]) ** 2) * E._f64(c["abs2"])[None, :]
    assert np.all(f["V1"] >= 0) and np.all(f["V1"] <= f["VT"] + slack) and np.all(f["VT"] <= f["V"][None, :] + slack)
    assert np.all(E._f64(f["V1"].sum(axis=0)) <= E._f64(f["V"] + slack[0]))


def test_one_dimension_has_no_interactions():
    kinds = ["mat25"]
    om_o, _ = make_pair(kinds, knots_for(kinds, 20))
    terms = np.arange(6, dtype=np.int64)[:, None]
    nodes = sample_x(np.random.default_rng(1), 9, kinds)
    ref = reference_of(om_o, nodes)
    m, Cv = S.tables_from_bases([ref.getbase(0)[0]], S.levels_of(terms), None)
    f = S.formulas(terms, theta_of(terms, 3, 2), m, Cv)
    tol = E._f64(f["tol_V"])
    assert np.all(np.abs(E._f64(f["V1"][0] - f["V"])) <= tol) and np.all(np.abs(E._f64(f["VT"][0] - f["V"])) <= tol)


def _inside(got, f):
    return {k: E.worst_ratio(got[k], f[k], f["tol_" + k]) for k in ("mu", "V", "V1", "VT")}


@pytest.mark.parametrize("name", GRID_CASES)
def test_float64_restatement_stays_inside_every_tolerance(name):
    import ob_oracle as O
    c = grid_case(name)
    mdl, levels, d = c["mdl"], c["levels"], len(c["levels"])
    # stage 1: tables from the float64 oracle's getbase, two passes in float64
    ratio = S.oracle_getbase_ratio(c["ref"], mdl["om_o"], c["nodes"], levels)
    Cc = E.constant_from_oracle_ratio(ratio)
    (m, Cv), (tol_m, tol_C) = S.ref_tables(c["ref"], levels, c["weights"], Cc)
    b = O.OuterBase(mdl["om_o"], c["nodes"])
    m64, C64 = S.tables_from_bases([b.getbase(l + 1) for l in range(d)], levels, c["weights"], dtype=np.float64)
    r1 = max(max(E.worst_ratio(m64[l], m[l], tol_m[l]), E.worst_ratio(C64[l], Cv[l], tol_C[l])) for l in range(d))
    # stage 2: the same float64 tables on both sides
    f = S.formulas(c["terms"], c["Theta"], m64, C64)
    r2 = _inside(S.formulas(c["terms"], c["Theta"], m64, C64, dtype=np.float64), f)
    # and through upper-triangular tiles of 16 terms, the order a tiled kernel sums in
    r3 = _inside(S.formulas(c["terms"], c["Theta"], m64, C64, dtype=np.float64,
                            pair_weights=S.tile_weights(len(c["terms"]), 16)), f)
    print("%s: oracle getbase ratio %.3g; float64 err / tolerance: tables %.3g, formulas %s, tiled %s" % (
        name, ratio, r1, ", ".join("%s %.3g" % kv for kv in r2.items()), ", ".join("%s %.3g" % kv for kv in r3.items())))
    assert r1 < 1 and max(r2.values()) < 1 and max(r3.values()) < 1


def test_the_instrument_fails_three_mutations():
    c = grid_case("mixed_d3")
    terms, Theta, p = c["terms"], c["Theta"], len(c["terms"])
    m64, C64 = S.pack_tables(c["m"], c["Cv"])
    m64, C64 = S.unpack_tables(m64, C64, c["levels"])
    f = S.formulas(terms, Theta, m64, C64)
    tile = 16
    I = np.arange(p) // tile

    def run(W, Th=Theta):
        return _inside(S.formulas(terms, Th, m64, C64, dtype=np.float64, pair_weights=W), f)
    good = run(S.tile_weights(p, tile))
    assert max(good.values()) < 1
    W = S.tile_weights(p, tile)
    W[np.ix_(I == 1, I == 1)] = 2.0                      # a diagonal tile counted twice
    twice = run(W)
    W = S.tile_weights(p, tile)
    W[np.ix_(I == 0, I == 2)] = 1.0                      # an off-diagonal tile counted once
    once = run(W)
    print("diagonal tile twice: %s; off-diagonal tile once: %s" % (twice, once))
    assert twice["V"] > 1 and twice["VT"] > 1 and once["V"] > 1 and once["VT"] > 1
    for shift in (1, -1):                                # response j read from column j +- 1
        rolled = run(S.tile_weights(p, tile), np.roll(Theta, shift, axis=1))
        print("columns shifted by %+d: %s" % (shift, rolled))
        assert min(rolled.values()) > 1


# ---- the library's host side ---------------------------------------------------------------------------
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


def test_python_names_and_makefile():
    import outerbase_amd as ob
    for name in ("input_moments", "uniform_nodes", "sobol", "main_effects", "InputMoments", "SobolResult"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert callable(ob.MultiFit.sobol) and callable(ob.MultiFit.main_effects)
    mk = open(os.path.join(ROOT, "outerbase_amd", "csrc", "Makefile")).read()
    assert "kernels_sobol.hip" in mk and "sobol.cpp" in mk


def test_gauss_legendre_weights_sum_to_the_interval():
    import outerbase_amd as ob
    lo, hi = np.array([0.0, -1.0, 2.0]), np.array([1.0, 3.0, 2.5])
    nodes, w = ob.uniform_nodes(lo, hi, order=17)
    assert nodes.shape == w.shape == (17, 3)
    assert np.all(nodes > lo[None, :]) and np.all(nodes < hi[None, :]) and np.all(w > 0)
    assert np.allclose(w.sum(axis=0), hi - lo, rtol=1e-14, atol=0)
    assert np.allclose((w * nodes ** 3).sum(axis=0), (hi ** 4 - lo ** 4) / 4, rtol=1e-13)   # exact to degree 33
    with pytest.raises(ValueError):
        ob.uniform_nodes([0.0, 1.0], [1.0, 1.0])
    with pytest.raises(ValueError):
        ob.uniform_nodes([0.0], [1.0], order=0)


def test_argument_errors_return_before_any_device_call():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    mdl = golden_model("mixed_d3")
    om, t = mdl["om_d"], ob.obmod._Terms(mdl["om_d"], mdl["terms"])
    buf = (C.c_double * 4096)()
    a = C.cast(buf, C.c_void_p)
    nm, nc, wsb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert lib.obhip_sobol_layout(None, C.byref(nm), C.byref(nc)) == 1
    assert lib.obhip_sobol_layout(t._h, C.byref(nm), C.byref(nc)) == 0
    levels = S.levels_of(mdl["terms"])
    assert nm.value == levels.sum() and nc.value == (levels ** 2).sum()
    mom = lib.obhip_dim_moments_dev
    assert mom(None, t._h, a, 4, 4, None, 0, a, a) == 1
    assert mom(om._h, None, a, 4, 4, None, 0, a, a) == 1
    assert mom(om._h, t._h, None, 4, 4, None, 0, a, a) == 1
    assert mom(om._h, t._h, a, 4, 4, None, 0, None, a) == 1
    assert mom(om._h, t._h, a, 4, 4, None, 0, a, None) == 1
    assert mom(om._h, t._h, a, 0, 0, None, 0, a, a) == 1                 # no nodes: no measure
    assert b"no measure" in lib.obhip_last_error()
    assert mom(om._h, t._h, a, 4, 3, None, 0, a, a) == 1                 # ldx below n
    assert mom(om._h, t._h, a, 4, 4, a, 3, a, a) == 1                    # ldw below n
    assert mom(om._h, t._h, a, (1 << 40) + 1, (1 << 40) + 1, None, 0, a, a) == 1
    hostmom = lib.obhip_dim_moments
    assert hostmom(None, t._h, a, 4, 4, None, 0, a, a) == 1
    assert hostmom(om._h, t._h, a, 0, 0, None, 0, a, a) == 1
    assert hostmom(om._h, t._h, a, 4, 3, None, 0, a, a) == 1
    assert hostmom(om._h, t._h, a, 4, 4, a, 3, a, a) == 1
    assert hostmom(om._h, t._h, a, 4, 4, None, 0, None, a) == 1
    wsf = lib.obhip_sobol_workspace_bytes
    assert wsf(40, 3, 2, None) == 1 and wsf(0, 3, 2, C.byref(wsb)) == 1 and wsf(40, 0, 2, C.byref(wsb)) == 1
    assert wsf(40, 256, 2, C.byref(wsb)) == 1 and wsf(40, 3, 0, C.byref(wsb)) == 1
    assert wsf(40, 3, 2, C.byref(wsb)) == 0 and wsb.value > 0
    sob = lib.obhip_sobol_dev
    assert sob(None, a, 2, a, a, a, a, a, wsb.value) == 1
    assert sob(t._h, None, 2, a, a, a, a, a, wsb.value) == 1
    assert sob(t._h, a, 2, None, a, a, a, a, wsb.value) == 1
    assert sob(t._h, a, 2, a, None, a, a, a, wsb.value) == 1
    assert sob(t._h, a, 2, a, a, None, a, a, wsb.value) == 1
    assert sob(t._h, a, 2, a, a, a, a, None, wsb.value) == 1
    assert sob(t._h, a, 0, a, a, a, a, a, wsb.value) == 1                # q = 0
    assert sob(t._h, a, 2, a, a, a, a, a, wsb.value - 1) == 1            # workspace too small
    assert b"workspace" in lib.obhip_last_error()
    hostsob = lib.obhip_sobol
    assert hostsob(None, a, 2, a, a, a, None) == 1 and hostsob(t._h, a, 0, a, a, a, None) == 1
    assert hostsob(t._h, None, 2, a, a, a, None) == 1 and hostsob(t._h, a, 2, a, a, None, None) == 1
    me = lib.obhip_main_effect_dev
    assert me(None, t._h, 0, a, 2, a, 4, a) == 1
    assert me(om._h, None, 0, a, 2, a, 4, a) == 1
    assert me(om._h, t._h, 0, None, 2, a, 4, a) == 1
    assert me(om._h, t._h, 0, a, 2, None, 4, a) == 1
    assert me(om._h, t._h, 0, a, 2, a, 4, None) == 1
    assert me(om._h, t._h, 3, a, 2, a, 4, a) == 1                        # dimension out of range
    assert me(om._h, t._h, 0, a, 0, a, 4, a) == 1
    assert me(om._h, t._h, 0, a, 2, a, 0, a) == 0                        # no grid points: a no-op
    # terms of another model's dimension count
    other = ob.outermod()
    ob.setcovfs(other, ["mat25"])
    ob.setknot(other, knots_for(["mat25"], 20))
    assert mom(other._h, t._h, a, 4, 4, None, 0, a, a) == 1
    assert me(other._h, t._h, 0, a, 2, a, 4, a) == 1
    # a level beyond 255
    kinds = ["mat25"]
    wide = ob.outermod()
    ob.setcovfs(wide, kinds)
    ob.setknot(wide, [np.linspace(0.001, 0.999, 300)])
    tw = ob.obmod._Terms(wide, np.array([[0], [256]], dtype=np.int64))
    assert lib.obhip_sobol_layout(tw._h, C.byref(nm), C.byref(nc)) == 1
    assert b"255" in lib.obhip_last_error()
    # tables beyond the LDS of a workgroup: 3 x 8 x 2 x 60^2 bytes > 160 KB
    kinds = ["mat25", "mat25"]
    big = ob.outermod()
    ob.setcovfs(big, kinds)
    ob.setknot(big, [np.linspace(0.001, 0.999, 64)] * 2)
    tb = ob.obmod._Terms(big, np.array([[0, 0], [59, 59]], dtype=np.int64))
    assert lib.obhip_sobol_layout(tb._h, C.byref(nm), C.byref(nc)) == 1
    assert b"LDS" in lib.obhip_last_error()


def test_shape_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    om, terms = mdl["om_d"], mdl["terms"]
    with pytest.raises(ValueError):
        ob.input_moments(om, terms, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        ob.input_moments(om, terms, np.zeros((0, 3)))
    with pytest.raises(ValueError):
        ob.input_moments(om, terms, np.full((4, 3), 0.5), weights=np.ones((3, 3)))
