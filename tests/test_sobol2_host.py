"""Host-side checks of the pairwise Sobol quantities (no GPU): the formulas of tests/sobol2_ref.py against a
brute-force ANOVA over the full tensor grid of nodes, the identities at d = 2, 3 and 5, the float64
restatement inside every tolerance, five mutations the instrument must fail, no tested value a pure
cancellation, and the library's host side -- symbols, Python names, argument errors before any device call."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import extended_jac_ref as J
import extended_ref as E
import sobol2_ref as S2
import sobol_ref as S
from conftest import knots_for
from test_sobol_host import golden_model, grid_case, reference_of

ld = np.longdouble
NEW = {"obhip_sobol2_layout": 3, "obhip_sobol2_workspace_bytes": 4, "obhip_sobol2_dev": 9,
       "obhip_interaction_effect_dev": 11, "obhip_sobol2": 7}
GRID_CASES = ["mixed_d3", "mixed_d3 weighted", "d5"]
# No tested V2 or VT2 is pure cancellation: sum |summands| / |value| stays below CANCEL_MAX, and the tolerance
# gamma_k . sum |summands| below DIGITS of the value -- a result inside its tolerance is right to six digits at
# least (gamma_{p^2} = 1.3e-10 at p = 1100, the largest case, leaves 7.5e3 of cancellation for that).
CANCEL_MAX = 1e5
DIGITS = 1e-6

# stage 2 on the GPU (test_gpu_sobol2.py) and its cancellation check here.  TW = 128 terms per tile, RC = 2
# responses per chunk, T = 5 dimensions per block of the output triangle (d = 5 | 6, 10 | 11: one more block),
# row offsets of 8 or 24 dimensions in registers (d = 8 | 9, 24 | 25).
PAIR2_CASES = [(1, 3, 1), (5, 1, 2), (127, 2, 2), (128, 8, 3), (129, 9, 5), (300, 5, 2), (300, 6, 3), (300, 10, 1),
               (300, 11, 2), (1100, 3, 3), (129, 24, 2), (127, 25, 3), (128, 40, 2), (300, 20, 5)]


@functools.lru_cache(maxsize=None)
def pair2_tables(p, d, q):
    """terms with 1 to 4 active dimensions drawn from a few hot ones (so that pairs interact), different level
    counts per dimension, random tables and coefficients; the references of sobol_ref and sobol2_ref"""
    rng = np.random.default_rng(2000 * p + 10 * d + q)
    levels = 2 + (np.arange(d) * 3 + rng.integers(0, 2, size=d)) % 5                     # 2 .. 6, neighbours differ
    levels[rng.integers(d)] = 9
    terms = np.zeros((p, d), dtype=np.int64)
    for k in range(1, p):
        dims = rng.choice(d, size=int(rng.integers(1, min(d, 4) + 1)), replace=False)
        terms[k, dims] = rng.integers(1, levels[dims])
    if p > 1:
        terms[p - 1] = levels - 1                                                        # every top level is used
    else:
        levels[:] = 1
    m, Cv = S.random_tables(rng, levels)
    Theta = rng.standard_normal((p, q)) * J.response_scales(q)[None, :]
    return dict(terms=terms, levels=levels, m=m, Cv=Cv, Theta=Theta, f=S.formulas(terms, Theta, m, Cv),
                f2=S2.formulas2(terms, Theta, m, Cv))


@functools.lru_cache(maxsize=None)
def grid_case2(name):
    c = grid_case(name)
    n = len(c["nodes"])
    rows, _ = S.grid_rows(c["nodes"])
    gref = reference_of(c["mdl"]["om_o"], rows)
    return dict(c, brute2=S2.brute_force2(gref, n, c["terms"], c["Theta"], c["weights"]),
                f2=S2.formulas2(c["terms"], c["Theta"], c["m"], c["Cv"]))


# ---- the instrument ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRID_CASES)
def test_pair_formulas_agree_with_the_brute_force_anova(name):
    """two algebraically different routes in long double: they differ by rounding only.  K = grid rows + p^2 +
    3 d + 4 summands at most on either route.  The scale is the brute force's: with a = E[(sum_k |theta_k B_k|)^2]
    (test_sobol_host's abs2), |h| <= |f| + E_i|f| + E_j|f| + E_ij|f| gives sum |summands| of E[h^2] <= 16 a by
    Jensen, and Var E[f | x_i, x_j] - V1_i - V1_j has three parts of at most a each: 16 a for both."""
    c = grid_case2(name)
    p, d = c["terms"].shape
    f, f2, b, b2 = S.formulas(c["terms"], c["Theta"], c["m"], c["Cv"]), c["f2"], c["brute"], c["brute2"]
    K = c["rows"] + p * p + 3 * d + 4
    scale = 2 * K * E.EPS * 16 * c["abs2"]
    i, j = f2["pairs"][:, 0], f2["pairs"][:, 1]
    worst = dict(V2=float(np.max(np.abs(f2["V2"] - (b2["Vc"] - b["V1"][i] - b["V1"][j])) / scale)),
                 Vc=float(np.max(np.abs(f2["V2"] + f["V1"][i] + f["V1"][j] - b2["Vc"]) / scale)),
                 VT2=float(np.max(np.abs(f2["VT2"] - b2["VT2"]) / scale)))
    print("%s (%d grid rows, p=%d): err / (2 K EPS 16 abs sum) %s" % (
        name, c["rows"], p, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) < 1e-2                     # a small fraction of the worst-case bound


def _small(d, p, q, seed):
    rng = np.random.default_rng(seed)
    levels = np.arange(2, 2 + d)
    terms = np.stack([rng.integers(0, levels[l], size=p) for l in range(d)], axis=1)
    terms[0] = 0
    terms[p - 1] = levels - 1
    m, Cv = S.random_tables(rng, levels)
    Theta = rng.standard_normal((p, q)) * J.response_scales(q)[None, :]
    return terms, Theta, m, Cv


def test_identities_at_two_and_three_dimensions():
    """long double on both sides; the slack is 1 % of the float64 tolerances of what enters (about twenty
    times the long-double bound of the same sums)"""
    terms, Theta, m, Cv = _small(2, 12, 3, 1)
    f, f2 = S.formulas(terms, Theta, m, Cv), S2.formulas2(terms, Theta, m, Cv)
    slack = 0.01 * (f["tol_V"] + f["tol_V1"].sum(axis=0) + f2["tol_V2"][0] + f2["tol_VT2"][0])
    assert np.all(np.abs(E._f64(f2["VT2"][0] - f2["V2"][0])) <= slack)
    assert np.all(np.abs(E._f64(f["V"] - f["V1"][0] - f["V1"][1] - f2["V2"][0])) <= slack)
    terms, Theta, m, Cv = _small(3, 40, 3, 2)
    f, f2 = S.formulas(terms, Theta, m, Cv), S2.formulas2(terms, Theta, m, Cv)
    assert [tuple(r) for r in f2["pairs"]] == [(0, 1), (0, 2), (1, 2)]
    slack = 0.01 * (f["tol_V"] + f["tol_V1"].sum(axis=0) + f["tol_VT"].sum(axis=0) + f2["tol_V2"].sum(axis=0)
                    + f2["tol_VT2"].sum(axis=0))
    V012 = f2["VT2"] - f2["V2"]
    assert np.all(np.abs(E._f64(V012[1] - V012[0])) <= slack) and np.all(np.abs(E._f64(V012[2] - V012[0])) <= slack)
    assert np.all(E._f64(V012[0]) > 100 * slack)                                   # and it is there to be seen
    assert np.all(np.abs(E._f64(f["VT"][0] - f["V1"][0] - f2["V2"][0] - f2["V2"][1] - V012[0])) <= slack)
    assert np.all(np.abs(E._f64(f["V"] - f["V1"].sum(axis=0) - f2["V2"].sum(axis=0) - V012[0])) <= slack)


def test_inequalities_at_five_dimensions():
    terms, Theta, m, Cv = _small(5, 60, 3, 3)
    f, f2 = S.formulas(terms, Theta, m, Cv), S2.formulas2(terms, Theta, m, Cv)
    i, j = f2["pairs"][:, 0], f2["pairs"][:, 1]
    slack = 0.01 * (f2["tol_VT2"] + f2["tol_V2"] + f["tol_VT"][i] + f["tol_VT"][j])
    assert np.all(f2["V2"] >= -slack) and np.all(f2["V2"] <= f2["VT2"] + slack)
    assert np.all(f2["VT2"] <= np.minimum(f["VT"][i], f["VT"][j]) + slack)


def _inside2(got, f2):
    return {k: E.worst_ratio(got[k], f2[k], f2["tol_" + k]) for k in ("V2", "VT2")}


def _inside_G(got, f2):
    return max(E.worst_ratio(got["G"][o], f2["G"][o], f2["tol_G"][o]) for o in range(len(f2["G"])))


@pytest.mark.parametrize("name", GRID_CASES)
def test_float64_restatement_stays_inside_every_tolerance(name):
    c = grid_case2(name)
    m64, C64 = S.unpack_tables(*S.pack_tables(c["m"], c["Cv"]), c["levels"])
    f2 = S2.formulas2(c["terms"], c["Theta"], m64, C64)
    g64 = S2.formulas2(c["terms"], c["Theta"], m64, C64, dtype=np.float64)
    t64 = S2.formulas2(c["terms"], c["Theta"], m64, C64, dtype=np.float64,
                       pair_weights=S.tile_weights(len(c["terms"]), 16))
    r, rt, rg = _inside2(g64, f2), _inside2(t64, f2), _inside_G(g64, f2)
    print("%s: float64 err / tolerance: G %.3g, formulas %s, tiled %s" % (name, rg, r, rt))
    assert rg < 1 and max(r.values()) < 1 and max(rt.values()) < 1


def test_the_instrument_fails_five_mutations():
    c = grid_case2("mixed_d3")
    terms, Theta, p = c["terms"], c["Theta"], len(c["terms"])
    m64, C64 = S.unpack_tables(*S.pack_tables(c["m"], c["Cv"]), c["levels"])
    f2 = S2.formulas2(terms, Theta, m64, C64)
    tile = 16
    I = np.arange(p) // tile

    def run(W, Th=Theta, **kw):
        return S2.formulas2(terms, Th, m64, C64, dtype=np.float64, pair_weights=W, **kw)
    good = run(S.tile_weights(p, tile))
    assert max(_inside2(good, f2).values()) < 1 and _inside_G(good, f2) < 1
    W = S.tile_weights(p, tile)
    W[np.ix_(I == 1, I == 1)] = 2.0                      # a diagonal tile pair counted twice
    twice = _inside2(run(W), f2)
    W = S.tile_weights(p, tile)
    W[np.ix_(I == 0, I == 2)] = 1.0                      # an off-diagonal one counted once
    once = _inside2(run(W), f2)
    print("diagonal tile twice: %s; off-diagonal tile once: %s" % (twice, once))
    assert twice["VT2"] > 1 and once["VT2"] > 1
    mid = run(S.tile_weights(p, tile), drop_middle=True)  # prod_{i<l<j} A_l dropped: pair (0, 2) only
    rm = [E.worst_ratio(mid["VT2"][o], f2["VT2"][o], f2["tol_VT2"][o]) for o in range(3)]
    print("middle product dropped: VT2 err / tolerance per pair %s" % rm)
    assert rm[0] < 1 and rm[1] > 1 and rm[2] < 1
    for a, b in ((0, 1), (1, 2), (0, 2)):                # two pair slots swapped
        perm = np.arange(3)
        perm[[a, b]] = perm[[b, a]]
        sw = dict(V2=good["V2"][perm], VT2=good["VT2"][perm])
        r = _inside2(sw, f2)
        print("pair slots %d and %d swapped: %s" % (a, b, r))
        assert min(r.values()) > 1
    for shift in (1, -1):                                # response j read from column j +- 1
        rolled = run(S.tile_weights(p, tile), np.roll(Theta, shift, axis=1))
        r = dict(_inside2(rolled, f2), G=_inside_G(rolled, f2))
        print("columns shifted by %+d: %s" % (shift, r))
        assert min(r.values()) > 1


def test_swapped_slots_of_the_packed_G_are_seen():
    """different level counts per dimension: G_01 and G_02 have different shapes, and the packed G with the two
    slots exchanged is outside tol_G"""
    c = pair2_tables(300, 5, 2)
    f2 = c["f2"]
    assert len({g.shape[:2] for g in f2["G"]}) > 3
    packed = S2.pack_G(f2["G"])
    tol = S2.pack_G([t for t in f2["tol_G"]])
    n0, n1 = f2["G"][0][:, :, 0].size, f2["G"][1][:, :, 0].size
    swapped = np.concatenate([packed[:, n0:n0 + n1], packed[:, :n0], packed[:, n0 + n1:]], axis=1)
    assert np.all(np.abs(packed - packed) <= tol) and np.max(np.abs(swapped - packed) / np.maximum(tol, 1e-300)) > 1


def _cancellation(f2):
    v2, vt2 = np.abs(E._f64(f2["V2"])), np.abs(E._f64(f2["VT2"]))
    return (max(float(np.max(f2["abs_V2"] / v2)), float(np.max(f2["abs_VT2"] / vt2))),
            max(float(np.max(f2["tol_V2"] / v2)), float(np.max(f2["tol_VT2"] / vt2))))


@pytest.mark.parametrize("name", GRID_CASES)
def test_no_grid_value_is_pure_cancellation(name):
    r, t = _cancellation(grid_case2(name)["f2"])
    print("%s: largest sum |summands| / |value| %.3g, tolerance / |value| %.3g" % (name, r, t))
    assert r < CANCEL_MAX and t < DIGITS


@pytest.mark.parametrize("p,d,q", [c for c in PAIR2_CASES if c[1] > 1])
def test_no_stage2_value_is_pure_cancellation(p, d, q):
    r, t = _cancellation(pair2_tables(p, d, q)["f2"])
    print("p=%d d=%d q=%d: largest sum |summands| / |value| %.3g, tolerance / |value| %.3g" % (p, d, q, r, t))
    assert r < CANCEL_MAX and t < DIGITS


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


def test_python_names():
    import outerbase_amd as ob
    for name in ("sobol2", "interaction_effects", "Sobol2Result"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert callable(ob.MultiFit.sobol2) and callable(ob.MultiFit.interaction_effects)


def test_argument_errors_return_before_any_device_call():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    mdl = golden_model("mixed_d3")
    om, t = mdl["om_d"], ob.obmod._Terms(mdl["om_d"], mdl["terms"])
    buf = (C.c_double * 4096)()
    a = C.cast(buf, C.c_void_p)
    npairs, nG, wsb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert lib.obhip_sobol2_layout(None, C.byref(npairs), C.byref(nG)) == 1
    assert lib.obhip_sobol2_layout(t._h, C.byref(npairs), C.byref(nG)) == 0
    L = S.levels_of(mdl["terms"])
    assert npairs.value == 3 and nG.value == L[0] * L[1] + L[0] * L[2] + L[1] * L[2]
    wsf = lib.obhip_sobol2_workspace_bytes
    assert wsf(40, 3, 2, None) == 1 and wsf(0, 3, 2, C.byref(wsb)) == 1 and wsf(40, 0, 2, C.byref(wsb)) == 1
    assert wsf(40, 256, 2, C.byref(wsb)) == 1 and wsf(40, 3, 0, C.byref(wsb)) == 1
    assert wsf(40, 3, 65536, C.byref(wsb)) == 1 and wsf((1 << 24) + 1, 3, 2, C.byref(wsb)) == 1
    assert wsf(40, 3, 2, C.byref(wsb)) == 0 and wsb.value > 0
    sob = lib.obhip_sobol2_dev
    assert sob(None, a, 2, a, a, a, a, a, wsb.value) == 1
    assert sob(t._h, None, 2, a, a, a, a, a, wsb.value) == 1
    assert sob(t._h, a, 2, None, a, a, a, a, wsb.value) == 1
    assert sob(t._h, a, 2, a, None, a, a, a, wsb.value) == 1
    assert sob(t._h, a, 2, a, a, None, a, a, wsb.value) == 1
    assert sob(t._h, a, 2, a, a, a, a, None, wsb.value) == 1
    assert sob(t._h, a, 0, a, a, a, a, a, wsb.value) == 1                # q = 0
    assert sob(t._h, a, 65536, a, a, a, a, a, wsb.value) == 1
    assert sob(t._h, a, 2, a, a, a, a, a, wsb.value - 1) == 1            # workspace too small
    assert b"workspace" in lib.obhip_last_error()
    host = lib.obhip_sobol2
    assert host(None, a, 2, a, a, a, None) == 1 and host(t._h, a, 0, a, a, a, None) == 1
    assert host(t._h, None, 2, a, a, a, None) == 1 and host(t._h, a, 2, a, a, None, None) == 1
    ie = lib.obhip_interaction_effect_dev
    assert ie(None, t._h, 0, 1, a, 2, a, 4, a, 4, a) == 1
    assert ie(om._h, None, 0, 1, a, 2, a, 4, a, 4, a) == 1
    assert ie(om._h, t._h, 0, 1, None, 2, a, 4, a, 4, a) == 1
    assert ie(om._h, t._h, 0, 1, a, 2, None, 4, a, 4, a) == 1
    assert ie(om._h, t._h, 0, 1, a, 2, a, 4, None, 4, a) == 1
    assert ie(om._h, t._h, 0, 1, a, 2, a, 4, a, 4, None) == 1
    assert ie(om._h, t._h, 0, 1, a, 0, a, 4, a, 4, a) == 1               # q = 0
    assert ie(om._h, t._h, 1, 1, a, 2, a, 4, a, 4, a) == 1               # the same dimension twice
    assert b"same" in lib.obhip_last_error()
    assert ie(om._h, t._h, 0, 3, a, 2, a, 4, a, 4, a) == 1               # dimension out of range
    assert ie(om._h, t._h, 3, 0, a, 2, a, 4, a, 4, a) == 1
    assert ie(om._h, t._h, 0, 1, a, 2, a, 0, a, 4, a) == 0               # no grid points: a no-op
    assert ie(om._h, t._h, 0, 1, a, 2, a, 4, a, 0, a) == 0
    # one dimension: no pairs, nothing written, OK -- before any device call
    one = ob.outermod()
    ob.setcovfs(one, ["mat25"])
    ob.setknot(one, knots_for(["mat25"], 20))
    t1 = ob.obmod._Terms(one, np.arange(4, dtype=np.int64)[:, None])
    assert lib.obhip_sobol2_layout(t1._h, C.byref(npairs), C.byref(nG)) == 0 and npairs.value == 0 and nG.value == 0
    assert sob(t1._h, a, 2, a, a, None, None, None, 0) == 0
    assert host(t1._h, a, 2, a, a, None, None) == 0
    assert ie(one._h, t._h, 0, 1, a, 2, a, 4, a, 4, a) == 1              # terms of another model's dimension count
    # the limits of obhip_sobol_dev: a level beyond 255, tables beyond the LDS of a workgroup
    wide = ob.outermod()
    ob.setcovfs(wide, ["mat25"] * 2)
    ob.setknot(wide, [np.linspace(0.001, 0.999, 300)] * 2)
    tw = ob.obmod._Terms(wide, np.array([[0, 0], [256, 1]], dtype=np.int64))
    assert lib.obhip_sobol2_layout(tw._h, C.byref(npairs), C.byref(nG)) == 1
    assert b"255" in lib.obhip_last_error()
    assert sob(tw._h, a, 2, a, a, a, a, a, 1 << 30) == 1
    big = ob.outermod()
    ob.setcovfs(big, ["mat25"] * 2)
    ob.setknot(big, [np.linspace(0.001, 0.999, 64)] * 2)
    tb = ob.obmod._Terms(big, np.array([[0, 0], [59, 59]], dtype=np.int64))
    assert lib.obhip_sobol2_layout(tb._h, C.byref(npairs), C.byref(nG)) == 1
    assert b"LDS" in lib.obhip_last_error()
    assert sob(tb._h, a, 2, a, a, a, a, a, 1 << 30) == 1


def test_shape_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    om, terms = mdl["om_d"], mdl["terms"]
    p = len(terms)
    g = np.linspace(0.1, 0.9, 5)
    with pytest.raises(ValueError):
        ob.sobol2(om, terms, np.zeros((p + 1, 2)), None)
    with pytest.raises(ValueError):
        ob.sobol2(om, terms, np.zeros((p, 0)), None)
    with pytest.raises(ValueError):
        ob.interaction_effects(om, terms, np.zeros(p), None, 1, 1, g, g)
    with pytest.raises(ValueError):
        ob.interaction_effects(om, terms, np.zeros(p), None, 0, 3, g, g)
    with pytest.raises(ValueError):
        ob.interaction_effects(om, terms, np.zeros(p), None, 0, 1, np.zeros((2, 2)), g)
    assert ob.interaction_effects(om, terms, np.zeros((p, 2)), None, 0, 1, g, np.zeros(0)).shape == (5, 0, 2)
