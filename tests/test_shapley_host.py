"""Host-side checks of the Shapley effects (no GPU): the library's Gauss-Legendre nodes against a long-double
rule, the three routes of tests/shapley_ref.py against each other, the identities that tie the effects to the
Sobol quantities, the float64 restatement inside every tolerance, six mutations the instrument must fail, no
tested value a pure cancellation, and the library's host side -- symbols, Python names, argument errors before
any device call."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import extended_jac_ref as J
import extended_ref as E
import shapley_ref as SH
import sobol2_ref as S2
import sobol_ref as S
from conftest import knots_for
from test_sobol2_host import CANCEL_MAX, DIGITS, pair2_tables
from test_sobol_host import golden_model, grid_case, reference_of

ld = np.longdouble
NEW = {"obhip_gauss_legendre01": 3, "obhip_shapley_layout": 4, "obhip_shapley_workspace_bytes": 4,
       "obhip_shapley_dev": 9, "obhip_shapley": 7}
GRID_CASES = ["mixed_d3", "mixed_d3 weighted", "d5"]
D5_GROUPS = {"default": None, "three players": [[0, 3], [1], [2, 4]], "one player": [[0, 1, 2, 3, 4]]}
GRID_PLAYERS = [(n, "default") for n in GRID_CASES] + [("d5", "three players"), ("d5", "one player")]

# stage 2 on the GPU (test_gpu_shapley.py) and its cancellation check here.  TW = 128 terms per tile; the kernel
# keeps 8, 24 or 40 player slots in registers (d = 8 | 9, 24 | 25) with 2, 2 or 1 responses per chunk, and beyond
# d = 40 reads d - 40 dimensions per pair from memory (d = 44, 60: players of several dimensions only).
STAGE2_CASES = [(1, 3, 1), (5, 1, 2), (127, 2, 2), (128, 8, 3), (129, 9, 5), (300, 5, 2), (300, 10, 1), (1100, 3, 3),
                (129, 24, 2), (127, 25, 3), (128, 40, 2), (300, 20, 5)]


def _sizes_up(d):
    """players of sizes 1, 2, 3, .. of consecutive dimensions, the last one takes what is left"""
    out, l, n = [], 0, 1
    while l < d:
        out.append(list(range(l, min(d, l + n))))
        l, n = l + n, n + 1
    if len(out) > 1 and len(out[-1]) < len(out[-2]):
        out[-2] += out.pop()
    return out


def groups_of(name, d):
    if name == "default":
        return None
    if name == "identity":
        return [[l] for l in range(d)]
    if name == "halves":
        return [list(range(d // 2)), list(range(d // 2, d))]
    if name == "even odd":
        return [list(range(0, d, 2)), list(range(1, d, 2))]
    if name == "thirds interleaved":
        return [list(range(r, d, 3)) for r in range(3)]
    if name == "one player":
        return [list(range(d))]
    if name == "sizes 1 2 3":
        return _sizes_up(d)
    if name == "across the chunk":                           # dimensions 3 and 24 on both sides of slot 24
        return [[3, 24]] + [[l] for l in range(d) if l not in (3, 24)]
    if name == "first and last":
        return [[0, d - 1]] + [[l] for l in range(1, d - 1)]
    if name == "forty players":                              # d > 40: the first d - 40 players take two dimensions
        extra = d - 40
        return [[2 * g, 2 * g + 1] for g in range(extra)] + [[l] for l in range(2 * extra, d)]
    raise KeyError(name)


GROUP_CASES = [(300, 10, 1, "halves"), (300, 10, 1, "even odd"), (300, 10, 1, "one player"),
               (300, 20, 5, "sizes 1 2 3"), (127, 25, 3, "across the chunk"), (128, 40, 2, "first and last"),
               (128, 40, 2, "identity"), (128, 44, 2, "forty players"), (128, 44, 2, "sizes 1 2 3"),
               (128, 60, 2, "thirds interleaved")]
ALL_STAGE2 = [c + ("default",) for c in STAGE2_CASES] + GROUP_CASES


@functools.lru_cache(maxsize=None)
def stage2_case(p, d, q, name):
    """test_sobol2_host's random tables and route (a) on them, for the players `name`"""
    c = pair2_tables(p, d, q)
    groups = groups_of(name, d)
    return dict(c, groups=groups, sh=SH.shapley(c["terms"], c["Theta"], c["m"], c["Cv"], groups))


@functools.lru_cache(maxsize=None)
def grid_case_sh(name, players):
    c = grid_case(name)
    groups = D5_GROUPS[players]
    n = len(c["nodes"])
    rows, _ = S.grid_rows(c["nodes"])
    gref = reference_of(c["mdl"]["om_o"], rows)
    return dict(c, groups=groups, sh=SH.shapley(c["terms"], c["Theta"], c["m"], c["Cv"], groups),
                sym=SH.shapley_symmetric(c["terms"], c["Theta"], c["m"], c["Cv"], groups),
                brute_sh=SH.shapley_brute(gref, n, c["terms"], c["Theta"], c["weights"], groups))


def double_rule(G):
    """the long-double rule rounded to double: what a float64 evaluation is given"""
    s, w = SH.gauss_legendre01(G)
    return E._f64(s), E._f64(w)


# ---- the quadrature nodes ---------------------------------------------------------------------------
def _lib_rule(G):
    from outerbase_amd._lib import lib
    s, w = (C.c_double * G)(), (C.c_double * G)()
    assert lib.obhip_gauss_legendre01(G, s, w) == 0
    return np.array(s), np.array(w)


@pytest.mark.parametrize("G", [1, 2, 3, 10, 20, 64, 128])
def test_library_nodes_are_the_long_double_rule_rounded(G):
    """both sides round a long-double result whose error is far below half a double ulp: they agree to one ulp.
    Moments: with nodes and weights one ulp (2^-52 relative) off at most, sum w s^j moves by at most
    (1 + j) 2^-52 sum w s^j; the long-double evaluation of the sum itself adds (G + j + 2) long-double roundings."""
    s, w = _lib_rule(G)
    rs, rw = double_rule(G)
    assert np.all(np.abs(s - rs) <= np.spacing(rs)) and np.all(np.abs(w - rw) <= np.spacing(rw))
    assert np.all(np.diff(s) > 0) and s[0] > 0 and s[-1] < 1
    sl, wl = np.asarray(s, dtype=ld), np.asarray(w, dtype=ld)
    worst, power = 0.0, np.ones(G, dtype=ld)
    for j in range(2 * G):
        got = np.sum(wl * power)
        tol = ((1 + j) * SH.ULP + (G + j + 2) * E.EPS) * float(got)
        worst = max(worst, float(abs(got - ld(1) / (j + 1))) / tol)
        power = power * sl
    print("G=%d: worst |sum w s^j - 1/(j+1)| / tolerance %.3g" % (G, worst))
    assert worst < 1


def test_long_double_rule_integrates_exactly():
    """the instrument's own rule: every moment below 2 G to long-double rounding"""
    for G in (1, 2, 5, 20, 128):
        s, w = SH.gauss_legendre01(G)
        power = np.ones(G, dtype=ld)
        for j in range(2 * G):
            assert abs(np.sum(w * power) - ld(1) / (j + 1)) < 64 * (G + j + 2) * E.EPS / (j + 1)
            power = power * s


def test_node_count_refusals():
    from outerbase_amd._lib import lib
    buf = (C.c_double * 256)()
    assert lib.obhip_gauss_legendre01(0, buf, buf) == 1 and lib.obhip_gauss_legendre01(129, buf, buf) == 1
    assert lib.obhip_gauss_legendre01(4, None, buf) == 1 and lib.obhip_gauss_legendre01(4, buf, None) == 1


# ---- the instrument ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,players", GRID_PLAYERS)
def test_three_routes_agree(name, players):
    """three algebraically different routes in long double: they differ by rounding only.  The scale is the brute
    force's: with a = E[(sum_k |theta_k B_k|)^2] (test_sobol_host's abs2) every Var E[f | x_u] has sum |summands|
    <= a, a V_u is 2^|u| of them and Sh_g takes V_u / |u| of the 2^(P-1) sets that hold g: 3^P a bounds all of it,
    over K = grid rows + p^2 + 3 d + 2 G + 4 summands on either route."""
    c = grid_case_sh(name, players)
    p, d = c["terms"].shape
    sh = c["sh"]
    P = len(sh["players"])
    K = c["rows"] + p * p + 3 * d + 2 * sh["G"] + 4
    scale = 2 * K * E.EPS * (3 ** P) * c["abs2"]
    worst = dict(quadrature_vs_symmetric=float(np.max(np.abs(sh["Sh"] - c["sym"]) / scale)),
                 quadrature_vs_brute=float(np.max(np.abs(sh["Sh"] - c["brute_sh"]) / scale)))
    print("%s, %s (%d grid rows, p=%d, P=%d): err / (2 K EPS 3^P abs sum) %s" % (
        name, players, c["rows"], p, P, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) < 1e-2                     # a small fraction of the worst-case bound


def _identity_cases():
    for name, players in GRID_PLAYERS:
        c = grid_case_sh(name, players)
        yield "%s, %s" % (name, players), c, c["sh"], S.formulas(c["terms"], c["Theta"], c["m"], c["Cv"])
    for p, d, q, name in ALL_STAGE2:
        c = stage2_case(p, d, q, name)
        yield "p=%d d=%d q=%d %s" % (p, d, q, name), c, c["sh"], c["f"]


def test_effects_sum_to_the_variance_and_one_player_takes_it_all():
    """long double on both sides; the slack is 1 % of the float64 tolerances of what enters"""
    for label, c, sh, f in _identity_cases():
        slack = 0.01 * (f["tol_V"] + sh["tol_Sh"].sum(axis=0))
        assert np.all(np.abs(E._f64(sh["Sh"].sum(axis=0) - f["V"])) <= slack), label
        if len(sh["players"]) == 1:
            assert np.all(np.abs(E._f64(sh["Sh"][0] - f["V"])) <= slack), label


def test_identity_partition_is_the_default_bit_for_bit():
    for p, d, q in ((300, 5, 2), (129, 9, 5)):
        c = pair2_tables(p, d, q)
        a = SH.shapley(c["terms"], c["Theta"], c["m"], c["Cv"], None)
        b = SH.shapley(c["terms"], c["Theta"], c["m"], c["Cv"], [[l] for l in range(d)])
        assert np.array_equal(a["Sh"], b["Sh"]) and np.array_equal(a["tol_Sh"], b["tol_Sh"])


def test_two_active_dimensions_per_term_split_the_pair_variances_evenly():
    """level 0 made a constant (its row and column of every C_l zero), so that a term varies in its active
    dimensions only and there is no ANOVA term beyond pairs: Sh_l = V1_l + sum_j V2_lj / 2"""
    rng = np.random.default_rng(29)
    d, p, q = 4, 40, 3
    levels = np.array([3, 4, 2, 5])
    terms = np.zeros((p, d), dtype=np.int64)
    for k in range(1, p):
        dims = rng.choice(d, size=int(rng.integers(1, 3)), replace=False)
        terms[k, dims] = rng.integers(1, levels[dims])
    terms[p - 1] = [levels[0] - 1, 0, 0, levels[3] - 1]
    terms[p - 2] = [0, levels[1] - 1, levels[2] - 1, 0]
    m, Cv = S.random_tables(rng, levels)
    for Cl in Cv:
        Cl[0, :] = 0.0
        Cl[:, 0] = 0.0
    Theta = rng.standard_normal((p, q)) * J.response_scales(q)[None, :]
    f, f2, sh = S.formulas(terms, Theta, m, Cv), S2.formulas2(terms, Theta, m, Cv), SH.shapley(terms, Theta, m, Cv)
    want = f["V1"].copy()
    for o, (i, j) in enumerate(f2["pairs"]):
        want[i] = want[i] + f2["V2"][o] / 2
        want[j] = want[j] + f2["V2"][o] / 2
    slack = 0.01 * (sh["tol_Sh"] + f["tol_V1"] + f2["tol_V2"].sum(axis=0)[None, :])
    assert np.all(np.abs(E._f64(sh["Sh"] - want)) <= slack)
    assert np.all(E._f64(f2["V2"]).max(axis=0) > 100 * slack.max(axis=0))             # and the pairs are there


def test_effects_lie_between_first_order_and_total_variances():
    """positive semi-definite tables: V1_l <= Sh_l <= VT_l up to the tolerances"""
    for label, c, sh, f in _identity_cases():
        if c["groups"] is not None:
            continue
        slack = sh["tol_Sh"] + f["tol_V1"] + f["tol_VT"]
        Sh = E._f64(sh["Sh"])
        assert np.all(E._f64(f["V1"]) <= Sh + slack) and np.all(Sh <= E._f64(f["VT"]) + slack), label


# ---- the float64 restatement and the mutations --------------------------------------------------------
def _tables64(c):
    return S.unpack_tables(*S.pack_tables(c["m"], c["Cv"]), c["levels"])


def _restate(c, ref, tile=16, **kw):
    """err / tolerance of a float64 evaluation through upper-triangular tiles of `tile` terms"""
    m64, C64 = _tables64(c)
    P = len(ref["players"])
    args = dict(groups=c["groups"], dtype=np.float64, pair_weights=S.tile_weights(len(c["terms"]), tile),
                rule=double_rule((P + 1) // 2))
    Theta = kw.pop("Theta", c["Theta"])
    args.update(kw)
    got = SH.shapley(c["terms"], Theta, m64, C64, **args)
    return E.worst_ratio(got["Sh"], ref["Sh"], ref["tol_Sh"])


def _ref64(c):
    m64, C64 = _tables64(c)
    return SH.shapley(c["terms"], c["Theta"], m64, C64, c["groups"])


@pytest.mark.parametrize("name,players", GRID_PLAYERS)
def test_float64_restatement_stays_inside_every_tolerance(name, players):
    c = grid_case_sh(name, players)
    ref = _ref64(c)
    m64, C64 = _tables64(c)
    plain = SH.shapley(c["terms"], c["Theta"], m64, C64, c["groups"], dtype=np.float64,
                       rule=double_rule(ref["G"]))
    r, rt = E.worst_ratio(plain["Sh"], ref["Sh"], ref["tol_Sh"]), _restate(c, ref)
    print("%s, %s: float64 err / tolerance: formulas %.3g, tiled %.3g" % (name, players, r, rt))
    assert r < 1 and rt < 1


@pytest.mark.parametrize("p,d,q,name", [(300, 5, 2, "default"), (300, 10, 1, "halves"), (300, 20, 5, "sizes 1 2 3"),
                                        (128, 40, 2, "first and last")])
def test_float64_restatement_stays_inside_the_stage2_tolerances(p, d, q, name):
    c = stage2_case(p, d, q, name)
    r = _restate(c, c["sh"], tile=128)
    print("p=%d d=%d q=%d %s: float64 err / tolerance %.3g" % (p, d, q, name, r))
    assert r < 1


def test_the_instrument_fails_six_mutations():
    seen = {}
    for name, players in (("mixed_d3", "default"), ("d5", "three players")):
        c = grid_case_sh(name, players)
        ref = _ref64(c)
        p, P, G = len(c["terms"]), len(ref["players"]), ref["G"]
        tile = 16
        I = np.arange(p) // tile
        assert _restate(c, ref) < 1
        W = S.tile_weights(p, tile)
        W[np.ix_(I == 1, I == 1)] = 2.0                    # a diagonal tile counted twice
        r = dict(diagonal_twice=_restate(c, ref, pair_weights=W))
        W = S.tile_weights(p, tile)
        W[np.ix_(I == 0, I == I.max())] = 1.0              # an off-diagonal tile counted once
        r["off_diagonal_once"] = _restate(c, ref, pair_weights=W)
        s, w = double_rule(G)
        if G > 1:                                          # one node dropped: the rule of G - 1 nodes
            r["node_dropped"] = _restate(c, ref, rule=double_rule(G - 1))
        r["nodes_on_minus_one_one"] = _restate(c, ref, rule=(2 * s - 1, 2 * w))
        if c["groups"] is not None:
            r["groups_ignored"] = _restate(c, ref, ignore_groups=True)
        for shift in (1, -1):                              # response j read from column j +- 1
            r["column_%+d" % shift] = _restate(c, ref, Theta=np.roll(c["Theta"], shift, axis=1))
        print("%s, %s: err / tolerance %s" % (name, players, ", ".join("%s %.3g" % kv for kv in r.items())))
        for k, v in r.items():
            seen[k] = max(seen.get(k, 0.0), v)
    assert set(seen) == {"diagonal_twice", "off_diagonal_once", "node_dropped", "nodes_on_minus_one_one",
                         "groups_ignored", "column_+1", "column_-1"}
    assert min(seen.values()) > 1, seen


def test_every_mutation_shows_on_a_stage2_shape():
    """the shapes the GPU test runs hold, for every mutation, a case outside its tolerance: tiles (p = 300: three,
    two of them off the diagonal), G > 1, players of several dimensions, q > 1"""
    c = stage2_case(300, 5, 2, "default")
    p, G = 300, c["sh"]["G"]
    I = np.arange(p) // 128
    W = S.tile_weights(p, 128)
    W[np.ix_(I == 1, I == 1)] = 2.0
    assert _restate(c, c["sh"], tile=128, pair_weights=W) > 1
    W = S.tile_weights(p, 128)
    W[np.ix_(I == 0, I == 2)] = 1.0
    assert _restate(c, c["sh"], tile=128, pair_weights=W) > 1
    s, w = double_rule(G)
    assert G == 3 and _restate(c, c["sh"], tile=128, rule=double_rule(G - 1)) > 1
    assert _restate(c, c["sh"], tile=128, rule=(2 * s - 1, 2 * w)) > 1
    assert _restate(c, c["sh"], tile=128, Theta=np.roll(c["Theta"], 1, axis=1)) > 1
    g = stage2_case(300, 10, 1, "halves")
    assert _restate(g, g["sh"], tile=128, ignore_groups=True) > 1


# ---- no value under test is a pure cancellation ---------------------------------------------------------
def _cancellation(sh):
    v = np.abs(E._f64(sh["Sh"]))
    return float(np.max(sh["abs_Sh"] / v)), float(np.max(sh["tol_Sh"] / v))


@pytest.mark.parametrize("name,players", GRID_PLAYERS)
def test_no_grid_value_is_pure_cancellation(name, players):
    r, t = _cancellation(grid_case_sh(name, players)["sh"])
    print("%s, %s: largest sum |summands| / |value| %.3g, tolerance / |value| %.3g" % (name, players, r, t))
    assert r < CANCEL_MAX and t < DIGITS


@pytest.mark.parametrize("p,d,q,name", ALL_STAGE2)
def test_no_stage2_value_is_pure_cancellation(p, d, q, name):
    r, t = _cancellation(stage2_case(p, d, q, name)["sh"])
    print("p=%d d=%d q=%d %s: largest sum |summands| / |value| %.3g, tolerance / |value| %.3g" % (p, d, q, name, r, t))
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
    for name in ("shapley", "ShapleyResult"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert callable(ob.MultiFit.shapley)


def _ids(*v):
    return (C.c_int32 * len(v))(*v)


def _model(d, knots=20):
    import outerbase_amd as ob
    om = ob.outermod()
    ob.setcovfs(om, ["mat25"] * d)
    ob.setknot(om, knots_for(["mat25"] * d, knots))
    return om


def test_argument_errors_return_before_any_device_call():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    mdl = golden_model("mixed_d3")
    t = ob.obmod._Terms(mdl["om_d"], mdl["terms"])
    buf = (C.c_double * 4096)()
    a = C.cast(buf, C.c_void_p)
    P, G, wsb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    lay = lib.obhip_shapley_layout
    assert lay(None, None, C.byref(P), C.byref(G)) == 1
    assert lay(t._h, None, C.byref(P), C.byref(G)) == 0 and (P.value, G.value) == (3, 2)
    assert lay(t._h, _ids(1, 0, 1), C.byref(P), C.byref(G)) == 0 and (P.value, G.value) == (2, 1)
    assert lay(t._h, _ids(0, 0, 0), None, None) == 0
    assert lay(t._h, _ids(0, 3, 1), C.byref(P), C.byref(G)) == 1                  # an id beyond d - 1
    assert lay(t._h, _ids(-1, 0, 1), C.byref(P), C.byref(G)) == 1                 # a negative id
    assert lay(t._h, _ids(0, 2, 2), C.byref(P), C.byref(G)) == 1                  # a gap: 1 is not used
    assert b"gap" in lib.obhip_last_error()
    assert lay(t._h, _ids(1, 1, 1), C.byref(P), C.byref(G)) == 1                  # 0 is not used
    wsf = lib.obhip_shapley_workspace_bytes
    assert wsf(40, 3, 2, None) == 1 and wsf(0, 3, 2, C.byref(wsb)) == 1 and wsf(40, 0, 2, C.byref(wsb)) == 1
    assert wsf(40, 256, 2, C.byref(wsb)) == 1 and wsf(40, 3, 0, C.byref(wsb)) == 1
    assert wsf(40, 3, 65536, C.byref(wsb)) == 1 and wsf((1 << 24) + 1, 3, 2, C.byref(wsb)) == 1
    assert wsf(40, 3, 2, C.byref(wsb)) == 0 and wsb.value > 0
    dev = lib.obhip_shapley_dev
    assert dev(None, None, a, 2, a, a, a, a, wsb.value) == 1
    assert dev(t._h, None, None, 2, a, a, a, a, wsb.value) == 1
    assert dev(t._h, None, a, 2, None, a, a, a, wsb.value) == 1
    assert dev(t._h, None, a, 2, a, None, a, a, wsb.value) == 1
    assert dev(t._h, None, a, 2, a, a, None, a, wsb.value) == 1
    assert dev(t._h, None, a, 2, a, a, a, None, wsb.value) == 1
    assert dev(t._h, None, a, 0, a, a, a, a, wsb.value) == 1                     # q = 0
    assert dev(t._h, None, a, 65536, a, a, a, a, wsb.value) == 1
    assert dev(t._h, None, a, 2, a, a, a, a, wsb.value - 1) == 1                 # workspace too small
    assert b"workspace" in lib.obhip_last_error()
    assert dev(t._h, _ids(0, 3, 1), a, 2, a, a, a, a, wsb.value) == 1            # bad ids
    assert dev(t._h, _ids(0, 2, 2), a, 2, a, a, a, a, wsb.value) == 1            # a gap in the ids
    host = lib.obhip_shapley
    assert host(None, None, a, 2, a, a, a) == 1 and host(t._h, None, a, 0, a, a, a) == 1
    assert host(t._h, None, None, 2, a, a, a) == 1 and host(t._h, None, a, 2, a, a, None) == 1
    assert host(t._h, _ids(0, 2, 2), a, 2, a, a, a) == 1
    # the player bound: 41 dimensions are 41 players unless they are grouped
    many = _model(41, 6)
    tm = ob.obmod._Terms(many, np.eye(41, dtype=np.int64)[:5])
    assert lay(tm._h, None, C.byref(P), C.byref(G)) == 1
    assert b"40" in lib.obhip_last_error() and b"players" in lib.obhip_last_error()
    assert wsf(5, 41, 2, C.byref(wsb)) == 0
    assert dev(tm._h, None, a, 2, a, a, a, a, wsb.value) == 1
    assert lay(tm._h, _ids(*([0, 0] + list(range(1, 40)))), C.byref(P), C.byref(G)) == 0
    assert (P.value, G.value) == (40, 20)
    # the limits of obhip_sobol_dev: a level beyond 255, tables beyond the LDS of a workgroup
    wide = ob.outermod()
    ob.setcovfs(wide, ["mat25"] * 2)
    ob.setknot(wide, [np.linspace(0.001, 0.999, 300)] * 2)
    tw = ob.obmod._Terms(wide, np.array([[0, 0], [256, 1]], dtype=np.int64))
    assert lay(tw._h, None, C.byref(P), C.byref(G)) == 1
    assert b"255" in lib.obhip_last_error()
    assert dev(tw._h, None, a, 2, a, a, a, a, 1 << 30) == 1
    big = ob.outermod()
    ob.setcovfs(big, ["mat25"] * 2)
    ob.setknot(big, [np.linspace(0.001, 0.999, 64)] * 2)
    tb = ob.obmod._Terms(big, np.array([[0, 0], [59, 59]], dtype=np.int64))
    assert lay(tb._h, None, C.byref(P), C.byref(G)) == 1
    assert b"LDS" in lib.obhip_last_error()
    assert dev(tb._h, None, a, 2, a, a, a, a, 1 << 30) == 1


def test_shape_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    om, terms = mdl["om_d"], mdl["terms"]
    p = len(terms)
    with pytest.raises(ValueError):
        ob.shapley(om, terms, np.zeros((p + 1, 2)), None)                        # Theta of the wrong height
    with pytest.raises(ValueError):
        ob.shapley(om, terms, np.zeros((p, 0)), None)
    for groups in ([[0, 1]], [[0, 1], [1, 2]], [[0], [1], [2], []], [[0, 1], [2, 3]], [[0, 1, 2, 2]]):
        with pytest.raises(ValueError):                                          # not a partition of range(d)
            ob.shapley(om, terms, np.zeros((p, 2)), None, groups=groups)
