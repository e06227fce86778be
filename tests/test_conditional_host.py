"""The instrument of the conditional moments itself (tests/conditional_ref.py), the plan of
csrc/conditional_plan.h and the host side of the new entries (no GPU):

  - the reference's M and W against a brute-force weighted mean and variance over the full tensor grid of the
    noise nodes (d = 3 with |E| = 2 and 12 nodes, d = 5 with |E| = 3 and 6 nodes, weights with zeros);
  - its gradients against central differences of its own values;
  - the grouped form c^T mE, c^T K c against the sum over pairs of terms;
  - the law of total variance and the main effect for |S| = 1 against sobol_ref.formulas;
  - five mutants the instrument must fail at the tolerance the device is held to;
  - tests/conditional_plan_check.cpp walks the plan as a program of its own, under the address and
    undefined-behaviour sanitizers;
  - the layout entry against the reference's grouping, and what the entries refuse without a device."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import conditional_ref as R
import extended_dx_ref as X
import extended_ref as E
import sobol_ref as S
from conftest import sample_x
from test_sobol_host import d5_model, golden_model, some_zero_weights, theta_of

ld = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 4
NEW = ("obhip_conditional_layout", "obhip_conditional_tables_dev", "obhip_conditional_moments_dev",
       "obhip_conditional_tables", "obhip_conditional_moments")


@functools.lru_cache(maxsize=None)
def case(name):
    """model, nodes and weights of the measure, the long-double tables, a few rows and the reference on them"""
    if name == "d3":
        mdl, n, noise, weights = golden_model("mixed_d3"), 12, [0, 2], None
    elif name == "d3 weighted":
        mdl, n, noise, weights = golden_model("mixed_d3"), 12, [1, 2], True
    elif name == "d3 one control":
        mdl, n, noise, weights = golden_model("mixed_d3"), 12, [0, 2], True
    else:
        mdl, n, noise, weights = d5_model(), 6, [0, 2, 3], True
    kinds, terms, om_o = mdl["kinds"], mdl["terms"], mdl["om_o"]
    d = len(kinds)
    rng = np.random.default_rng(len(name))
    nodes = sample_x(rng, n, kinds)
    w = some_zero_weights(rng, n, d) if weights else None
    x = sample_x(rng, 7, kinds)
    Theta = theta_of(terms, Q, 3 + len(name))
    levels = S.levels_of(terms)
    nref = E.ExtendedRef(om_o.kinds, [om_o.knots_of(k) for k in range(d)], om_o.hyp, om_o.rotmat, nodes)
    m, Cv = S.tables_from_bases([nref.getbase(l)[0] for l in range(d)], levels, w)
    ref = X.reference_dx_of(om_o, x)
    Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, om_o, x, terms))
    f = R.moments(ref, terms, Theta, noise, m, Cv, Cc, grad=True)
    return dict(mdl=mdl, kinds=kinds, terms=terms, om_o=om_o, d=d, noise=noise, nodes=nodes, w=w, x=x, Theta=Theta,
                m=m, Cv=Cv, ref=ref, C=Cc, f=f, n=n)


# ---- the instrument ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d3", "d3 weighted", "d5"])
def test_reference_agrees_with_the_brute_force_over_the_noise_grid(name):
    """two algebraically different routes in long double: they differ by rounding only.  K = grid rows + p^2 +
    3 d + 4 summands at most on either route; the absolute sums are those of the brute force (the weighted mean of
    sum_k |theta_k B_k| and of its square), which bound the formulas' as in test_sobol_host"""
    c = case(name)
    noise, d, n = c["noise"], c["d"], c["n"]
    grid, idx = S.grid_rows(c["nodes"][:, noise])
    wn = S.normalised_weights(c["w"], n, d)
    wr = np.prod(wn[idx, np.asarray(noise)[None, :]], axis=1)
    full = np.repeat(c["x"], len(grid), axis=0)
    full[:, noise] = np.tile(grid, (len(c["x"]), 1))
    B, _ = X.reference_dx_of(c["om_o"], full).getmat(c["terms"])
    Th = np.asarray(c["Theta"], dtype=ld)
    F = (B @ Th).reshape(len(c["x"]), len(grid), Q)
    aF = (np.abs(B) @ np.abs(Th)).reshape(F.shape)
    mean = np.einsum("b,abj->aj", wr, F)
    var = np.einsum("b,abj->aj", wr, (F - mean[:, None, :]) ** 2)
    abs1, abs2 = np.einsum("b,abj->aj", wr, aF), np.einsum("b,abj->aj", wr, aF * aF)
    p = len(c["terms"])
    K = len(grid) + p * p + 3 * d + 4
    rm = float(np.max(np.abs(c["f"]["M"] - mean) / (2 * K * E.EPS * abs1)))
    rv = float(np.max(np.abs(c["f"]["W"] - var) / (2 * K * E.EPS * abs2)))
    print("%s (%d grid rows, p=%d): err / (2 K EPS abs sum) mean %.3g, variance %.3g" % (name, len(grid), p, rm, rv))
    assert rm < 1 and rv < 1
    assert np.all(E._f64(var) > 0)


@pytest.mark.parametrize("name", ["d3 weighted", "d5"])
def test_reference_gradients_agree_with_central_differences_of_its_own_values(name):
    """D(h) = (v(x + h e_l) - v(x - h e_l)) / (2 h) in long double at h and h / 2.  The truncation error falls by
    four from h to h / 2, so that of D(h / 2) is a third of |D(h) - D(h / 2)|; allowed: that difference itself, plus
    the rounding of the difference quotient, 8 EPS (sum of magnitudes) / h"""
    c = case(name)
    ctrl = list(R.control_dims(c["d"], c["noise"]))
    f = c["f"]

    def values(x):
        ref = X.reference_dx_of(c["om_o"], x)
        g = R.moments(ref, c["terms"], c["Theta"], c["noise"], c["m"], c["Cv"], c["C"])
        return g["M"], g["W"]
    worst = 0.0
    h = 1e-3
    for a, l in enumerate(ctrl):
        D = []
        for hh in (h, h / 2):
            xp, xm = c["x"].copy(), c["x"].copy()
            xp[:, l] += hh
            xm[:, l] -= hh
            step = np.asarray(xp[:, l], dtype=ld) - np.asarray(xm[:, l], dtype=ld)
            (Mp, Wp), (Mm, Wm) = values(xp), values(xm)
            D.append(((Mp - Mm) / step[:, None], (Wp - Wm) / step[:, None]))
        for got, d1, d2, mag in ((f["dM"][:, a], D[0][0], D[1][0], f["abs_M"]),
                                 (f["dW"][:, a], D[0][1], D[1][1], f["abs_M"] ** 2)):
            allow = np.abs(d1 - d2) + 8 * E.EPS * mag / (h / 2)
            worst = max(worst, float(np.max(np.abs(got - d2) / allow)))
    print("%s: gradient against central differences, err / allowed %.3g" % (name, worst))
    assert worst < 1


@pytest.mark.parametrize("name", ["d3", "d3 weighted", "d5"])
def test_grouped_form_agrees_with_the_sum_over_pairs_of_terms(name):
    c = case(name)
    S_ = list(R.control_dims(c["d"], c["noise"]))
    P, _ = R.side_products(c["ref"], c["terms"], S_)
    worst = 0.0
    for j in range(Q):
        M, W = R.grouped_moments(P, c["Theta"][:, j], c["terms"], c["noise"], c["m"], c["Cv"])
        worst = max(worst, float(np.max(np.abs(M - c["f"]["M"][:, j]) / c["f"]["tol_M"][:, j])),
                    float(np.max(np.abs(W - c["f"]["W"][:, j]) / c["f"]["tol_W"][:, j])))
    print("%s: grouped against ungrouped, err / device tolerance %.3g" % (name, worst))
    assert worst < 1e-3                      # two long-double routes: far inside what a float64 result is allowed


def test_law_of_total_variance_and_main_effect_for_one_control_dimension():
    """|S| = 1, x = the nodes of that dimension: sum_i w^_i W_i = V - V1_l and M_i = sum_t g_l[t] R_lt(x_i) (the
    main effect plus mu), against sobol_ref.formulas on the same long-double tables; both sides long double:
    allowed 2 (n + p^2 + 3 d + 4) EPS of the sums of magnitudes (tol_V / gamma and abs_M)"""
    c = case("d3 one control")
    l, d, n = 1, c["d"], c["n"]
    x = np.tile(c["x"][:1], (n, 1))
    x[:, l] = c["nodes"][:, l]
    ref = X.reference_dx_of(c["om_o"], x)
    f = R.moments(ref, c["terms"], c["Theta"], c["noise"], c["m"], c["Cv"], c["C"])
    fs = S.formulas(c["terms"], c["Theta"], c["m"], c["Cv"])
    wn = S.normalised_weights(c["w"], n, d)[:, l]
    p = len(c["terms"])
    K = n + p * p + 3 * d + 4
    absV = fs["tol_V"] / E.gamma(p * p + 3 * d + 4)
    r1 = float(np.max(np.abs(wn @ f["W"] - (fs["V"] - fs["V1"][l])) / (2 * K * E.EPS * absV)))
    Rl = ref.getbase(l)[0][:, :len(c["m"][l])]
    r2 = float(np.max(np.abs(f["M"] - Rl @ fs["g"][l]) / (2 * K * E.EPS * f["abs_M"])))
    print("law of total variance %.3g, main effect %.3g of 2 K EPS abs sum" % (r1, r2))
    assert r1 < 1 and r2 < 1


# ---- the failures the chosen inputs must be able to see ----------------------------------------------------
def test_mutants_land_above_the_tolerance():
    """d = 3, E = {0, 2}, the golden terms: clean, the grouped form is within the device's tolerance; each mutant is
    above it in M or W at some row"""
    c = case("d3")
    f = c["f"]
    S_ = list(R.control_dims(c["d"], c["noise"]))
    P, _ = R.side_products(c["ref"], c["terms"], S_)
    gof, tuples = R.groups_of(c["terms"], c["noise"])
    assert len(tuples) > 16                                   # a 16-wide block of groups can be left out
    j = 1

    def ratio(M, W, col=j):
        return max(E.worst_ratio(E._f64(M), f["M"][:, col], f["tol_M"][:, col]),
                   E.worst_ratio(E._f64(W), f["W"][:, col], f["tol_W"][:, col]))
    args = (c["terms"], c["noise"], c["m"], c["Cv"])
    assert ratio(*R.grouped_moments(P, c["Theta"][:, j], *args)) < 1
    mutants = {
        "one group counted twice": R.grouped_moments(P, c["Theta"][:, j], *args, twice=3),
        "C of one noise dimension replaced by A": R.grouped_moments(P, c["Theta"][:, j], *args, c_for_a=2),
        "one 16-wide block of groups left out of Y": R.grouped_moments(P, c["Theta"][:, j], *args, skip_block=0),
        "the neighbouring response column": R.grouped_moments(P, c["Theta"][:, j + 1], *args),
    }
    # one noise dimension treated as a control: its factor taken at the row instead of averaged
    P2, _ = R.side_products(c["ref"], c["terms"], sorted(S_ + [2]))
    mutants["one noise dimension treated as a control"] = R.grouped_moments(P2, c["Theta"][:, j], c["terms"], [0],
                                                                            c["m"], c["Cv"])
    for what, (M, W) in mutants.items():
        r = ratio(M, W)
        print("mutant %s: err/tolerance %.3g" % (what, r))
        assert r > 1, what
    # the columns are scaled 1e-3 .. 1e3 and every column is told from its neighbour
    assert E._f64(np.abs(c["Theta"]).max(axis=0)).max() / E._f64(np.abs(c["Theta"]).max(axis=0)).min() > 1e5
    for col in range(Q - 1):
        assert ratio(*R.grouped_moments(P, c["Theta"][:, col + 1], *args), col=col) > 1


# ---- the plan ---------------------------------------------------------------------------------------------
def test_plan_walked_by_a_program_of_its_own(tmp_path):
    # any host C++17 compiler will do: the program is plain C++ (the ROCm tree brings clang++ where g++ is missing)
    found = [shutil.which(c) for c in ("g++", "c++", "clang++")] + \
        [c for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(c)]
    found = [c for c in found if c]
    assert found, "no host C++ compiler: the only walk of the plan cannot run"
    exe = str(tmp_path / "conditional_plan_check")
    subprocess.run([found[0], "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "conditional_plan_check.cpp"), "-o", exe],
                   check=True)
    result = subprocess.run([exe], capture_output=True, text=True)
    assert result.stderr == "", result.stderr
    assert result.returncode == 0, result.stdout
    last = result.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000, result.stdout


def test_plan_header_is_plain_cpp():
    with open(os.path.join(ROOT, "outerbase_amd", "csrc", "conditional_plan.h")) as f:
        plain, frame = f.read().split("#if defined(__HIPCC__)")
    assert [ln.split()[1] for ln in plain.splitlines() if ln.startswith("#include")] == \
        ["<algorithm>", "<cstdint>", "<vector>", '"row_chunks.h"']
    assert "getenv" not in plain + frame and "hip/" not in plain and "__device__" not in plain


# ---- the library's host side ----------------------------------------------------------------------------------
def test_symbols_python_names_and_makefile():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    for name in NEW:
        assert hasattr(lib, name), name
    for name in ("conditional_layout", "conditional_moments", "conditional_tables", "ConditionalResult"):
        assert hasattr(ob, name) and name in ob.__all__
    assert hasattr(ob.MultiFit, "conditional")
    mk = open(os.path.join(ROOT, "outerbase_amd", "csrc", "Makefile")).read()
    for src in ("conditional.cpp", "kernels_conditional.hip", "conditional_plan.h"):
        assert src in mk


@pytest.mark.parametrize("name,noise", [("mixed_d3", [0]), ("mixed_d3", [0, 2]), ("mat25_d8", [1, 4, 6]),
                                        ("mat25_d8", [0, 1, 2, 3, 4, 5, 6])])
def test_layout_entry_agrees_with_the_reference_grouping(name, noise):
    import outerbase_amd as ob
    mdl = golden_model(name)
    lay = ob.conditional_layout(mdl["om_d"], mdl["terms"], noise)
    gof, tuples = R.groups_of(mdl["terms"], noise)
    assert lay["n_groups"] == len(tuples) and np.array_equal(lay["group_of"], gof)
    assert np.array_equal(lay["control_dims"], R.control_dims(len(mdl["kinds"]), noise))
    used = sum(len(set(mdl["terms"][:, l]) - {0}) for l in lay["control_dims"])
    assert lay["mu_s"] == 1 + used and lay["fused"]


def test_refusals_without_a_device():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    mdl = golden_model("mixed_d3")
    t = ob.obmod._Terms(mdl["om_d"], mdl["terms"])
    G = C.c_uint64(77)
    buf = (C.c_double * 8)()
    a = C.addressof(buf)

    def u32(v):
        return np.ascontiguousarray(v, dtype=np.uint32)

    def refused(name, *args):
        rc = getattr(lib, name)(*args)
        assert rc == 1, (name, rc)                                     # OBHIP_ERR_INVALID
        assert lib.obhip_last_error()
    for de in ([], [0, 1, 2], [2, 0], [1, 1], [3]):
        v = u32(de)
        refused("obhip_conditional_layout", t._h, v.ctypes.data, v.size, C.byref(G), None, None, None)
        refused("obhip_conditional_tables_dev", t._h, v.ctypes.data, v.size, a, a, a, a)
        refused("obhip_conditional_moments_dev", mdl["om_d"]._h, t._h, a, 1, v.ctypes.data, v.size, a, a, a, 1, 0,
                a, a, a, a)
    one = u32([1])
    refused("obhip_conditional_layout", None, one.ctypes.data, 1, C.byref(G), None, None, None)
    refused("obhip_conditional_layout", t._h, None, 1, C.byref(G), None, None, None)
    assert G.value == 77                                               # a refused call writes nothing
    for kw in (dict(q=0), dict(q=65536), dict(n=(1 << 40) + 1), dict(chunk=100), dict(chunk=64), dict(chunk=(1 << 30) + 128)):
        q, n, chunk = kw.get("q", 1), kw.get("n", 1), kw.get("chunk", 0)
        refused("obhip_conditional_moments_dev", mdl["om_d"]._h, t._h, a, q, one.ctypes.data, 1, a, a, a, n, chunk,
                a, a, a, a)
        refused("obhip_conditional_moments", mdl["om_d"]._h, t._h, a, q, one.ctypes.data, 1, a, a, a, n, max(n, 1),
                chunk, a, a, a, a)
    for null in range(4):                                              # model, terms, Theta, tables
        args = [mdl["om_d"]._h, t._h, a, 1, one.ctypes.data, 1, a, a, a, 1, 0, a, a, a, a]
        args[(0, 1, 2, 6)[null]] = None
        refused("obhip_conditional_moments_dev", *args)
    refused("obhip_conditional_moments_dev", mdl["om_d"]._h, t._h, a, 1, one.ctypes.data, 1, a, a, None, 1, 0, a, a, a, a)
    refused("obhip_conditional_tables_dev", t._h, one.ctypes.data, 1, a, a, None, a)
    refused("obhip_conditional_tables", t._h, one.ctypes.data, 1, a, a, a, None)
    assert not any(buf)                                                # nothing written
    assert lib.obhip_conditional_moments_dev(mdl["om_d"]._h, t._h, a, 1, one.ctypes.data, 1, a, a, None, 0, 0,
                                             a, a, a, a) == 0          # n = 0: a no-op
    assert lib.obhip_conditional_layout(t._h, one.ctypes.data, 1, C.byref(G), None, None, None) == 0 and G.value >= 1
    for bad in ([], [0, 1, 2], [2, 0], [1, 1], [3], [-1]):
        with pytest.raises(ValueError):
            ob.conditional_layout(mdl["om_d"], t, bad)


def test_limits_of_the_sobol_passes_refuse_without_a_device():
    """a level of 256, 256 dimensions and noise tables beyond the LDS of a workgroup (two 60-level noise dimensions)
    are OBHIP_ERR_INVALID from the layout, the tables and the moments entries, nothing written; with one of the two
    wide dimensions as noise the layout goes through.  p > 2^24 cannot be built through an entry at a size a test
    can afford; tests/conditional_plan_check.cpp walks that refusal on the plan."""
    import outerbase_amd as ob
    from outerbase_amd._lib import lib

    def mk(knots):
        om = ob.outermod()
        ob.setcovfs(om, ["mat25"] * len(knots))
        ob.setknot(om, knots)
        return om
    lvl = mk([np.linspace(0.001, 0.999, 300), np.linspace(0.001, 0.999, 20)])
    big = mk([np.linspace(0.001, 0.999, 64)] * 2 + [np.linspace(0.001, 0.999, 20)])
    d256 = mk([np.linspace(0.001, 0.999, 4)] * 256)
    t256 = np.zeros((2, 256), dtype=np.int64)
    t256[1, 0] = 1
    cases = [(lvl, [[0, 0], [256, 1]], [0], b"255"), (lvl, [[0, 0], [256, 1]], [1], b"255"),
             (big, [[0, 0, 0], [59, 59, 1]], [0, 1], b"LDS"), (d256, t256, [0], b"255 dimensions")]
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    G = C.c_uint64(77)
    for om, terms, noise, word in cases:
        t = ob.obmod._Terms(om, np.ascontiguousarray(terms, dtype=np.int64))
        de = np.ascontiguousarray(noise, dtype=np.uint32)
        calls = [("obhip_conditional_layout", (t._h, de.ctypes.data, de.size, C.byref(G), None, None, None)),
                 ("obhip_conditional_tables_dev", (t._h, de.ctypes.data, de.size, a, a, a, a)),
                 ("obhip_conditional_tables", (t._h, de.ctypes.data, de.size, a, a, a, a)),
                 ("obhip_conditional_moments_dev", (om._h, t._h, a, 1, de.ctypes.data, de.size, a, a, a, 1, 0, a, a, a, a)),
                 ("obhip_conditional_moments", (om._h, t._h, a, 1, de.ctypes.data, de.size, a, a, a, 1, 1, 0, a, a, a, a))]
        for name, args in calls:
            assert getattr(lib, name)(*args) == 1, (name, word)
            assert word in lib.obhip_last_error(), (name, lib.obhip_last_error())
    assert G.value == 77 and not any(buf)
    t = ob.obmod._Terms(big, np.array([[0, 0, 0], [59, 59, 1]], dtype=np.int64))
    one = np.ascontiguousarray([0], dtype=np.uint32)
    assert lib.obhip_conditional_layout(t._h, one.ctypes.data, 1, C.byref(G), None, None, None) == 0 and G.value == 2
