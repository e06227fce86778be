"""The shapes of test_gpu_grad_plans.py on the host (no GPU): the float64 oracle and the float64 restatement
of the fused decomposition (grad_plan_ref.py) sit inside the per-entry tolerance of every one of the eight
hyper-gradient products on every shape, no shape needs the cap of C, and every defect staged on the
restatement lands at least ten times above that tolerance on the very shape the device is run on."""
import functools

import numpy as np
import pytest

import extended_ref as E
import grad_plan_ref as G
from conftest import knots_for, sample_x
from test_extended_ref import oracle_model
from test_gpu_parity import random_terms

PROBE_ROWS = 300
PRODUCTS = ("getmat_gradhyp", "matmul_gradhyp", "matmul_gradhyp_dot", "tmatmul_gradhyp", "sqmm_gradhyp",
            "sqtmm_gradhyp", "sqcolsums_gradhyp", "residvar_gradhyp")


def _cube(om, terms, x):
    import ob_oracle as O
    knots = [om.knots_of(k) for k in range(om.d)]
    ref = E.ExtendedRef(om.kinds, knots, om.hyp, om.rotmat, x, om.rotmat_gradhyp)
    B, bB = ref.getmat(terms)
    dB, bdB = ref.getmat_gradhyp(terms)
    bo = O.OuterBase(om, x, dograd=True)
    ratio = max(E.worst_ratio(O.ob_getmat(bo, terms), B, bB), E.worst_ratio(O.ob_getmat_gradhyp(bo, terms), dB, bdB))
    return ref, B, bB, dB, bdB, bo, ratio


@functools.lru_cache(maxsize=2)
def reference(name):
    """the case's model data, inputs, long double products with their tolerances (want[q], tol[q]), the float64
    oracle's products and C -- built once, shared by the host and the device tests, never written to"""
    import ob_oracle as O
    c = G.CASES[name]
    kinds, n = c["kinds"], c["n"]
    om = oracle_model(kinds, knots_for(kinds, c["m"]))
    terms = G.case_terms(name, random_terms)
    p = len(terms)
    rng = np.random.default_rng(G.SEED[name] + 1)
    x = sample_x(rng, n, kinds)
    a, v = rng.standard_normal(p), rng.standard_normal(n)         # both signed
    ref, B, bB, dB, bdB, bo, ratio = _cube(om, terms, x)
    probe = ratio
    if n < PROBE_ROWS // 2:     # C belongs to the model and the terms, not to a handful of rows (test_gpu_extended.rows)
        probe = _cube(om, terms, sample_x(np.random.default_rng(G.SEED[name] + 2), PROBE_ROWS, kinds))[-1]
    C = E.constant_from_oracle_ratio(max(ratio, probe))
    varc, bvarc = E.term_var(om.basisvar, om.knotptst, terms)
    lv = om.getlvar_gradhyp(terms)                                  # entries of logbasisvar_gradhyp: data
    r = dict(name=name, om=om, kinds=kinds, terms=terms, x=x, a=a, v=v, n=n, p=p, C=C, ratio=max(ratio, probe),
             ref=ref, varc=np.asarray(varc, dtype=np.float64))
    pairs = {
        "getmat_gradhyp": (dB, C * np.asarray(bdB, dtype=np.float64)),
        "matmul_gradhyp": E.ref_matmul_gradhyp(dB, bdB, a, C),
        "matmul_gradhyp_dot": E.ref_matmul_gradhyp_dot(dB, bdB, a, v, C),
        "tmatmul_gradhyp": E.ref_tmatmul_gradhyp(dB, bdB, v, C),
        "sqmm_gradhyp": E.ref_sqmm_gradhyp(B, bB, dB, bdB, a, C),
        "sqtmm_gradhyp": E.ref_sqtmm_gradhyp(B, bB, dB, bdB, v, C),
        "sqcolsums_gradhyp": E.ref_sqcolsums_gradhyp(B, bB, dB, bdB, C),
        "residvar_gradhyp": E.ref_residvar_gradhyp(B, bB, dB, bdB, varc, bvarc, lv, C),
    }
    r["want"] = {q: w for q, (w, t) in pairs.items()}
    r["tol"] = {q: t for q, (w, t) in pairs.items()}
    mm = O.ob_mm_gradhyp(bo, terms, a)[1]
    r["oracle"] = {
        "getmat_gradhyp": O.ob_getmat_gradhyp(bo, terms), "matmul_gradhyp": mm, "matmul_gradhyp_dot": mm.T @ v,
        "tmatmul_gradhyp": O.ob_tmm_gradhyp(bo, terms, v)[1], "sqmm_gradhyp": O.ob_sqmm_gradhyp(bo, terms, a),
        "sqtmm_gradhyp": O.ob_sqtmm_gradhyp(bo, terms, v), "sqcolsums_gradhyp": O.ob_sqcolsums_gradhyp(bo, terms),
        "residvar_gradhyp": O.ob_residvar_gradhyp(bo, terms),
    }
    assert set(r["want"]) == set(r["oracle"]) == set(PRODUCTS)
    print("%s | n = %d, p = %d, nhyp = %d: oracle err/bound %.3g, C = %.3g" % (name, n, p, ref.nhyp, r["ratio"], C))
    return r


def restated(r, defect=None, only=None):
    """the restatement's products of a case whose views fit the fused pass (the transposed ones by the fused
    plan whatever plan the device takes: the arithmetic restated is the decomposition)"""
    F = G.Factors(r["ref"])
    numhyp = [E.NUMHYP[k] for k in r["kinds"]]
    groups = G.d3_groups(r["terms"], numhyp)
    if groups is None:
        return None
    d3 = [(q["nsplit"], q["tps"]) for q in (G.d3_geometry(g, r["n"]) for g in groups)]
    dense = G.dense_geometry(r["p"], r["n"])
    a, v, terms = r["a"], r["v"], r["terms"]
    out = {}
    if only in (None, "tmatmul_gradhyp"):
        out["tmatmul_gradhyp"] = G.fused_tmm(F, terms, groups, v, False, dense, d3, defect)
    if only in (None, "sqtmm_gradhyp"):
        out["sqtmm_gradhyp"] = G.fused_tmm(F, terms, groups, v, True, dense, d3, defect)
    if only is None:
        out["sqcolsums_gradhyp"] = G.fused_tmm(F, terms, groups, np.ones(r["n"]), True, dense, d3)
        out["matmul_gradhyp"] = G.fused_mm(F, terms, a, False)
        out["matmul_gradhyp_dot"] = out["matmul_gradhyp"].T @ v
        out["sqmm_gradhyp"] = G.fused_mm(F, terms, a, True)
        lv2 = r["om"].getlvar_gradhyp(terms) * r["varc"][:, None]
        P = F.others(terms)
        out["residvar_gradhyp"] = -G.fused_mm(F, terms, r["varc"], True) - ((P * P) * (F.s * F.s)[:, None]) @ lv2
    return out


@pytest.mark.parametrize("name", list(G.CASES))
def test_oracle_and_restatement_are_inside_every_tolerance(name):
    r = reference(name)
    assert r["C"] < E.C_CAP, "the case sits at the cap of C: give it shorter length scales, do not loosen"
    worst = {}
    for q in PRODUCTS:
        worst[q] = E.worst_ratio(r["oracle"][q], r["want"][q], r["tol"][q])
        assert worst[q] <= 1.0, (name, q, worst[q])
    assert worst["getmat_gradhyp"] <= 0.125 + 1e-12                     # C is eight times the oracle's own ratio
    line = "%s | oracle err/tol: %s" % (name, ", ".join("%s %.3g" % (q, worst[q]) for q in PRODUCTS))
    got = restated(r)
    if got is None:
        assert G.CASES[name]["expect"]["plan"] != "Fused"
        print(line + "; no view of these terms fits the fused pass")
        return
    mine = {q: E.worst_ratio(got[q], r["want"][q], r["tol"][q]) for q in got}
    print(line + "\n%s | restatement err/tol: %s" % (name, ", ".join("%s %.3g" % (q, mine[q]) for q in got)))
    for q in got:
        assert mine[q] <= 1.0, (name, q, mine[q])


def test_the_cases_reach_the_groupings_they_are_named_for():
    """what can be read off the terms alone: the groups, their widths and the launch geometry on 256 compute
    units (the device tests assert the same from the library's own report, whatever its device has)"""
    for name, c in G.CASES.items():
        e = c["expect"]
        terms = G.case_terms(name, random_terms)
        groups = G.d3_groups(terms, [E.NUMHYP[k] for k in c["kinds"]])
        if e.get("wide") or e.get("all_have_first"):
            assert groups is None, name
            continue
        assert groups, name
        geo = [G.d3_geometry(g, c["n"]) for g in groups]
        for key, field in (("nu", "nu"), ("pblocks", "pblocks"), ("p_pad", "p_pad")):
            if key in e:
                assert {q[field] for q in geo} == e[key], (name, key, geo)
        for key in ("W", "nh"):
            if key in e:
                assert {g[key] for g in groups} == e[key], (name, key)
        if "nhseq" in e:
            assert [g["nh"] for g in groups] == e["nhseq"], name
        if "groups" in e:
            assert len(groups) >= e["groups"], name
        if "d3split" in e:
            assert {(q["nsplit"], q["tps"]) for q in geo} == {e["d3split"]}, (name, geo)
        if "densesplit" in e:
            assert G.dense_geometry(len(terms), c["n"]) == e["densesplit"], name
    g = G.d3_groups(G.case_terms("nu4 one block n700", random_terms), [1] * 6)
    assert len(g) == 1 and 1024 < g[0]["p"] <= 2048
    g = G.d3_groups(G.case_terms("nu4 two blocks n700", random_terms), [1] * 6)
    assert len(g) == 1 and g[0]["p"] > 2048


def _defect_arguments(kind, groups, geo):
    if kind == "drop split":
        assert geo[0]["nsplit"] >= 2
        return (kind, 0, (0, 0), geo[0]["nsplit"] - 1)
    if kind in ("ragged w2", "half variant"):
        return (kind, 0)
    if kind in ("swap pair", "no factor 2"):
        return (kind, 0, 1)
    if kind == "wrong block":
        assert geo[0]["pblocks"] == 2 and geo[0]["nu"] == 4
        return (kind, 0, 0, 4)               # unit 0 of wave 0: run 0 is block 0's, run 4 block 1's
    if kind == "previous table":
        assert len(groups) >= 2
        return (kind, 1, 0)
    return (kind, 64, 2)


@pytest.mark.parametrize("what", list(G.DEFECTS))
def test_staged_defects_land_ten_times_above_the_tolerance(what):
    kind, name = G.DEFECTS[what]
    r = reference(name)
    groups = G.d3_groups(r["terms"], [E.NUMHYP[k] for k in r["kinds"]])
    geo = [G.d3_geometry(g, r["n"]) for g in groups]
    if kind in ("swap pair", "no factor 2"):
        assert groups[0]["nh"] == 2
    if kind == "ragged w2":
        assert r["n"] % 64
    q = "sqtmm_gradhyp" if kind in ("ragged w2", "no factor 2") else "tmatmul_gradhyp"
    want, tol = r["want"][q], r["tol"][q]
    clean = restated(r, None, q)[q]
    broken = restated(r, _defect_arguments(kind, groups, geo), q)[q]
    assert E.worst_ratio(clean, want, tol) <= 1.0
    worst = E.worst_ratio(broken, want, tol)
    flat = E.maxnorm_relerr(broken, want)
    print("%s (%s, %s): %.3g x tolerance on %d entries; max-norm error %.3g: the flat 1e-9 %s it" % (
        what, name, q, worst, int((E.ratio_map(broken, want, tol) > 1).sum()), flat,
        "passes" if flat < 1e-9 else "catches"))
    assert worst >= 10.0, (what, worst)


def test_the_report_entry_is_on_the_surface():
    """obhip_grad_plan_info: declared in include/obhip.h (so bound), purely additive, refuses null handles
    before it touches a device; outerbase.grad_plan_info is its accessor"""
    import outerbase_amd as ob
    from outerbase_amd import _lib
    assert _lib.lib.obhip_abi_version() == 5
    assert len(_lib.PROTOS["obhip_grad_plan_info"][1]) == 6
    assert callable(ob.outerbase.grad_plan_info)
    info = np.zeros(16, dtype=np.uint64)
    assert _lib.lib.obhip_grad_plan_info(None, None, info.ctypes.data, None, None, None) != 0
    assert b"null argument" in _lib.lib.obhip_last_error()
