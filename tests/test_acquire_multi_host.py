"""Host-side checks of the acquisition picks over several responses (no GPU): the closed form of the expected
hypervolume improvement against the definition by two-dimensional quadrature, the recurrences (one a, one d downdate,
q mean downdates) against explicit refits, the float64 restatement inside its allowance on every case
test_gpu_acquire_multi.py uses with the conditions those cases must meet, seven staged faults the instrument must
see, the front rule walked by a program of its own under the sanitizers, and the library's host side -- symbols,
Python names, argument errors that return before any device call."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import acquire_multi_ref as M
import acquire_ref as A
import extended_ref as E
from test_acquire_host import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ld = np.longdouble
NEW = {"obhip_acquire_multi_dev": 26, "obhip_acquire_multi": 26, "obhip_acquire_multi_layout": 6}
QS = (1, 2, 4)
P_HOST, M_HOST, K_HOST = 37, 60, 5


@functools.lru_cache(maxsize=None)
def mcase(name, p, m, seed, q):
    om_o, om_d, terms = model(name, p)
    return M.seeded_case(om_o, terms, m, seed, q), om_d, terms


@functools.lru_cache(maxsize=None)
def built(name, p, m, k, seed, q, criterion, lie, F0=3, best=True):
    """case, the reference along its own picks, C of the case and call -- computed once, shared, left unchanged; None:
    the criterion does not exist for this q"""
    mc, om_d, terms = mcase(name, p, m, seed, q)
    cfg = M.config_of(mc, criterion, lie, F0, best)
    if cfg is None:
        return None
    picks, ystar, st = M.states(mc, cfg, None, k)
    Cc, r = M.constant_of(mc, cfg, st, picks)
    return dict(mc=mc, cfg=cfg, picks=picks, ystar=ystar, st=st, C=Cc, r=r, om_d=om_d, terms=terms)


def main_built(q, criterion, lie, **kw):
    name, p, m, k = M.SHAPE
    return built(name, p, m, k, M.SEED + q, q, criterion, lie, **kw)


def host_built(q, criterion, lie, **kw):
    return built("d3", P_HOST, M_HOST, K_HOST, 31 + q, q, criterion, lie, **kw)


# ---- the closed form against the definition ----------------------------------------------------------------
# The quadrature runs at 18 digits and up to degree 5 of mpmath's rule (about 1e4 nodes per cell).  Its estimate is the
# difference of two successive levels: once they agree to the working precision it reports figures below the roundoff
# of the sum of the node values it has just formed, so the comparison allows that roundoff beside the estimate: 1e4
# units of 1e-18, 1e-14 relative, a hundred times under the 1e-12 the estimate itself is held to.
QUAD_DPS, QUAD_FLOOR = 18, 1e-14
FRONTS = {0: [], 1: [(0.3, 0.5)], 3: [(-0.4, 1.1), (0.2, 0.6), (0.9, -0.3)]}


def quad_ehvi(front, r, ms1, ms2, sd, extra=()):
    """E[HVI(y)] by mpmath.quad over the plane, split at the front's coordinates -> (value, error estimate)"""
    import mpmath as mp
    mp.mp.dps = QUAD_DPS
    fr = [(mp.mpf(a), mp.mpf(b)) for a, b in front]
    rr = (mp.mpf(r[0]), mp.mpf(r[1]))
    pdf = lambda y, m: mp.exp(-((y - m) / sd) ** 2 / 2) / (sd * mp.sqrt(2 * mp.pi))
    f = lambda y1, y2: M.hvi(fr, rr, (y1, y2)) * pdf(y1, ms1) * pdf(y2, ms2)
    x1 = sorted(set([p[0] for p in fr] + [mp.mpf(v) for v in extra if v < rr[0]]))
    x2 = sorted(set([p[1] for p in fr] + [mp.mpf(v) for v in extra if v < rr[1]]))
    lo1, lo2 = ms1 - 40 * sd, ms2 - 40 * sd                    # the densities are below 1e-340 beyond
    x1, x2 = [v for v in x1 if v > lo1], [v for v in x2 if v > lo2]
    return mp.quad(f, [min(lo1, rr[0] - 1)] + x1 + [rr[0]], [min(lo2, rr[1] - 1)] + x2 + [rr[1]], error=True, maxdegree=5)


@pytest.mark.parametrize("F", [0, 1, 3])
def test_strip_sum_agrees_with_the_quadrature_of_the_definition(F):
    """HVI(y) is the area of {z : y <= z < r, no front point <= z} (acquire_multi_ref.hvi, by slabs of the box minus
    the dominated boxes); its expectation under two independent normals by quadrature must agree with the strip sum
    within ten times the quadrature's own error estimate, which must be below 1e-12 relative"""
    import mpmath as mp
    mp.mp.dps = QUAD_DPS
    front, r = FRONTS[F], (1.5, 1.7)
    ms1, ms2, sd = mp.mpf("0.1"), mp.mpf("0.35"), mp.mpf("0.6")
    want, err = quad_ehvi(front, r, ms1, ms2, sd)
    got = M.ehvi_mp([(mp.mpf(a), mp.mpf(b)) for a, b in front], (mp.mpf(r[0]), mp.mpf(r[1])), ms1, ms2, sd * sd)
    print("F = %d: strip sum %s, quadrature %s, its error estimate %s, difference %s" % (
        F, mp.nstr(got, 18), mp.nstr(want, 18), mp.nstr(err, 3), mp.nstr(abs(got - want), 3)))
    mp.mp.dps = 50
    assert err < 1e-12 * abs(want)
    assert abs(got - want) <= 10 * max(err, QUAD_FLOOR * abs(want))


def test_strip_sum_at_a_tiny_sd_and_at_sd_zero():
    """sd = 1e-3: the quadrature is split at the means too; sd = 0: the value is HVI(ms) exactly, also where the mean
    lies on a front coordinate, is dominated or lies outside the box"""
    import mpmath as mp
    mp.mp.dps = QUAD_DPS
    front, r = FRONTS[1], (1.5, 1.7)
    ms1, ms2, sd = mp.mpf("0.1"), mp.mpf("0.35"), mp.mpf("0.001")
    ext = [ms1 - 12 * sd, ms1, ms1 + 12 * sd, ms2 - 12 * sd, ms2, ms2 + 12 * sd]
    want, err = quad_ehvi(front, r, ms1, ms2, sd, extra=ext)
    fr, rr = [(mp.mpf(a), mp.mpf(b)) for a, b in front], (mp.mpf(r[0]), mp.mpf(r[1]))
    got = M.ehvi_mp(fr, rr, ms1, ms2, sd * sd)
    print("sd = 1e-3: strip sum %s, quadrature %s, its error estimate %s" % (mp.nstr(got, 18), mp.nstr(want, 18), mp.nstr(err, 3)))
    mp.mp.dps = 50
    assert err < 1e-12 * abs(want) and abs(got - want) <= 10 * max(err, QUAD_FLOOR * abs(want))
    for F in (0, 1, 3):
        fr = [(mp.mpf(a), mp.mpf(b)) for a, b in FRONTS[F]]
        for y in [(0.1, 0.35), (-1.0, -1.0), (0.2, 0.6), (0.5, 0.9), (0.2, 0.2), (1.5, 0.0), (2.0, 2.0), (-0.4, 1.2)]:
            y = (mp.mpf(y[0]), mp.mpf(y[1]))
            assert M.ehvi_mp(fr, rr, y[0], y[1], mp.mpf(0)) == M.hvi(fr, rr, y), (F, y)


def test_front_rule_one_point_after_the_other_gives_the_undominated_set():
    """the device's insertion rule (acquire_multi_ref.insert) against pareto(), brute force, on a coarse grid with
    ties, duplicates and points outside the box, in two orders"""
    rng = np.random.default_rng(7)
    for trial in range(200):
        pts = [(float(a), float(b), 0.0, 0.0) for a, b in np.floor(rng.random((1 + trial % 30, 2)) * 12) / 10]
        r = (0.8, 0.9)
        for order in (pts, pts[::-1]):
            front = []
            for y in order:
                front = M.insert(front, y, r)
            assert [(p[0], p[1]) for p in front] == [(p[0], p[1]) for p in M.pareto(pts, r)]
            assert all(a[0] < b[0] and a[1] > b[1] for a, b in zip(front[:-1], front[1:]))


def test_front_rule_walked_by_a_program_of_its_own(tmp_path):
    """csrc/acquire_front.h is what the host normalises with and the pick kernel inserts with: plain C++, run here
    under the address and undefined-behaviour sanitizers against a brute-force set and at the capacity"""
    found = [shutil.which(c) for c in ("g++", "c++", "clang++")] + \
        [c for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(c)]
    found = [c for c in found if c]
    assert found, "no host C++ compiler: the walk of the front rule cannot run"
    exe = str(tmp_path / "acquire_front_check")
    subprocess.run([found[0], "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "acquire_front_check.cpp"), "-o", exe], check=True)
    result = subprocess.run([exe], capture_output=True, text=True)
    assert result.stderr == "", result.stderr
    assert result.returncode == 0, result.stdout
    assert result.stdout.split() == ["ok", "201"]


# ---- the recurrences ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lie", A.LIES)
@pytest.mark.parametrize("criterion", [M.CEI, M.EHVI])
def test_recurrences_agree_with_explicit_refits(criterion, lie):
    """q = 3, k = 5: one a, ONE downdate of d and q downdates of mu in long double against inv(H_t) and the q theta_t,r
    formed afresh at every step: the same picks, every mu, d, score, the front and the incumbent to 64 long-double
    roundoffs per summand and magnitude"""
    b = host_built(3, criterion, lie)
    mc, cfg, picks = b["mc"], b["cfg"], b["picks"]
    assert len(picks) == K_HOST
    got = M.recurrence64(mc, cfg, K_HOST, extended=True)
    assert list(got["index"]) == picks
    _, _, st = M.states(mc, cfg, picks, K_HOST, rnd=E.EPS)
    r = M.ratios(got, st, cfg, 64 * E.EPS)
    print("%r p=%d m=%d k=%d: long-double recurrences, err / (64 eps K magnitudes) %s"
          % (cfg, mc.p, mc.m, K_HOST, ", ".join("%s %.3g" % kv for kv in r.items())))
    assert max(r.values()) < 1


# ---- the committed cases ----------------------------------------------------------------------------------
def conditions(label, b, k, exempt=()):
    """what a case must meet on the reference alone: the constant not capped, at every step the top two scores more
    than one allowance apart, every believed-feasibility decision further from its limit than the mean's allowance"""
    st = b["st"]
    assert 8 * b["r"] < E.C_CAP, "%s: the constant is capped: the bound does not describe this case" % label
    gap = M.gap_ratio(st, b["C"], exempt)
    margin = min([s["margin"] for s in st if "margin" in s] + [np.inf])
    assert gap > 1, "%s: the top two scores are %.3g allowances apart: choose another seed" % (label, gap)
    assert margin > b["C"], "%s: a feasibility decision lies within the mean's allowance: choose another seed" % label
    return gap, margin


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("lie", A.LIES)
@pytest.mark.parametrize("criterion", M.CRITERIA)
def test_float64_restatement_stays_inside_its_allowance_and_the_cases_are_decided(criterion, lie, q):
    b = main_built(q, criterion, lie)
    if b is None:
        assert criterion == M.EHVI and q == 1                     # two objectives need two responses
        return
    mc, cfg, st, picks = b["mc"], b["cfg"], b["st"], b["picks"]
    k = M.SHAPE[3]
    got = M.recurrence64(mc, cfg, k)
    gap, margin = conditions(repr(cfg), b, k)
    w = M.ratios(got, st, cfg, b["C"])
    print("%r: float64 restatement err / bound %.3g (C = %.3g, cap %.3g), err / tolerance %s, smallest gap / allowance "
          "%.3g, feasible picks %s, front sizes %s" % (cfg, b["r"], b["C"], E.C_CAP, ", ".join("%s %.3g" % kv for kv in w.items()),
                                                      gap, [s.get("feasible") for s in st[:-1]], [len(s["front"]) for s in st]))
    assert len(picks) == k
    assert list(got["index"]) == picks and max(w.values()) < 1


def test_the_cases_exercise_the_feasibility_switch_and_the_front():
    """among the committed calls: a believed-feasible and a believed-infeasible pick, a front that grows, and a front
    that loses a point to a pick"""
    seen = set()
    for q in (2, 4):
        for lie in A.LIES:
            st = main_built(q, M.CEI, lie)["st"]
            seen |= {("feasible", s["feasible"]) for s in st if "feasible" in s}
            st = main_built(q, M.EHVI, lie)["st"]
            for a, b in zip(st[:-1], st[1:]):
                fa, fb = {(p[0], p[1]) for p in a["front"]}, {(p[0], p[1]) for p in b["front"]}
                if fb - fa:
                    seen.add("extended")
                if fa - fb:
                    seen.add("knocked out")
    print(sorted(map(str, seen)))
    assert {("feasible", True), ("feasible", False), "extended", "knocked out"} <= seen


# ---- staged faults ------------------------------------------------------------------------------------------
def test_the_instrument_sees_seven_staged_faults():
    def run(b, mutate, k=None):
        k = len(b["picks"]) if k is None else k
        got = M.recurrence64(b["mc"], b["cfg"], k, force=b["picks"], mutate=mutate)
        return got, M.ratios(got, b["st"], b["cfg"], b["C"])
    ehvi, cei = host_built(3, M.EHVI, A.BELIEVER), host_built(3, M.CEI, A.CONSTANT)
    for b in (ehvi, cei):
        got, good = run(b, None)
        assert max(good.values()) < 1 and list(got["own"]) == b["picks"]
    assert len(ehvi["st"][0]["front"]) >= 1 and len(ehvi["cfg"].cons) >= 1
    for mutate in ("strip left out", "c_s from front point s"):
        got, r = run(ehvi, mutate)
        print("%s: %s" % (mutate, r))
        assert r["score0"] > 1 and r["pof0"] < 1 and r["mean"] < 1
    # a constraint factor missing, a >= constraint scored as <=
    four = host_built(4, M.CEI, A.BELIEVER)
    assert any(four["cfg"].g[j] < 0 for j in four["cfg"].cons) and len(four["cfg"].cons) >= 2
    for mutate in ("constraint factor missing", ">= scored as <="):
        got, r = run(four, mutate)
        print("%s: %s" % (mutate, r))
        assert r["score0"] > 1 and r["pof0"] > 1 and r["mean"] < 1
    # d downdated once per response: the variance after the picks
    got, r = run(cei, "d downdated per response")
    print("d downdated per response: %s" % r)
    assert r["var"] > 1 and r["mean"] < 1
    # a believed-infeasible pick moves the incumbent: the case must hold such a pick that improves on the incumbent
    b = next((c for c in (host_built(q, M.CEI, lie, best=bst) for q in (2, 3, 4) for lie in A.LIES for bst in (True, False))
              if any(s.get("feasible") is False for s in c["st"])), None)
    assert b is not None, "no committed host case has a believed-infeasible pick"
    got, r = run(b, "infeasible pick moves the incumbent")
    print("infeasible pick moves the incumbent (%r): %s, own picks %s against %s" % (b["cfg"], r, list(got["own"]), b["picks"]))
    assert r["best"] > 1 or r.get("score", 0) > 1 or list(got["own"]) != b["picks"]
    # a dominated point left in the front: the case must knock a point out
    b = next((c for c in (host_built(q, M.EHVI, lie, F0=f) for q in (2, 3, 4) for lie in A.LIES for f in (3, 7))
              if any({(p[0], p[1]) for p in s0["front"]} - {(p[0], p[1]) for p in s1["front"]} for s0, s1 in zip(c["st"][:-1], c["st"][1:]))), None)
    assert b is not None, "no committed host case knocks a point out of the front"
    got, r = run(b, "dominated point left in the front")
    print("dominated point left in the front (%r): %s" % (b["cfg"], r))
    assert r["front"] > 1


# ---- the library's host side ------------------------------------------------------------------------------
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


def test_python_names_makefile_and_no_switch_of_its_own():
    import outerbase_amd as ob
    assert "AcquireMultiResult" in ob.__all__ and hasattr(ob, "AcquireMultiResult")
    assert callable(ob.Posterior.acquire_multi)
    assert "picks do not move" in ob.Posterior.acquire_multi.__doc__
    csrc = os.path.join(ROOT, "outerbase_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "kernels_acquire_multi.hip" in mk and "acquire_multi.cpp" in mk and "acquire_front.h" in mk
    for f in ("kernels_acquire_multi.hip", "acquire_multi.cpp", "acquire_front.h"):
        src = open(os.path.join(csrc, f)).read()
        code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
        assert "getenv" not in code, f                                   # the switch lives in launch_predict
        assert "atomic" not in code and "Cooperative" not in code and "grid_group" not in code, f
    # the argmax comparison exists once, in the header both kernel files include
    assert "bool beats(" in open(os.path.join(csrc, "acquire_device.h")).read()
    for f in ("kernels_acquire.hip", "kernels_acquire_multi.hip"):
        assert "bool beats(" not in open(os.path.join(csrc, f)).read(), f


def test_layout_entry():
    from outerbase_amd._lib import lib
    lds, mq, mf = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert lib.obhip_acquire_multi_layout(4, 3, 2048, C.byref(lds), C.byref(mq), C.byref(mf)) == 0
    assert (mq.value, mf.value) == (16, 2048) and lds.value >= 2 * 2049 * 8 and lds.value <= 40 * 1024
    small = C.c_uint64(0)
    assert lib.obhip_acquire_multi_layout(4, 0, 100, C.byref(small), None, None) == 0 and small.value < 1024
    for q, crit, cap in ((0, 0, 0), (17, 0, 0), (1, 4, 0), (1, -1, 0), (2, 3, 2049)):
        lds.value = 77
        assert lib.obhip_acquire_multi_layout(q, crit, cap, C.byref(lds), None, None) == 1 and lds.value == 77


def test_argument_errors_return_before_any_device_call():
    from outerbase_amd._lib import lib
    buf = (C.c_double * 8192)()
    a = C.cast(buf, C.c_void_p)
    n, nf, bo = C.c_uint64(77), C.c_uint64(78), C.c_double(79.0)
    nan, inf = float("nan"), float("inf")
    i32 = lambda v: (C.c_int32 * len(v))(*v)
    f64 = lambda v: (C.c_double * len(v))(*v)
    for f in (lib.obhip_acquire_multi_dev, lib.obhip_acquire_multi):
        def refused(msg, q=2, crit=0, roles=(0, 1), signs=(1.0, -1.0), limits=(0.0, 0.5), xi=0.0, front=None, F0=0, lie=0,
                    lv=None, m=10, k=3, theta=a, x=a, index=a, score=a, np_=C.byref(n)):
            rc = f(None, theta, q, x, m, crit, None if roles is None else i32(roles), f64(signs), f64(limits), xi,
                   None if front is None else f64(front), F0, lie, None if lv is None else f64(lv), None, k, index, score,
                   None, None, None, None, a, C.byref(nf), C.byref(bo), np_)
            assert rc == 1 and msg in lib.obhip_last_error(), (msg, rc, lib.obhip_last_error())
        refused(b"m = 0", m=0)
        refused(b"k = 0", k=0)
        refused(b"q must be", q=0)
        refused(b"q must be", q=17)
        refused(b"criterion", crit=4)
        refused(b"criterion", crit=-1)
        refused(b"lie must be", lie=2)
        refused(b"null roles", roles=None)
        refused(b"roles must be", roles=(0, 3))
        refused(b"signs must be", signs=(1.0, 0.5))
        refused(b"takes 1 objectives", roles=(0, 0))                       # two objectives with CEI
        refused(b"takes 1 objectives", roles=(1, 1))
        refused(b"takes 2 objectives", crit=3)
        refused(b"takes 0 objectives", crit=2)
        refused(b"at least one constraint", crit=2, roles=(2, 2))
        for bad in (nan, inf, -inf):
            refused(b"xi", xi=bad)
            refused(b"limit must be finite", limits=(0.0, bad))
            refused(b"reference point", crit=3, roles=(0, 0), limits=(bad, 0.0))
            refused(b"front's points", crit=3, roles=(0, 0), front=(0.0, bad), F0=1)
            refused(b"lie_value", lie=1, lv=(0.0, bad))
        refused(b"incumbent", limits=(nan, 0.5))
        refused(b"incumbent", limits=(-inf, 0.5))                          # minimised: -inf is not "no run yet"
        refused(b"incumbent", signs=(-1.0, 1.0), limits=(inf, 0.5))        # maximised: +inf in the caller's sign is
        refused(b"null posterior", limits=(inf, 0.5))                      # +inf in the signed sense goes through
        refused(b"null posterior", signs=(-1.0, 1.0), limits=(-inf, 0.5))
        refused(b"null lie_value", lie=1)
        refused(b"null front0", crit=3, roles=(0, 0), F0=2)
        refused(b"2048", crit=3, roles=(0, 0), front=(0.0,) * 4090, F0=2045, k=4)
        refused(b"null posterior", crit=3, roles=(0, 0), front=(0.0,) * 4090, F0=2045, k=3)
        refused(b"null candidates", x=None)
        refused(b"null outputs", index=None)
        refused(b"null outputs", score=None)
        refused(b"null outputs", np_=None)
        refused(b"d_Theta is null", theta=None)
        refused(b"null posterior")
    assert (n.value, nf.value, bo.value) == (77, 78, 79.0) and not any(buf)     # a refused call changes nothing


def test_shape_and_argument_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    from test_sobol_host import golden_model
    mdl = golden_model("mixed_d3")
    om, terms = mdl["om_d"], mdl["terms"]
    post = ob.Posterior(om, ob.obmod._terms_of(om, terms), C.c_void_p(1))               # never reaches the library
    p = len(terms)
    try:
        x, Th = np.full((5, 3), 0.5), np.zeros((p, 3))
        ok = dict(objective=0, best=0.0, constraints=[(1, "<=", 0.5)])
        bad = [dict(ok, k=0), dict(ok, criterion="ei"), dict(ok, criterion="ehvi"), dict(ok, objective=(0, 1)),
               dict(ok, objective=3), dict(ok, objective=1), dict(ok, constraints=[(1, "<", 0.5)]),
               dict(ok, constraints=[(1, "<=", float("nan"))]), dict(ok, constraints=[(1, "<=", 0.5), (1, ">=", 0.1)]),
               dict(ok, constraints=[(5, "<=", 0.5)]), dict(ok, best=float("nan")), dict(ok, xi=float("inf")),
               dict(ok, lie="liar"), dict(ok, lie="constant"), dict(ok, lie="constant", lie_value=[0.0, 0.0]),
               dict(ok, lie="constant", lie_value=[0.0, float("nan"), 0.0]), dict(ok, skip=np.zeros(4)),
               dict(ok, ref=[0.0, 0.0]), dict(ok, front=[[0.0, 0.0]]), dict(ok, maximize=[True, False]),
               dict(objective=None), dict(criterion="pof", objective=0, constraints=[(1, "<=", 0.5)]),
               dict(objective=(0, 2)), dict(objective=(2, 0), ref=[1.0, 1.0]), dict(objective=(0, 2), ref=[1.0, float("inf")]),
               dict(objective=(0, 2), ref=[1.0, 1.0], best=0.0), dict(objective=(0, 2), ref=[1.0, 1.0], front=[[0.0, float("nan")]]),
               dict(objective=(0, 2), ref=[1.0, 1.0], front=np.zeros((2047, 2)), k=2)]
        for kw in bad:
            with pytest.raises(ValueError):
                post.acquire_multi(x, Th, **{"k": 2, **kw})
        with pytest.raises(ValueError):
            post.acquire_multi(x[:, :2], Th, **ok)
        with pytest.raises(ValueError):
            post.acquire_multi(x[:0], Th, **ok)
        with pytest.raises(ValueError):
            post.acquire_multi(x, Th[:-1], **ok)
        with pytest.raises(ValueError):
            post.acquire_multi(x, np.zeros((p, 17)), **ok)
        post.meansd = np.array([[0.0, 1.0, 5.0]] * 2)
        with pytest.raises(ValueError):                                                 # meansd of another q
            post.acquire_multi(x, Th, **ok)
        post.meansd = np.array([[0.0, 1.0, 5.0], [0.0, 0.0, 5.0], [0.0, 1.0, 5.0]])
        with pytest.raises(ValueError):                                                 # a scale <= 0, as in _scale
            post.acquire_multi(x, Th, **ok)
    finally:
        post._h = None


@pytest.mark.parametrize("what", ["F0=0", "F0=1", "F0=7", "m=1", "m=257", "no incumbent"])
def test_the_further_cases_of_the_gpu_file_are_decided(what):
    """the other calls test_gpu_acquire_multi.py makes, on the reference alone: the same conditions"""
    name, p, _, k = M.SHAPE
    if what.startswith("F0"):
        bs = [main_built(2, M.EHVI, A.BELIEVER, F0=int(what[3:]))]
    elif what.startswith("m="):
        bs = [built(name, p, int(what[2:]), k, M.SEED + 50 + int(what[2:]), 2, crit, A.CONSTANT) for crit in (M.CEI, M.EHVI)]
    else:
        bs = [main_built(q, M.CEI, lie, best=False) for q in (2, 4) for lie in A.LIES]
    for b in bs:
        gap, margin = conditions("%s %r" % (what, b["cfg"]), b, k)
        got = M.recurrence64(b["mc"], b["cfg"], k)
        w = M.ratios(got, b["st"], b["cfg"], b["C"])
        print("%s %r: gap / allowance %.3g, err / tolerance %s" % (what, b["cfg"], gap, w))
        assert list(got["index"]) == b["picks"] and max(w.values()) < 1
