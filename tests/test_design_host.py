"""Host-side checks of the sequential design (no GPU): the downdating recurrences against explicit
long-double refits (tests/design_ref.py), the float64 restatement inside its allowance, three mutations
the instrument must reject, the identities of the two criteria, and the library's host side -- symbols,
Python names, the Makefile, no new switch, argument errors that return before any device call."""
import ctypes as C
import functools
import glob
import os
import re

import numpy as np
import pytest

import design_ref as D
import extended_ref as E
from test_sobol_host import golden_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ld = np.longdouble
NEW = {"obhip_posterior_create_dev": 5, "obhip_posterior_destroy": 1, "obhip_posterior_info": 4,
       "obhip_normal_acc_posterior_dev": 5, "obhip_posterior_var_dev": 5, "obhip_posterior_condition_dev": 4,
       "obhip_design_select_dev": 15, "obhip_design_select": 15}
P_HOST, M_HOST, K_HOST = 37, 130, 12
CRITERIA = [D.MAXVAR, D.IMSE]


@functools.lru_cache(maxsize=None)
def host_case(criterion, weighted=False):
    """p = 37, m = 130, 12 steps on the golden mixed_d3 model; weighted: one candidate a million times the rest"""
    mdl = golden_model("mixed_d3")
    terms = np.ascontiguousarray(mdl["om_o"].selectterms(P_HOST))
    w = None
    if weighted:
        w = np.ones(M_HOST)
        w[7] = 1e6
    c = D.seeded_case(mdl["om_o"], terms, M_HOST, criterion, seed=11, weights=w)
    picks, st = D.states(c, None, K_HOST)
    return c, picks, st


@pytest.mark.parametrize("criterion", CRITERIA)
def test_recurrences_agree_with_explicit_refits(criterion):
    """the downdates in long double against inv(H + sum b b^T / nu) formed afresh at every step: the same picks,
    and every score, variance, num and trace to 64 long-double roundoffs per summand and magnitude"""
    c, picks, st = host_case(criterion)
    assert len(picks) == K_HOST
    got = D.recurrence64(c, K_HOST, extended=True)
    assert list(got["index"]) == picks
    r = D.ratios(got, st, 64 * E.EPS)
    rel = float(np.max(np.abs(E._f64(got["trace"] - np.array([s["trace"] for s in st], dtype=ld))
                              / np.maximum(np.abs(E._f64(got["trace"])), 1e-300))))
    print("%s p=%d m=%d k=%d: long-double recurrences, err / (64 eps K magnitudes) %s; traces agree to %.3g relative"
          % (criterion, c.p, c.m, K_HOST, ", ".join("%s %.3g" % kv for kv in r.items()), rel))
    assert max(r.values()) < 1
    assert rel < 1e-15


@pytest.mark.parametrize("criterion", CRITERIA)
def test_float64_restatement_stays_inside_its_allowance(criterion):
    c, picks, st = host_case(criterion)
    Cc, r = D.constant_of(c, st, picks)
    got = D.recurrence64(c, K_HOST)
    gap = D.gap_ratio(st, Cc)
    w = D.ratios(got, st, Cc)
    print("%s: float64 restatement err / bound %.3g (C = %.3g, cap %.3g), err / tolerance %s, smallest gap / allowance %.3g"
          % (criterion, r, Cc, E.C_CAP, ", ".join("%s %.3g" % kv for kv in w.items()), gap))
    assert 8 * r < E.C_CAP, "the constant is capped: the bound does not describe this case"
    assert gap > 1000, "the seeded candidates do not separate the top two scores"
    assert list(got["index"]) == picks and max(w.values()) < 1


def test_the_instrument_rejects_three_mutations():
    c, picks, st = host_case(D.IMSE)
    Cc, _ = D.constant_of(c, st, picks)
    good = D.ratios(D.recurrence64(c, K_HOST, force=picks), st, Cc)
    assert max(good.values()) < 1
    no_nu = D.ratios(D.recurrence64(c, K_HOST, force=picks, mutate="gamma without nu"), st, Cc)
    no_tau = D.ratios(D.recurrence64(c, K_HOST, force=picks, mutate="tau term dropped"), st, Cc)
    print("gamma without nu: %s; a^2 tau / gamma^2 dropped: %s" % (no_nu, no_tau))
    assert no_nu["var"] > 1 and no_nu["trace"] > 1 and no_nu["num"] > 1
    assert no_tau["num"] > 1 and no_tau["score"] > 1 and no_tau["var"] < 1       # d does not depend on tau
    # the same for maxvar's gamma
    cm, pm, sm = host_case(D.MAXVAR)
    Cm, _ = D.constant_of(cm, sm, pm)
    mv = D.ratios(D.recurrence64(cm, K_HOST, force=pm, mutate="gamma without nu"), sm, Cm)
    assert mv["var"] > 1 and mv["trace"] > 1
    # a picked row that is not masked: one heavily weighted candidate is picked again and again
    for crit in CRITERIA:
        cw, pw, _ = host_case(crit, True)
        assert pw[0] == 7 and len(set(pw)) == K_HOST
        bad = D.recurrence64(cw, K_HOST, mutate="picked row not masked")
        print("%s, picked row not masked: picks %s" % (crit, list(bad["index"])))
        assert list(bad["index"]) != pw and list(bad["index"]).count(7) > 1
        assert list(D.recurrence64(cw, K_HOST)["index"]) == pw


def test_identities_of_the_two_criteria():
    c, picks, st = host_case(D.MAXVAR)
    # greedy D-optimality: the trace is the growth of log det H
    gain = st[-1]["logdet"] - st[0]["logdet"]
    assert abs(float(st[-1]["trace"] - gain)) <= 64 * E.EPS * c.p * abs(float(gain))
    got = D.recurrence64(c, K_HOST)
    Cc, _ = D.constant_of(c, st, picks)
    assert abs(float(got["trace"][-1] - gain)) <= Cc * st[-1]["bound_trace"]
    # conditioning never raises a variance
    for a, b in zip(st[:-1], st[1:]):
        assert np.all(b["d"] <= a["d"])
    # I-optimality with unit weights: the scores are the drops of the integrated variance
    ci, pi, si = host_case(D.IMSE)
    drops = sum(si[t]["score"][pi[t]] for t in range(K_HOST))
    total = si[0]["trace"] - si[-1]["trace"]
    assert abs(float(drops - total)) <= 64 * E.EPS * (c.p + K_HOST) * float(si[0]["trace"])
    assert np.all(np.diff(E._f64(np.array([s["trace"] for s in si], dtype=ld))) < 0)
    for a, b in zip(si[:-1], si[1:]):
        assert np.all(b["d"] <= a["d"])


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


def test_python_names_makefile_and_no_new_switch():
    import outerbase_amd as ob
    for name in ("Posterior", "DesignResult"):
        assert name in ob.__all__ and hasattr(ob, name)
    for meth in ("from_hessian", "var", "condition", "select", "logdet"):
        assert hasattr(ob.Posterior, meth)
    assert callable(ob.NewtonAccumulator.posterior)
    assert "scale" in ob.Posterior.select.__doc__                       # the picks do not depend on the response scale
    csrc = os.path.join(ROOT, "outerbase_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "kernels_design.hip" in mk and "design.cpp" in mk
    read = set()
    for f in ("kernels_design.hip", "design.cpp", "posterior.cpp"):
        read |= set(re.findall(r'getenv\("(OBHIP_[A-Z0-9_]+)"\)', open(os.path.join(csrc, f)).read()))
    assert read == {"OBHIP_FORCE_GENERIC"}
    # the step is kernel boundaries only: nothing cooperative, no atomics in the new kernels
    src = open(os.path.join(csrc, "kernels_design.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert "atomic" not in code and "Cooperative" not in code and "grid_group" not in code


def test_argument_errors_return_before_any_device_call():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    from conftest import knots_for
    mdl = golden_model("mixed_d3")
    om, t = mdl["om_d"], ob.obmod._Terms(mdl["om_d"], mdl["terms"])
    buf = (C.c_double * 4096)()
    a = C.cast(buf, C.c_void_p)
    h, n = C.c_void_p(), C.c_uint64(77)
    sel = lib.obhip_design_select_dev
    for f in (sel, lib.obhip_design_select):
        assert f(None, a, 10, 0, None, 0, None, None, 0, 0, a, a, a, a, C.byref(n)) == 1      # k = 0
        assert b"k = 0" in lib.obhip_last_error()
        assert f(None, a, 0, 0, None, 0, None, None, 3, 0, a, a, a, a, C.byref(n)) == 1       # no candidates
        assert f(None, a, 10, 2, None, 0, None, None, 3, 0, a, a, a, a, C.byref(n)) == 1      # no such criterion
        assert b"criterion" in lib.obhip_last_error()
        assert f(None, a, 10, 1, None, 0, None, None, 3, 0, a, a, a, a, C.byref(n)) == 1      # imse without a reference
        assert b"reference" in lib.obhip_last_error()
        assert f(None, a, 10, 1, a, 0, None, None, 3, 0, a, a, a, a, C.byref(n)) == 1
        assert b"reference" in lib.obhip_last_error()
        assert f(None, None, 10, 0, None, 0, None, None, 3, 0, a, a, a, a, C.byref(n)) == 1
        assert f(None, a, 10, 0, None, 0, None, None, 3, 0, None, a, a, a, C.byref(n)) == 1   # NULL outputs
        assert b"outputs" in lib.obhip_last_error()
        assert f(None, a, 10, 0, None, 0, None, None, 3, 0, a, None, a, a, C.byref(n)) == 1
        assert f(None, a, 10, 0, None, 0, None, None, 3, 0, a, a, a, a, None) == 1
        assert f(None, a, 10, 0, None, 0, None, None, 3, 0, a, a, None, None, C.byref(n)) == 1  # var, trace may be NULL:
        assert b"null posterior" in lib.obhip_last_error()                                      # ... the handle is what is missing
    assert n.value == 77                                                                        # a refused call changes nothing
    create = lib.obhip_posterior_create_dev
    assert create(None, om._h, t._h, a, 0.0) == 1 and create(C.byref(h), None, t._h, a, 0.0) == 1
    assert create(C.byref(h), om._h, None, a, 0.0) == 1 and create(C.byref(h), om._h, t._h, None, 0.0) == 1
    assert create(C.byref(h), om._h, t._h, a, float("nan")) == 1
    # terms of another model's dimension count: p and d cannot belong together
    other = ob.outermod()
    ob.setcovfs(other, ["mat25"])
    ob.setknot(other, knots_for(["mat25"], 20))
    assert create(C.byref(h), other._h, t._h, a, 0.0) == 1
    assert h.value is None
    assert lib.obhip_posterior_info(None, None, None, None) == 1
    assert lib.obhip_posterior_var_dev(None, a, 4, a, 0) == 1
    assert lib.obhip_posterior_condition_dev(None, a, 4, C.byref(h)) == 1
    assert lib.obhip_normal_acc_posterior_dev(None, None, 0.0, 6.0, C.byref(h)) == 1
    assert lib.obhip_posterior_destroy(None) == 0


def test_shape_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    om, terms = mdl["om_d"], mdl["terms"]
    with pytest.raises(ValueError):
        ob.Posterior.from_hessian(om, terms, np.eye(len(terms) + 1), 0.0)               # mismatched p
    post = ob.Posterior(om, ob.obmod._terms_of(om, terms), C.c_void_p(1))               # never reaches the library
    try:
        x = np.full((5, 3), 0.5)
        with pytest.raises(ValueError):
            post.select(x, 0)
        with pytest.raises(ValueError):
            post.select(x[:, :2], 2)
        with pytest.raises(ValueError):
            post.select(x, 2, criterion="imse")
        with pytest.raises(ValueError):
            post.select(x, 2, criterion="ei")
        with pytest.raises(ValueError):
            post.select(x, 2, weights=np.ones(4))
        with pytest.raises(ValueError):
            post.select(x, 2, criterion="imse", reference=x, ref_weights=np.ones(4))
        with pytest.raises(ValueError):
            post.var(x[:, :2])
        with pytest.raises(ValueError):
            post.condition(x[:0])
    finally:
        post._h = None
