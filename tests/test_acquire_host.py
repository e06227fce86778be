"""Host-side checks of the acquisition picks (no GPU): the long-double part of the reference (tests/acquire_ref.py)
against mpmath's own Cholesky, the recurrences of mu and d against explicit refits, the float64 restatement inside
its allowance on every case test_gpu_acquire.py uses, the conditions those cases must meet, six mutations the
instrument must reject, and the library's host side -- symbols, Python names, the Makefile, no switch of its own,
argument errors that return before any device call."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import acquire_ref as A
import design_ref as D
import extended_ref as E
from test_sobol_host import d5_model, golden_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ld = np.longdouble
NEW = {"obhip_acquire_dev": 17, "obhip_acquire": 17}
P_HOST, M_HOST, K_HOST = 37, 130, 12


@functools.lru_cache(maxsize=None)
def model(name, p):
    mdl = {"d3": lambda: golden_model("mixed_d3"), "d8": lambda: golden_model("ref_basic_d8"), "d5": d5_model}[name]()
    terms = np.ascontiguousarray(mdl["om_o"].selectterms(p))
    assert len(terms) == p
    return mdl["om_o"], mdl["om_d"], terms


@functools.lru_cache(maxsize=None)
def wide_model():
    from test_gpu_predict_grad import wide
    kinds, om_o, om_d, terms, used, _ = wide()
    assert used == 198
    return om_o, om_d, np.ascontiguousarray(terms)


@functools.lru_cache(maxsize=None)
def shape_case(name, p, m, k, seed):
    om_o, om_d, terms = wide_model() if name == "wide" else model(name, p)
    c = A.seeded_case(om_o, terms, m, seed)
    return c, om_d, terms, A.configs_of(c)


@functools.lru_cache(maxsize=None)
def built(name, p, m, k, seed, ci):
    """case, the reference along its own picks, C of the case and call -- computed once, shared, left unchanged"""
    c, om_d, terms, cfgs = shape_case(name, p, m, k, seed)
    cfg = cfgs[ci]
    picks, ystar, st = A.states(c, cfg, None, k)
    Cc, r = A.constant_of(c, cfg, st, picks)
    return dict(c=c, cfg=cfg, picks=picks, ystar=ystar, st=st, C=Cc, r=r, om_d=om_d, terms=terms)


def host_built(ci):
    return built("d3", P_HOST, M_HOST, K_HOST, 11, ci)


def cfg_index(crit, lie, mx):
    return (A.CRITERIA.index(crit) * 2 + A.LIES.index(lie)) * 2 + int(mx)


# ---- the instrument ------------------------------------------------------------------------------------
def mp_cholesky(H):
    """mpmath's own Cholesky at 50 digits of the long-double H, back as long double"""
    import mpmath
    mpmath.mp.dps = 50
    p = H.shape[0]
    M = mpmath.matrix(p, p)
    for i in range(p):
        for j in range(p):
            M[i, j] = A.to_mp(H[i, j])
    L = mpmath.cholesky(M)
    out = np.zeros((p, p), dtype=ld)
    for i in range(p):
        for j in range(i + 1):
            out[i, j] = A.from_mp(L[i, j])
    return out


@pytest.mark.parametrize("lie", A.LIES)
def test_the_reference_against_mpmaths_own_cholesky(lie):
    """p = 12, m = 7, k = 3: mu, d and the scores of every step with posterior_ref.cholesky_ld and with mpmath's
    factor agree to 64 long-double roundoffs per summand and magnitude, and the picks are the same"""
    om_o, _, terms = model("d3", 12)
    c = A.seeded_case(om_o, terms, 7, 5)
    for cfg in A.configs_of(c):
        if cfg.lie != lie:
            continue
        picks, ys, st = A.states(c, cfg, None, 3)
        picks2, ys2, st2 = A.states(c, cfg, None, 3, cholesky=mp_cholesky)
        assert picks == picks2 and len(picks) == 3
        worst = 0.0
        for a, b in zip(st, st2):
            tol = 64 * E.EPS
            worst = max(worst, E.worst_ratio(a["mu"], b["mu"], tol * b["bound_mu"]), E.worst_ratio(a["d"], b["d"], tol * b["bound_d"]))
            if "raw" in a:
                worst = max(worst, E.worst_ratio(a["raw"], b["raw"], tol * b["bound_score"] + 64 * E.EPS * np.abs(E._f64(b["raw"]))))
        print("%r: cholesky_ld against mpmath's Cholesky, err / (64 eps K magnitudes) %.3g" % (cfg, worst))
        assert worst < 1


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("lie", A.LIES)
@pytest.mark.parametrize("crit", A.CRITERIA)
def test_recurrences_agree_with_explicit_refits(crit, lie, maximize):
    """the downdates of mu and d in long double against inv(H_t) and theta_t formed afresh at every step: the same
    picks, and every mu, d and score to 64 long-double roundoffs per summand and magnitude"""
    b = host_built(cfg_index(crit, lie, maximize))
    c, cfg, picks = b["c"], b["cfg"], b["picks"]
    assert len(picks) == K_HOST
    got = A.recurrence64(c, cfg, K_HOST, extended=True)
    assert list(got["index"]) == picks
    _, _, st = A.states(c, cfg, picks, K_HOST, rnd=E.EPS)
    r = A.ratios(got, st, 64 * E.EPS)
    print("%r p=%d m=%d k=%d: long-double recurrences, err / (64 eps K magnitudes) %s"
          % (cfg, c.p, c.m, K_HOST, ", ".join("%s %.3g" % kv for kv in r.items())))
    assert max(r.values()) < 1


@pytest.mark.parametrize("name,p,m,k,seed", A.SHAPES + [A.WIDE, ("d3", P_HOST, M_HOST, K_HOST, 11)])
def test_float64_restatement_stays_inside_its_allowance_and_the_cases_are_decided(name, p, m, k, seed):
    """on every case the GPU file uses, on the reference alone: the float64 restatement inside its allowance with
    8 r < C_CAP, and the top two eligible scores of every step more than 1000 allowances apart"""
    for ci in range(16):
        b = built(name, p, m, k, seed, ci)
        c, cfg, st, picks = b["c"], b["cfg"], b["st"], b["picks"]
        got = A.recurrence64(c, cfg, k)
        gap = A.gap_ratio(st, b["C"])
        w = A.ratios(got, st, b["C"])
        print("%s p=%d m=%d k=%d %r: float64 restatement err / bound %.3g (C = %.3g, cap %.3g), err / tolerance %s, "
              "smallest gap / allowance %.3g" % (name, c.p, m, k, cfg, b["r"], b["C"], E.C_CAP,
                                                 ", ".join("%s %.3g" % kv for kv in w.items()), gap))
        assert 8 * b["r"] < E.C_CAP, "the constant is capped: the bound does not describe this case"
        assert gap > 1000, "the seeded candidates do not separate the top two scores: choose another seed"
        assert len(picks) == min(k, m)
        assert list(got["index"]) == picks and max(w.values()) < 1


def test_the_criteria_trade_mean_against_variance_and_the_lie_decides():
    """EI, PI and LCB pick neither the k lowest means nor select(maxvar)'s picks; the constant liar and the believer
    part ways from the second pick on"""
    for crit in (A.EI, A.PI, A.LCB):
        b = host_built(cfg_index(crit, A.BELIEVER, False))
        c, picks = b["c"], b["picks"]
        lowest = list(np.argsort(E._f64(b["st"][0]["mu"]), kind="stable")[:K_HOST])
        dc = D.make_case(model("d3", P_HOST)[0], c.terms, c.H, c.sigma, c.xcand, D.MAXVAR)
        maxvar = D.states(dc, None, K_HOST)[0]
        print("%s picks %s; lowest means %s; maxvar %s" % (crit, picks, lowest, maxvar))
        assert set(picks) != set(lowest) and set(picks) != set(maxvar) and picks != maxvar
    differ = 0
    for crit in A.CRITERIA:
        one, two = host_built(cfg_index(crit, A.BELIEVER, False)), host_built(cfg_index(crit, A.CONSTANT, False))
        assert one["picks"][0] == two["picks"][0]                          # the first pick is made before any lie
        differ += one["picks"][1:] != two["picks"][1:]
    assert differ >= 1


def test_the_instrument_rejects_six_mutations():
    def run(ci, mutate, follow=True):
        b = host_built(ci)
        got = A.recurrence64(b["c"], b["cfg"], K_HOST, force=b["picks"] if follow else None, mutate=mutate)
        return b, got, A.ratios(got, b["st"], b["C"]) if follow else None
    for ci in range(16):
        b, got, good = run(ci, None)
        assert max(good.values()) < 1 and list(got["own"]) == b["picks"]
    # the a delta / gamma mean update dropped under the liar: the means are off
    b, got, r = run(cfg_index(A.EI, A.CONSTANT, False), "mean update dropped")
    print("mean update dropped: %s" % r)
    assert r["mean"] > 1 and r["var"] < 1
    # the incumbent not updated: the constant lie lies below best - ... only when the lie improves on best
    b = host_built(cfg_index(A.EI, A.BELIEVER, False))
    assert any(float(A.incumbent(b["cfg"], b["ystar"][:t + 1])) < b["cfg"].best for t in range(K_HOST)), \
        "no believer value improves on the incumbent: the mutation cannot show"
    b, got, r = run(cfg_index(A.EI, A.BELIEVER, False), "incumbent not updated")
    print("incumbent not updated: %s, own picks %s" % (r, list(got["own"])))
    assert r["score"] > 1 or list(got["own"]) != b["picks"]
    # Phi(-u) for Phi(u)
    for crit in (A.EI, A.PI):
        b, got, r = run(cfg_index(crit, A.BELIEVER, False), "Phi(-u)")
        print("Phi(-u), %s: %s" % (crit, r))
        assert r["score0"] > 1 and r["score"] > 1 and r["mean"] < 1
    # maximize ignored (the straddle is even in mu - level: there the direction changes nothing, and must not)
    for crit in (A.EI, A.PI, A.LCB):
        b, got, r = run(cfg_index(crit, A.BELIEVER, True), "maximize ignored")
        assert r["score0"] > 1 and list(got["own"]) != b["picks"], crit
    assert host_built(cfg_index(A.STRADDLE, A.BELIEVER, True))["picks"] == host_built(cfg_index(A.STRADDLE, A.BELIEVER, False))["picks"]
    # sd taken with the noise
    for crit in A.CRITERIA:
        b, got, r = run(cfg_index(crit, A.BELIEVER, False), "sd with the noise")
        assert r["score0"] > 1 and r["var"] < 1, crit
    # a picked row not masked: LCB under the believer picks its first row again, whose mean did not move
    b, got, _ = run(cfg_index(A.LCB, A.BELIEVER, False), "picked row not masked", follow=False)
    print("picked row not masked: picks %s" % list(got["index"]))
    assert len(set(b["picks"])) == K_HOST and list(got["index"]) != b["picks"]
    assert len(set(got["index"])) < K_HOST or list(got["index"]) != b["picks"]


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


def test_python_names_makefile_and_no_switch_of_its_own():
    import outerbase_amd as ob
    assert "AcquireResult" in ob.__all__ and hasattr(ob, "AcquireResult")
    assert callable(ob.Posterior.acquire)
    assert "picks do not move" in ob.Posterior.acquire.__doc__
    csrc = os.path.join(ROOT, "outerbase_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "kernels_acquire.hip" in mk and "acquire.cpp" in mk
    for f in ("kernels_acquire.hip", "acquire.cpp"):
        src = open(os.path.join(csrc, f)).read()
        code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
        assert "getenv" not in code, f                                   # the switch lives in launch_predict
        assert "atomic" not in code and "Cooperative" not in code and "grid_group" not in code, f


def test_argument_errors_return_before_any_device_call():
    from outerbase_amd._lib import lib
    buf = (C.c_double * 4096)()
    a = C.cast(buf, C.c_void_p)
    n = C.c_uint64(77)
    nan, inf = float("nan"), float("inf")

    def par(best=0.0, xi=0.0, kappa=1.96, level=0.0):
        return (C.c_double * 4)(best, xi, kappa, level)
    for f in (lib.obhip_acquire_dev, lib.obhip_acquire):
        def refused(msg, theta=a, x=a, m=10, crit=0, params=par(), lie=0, lv=0.0, k=3, index=a, score=a, np_=C.byref(n)):
            assert f(None, theta, x, m, crit, params, 0, lie, lv, None, k, index, score, None, None, None, np_) == 1
            assert msg in lib.obhip_last_error(), (msg, lib.obhip_last_error())
        refused(b"m = 0", m=0)
        refused(b"k = 0", k=0)
        refused(b"criterion", crit=4)
        refused(b"criterion", crit=-1)
        refused(b"lie must be", lie=2)
        refused(b"params", params=None)
        for bad in (nan, inf):
            refused(b"best", params=par(best=bad))
            refused(b"best", crit=1, params=par(best=bad))
            refused(b"level", crit=3, params=par(level=bad))
            refused(b"kappa", crit=2, params=par(kappa=bad))
            refused(b"xi", params=par(xi=bad))
            refused(b"lie_value", lie=1, lv=bad)
        refused(b"kappa", crit=2, params=par(kappa=-0.5))
        refused(b"null posterior", crit=2, params=par(best=nan, level=nan))       # best and level are not LCB's
        refused(b"null posterior", lv=nan)                                        # nor the lie value the believer's
        refused(b"null candidates", x=None)
        refused(b"null outputs", index=None)
        refused(b"null outputs", score=None)
        refused(b"null outputs", np_=None)
        refused(b"d_theta is null", theta=None)
        refused(b"null posterior")                                               # score0, mean, var may be NULL
    assert n.value == 77                                                         # a refused call changes nothing


def test_shape_and_argument_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    om, terms = mdl["om_d"], mdl["terms"]
    post = ob.Posterior(om, ob.obmod._terms_of(om, terms), C.c_void_p(1))               # never reaches the library
    p = len(terms)
    try:
        x, th = np.full((5, 3), 0.5), np.zeros(p)
        bad = [dict(k=0), dict(criterion="maxvar"), dict(criterion="ei"), dict(criterion="pi"), dict(criterion="straddle"),
               dict(criterion="lcb", lie="constant"), dict(criterion="lcb", lie="liar"),
               dict(criterion="ei", best=float("nan")), dict(criterion="lcb", kappa=-1.0),
               dict(criterion="lcb", kappa=float("inf")), dict(criterion="ei", best=0.0, xi=float("nan")),
               dict(criterion="straddle", level=float("inf")), dict(criterion="lcb", lie="constant", lie_value=float("nan")),
               dict(criterion="lcb", skip=np.zeros(4))]
        for kw in bad:
            with pytest.raises(ValueError):
                post.acquire(x, th, **{"k": 2, **kw})
        with pytest.raises(ValueError):
            post.acquire(x[:, :2], th, criterion="lcb")
        with pytest.raises(ValueError):
            post.acquire(x[:0], th, criterion="lcb")
        with pytest.raises(ValueError):
            post.acquire(x, th[:-1], criterion="lcb")
        post.meansd = np.array([[0.0, 0.0, 5.0]])
        with pytest.raises(ValueError):                                                 # a scale <= 0, as in _scale
            post.acquire(x, th, criterion="lcb", response=0)
        with pytest.raises(ValueError):
            post.select(x, 2, criterion="ei")                                           # select is what it was
    finally:
        post._h = None
