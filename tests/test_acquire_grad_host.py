"""Host-side checks of the acquisition gradients (no GPU): the analytic gradients of the reference
(tests/acquire_grad_ref.py) against central differences of its own long-double scores, the float64 restatement of the
device's operation order inside its allowance on every case test_gpu_acquire_grad.py uses, the conditions those cases
must meet, six mutations the instrument must reject, the d <= 0 rule, and the library's host side -- symbols, Python
names, the Makefile, argument errors that return before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

import acquire_grad_ref as R
import acquire_ref as A
import extended_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ld = np.longdouble
NEW = {"obhip_posterior_var_grad_dev": 7, "obhip_acquire_grad_dev": 14, "obhip_acquire_grad": 14,
       "obhip_acquire_grad_layout": 4}


# ---- the instrument ------------------------------------------------------------------------------------
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("crit", A.CRITERIA)
def test_analytic_gradients_against_central_differences_of_the_references_own_scores(crit, maximize):
    """d5 p=130, the first 10 rows, every dimension: central differences of the long-double scores with h = 2^-10 and
    2^-11 (the angle: times 2 pi).  The disagreement with the analytic gradient falls by a factor in [3, 5] (4 = second
    order) in EVERY entry.  (The scores are three times differentiable between the knots; the steps are far below
    the knot spacing of 1 / 20, and a row that straddles a knot would show as a ratio near 2.)"""
    c, cfgs = R.case("d5 p=130")
    cfg = cfgs[R.cfg_index(crit, maximize)]
    rows = slice(0, 10)
    want = R.reference(c, cfg)["grad"][0][rows]
    x0 = c.x[rows]
    worst = [np.inf, 0.0]
    for l in range(c.d):
        e = []
        for h in (2.0 ** -10, 2.0 ** -11):
            h = h * (6.283185 if c.om_o.kinds[l] == "mat25ang" else 1.0)
            xp, xm = x0.copy(), x0.copy()
            xp[:, l] += h
            xm[:, l] -= h
            hh = ld(xp[0, l]) - ld(xm[0, l])
            fd = (R.scores_at(c, cfg, xp) - R.scores_at(c, cfg, xm)) / np.array(xp[:, l] - xm[:, l], dtype=ld)
            e.append(np.abs(E._f64(fd - want[:, l])))
            assert hh > 0
        ratio = e[0] / e[1]
        print("%r dimension %d: disagreement %.3g -> %.3g, ratios %.4g .. %.4g" % (cfg, l, e[0].max(), e[1].max(),
                                                                                    ratio.min(), ratio.max()))
        worst = [min(worst[0], ratio.min()), max(worst[1], ratio.max())]
    assert worst[0] >= 3.0 and worst[1] <= 5.0, worst


@pytest.mark.parametrize("name", list(R.CASES))
def test_float64_restatement_stays_inside_its_allowance_and_the_cases_meet_their_conditions(name):
    """on every case the GPU file uses, on the reference alone: the float64 restatement inside its allowance in every
    entry of all six outputs with 8 r < C_CAP; every d_i more than 1000 of its allowances; for the straddle the level
    the float32-rounded midpoint of the two middle latent means and no |mu - level| within 1000 allowances of mu; no row
    left out of any comparison"""
    c, cfgs = R.case(name)
    assert len(cfgs) == 8
    mu = np.sort(E._f64(c.mu))
    mid = float(np.float32(0.5 * (mu[c.n // 2 - 1] + mu[c.n // 2])))
    for ci, cfg in enumerate(cfgs):
        b = R.built(name, ci)
        got = R.restatement64(c, cfg)
        for q in R.QUANTITIES:                                           # every row and entry is compared
            assert got[q].shape == b["ref"][q][0].shape == ((c.n,) if got[q].ndim == 1 else (c.n, c.d)), q
            assert np.all(np.isfinite(E._f64(b["ref"][q][0]))) and np.all(np.isfinite(b["ref"][q][1])), q
        w = R.ratios(got, b["ref"], b["C"])
        dmin, lmin = R.conditions(c, cfg, b["C"])
        print("%s %r: float64 restatement err / bound %.3g (C = %.3g, cap %.3g), err / tolerance %s; smallest d / "
              "allowance %.3g, smallest |mu - level| / allowance %.3g" % (
                  name, cfg, b["r"], b["C"], E.C_CAP, ", ".join("%s %.3g" % kv for kv in w.items()), dmin, lmin))
        assert 8 * b["r"] < E.C_CAP, "the constant is capped: the bound does not describe this case"
        assert set(w) == set(R.QUANTITIES) and max(w.values()) < 1
        assert dmin > 1000, "a latent variance is within 1000 allowances of zero: choose another seed"
        assert cfg.level == mid
        if cfg.criterion == A.STRADDLE:
            assert lmin > 1000, "a latent mean is within 1000 allowances of the level: choose another seed"
    # var_grad alone: the same two quantities without a criterion
    w = R.ratios(R.restatement64(c), R.built(name, 0)["ref"], R.built(name, 0)["C"])
    assert set(w) == {"var", "grad_var"} and max(w.values()) < 1


def test_the_instrument_rejects_six_mutations():
    """each with the size it is caught at (worst err / tolerance of the quantity it must move)"""
    name = "d5 p=130"
    c, cfgs = R.case(name)

    def run(crit, mx, mutate):
        ci = R.cfg_index(crit, mx)
        b = R.built(name, ci)
        return R.ratios(R.restatement64(c, b["cfg"], mutate), b["ref"], b["C"])
    for crit in A.CRITERIA:
        for mx in (False, True):
            assert max(run(crit, mx, None).values()) < 1
    # the factor 2 of dd dropped: the variance gradient and every score gradient that has a dsd part
    r = run(A.EI, False, "factor 2 of dd dropped")
    print("factor 2 of dd dropped: %s" % r)
    assert r["grad_var"] > 1000 and r["grad"] > 1000 and r["var"] < 1 and r["grad_mean"] < 1 and r["score"] < 1
    # the rho_l term dropped: both gradients, no value
    r = run(A.LCB, False, "rho term dropped")
    print("rho term dropped: %s" % r)
    assert r["grad_var"] > 1000 and r["grad_mean"] > 1000 and r["grad"] > 1000 and max(r["var"], r["mean"], r["score"]) < 1
    # dsd without 1 / (2 sd): the score gradients only
    for crit in A.CRITERIA:
        r = run(crit, False, "dsd without 1/(2 sd)")
        print("dsd without 1/(2 sd), %s: %s" % (crit, r))
        assert r["grad"] > 1000 and max(v for q, v in r.items() if q != "grad") < 1, crit
    # maximize not applied to dmu: under maximize only
    for crit in A.CRITERIA:
        r = run(crit, True, "maximize not applied to dmu")
        print("maximize not applied to dmu, %s: %s" % (crit, r))
        assert r["grad"] > 1000 and max(v for q, v in r.items() if q != "grad") < 1, crit
        assert max(run(crit, False, "maximize not applied to dmu").values()) < 1
    # sign(mu~ - level) dropped: the straddle's gradient (the level is the median: half the rows have the other sign)
    r = run(A.STRADDLE, False, "sign dropped")
    print("sign dropped: %s" % r)
    assert r["grad"] > 1000 and max(v for q, v in r.items() if q != "grad") < 1
    # S replaced by diag(c), c = diag(inv(H)): obhip_predict_grad_dev's diagonal variance and its gradient
    r = run(A.EI, False, "S replaced by diag(c)")
    print("S replaced by diag(c): %s" % r)
    assert r["var"] > 1000 and r["grad_var"] > 1000 and r["mean"] < 1 and r["grad_mean"] < 1


def test_the_rule_where_the_variance_is_not_positive():
    """gradient64, the restatement's epilogue: dsd = 0, EI -dmu~ where t > 0 and 0 elsewhere, PI 0, and the scores
    acquire's sd = 0 branches"""
    mu = np.array([-1.0, 1.0, -1.0, 1.0, 0.25])
    d = np.array([0.0, 0.0, -1e-3, -1e-3, 0.0])
    dmu = np.array([[0.5, -2.0]] * 5)
    dd = np.array([[3.0, 7.0]] * 5)
    for mx in (False, True):
        sgn = -1.0 if mx else 1.0
        par = dict(best=sgn * 0.25, xi=0.0, kappa=1.5, level=sgn * 0.25, maximize=mx)
        m = sgn * mu                                                      # the rows in the caller's sign
        t = 0.25 - mu
        s, g = R.gradient64(A.Config(A.EI, **par), m, d, dmu, dd)
        assert np.array_equal(s, np.maximum(t, 0.0)) and np.array_equal(g, np.where((t > 0)[:, None], -sgn * dmu, 0.0))
        s, g = R.gradient64(A.Config(A.PI, **par), m, d, dmu, dd)
        assert np.array_equal(s, (t > 0) * 1.0) and not np.any(g)
        s, g = R.gradient64(A.Config(A.LCB, **par), m, d, dmu, dd)
        assert np.array_equal(s, -mu) and np.array_equal(g, -sgn * dmu)
        s, g = R.gradient64(A.Config(A.STRADDLE, **par), m, d, dmu, dd)
        assert np.array_equal(s, -np.abs(mu - 0.25)) and np.array_equal(g, -np.sign(mu - 0.25)[:, None] * sgn * dmu)
        assert not np.any(g[4])                                           # sign(0) = 0


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
    for name in ("AcquireGradResult", "TorchAcquisition"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert callable(ob.Posterior.acquire_grad) and callable(ob.Posterior.var_grad)
    doc = ob.Posterior.acquire_grad.__doc__
    for word in ("-Phi(u) dmu + phi(u) dsd", "d <= 0", "not finite", "chunk_rows", "sca^2", "AcquireGradResult"):
        assert word in doc, word
    assert "once" in ob.TorchAcquisition.__doc__
    csrc = os.path.join(ROOT, "outerbase_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "kernels_acquire_dx.hip" in mk and "acquire_dx.cpp" in mk
    envs = set()
    for f in ("kernels_acquire_dx.hip", "acquire_dx.cpp"):
        src = open(os.path.join(csrc, f)).read()
        code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
        assert "atomic" not in code and "Cooperative" not in code and "grid_group" not in code, f
        envs |= {ln.split('getenv("')[1].split('"')[0] for ln in code.splitlines() if 'getenv("' in ln}
    assert envs == {"OBHIP_FORCE_GENERIC"}                               # the switch of every fused kernel, no other


def test_argument_errors_return_before_any_device_call():
    from outerbase_amd._lib import lib
    buf = (C.c_double * 4096)()
    a = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def par(best=0.0, xi=0.0, kappa=1.96, level=0.0):
        return (C.c_double * 4)(best, xi, kappa, level)
    for f in (lib.obhip_acquire_grad_dev, lib.obhip_acquire_grad):
        def refused(msg, theta=a, x=a, n=10, crit=0, params=par(), chunk=0, score=a, grad=a):
            assert f(None, theta, x, n, crit, params, 0, chunk, score, grad, None, None, None, None) == 1
            assert msg in lib.obhip_last_error(), (msg, lib.obhip_last_error())
        refused(b"criterion", crit=4)
        refused(b"criterion", crit=-1)
        refused(b"params", params=None)
        for bad in (nan, inf):
            refused(b"best", params=par(best=bad))
            refused(b"best", crit=1, params=par(best=bad))
            refused(b"level", crit=3, params=par(level=bad))
            refused(b"kappa", crit=2, params=par(kappa=bad))
            refused(b"xi", params=par(xi=bad))
        refused(b"kappa", crit=2, params=par(kappa=-0.5))
        refused(b"null posterior", crit=2, params=par(best=nan, level=nan))       # best and level are not LCB's
        refused(b"theta is null", theta=None)
        refused(b"null outputs", score=None)
        refused(b"null outputs", grad=None)
        for chunk in (1, 64, 127, 129, 2 ** 40 + 1):
            refused(b"chunk_rows", chunk=chunk)
        refused(b"2^40 rows", n=2 ** 40 + 1)
        refused(b"null x", x=None)
        refused(b"null posterior")                                               # mean, var and their gradients may be NULL
        refused(b"null posterior", chunk=128)
        refused(b"null posterior", n=0, x=None, score=None, grad=None)            # n = 0 needs no buffers, but a handle
    f = lib.obhip_posterior_var_grad_dev

    def refused(msg, x=a, n=10, chunk=0, var=a, grad=a):
        assert f(None, x, n, chunk, 0, var, grad) == 1
        assert msg in lib.obhip_last_error(), (msg, lib.obhip_last_error())
    refused(b"null outputs", var=None)
    refused(b"null outputs", grad=None)
    for chunk in (1, 127, 130):
        refused(b"chunk_rows", chunk=chunk)
    refused(b"2^40 rows", n=2 ** 40 + 1)
    refused(b"null x", x=None)
    refused(b"null posterior")
    assert lib.obhip_acquire_grad_layout(None, None, None, None) == 1 and b"null posterior" in lib.obhip_last_error()
    assert not any(buf)                                                          # a refused call changes nothing


def test_shape_and_argument_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    from test_sobol_host import golden_model
    mdl = golden_model("mixed_d3")
    om, terms = mdl["om_d"], mdl["terms"]
    post = ob.Posterior(om, ob.obmod._terms_of(om, terms), C.c_void_p(1))               # never reaches the library
    p = len(terms)
    try:
        x, th = np.full((5, 3), 0.5), np.zeros(p)
        bad = [dict(criterion="maxvar"), dict(criterion="ei"), dict(criterion="pi"), dict(criterion="straddle"),
               dict(criterion="ei", best=float("nan")), dict(criterion="lcb", kappa=-1.0),
               dict(criterion="lcb", kappa=float("inf")), dict(criterion="ei", best=0.0, xi=float("nan")),
               dict(criterion="straddle", level=float("inf")), dict(criterion="lcb", chunk_rows=64),
               dict(criterion="lcb", chunk_rows=-128), dict(criterion="lcb", chunk_rows=200)]
        for kw in bad:
            with pytest.raises(ValueError):
                post.acquire_grad(x, th, **kw)
        with pytest.raises(ValueError):
            post.acquire_grad(x[:, :2], th, criterion="lcb")
        with pytest.raises(ValueError):
            post.acquire_grad(x, th[:-1], criterion="lcb")
        for kw in (dict(chunk_rows=1), dict(chunk_rows=-128)):
            with pytest.raises(ValueError):
                post.var_grad(x, **kw)
        with pytest.raises(ValueError):
            post.var_grad(x[:, :2])
        empty = post.acquire_grad(x[:0], th, criterion="lcb")                            # no rows: no call
        assert empty.score.shape == (0,) and empty.grad.shape == (0, 3) and empty.grad_var.shape == (0, 3)
        v, g = post.var_grad(x[:0])
        assert v.shape == (0,) and g.shape == (0, 3)
        post.meansd = np.array([[0.0, 0.0, 5.0]])
        with pytest.raises(ValueError):                                                 # a scale <= 0, as in _scale
            post.acquire_grad(x, th, criterion="lcb", response=0)
        with pytest.raises(ValueError):
            post.select(x, 2, criterion="ei")                                           # select is what it was
    finally:
        post._h = None
