"""The input-gradient predictor on the GPU (obhip_predict_grad_dev and what is built on it) against
the extended-precision reference of tests/extended_dx_ref.py: every entry of mean, grad, var and
gradvar within C . bound + gamma_p . sum |summands|, C eight times the float64 restatement's own
err / bound on the same case (at most 2e-13).  Fused kernel and the HBM-tile fallback, tile edges,
the pass logic, interval tables and knot loop, rows on knots and x = 0.02 in mat25pow dimensions."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import extended_dx_ref as X
import extended_ref as E
from conftest import knots_for, make_pair, sample_x
from test_predict_grad_host import special_rows

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 129)          # the edges of the 64-row tile
NMAX = 129
SIGMA = -0.4

MIX4 = ["mat25", "mat25pow", "mat25ang", "mat25"]
MIX11 = ["mat25", "mat25pow", "mat25ang", "mat25", "mat25", "mat25pow", "mat25", "mat25ang", "mat25",
         "mat25pow", "mat25"]


def _hyp(kinds, seed):
    """non-zero hyper-parameters, a few tenths either side of the defaults' scale"""
    rng = np.random.default_rng(seed)
    nh = sum(E.NUMHYP[k] for k in kinds)
    h = rng.uniform(0.1, 0.4, nh) * rng.choice([-1.0, 1.0], nh)
    return h


MODELS = {
    # name: (kinds, knots per dimension (int, or a list with one entry per dimension))
    "d1": (["mat25"], 20),
    "d4": (MIX4, 20),
    "d11": (MIX11, 20),
    "d4 knots130": (MIX4, [20, 20, 20, 130]),       # 130 knots: no interval tables, the knot loop
}


@functools.lru_cache(maxsize=None)
def model(name):
    kinds, m = MODELS[name]
    if isinstance(m, int):
        knots = knots_for(kinds, m)
    else:
        knots = [knots_for([kd], mk)[0] for kd, mk in zip(kinds, m)]
    om_o, om_d = make_pair(kinds, knots, hyp=_hyp(kinds, len(name)))
    x = special_rows(np.random.default_rng(len(kinds)), NMAX, kinds, knots)
    return dict(kinds=kinds, knots=knots, om_o=om_o, om_d=om_d, x=x, ref=X.reference_dx_of(om_o, x))


def terms_of(name, p):
    m = model(name)
    d = len(m["kinds"])
    if p == 1:
        return np.zeros((1, d), dtype=np.int64)                   # the constant term alone
    if name == "d1":
        return np.arange(p, dtype=np.int64)[:, None]
    t = m["om_o"].selectterms(3 * p + 8)
    if name == "d11":
        t = t.copy()
        t[:, 7] = 0                                               # a dimension no term uses
        _, first = np.unique(t, axis=0, return_index=True)
        t = t[np.sort(first)]
    assert len(t) >= p and not t[0].any()
    return np.ascontiguousarray(t[:p])


@functools.lru_cache(maxsize=None)
def case(name, p, kind="select"):
    """terms, coefficients and the reference values with their tolerances on the NMAX rows of the
    model, computed once; a call on the first n rows is compared with the first n rows of these"""
    m = model(name)
    rng = np.random.default_rng(p + len(name))
    d = len(m["kinds"])
    if kind == "select":
        terms = terms_of(name, p)
    elif kind == "long":                                          # 9 .. 11 factors per term
        terms = np.zeros((p, d), dtype=np.int64)
        for k in range(1, p):
            dims = rng.choice(d, size=int(rng.integers(9, d + 1)), replace=False)
            terms[k, dims] = rng.integers(1, 4, size=len(dims))
        terms = np.unique(terms, axis=0)
        assert np.max((terms > 0).sum(1)) >= 9
    p = len(terms)
    theta = rng.standard_normal(p)
    cv = rng.uniform(0.1, 1.0, p)
    ref, om_o, x = m["ref"], m["om_o"], m["x"]
    Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, om_o, x, terms))
    B, bB = ref.getmat(terms)
    c = dict(terms=terms, theta=theta, cv=cv, C=Cc)
    c["mean"] = E.ref_matmul(B, bB, theta, Cc)
    c["var"] = E.ref_predict_var(B, bB, cv, SIGMA, Cc)
    c["grad"] = ref.ref_grad_mean(terms, theta, Cc)
    c["gradvar"] = ref.ref_grad_var(terms, cv, Cc)
    return c


def run_dev(om_d, terms, theta, x, cv=None, want_mean=True, pass_gradvar=None):
    """obhip_predict_grad_dev on torch buffers; outputs pre-filled with NaN sentinels.  d_var is always
    passed; d_gradvar with coeffvar only (without it the entry refuses the call) unless told to"""
    if pass_gradvar is None:
        pass_gradvar = cv is not None
    import torch
    import outerbase_amd as ob
    from outerbase_amd._lib import call
    t = ob.obmod._terms_of(om_d, terms)
    n, d = x.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
    dth = torch.from_numpy(np.ascontiguousarray(theta)).to(dev)
    nan = float("nan")
    mean = torch.full((n,), nan, dtype=torch.float64, device=dev)
    grad = torch.full((d, n), nan, dtype=torch.float64, device=dev)
    var = torch.full((n,), nan, dtype=torch.float64, device=dev)
    gv = torch.full((d, n), nan, dtype=torch.float64, device=dev)
    dcv = None if cv is None else torch.from_numpy(np.ascontiguousarray(cv)).to(dev)
    call("obhip_predict_grad_dev", om_d._h, t._h, dth.data_ptr(), dx.data_ptr(), n,
         mean.data_ptr() if want_mean else None, grad.data_ptr(), None if dcv is None else dcv.data_ptr(), SIGMA,
         var.data_ptr(), gv.data_ptr() if pass_gradvar else None)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), grad.cpu().numpy().T, var.cpu().numpy(), gv.cpu().numpy().T


def worst_of(c, n, mean, grad, var=None, gradvar=None):
    out = {"mean": E.worst_ratio(mean, c["mean"][0][:n], c["mean"][1][:n]),
           "grad": E.worst_ratio(grad, c["grad"][0][:n], c["grad"][1][:n])}
    if var is not None:
        out["var"] = E.worst_ratio(var, c["var"][0][:n], c["var"][1][:n])
        out["gradvar"] = E.worst_ratio(gradvar, c["gradvar"][0][:n], c["gradvar"][1][:n])
    return out


def check_case(name, p, kind, label):
    m, c = model(name), case(name, p, kind)
    lines, worst = [], 0.0
    for n in NS:
        got = run_dev(m["om_d"], c["terms"], c["theta"], m["x"][:n], c["cv"])
        w = worst_of(c, n, *got)
        lines.append("%s %s p=%d n=%d: err/tolerance %s" % (label, name, len(c["terms"]), n,
                     ", ".join("%s %.3g" % kv for kv in w.items())))
        worst = max(worst, max(w.values()))
    print("\n".join(lines))
    assert worst < 1, "\n".join(lines)


CASES = [("d1", 1), ("d1", 2), ("d1", 20), ("d4", 1), ("d4", 2), ("d4", 63), ("d4", 65), ("d4", 130), ("d4", 300),
         ("d11", 1), ("d11", 65), ("d11", 300), ("d4 knots130", 65)]


@pytest.mark.parametrize("name,p", CASES)
def test_fused_kernel_against_extended_reference(name, p, monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    check_case(name, p, "select", "fused")


@pytest.mark.parametrize("name,p", CASES)
def test_fallback_against_extended_reference(name, p, monkeypatch):
    monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    check_case(name, p, "select", "fallback")


def test_unused_dimension_and_constant_term():
    """the views of dimension 7 of d11 are empty (gradient rho_7 . mean), those of the constant term
    alone are empty in every dimension (gradient s rho_l theta_0)"""
    import outerbase_amd as ob
    m = model("d11")
    views = ob.term_dim_views(m["om_d"], case("d11", 65)["terms"])
    assert len(views[7]) == 0 and all(len(v) > 0 for l, v in enumerate(views) if l != 7)
    assert all(len(v) == 0 for v in ob.term_dim_views(m["om_d"], case("d11", 1)["terms"]))
    _, grad, _, _ = run_dev(m["om_d"], case("d11", 65)["terms"], case("d11", 65)["theta"], m["x"])
    assert np.all(np.isfinite(grad)) and np.any(grad[:, 7] != 0)


def test_terms_of_nine_to_eleven_factors_take_the_fallback(monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    check_case("d11", 40, "long", "9-11 factors")


@functools.lru_cache(maxsize=None)
def wide():
    """more used columns than the fused kernel's tile holds: 2 Mu + d + 31 > 320"""
    rng = np.random.default_rng(40)
    d, mk = 40, 6
    kinds = [["mat25", "mat25pow", "mat25ang"][k % 3] for k in range(d)]
    knots = []
    for kd in kinds:
        g = np.linspace(0.03, 0.97, mk)
        knots.append(g * 6.283185 if kd == "mat25ang" else g)
    om_o, om_d = make_pair(kinds, knots, hyp=_hyp(kinds, 40))
    terms = np.zeros((400, d), dtype=np.int64)
    for k in range(1, 400):
        dims = rng.choice(d, size=int(rng.integers(1, 4)), replace=False)
        terms[k, dims] = rng.integers(1, mk, size=len(dims))
    terms = np.unique(terms, axis=0)
    used = sum(len(np.unique(terms[:, l][terms[:, l] > 0])) for l in range(d)) + 1
    x = special_rows(rng, 65, kinds, knots)
    return kinds, om_o, om_d, terms, used, x


def test_term_set_beyond_the_fused_domain(monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    kinds, om_o, om_d, terms, used, x = wide()
    assert 2 * used + len(kinds) + 31 > 320          # predict_dx_supports says no
    ref = X.reference_dx_of(om_o, x)
    rng = np.random.default_rng(5)
    theta, cv = rng.standard_normal(len(terms)), rng.uniform(0.1, 1.0, len(terms))
    Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, om_o, x, terms))
    B, bB = ref.getmat(terms)
    c = dict(mean=E.ref_matmul(B, bB, theta, Cc), var=E.ref_predict_var(B, bB, cv, SIGMA, Cc),
             grad=ref.ref_grad_mean(terms, theta, Cc), gradvar=ref.ref_grad_var(terms, cv, Cc))
    w = worst_of(c, len(x), *run_dev(om_d, terms, theta, x, cv))
    line = "wide d=40 p=%d used=%d: err/tolerance %s" % (len(terms), used, ", ".join("%s %.3g" % kv for kv in w.items()))
    print(line)
    assert max(w.values()) < 1, line


@pytest.mark.parametrize("generic", [False, True])
def test_null_coeffvar_leaves_the_variance_outputs_untouched_and_null_mean_is_accepted(generic, monkeypatch):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    m, c = model("d4"), case("d4", 130)
    mean, grad, var, gv = run_dev(m["om_d"], c["terms"], c["theta"], m["x"][:65], cv=None, want_mean=False)
    assert np.all(np.isnan(mean)) and np.all(np.isnan(var)) and np.all(np.isnan(gv))
    w = E.worst_ratio(grad, c["grad"][0][:65], c["grad"][1][:65])
    print("mean = NULL, coeffvar = NULL: grad err/tolerance %.3g" % w)
    assert w < 1
    # d_gradvar without d_coeffvar is an argument error: refused before any device call
    import outerbase_amd as ob
    with pytest.raises(ob.ObhipError, match="gradvar needs coeffvar"):
        run_dev(m["om_d"], c["terms"], c["theta"], m["x"][:65], cv=None, pass_gradvar=True)


@pytest.mark.parametrize("generic", [False, True])
def test_two_calls_give_identical_bits(generic, monkeypatch):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    m, c = model("d11"), case("d11", 300)
    a = run_dev(m["om_d"], c["terms"], c["theta"], m["x"], c["cv"])
    b = run_dev(m["om_d"], c["terms"], c["theta"], m["x"], c["cv"])
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_host_entry(monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    import outerbase_amd as ob
    m, c = model("d4"), case("d4", 130)
    n = 65
    got = ob.predict_grad(m["om_d"], c["terms"], c["theta"], m["x"][:n], coeffvar=c["cv"], sigma=SIGMA)
    w = worst_of(c, n, *got)
    print("host entry: err/tolerance %s" % ", ".join("%s %.3g" % kv for kv in w.items()))
    assert max(w.values()) < 1
    mean, grad = ob.predict_grad(m["om_d"], c["terms"], c["theta"], m["x"][:n])
    assert np.array_equal(mean, got[0]) and np.array_equal(grad, got[1])
    # a row slice of a larger column-major matrix: ldx, ldg above n
    from outerbase_amd._lib import call, ptr
    xf = np.asfortranarray(m["x"])
    gbig = np.full((NMAX, 4), np.nan, order="F")
    t = ob.obmod._terms_of(m["om_d"], c["terms"])
    call("obhip_predict_grad", m["om_d"]._h, t._h, ptr(c["theta"]), ptr(xf), n, NMAX, None, ptr(gbig), NMAX,
         None, 0.0, None, None)
    assert np.array_equal(gbig[:n], got[1]) and np.all(np.isnan(gbig[n:]))


def test_with_the_interval_tables_and_without_them(monkeypatch):
    """the same model and rows through both evaluations of a dimension: 20 knots with the levels the
    terms use (interval tables) and, with a level-19 term added in every dimension, all 20 levels,
    whose tables no longer fit (the knot loop); both within the same tolerance"""
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    kinds = ["mat25", "mat25pow", "mat25"]
    knots = knots_for(kinds, 20)
    om_o, om_d = make_pair(kinds, knots, hyp=_hyp(kinds, 3))
    x = special_rows(np.random.default_rng(11), 65, kinds, knots)
    ref = X.reference_dx_of(om_o, x)
    base = om_o.selectterms(60)
    assert base.max() <= 15      # 20 + 21 x 16 x 6 doubles of tables fit the 2048 the kernels keep
    for label, extra in (("tables", None), ("knot loop", 19)):
        terms = base if extra is None else np.vstack([base, [[extra, 0, 0]], [[0, extra, 0]], [[0, 0, extra]]])
        rng = np.random.default_rng(60)
        theta, cv = rng.standard_normal(len(terms)), rng.uniform(0.1, 1.0, len(terms))
        if extra is not None:
            theta[-3:] = 0.0     # the same function: the added terms only switch the evaluation
            cv[-3:] = 0.0
        Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, om_o, x, base))
        B, bB = ref.getmat(terms)
        c = dict(mean=E.ref_matmul(B, bB, theta, Cc), var=E.ref_predict_var(B, bB, cv, SIGMA, Cc),
                 grad=ref.ref_grad_mean(terms, theta, Cc), gradvar=ref.ref_grad_var(terms, cv, Cc))
        w = worst_of(c, len(x), *run_dev(om_d, terms, theta, x, cv))
        line = "%s: err/tolerance %s" % (label, ", ".join("%s %.3g" % kv for kv in w.items()))
        print(line)
        assert max(w.values()) < 1, line


# ---- what is built on the entry ------------------------------------------------------------------
def _destandardised(want, tol, sca, cent=None):
    """value and tolerance of sca . v (+ cent) in float64: the multiplication rounds once, the
    addition once more"""
    w = np.asarray(want, dtype=np.longdouble) * np.longdouble(sca)
    t = np.asarray(tol) * abs(sca) + E.gamma(1) * np.abs(E._f64(w))
    if cent is not None:
        w = w + np.longdouble(cent)
        t = t + E.gamma(2) * (np.abs(E._f64(w)) + abs(cent))
    return w, t


def test_multifit_predict_grad_destandardises(monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    import outerbase_amd as ob
    m, c = model("d4"), case("d4", 65)
    rng = np.random.default_rng(9)
    xtr = sample_x(rng, 400, m["kinds"])
    Y = np.stack([np.sin(3 * xtr[:, 0]) + xtr[:, 1], 5.0 + 2.0 * xtr[:, 3] * xtr[:, 1], np.cos(xtr[:, 2]) * 0.1], axis=1)
    Y += 0.01 * rng.standard_normal(Y.shape)
    mf = ob.fit_newton_multi(m["om_d"], c["terms"], xtr, Y)
    n = 65
    x, ref = m["x"][:n], m["ref"]
    mean, grad, var, gradvar = mf.predict_grad(x, var=True)
    assert mean.shape == var.shape == (n, 3) and grad.shape == gradvar.shape == (n, 4, 3)
    mean2, grad2 = mf.predict_grad(x)
    assert np.array_equal(mean2, mean) and np.array_equal(grad2, grad)
    B, bB = ref.getmat(c["terms"])
    B, bB = B[:n], bB[:n]
    cvar = 1.0 / mf.diagH
    worst = {}
    for j in range(3):
        th, sca, cent = mf.coeff[:, j], float(mf.y_sca[j]), float(mf.y_cent[j])
        wm = _destandardised(*E.ref_matmul(B, bB, th, c["C"]), sca, cent)
        gw, gt = ref.ref_grad_mean(c["terms"], th, c["C"])
        wg = _destandardised(gw[:n], gt[:n], sca)
        wv = _destandardised(*E.ref_predict_var(B, bB, cvar, mf.sigma, c["C"]), sca * sca)
        vw, vt = ref.ref_grad_var(c["terms"], cvar, c["C"])
        wgv = _destandardised(vw[:n], vt[:n], sca * sca)
        for key, got, (w, t) in (("mean", mean[:, j], wm), ("grad", grad[:, :, j], wg), ("var", var[:, j], wv),
                                 ("gradvar", gradvar[:, :, j], wgv)):
            worst[key] = max(worst.get(key, 0.0), E.worst_ratio(got, w, t))
    print("MultiFit.predict_grad q=3: err/tolerance %s" % ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert max(worst.values()) < 1
    # the existing predictor agrees with the new mean to rounding of the de-standardisation
    assert np.allclose(mf.predict(x), mean, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("lik_name", ["loglik_std", "loglik_gauss"])
def test_predictor_gradmean(lik_name, monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    import outerbase_amd as ob
    m, c = model("d4"), case("d4", 65)
    rng = np.random.default_rng(13)
    xtr = sample_x(rng, 300, m["kinds"])
    y = np.sin(3 * xtr[:, 0]) + xtr[:, 1] * xtr[:, 3] + 0.01 * rng.standard_normal(300)
    y = (y - y.mean()) / y.std(ddof=1)
    lik = getattr(ob, lik_name)(m["om_d"], c["terms"], y, xtr)
    lp = ob.lpdfvec(lik, ob.logpr_gauss(m["om_d"], c["terms"]))
    if lik_name == "loglik_std":
        lp.optnewton()
    else:
        lp.optcg(1e-10, 500)
    pred = ob.predictor(lp)
    n = 65
    pred.update(m["x"][:n])
    g = pred.gradmean()
    assert g.shape == (n, 4)
    th = np.asarray(lik.coeff, dtype=np.float64)
    assert np.any(th != 0)
    want, tol = m["ref"].ref_grad_mean(c["terms"], th, c["C"])
    w = E.worst_ratio(g, want[:n], tol[:n])
    print("%s predictor.gradmean: err/tolerance %.3g" % (lik_name, w))
    assert w < 1
    # obpred_grad de-standardises it
    out = ob.obpred_grad(dict(predobj=pred, y_cent=2.0, y_sca=3.0), m["x"][:n])
    assert set(out) == {"mean", "var", "gradmean"} and np.array_equal(out["gradmean"], 3.0 * g)
