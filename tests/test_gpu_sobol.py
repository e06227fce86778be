"""Sobol indices and main effects on the GPU (obhip_dim_moments_dev, obhip_sobol_dev,
obhip_main_effect_dev and what is built on them) against the long-double reference of tests/sobol_ref.py.

Stage 1 (moment tables): every entry within tol_m / tol_C, C eight times the float64 oracle's own
getbase err / bound on the same nodes.  Stage 2 (pair sums on random float64 tables): every output within
its own gamma . sum |summands|.  End to end: device tables, then device sums, against long-double sums of
long-double tables; allowance eight times the float64 restatement's own error on the same case.
Every test prints err / tolerance.

TW = 128 is the pair kernel's term-tile width, RC = 2 its response chunk; 8 and 24 are the dimensions it
accumulates per pass (d = 9, 25, 40 cross those edges)."""
import ctypes as C
import functools

import numpy as np
import pytest

import extended_jac_ref as J
import extended_ref as E
import sobol_ref as S
from conftest import knots_for, make_pair, sample_x
from test_sobol_host import d5_model, golden_model, reference_of, some_zero_weights, theta_of

pytestmark = pytest.mark.gpu

TW, RC = 128, 2
NS = (1, 37, 64, 65, 1000)
NMAX = 1000
NAN = float("nan")
ld = np.longdouble


def _dev():
    import torch
    from outerbase_amd._lib import call
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return torch, call, dev


# ---- stage 1: the moment tables ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moment_model(name):
    if name == "knots130":
        kinds = ["mat25", "mat25pow", "mat25ang", "mat25"]
        knots = [knots_for([kd], mk)[0] for kd, mk in zip(kinds, [20, 20, 20, 130])]   # 130 knots: the knot loop
        om_o, om_d = make_pair(kinds, knots)
        terms = np.ascontiguousarray(om_o.selectterms(30))
    else:
        g = golden_model(name)
        kinds, om_o, om_d, terms = g["kinds"], g["om_o"], g["om_d"], g["terms"]
    rng = np.random.default_rng(len(name))
    x = sample_x(rng, NMAX, kinds)
    w = some_zero_weights(rng, NMAX, len(kinds))
    ref = reference_of(om_o, x)
    levels = S.levels_of(terms)
    Cc = E.constant_from_oracle_ratio(S.oracle_getbase_ratio(ref, om_o, x, levels))
    return dict(kinds=kinds, om_o=om_o, om_d=om_d, terms=terms, x=x, w=w, ref=ref, levels=levels, C=Cc)


def run_moments(om_d, terms, x, w=None, pad=0, wpad=0):
    """obhip_dim_moments_dev on NaN-padded torch buffers -> (packed mean, packed cov)"""
    import outerbase_amd as ob
    torch, call, dev = _dev()
    t = ob.obmod._terms_of(om_d, terms)
    n, d = x.shape
    xp = np.full((d, n + pad), NAN)
    xp[:, :n] = x.T
    dx = torch.from_numpy(xp).to(dev)
    dw = None
    if w is not None:
        wp = np.full((d, n + wpad), NAN)
        wp[:, :n] = w.T
        dw = torch.from_numpy(wp).to(dev)
    levels = S.levels_of(terms)
    mean = torch.full((int(levels.sum()),), NAN, dtype=torch.float64, device=dev)
    cov = torch.full((int((levels ** 2).sum()),), NAN, dtype=torch.float64, device=dev)
    call("obhip_dim_moments_dev", om_d._h, t._h, dx.data_ptr(), n, n + pad, None if dw is None else dw.data_ptr(),
         n + wpad, mean.data_ptr(), cov.data_ptr())
    torch.cuda.synchronize()
    return mean.cpu().numpy(), cov.cpu().numpy()


@pytest.mark.parametrize("name", ["mixed_d3", "mat25_d8", "knots130"])
def test_moment_tables_against_extended_reference(name):
    c = moment_model(name)
    lines, worst = [], 0.0
    for n in NS:
        for mode in ("none", "weights", "padded weights"):
            w = None if mode == "none" else c["w"][:n]
            pm, pc = run_moments(c["om_d"], c["terms"], c["x"][:n], w, pad=3, wpad=5 if mode == "padded weights" else 0)
            pm2, pc2 = run_moments(c["om_d"], c["terms"], c["x"][:n], w, pad=0, wpad=0)
            same = np.array_equal(pm, pm2) and np.array_equal(pc, pc2)           # two calls, other padding
            gm, gc = S.unpack_tables(pm, pc, c["levels"])
            (m, Cv), (tm, tc) = S.ref_tables(S.RowSlice(c["ref"], n), c["levels"], w, c["C"])
            r = max(max(E.worst_ratio(gm[l], m[l], tm[l]), E.worst_ratio(gc[l], Cv[l], tc[l]))
                    for l in range(len(c["levels"])))
            sym = all(np.array_equal(a, a.T) for a in gc)
            worst = max(worst, r)
            if not (r < 1 and same and sym):
                lines.append("%s n=%d %s: err/tolerance %.3g, same bits %s, symmetric %s" % (name, n, mode, r, same, sym))
    print("%s (C = %.3g): worst err/tolerance %.3g" % (name, c["C"], worst))
    assert not lines, "\n".join(lines)


def test_bad_weights_are_a_numeric_error():
    from outerbase_amd import ObhipError
    c = moment_model("mixed_d3")
    n = 65
    for what in ("zero column", "negative", "nan", "inf"):
        w = c["w"][:n].copy()
        if what == "zero column":
            w[:, 1] = 0.0
        else:
            w[40, 2] = {"negative": -0.5, "nan": NAN, "inf": float("inf")}[what]
        with pytest.raises(ObhipError) as e:
            run_moments(c["om_d"], c["terms"], c["x"][:n], w)
        assert e.value.code == 5, what                                           # OBHIP_ERR_NUMERIC
    run_moments(c["om_d"], c["terms"], c["x"][:n], c["w"][:n])                   # and the library goes on


# ---- stage 2: the pair sums on random tables -----------------------------------------------------------
PAIR_CASES = [(1, 1, 1), (5, 3, RC), (TW, 8, RC + 1), (TW + 1, 20, 2 * RC + 1), (2 * TW + 2, 3, 2 * RC + 1),
              (257, 40, RC), (257, 9, RC + 1), (40, 25, 1), (300, 20, 1), (1100, 3, RC + 1)]


@functools.lru_cache(maxsize=None)
def pair_case(p, d, q):
    import outerbase_amd as ob
    rng = np.random.default_rng(1000 * p + 10 * d + q)
    levels = rng.integers(2, 6, size=d)
    levels[rng.integers(d)] = 9
    terms = np.zeros((p, d), dtype=np.int64)
    for k in range(1, p):
        dims = rng.choice(d, size=int(rng.integers(1, min(d, 4) + 1)), replace=False)
        terms[k, dims] = rng.integers(1, levels[dims])
    if p > 1:
        terms[p - 1] = levels - 1                                                # every dimension's top level is used
    else:
        levels[:] = 1
    kinds = ["mat25"] * d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    m, Cv = S.random_tables(rng, levels)
    Theta = rng.standard_normal((p, q)) * J.response_scales(q)[None, :]
    return dict(om=om, t=ob.obmod._Terms(om, terms), terms=terms, levels=levels, m=m, Cv=Cv, Theta=Theta,
                f=S.formulas(terms, Theta, m, Cv))


def run_sobol(t, Theta, pm, pc, with_g=True):
    torch, call, dev = _dev()
    q, d = Theta.shape[1], t.d
    wsb = C.c_uint64(0)
    call("obhip_sobol_workspace_bytes", t.p, d, q, C.byref(wsb))
    ws = torch.full((wsb.value // 8,), NAN, dtype=torch.float64, device=dev)
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    dm, dc = torch.from_numpy(pm).to(dev), torch.from_numpy(pc).to(dev)
    out = torch.full((q, 2 + 2 * d), NAN, dtype=torch.float64, device=dev)
    g = torch.full((q, len(pm)), NAN, dtype=torch.float64, device=dev) if with_g else None
    call("obhip_sobol_dev", t._h, dth.data_ptr(), q, dm.data_ptr(), dc.data_ptr(), out.data_ptr(),
         None if g is None else g.data_ptr(), ws.data_ptr(), wsb.value)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if g is None else g.cpu().numpy()


def split_out(out, d):
    return dict(mu=out[:, 0], V=out[:, 1], V1=out[:, 2:2 + d].T, VT=out[:, 2 + d:].T)


@pytest.mark.parametrize("p,d,q", PAIR_CASES)
def test_pair_sums_on_random_tables(p, d, q):
    c = pair_case(p, d, q)
    assert not c["terms"][0].any()                                               # the all-zero-level term
    pm, pc = S.pack_tables(c["m"], c["Cv"])
    out, g = run_sobol(c["t"], c["Theta"], pm, pc)
    out2, g2 = run_sobol(c["t"], c["Theta"], pm, pc)
    out3, _ = run_sobol(c["t"], c["Theta"], pm, pc, with_g=False)
    f, got = c["f"], split_out(out, d)
    r = {k: E.worst_ratio(got[k], f[k], f["tol_" + k]) for k in ("mu", "V", "V1", "VT")}
    off = np.concatenate([[0], np.cumsum(c["levels"])])
    r["g"] = max(E.worst_ratio(g[:, off[l]:off[l + 1]].T, f["g"][l], f["tol_g"][l]) for l in range(d))
    print("p=%d d=%d q=%d: err/tolerance %s" % (p, d, q, ", ".join("%s %.3g" % kv for kv in r.items())))
    assert np.all(np.isfinite(out))
    assert max(r.values()) < 1
    assert np.array_equal(out, out2) and np.array_equal(g, g2)                   # the same bits on every call
    assert np.array_equal(out, out3)                                             # with and without d_g


# ---- end to end ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e_case(name):
    import ob_oracle as O
    mdl = golden_model(name) if name != "d5" else d5_model()
    kinds, terms, om_o = mdl["kinds"], mdl["terms"], mdl["om_o"]
    d = len(kinds)
    rng = np.random.default_rng(7 + d)
    n = 200
    nodes, w = sample_x(rng, n, kinds), some_zero_weights(rng, n, d)
    Theta = theta_of(terms, 5, 11 + d)
    levels = S.levels_of(terms)
    ref = reference_of(om_o, nodes)
    m, Cv = S.tables_from_bases([ref.getbase(l)[0] for l in range(d)], levels, w)
    f = S.formulas(terms, Theta, m, Cv)
    b = O.OuterBase(om_o, nodes)
    m64, C64 = S.tables_from_bases([b.getbase(l + 1) for l in range(d)], levels, w, dtype=np.float64)
    f64 = S.formulas(terms, Theta, m64, C64, dtype=np.float64)
    return dict(mdl=mdl, nodes=nodes, w=w, Theta=Theta, levels=levels, f=f, f64=f64)


@pytest.mark.parametrize("name", ["mixed_d3", "mat25_d8"])
def test_sobol_end_to_end(name):
    """per entry the scale is the stage-2 tolerance (gamma . sum |summands|); the float64 restatement's worst
    err / scale is measured here, and the device is allowed eight times that"""
    import outerbase_amd as ob
    c = e2e_case(name)
    mdl, f, f64 = c["mdl"], c["f"], c["f64"]
    mom = ob.input_moments(mdl["om_d"], mdl["terms"], c["nodes"], c["w"])
    res = ob.sobol(mdl["om_d"], mdl["terms"], c["Theta"], mom)
    got = dict(mu=res.mean, V=res.var, V1=res.first_var, VT=res.total_var)
    keys = ("mu", "V", "V1", "VT")
    r64 = max(E.worst_ratio(f64[k], f[k], f["tol_" + k]) for k in keys)
    rdev = max(E.worst_ratio(got[k], f[k], f["tol_" + k]) for k in keys)
    print("%s end to end: float64 restatement %.3g, device %.3g of the scale; device / restatement %.3g" % (
        name, r64, rdev, rdev / r64))
    assert rdev <= 8 * r64
    assert np.all(np.abs(res.first - E._f64(f["V1"] / f["V"][None, :])) < 1e-9)
    assert np.all(np.abs(res.total - E._f64(f["VT"] / f["V"][None, :])) < 1e-9)
    assert np.all(res.first <= res.total + 1e-12) and np.all(res.total <= 1 + 1e-12)


@pytest.mark.parametrize("name,dim", [("mixed_d3", 2), ("mat25_d8", 5), ("mixed_d3", 1)])
def test_main_effect_curve(name, dim):
    """130 grid points (three blocks of 64 lanes, the last one partly filled) against sum_t g[t] R[:, t] - mu in
    long double, g and mu as the device returned them: C . bound + gamma_{L+2} . sum |summands|"""
    import outerbase_amd as ob
    c = e2e_case(name)
    mdl = c["mdl"]
    mom = ob.input_moments(mdl["om_d"], mdl["terms"], c["nodes"], c["w"])
    res = ob.sobol(mdl["om_d"], mdl["terms"], c["Theta"], mom)
    grid = np.sort(sample_x(np.random.default_rng(130), 130, mdl["kinds"])[:, dim])
    curve = ob.main_effects(mdl["om_d"], mdl["terms"], c["Theta"], mom, dim, grid)
    assert curve.shape == (130, c["Theta"].shape[1])
    x = np.tile(c["nodes"][:1], (130, 1))
    x[:, dim] = grid
    ref = reference_of(mdl["om_o"], x)
    Cc = E.constant_from_oracle_ratio(S.oracle_getbase_ratio(ref, mdl["om_o"], x, c["levels"]))
    L, off = c["levels"][dim], int(c["levels"][:dim].sum())
    R, bR = (a[:, :L] for a in ref.getbase(dim))
    g = res.g.cpu().numpy()[:, off:off + L].T                                    # L x q
    want = R @ np.asarray(g, dtype=ld) - np.asarray(res.mean, dtype=ld)[None, :]
    tol = Cc * (E._f64(bR) @ np.abs(g)) + E.gamma(L + 2) * (np.abs(E._f64(R)) @ np.abs(g) + np.abs(res.mean)[None, :])
    r = E.worst_ratio(curve, want, tol)
    print("%s main effect of dimension %d: err/tolerance %.3g" % (name, dim, r))
    assert r < 1


def test_multifit_sobol_is_the_module_function_in_raw_units():
    import outerbase_amd as ob
    c = e2e_case("mixed_d3")
    mdl, q = c["mdl"], c["Theta"].shape[1]
    rng = np.random.default_rng(5)
    meansd = np.stack([rng.standard_normal(q), rng.uniform(0.5, 3.0, q), np.ones(q)], axis=1)
    t = ob.obmod._Terms(mdl["om_d"], mdl["terms"])
    mf = ob.MultiFit(mdl["om_d"], t, c["Theta"], meansd, np.ones(len(mdl["terms"])), 0.0, 6.0)
    res = mf.sobol(c["nodes"], c["w"])
    mom = ob.input_moments(mdl["om_d"], t, c["nodes"], c["w"])
    base = ob.sobol(mdl["om_d"], t, c["Theta"], mom)
    cent, sca = meansd[:, 0], meansd[:, 1]
    assert np.array_equal(res.mean, cent + sca * base.mean)
    assert np.array_equal(res.var, base.var * (sca * sca))
    assert np.array_equal(res.first_var, base.first_var * (sca * sca)[None, :])
    assert np.array_equal(res.total_var, base.total_var * (sca * sca)[None, :])
    assert np.array_equal(res.first, base.first) and np.array_equal(res.total, base.total)
    grid = np.linspace(0.1, 0.9, 7)
    assert np.array_equal(mf.main_effects(0, grid, c["nodes"], c["w"]),
                          ob.main_effects(mdl["om_d"], t, c["Theta"], mom, 0, grid) * sca[None, :])


def test_zero_coefficients_give_zero_variances_and_nan_indices():
    import outerbase_amd as ob
    c = e2e_case("mixed_d3")
    mdl = c["mdl"]
    mom = ob.input_moments(mdl["om_d"], mdl["terms"], c["nodes"])
    res = ob.sobol(mdl["om_d"], mdl["terms"], np.zeros((len(mdl["terms"]), 3)), mom)
    assert np.all(res.mean == 0) and np.all(res.var == 0) and np.all(res.first_var == 0) and np.all(res.total_var == 0)
    assert np.all(np.isnan(res.first)) and np.all(np.isnan(res.total))


def test_uniform_measure_by_gauss_legendre_nodes():
    """the quadrature route: 16 nodes per dimension with their weights, against the long-double tables of the
    same discrete measure"""
    import outerbase_amd as ob
    mdl = golden_model("mat25_d8")
    d = len(mdl["kinds"])
    nodes, w = ob.uniform_nodes(np.full(d, 0.05), np.full(d, 0.95), order=16)
    Theta = theta_of(mdl["terms"], 3, 2)
    levels = S.levels_of(mdl["terms"])
    ref = reference_of(mdl["om_o"], nodes)
    Cc = E.constant_from_oracle_ratio(S.oracle_getbase_ratio(ref, mdl["om_o"], nodes, levels))
    (m, Cv), (tm, tc) = S.ref_tables(ref, levels, w, Cc)
    mom = ob.input_moments(mdl["om_d"], mdl["terms"], nodes, w)
    r = max(max(E.worst_ratio(mom.mean[l], m[l], tm[l]), E.worst_ratio(mom.cov[l], Cv[l], tc[l])) for l in range(d))
    res = ob.sobol(mdl["om_d"], mdl["terms"], Theta, mom)
    f = S.formulas(mdl["terms"], Theta, mom.mean, mom.cov)
    got = dict(mu=res.mean, V=res.var, V1=res.first_var, VT=res.total_var)
    r2 = max(E.worst_ratio(got[k], f[k], f["tol_" + k]) for k in got)
    print("Gauss-Legendre nodes: tables %.3g, sums on the device's tables %.3g of the tolerance" % (r, r2))
    assert r < 1 and r2 < 1
