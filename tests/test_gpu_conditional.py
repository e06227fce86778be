"""Conditional moments on the GPU (obhip_conditional_tables_dev, obhip_conditional_moments_dev and what is built on
them) against the long-double reference of tests/conditional_ref.py, which sums over pairs of terms without any
grouping.

Group tables on random float64 tables: every entry within gamma . sum |summands|, K symmetric to the bit, the same
bits on two calls.  Row pass: the device's own float64 moment tables on both sides, every output within
C . bound + gamma_k . sum |summands| (k = p + d + 4 for M and dM, p^2 + 3 d + 4 for W and dW), C eight times the
float64 restatement's own err / bound on the case; on the LDS route and under OBHIP_FORCE_GENERIC.  Then the
chunking, the NULL outputs, the cross-checks against the entries that exist, the route through predict_product,
MultiFit.conditional and the refusals.  Every test prints err / tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import conditional_ref as R
import extended_dx_ref as X
import extended_jac_ref as J
import extended_ref as E
import sobol_ref as S
from conftest import knots_for, make_pair, sample_x
from test_sobol_host import golden_model, some_zero_weights, theta_of

pytestmark = pytest.mark.gpu

NAN = float("nan")
ld = np.longdouble
NS = (1, 63, 64, 65, 200)
NMAX = 200


def _dev():
    import torch
    from outerbase_amd._lib import call
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return torch, call, dev


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


# ---- the group tables on random tables --------------------------------------------------------------------
TABLE_CASES = [(1, 1, 3), (15, 2, 5), (16, 1, 4), (17, 2, 5), (129, 7, 9), (129, 2, 40)]


@functools.lru_cache(maxsize=None)
def table_case(G, ne, d):
    import outerbase_amd as ob
    rng = np.random.default_rng(100 * G + 10 * ne + d)
    noise = np.sort(rng.choice(d, size=ne, replace=False))
    levels = rng.integers(2, 5, size=d)
    if ne == 1:
        levels[noise[0]] = max(G, 2)
    elif ne == 2:
        levels[noise] = 12
    tuples = set()
    while len(tuples) < G:
        tuples.add(tuple(int(rng.integers(0, levels[l])) for l in noise) if G > 1 else (0,) * ne)
    tuples = [list(t) for t in tuples]
    rng.shuffle(tuples)
    p = G + 7
    terms = np.zeros((p, d), dtype=np.int64)
    ctrl = R.control_dims(d, noise)
    seen = set()
    for k in range(p):
        terms[k, noise] = tuples[k] if k < G else tuples[int(rng.integers(G))]
        while True:                                              # distinct terms: a fresh tuple on the control side
            terms[k, ctrl] = [int(rng.integers(0, levels[l])) for l in ctrl]
            if tuple(terms[k]) not in seen:
                seen.add(tuple(terms[k]))
                break
    levels = terms.max(axis=0) + 1
    kinds = ["mat25"] * d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    m, Cv = S.random_tables(rng, levels)
    return dict(om=om, t=ob.obmod._Terms(om, terms), terms=terms, noise=noise, levels=levels, m=m, Cv=Cv)


def run_tables(t, noise, pm, pc, G):
    torch, call, dev = _dev()
    de = _u32(noise)
    dm, dc = torch.from_numpy(pm).to(dev), torch.from_numpy(pc).to(dev)
    mE = torch.full((G,), NAN, dtype=torch.float64, device=dev)
    K = torch.full((G, G), NAN, dtype=torch.float64, device=dev)
    call("obhip_conditional_tables_dev", t._h, de.ctypes.data, de.size, dm.data_ptr(), dc.data_ptr(), mE.data_ptr(),
         K.data_ptr())
    torch.cuda.synchronize()
    return mE.cpu().numpy(), K.cpu().numpy()


@pytest.mark.parametrize("G,ne,d", TABLE_CASES)
def test_group_tables_on_random_tables(G, ne, d):
    import outerbase_amd as ob
    c = table_case(G, ne, d)
    lay = ob.conditional_layout(c["om"], c["t"], c["noise"])
    gof, tuples = R.groups_of(c["terms"], c["noise"])
    assert lay["n_groups"] == G == len(tuples) and np.array_equal(lay["group_of"], gof)
    pm, pc = S.pack_tables(c["m"], c["Cv"])
    mE, K = run_tables(c["t"], c["noise"], pm, pc, G)
    mE2, K2 = run_tables(c["t"], c["noise"], pm, pc, G)
    wm, wK, tm, tK = R.group_tables(tuples, [c["m"][l] for l in c["noise"]], [c["Cv"][l] for l in c["noise"]])
    rm, rK = E.worst_ratio(mE, wm, tm), E.worst_ratio(K, wK, tK)
    print("G=%d |E|=%d d=%d: err/tolerance mE %.3g, K %.3g" % (G, ne, d, rm, rK))
    assert np.all(np.isfinite(mE)) and np.all(np.isfinite(K))
    assert rm < 1 and rK < 1
    assert np.array_equal(K, K.T)                                            # symmetric to the bit
    assert np.array_equal(mE, mE2) and np.array_equal(K, K2)                 # the same bits on every call


# ---- the row pass -----------------------------------------------------------------------------------------
def _hyp(kinds, seed):
    rng = np.random.default_rng(seed)
    nh = sum(E.NUMHYP[k] for k in kinds)
    return rng.uniform(0.1, 0.4, nh) * rng.choice([-1.0, 1.0], nh)


@functools.lru_cache(maxsize=None)
def model(name):
    if name in ("mixed_d3", "mat25_d8"):
        g = golden_model(name)
        return dict(kinds=g["kinds"], om_o=g["om_o"], om_d=g["om_d"])
    d = {"d12": 12, "d40": 40}[name]
    kinds = (["mat25", "mat25pow", "mat25ang"] * 14)[:d]
    om_o, om_d = make_pair(kinds, knots_for(kinds, 12), hyp=_hyp(kinds, d))
    return dict(kinds=kinds, om_o=om_o, om_d=om_d)


def random_terms(rng, p, d, levmax, nfac, fixed=None):
    """p distinct terms with nfac(rng) factors each at levels 1 .. levmax; fixed: {dimension: level} of every term"""
    seen, out = set(), []
    while len(out) < p:
        t = np.zeros(d, dtype=np.int64)
        free = [l for l in range(d) if not fixed or l not in fixed]
        dims = rng.choice(free, size=min(len(free), int(nfac(rng))), replace=False)
        t[dims] = rng.integers(1, levmax + 1, size=len(dims))
        for l, v in (fixed or {}).items():
            t[l] = v
        if tuple(t) not in seen:
            seen.add(tuple(t))
            out.append(t)
    return np.stack(out)


# name -> (model, terms (callable of the model), noise dimensions, q)
def _select(p):
    return lambda mdl: np.ascontiguousarray(mdl["om_o"].selectterms(p))


ROW_CASES = {
    "d3 p127 first": ("mixed_d3", _select(127), [0], 1),
    "d3 p129 last": ("mixed_d3", _select(129), [2], 3),
    "d3 p300 all but one": ("mixed_d3", _select(300), [0, 2], 3),
    "d3 p1 one": ("mixed_d3", _select(1), [1], 1),
    "d8 p300 interleaved": ("mat25_d8", _select(300), [0, 2, 4, 6], 3),
    "d8 p129 last": ("mat25_d8", _select(129), [7], 1),
    "d8 p127 all but one": ("mat25_d8", _select(127), [0, 1, 2, 3, 4, 5, 6], 3),
    "d8 p300 first": ("mat25_d8", _select(300), [0], 1),
    # every term at level 0 on E: one group, a small positive variance
    "d8 level 0 on E": ("mat25_d8", lambda mdl: random_terms(np.random.default_rng(1), 129, 8, 3,
                                                              lambda r: r.integers(1, 4), {1: 0, 5: 0}), [1, 5], 3),
    # every term a group of its own
    "d8 G = p": ("mat25_d8", lambda mdl: np.array([[k % 5, 1 + k % 2, 0, k // 5, 0, k % 3, 0, 2] for k in range(40)]),
                 [0, 3], 1),
    # 9 to 11 factors on S: beyond the 8 the LDS route takes
    "d12 9-11 factors": ("d12", lambda mdl: random_terms(np.random.default_rng(2), 40, 12, 2,
                                                         lambda r: r.integers(10, 13)), [3], 3),
    # 39 control dimensions with four used levels each: the derivative tile is beyond the LDS
    "d40 beyond the LDS tile": ("d40", lambda mdl: np.concatenate([
        random_terms(np.random.default_rng(3), 150, 40, 4, lambda r: r.integers(1, 4)),
        np.full((1, 40), 4, dtype=np.int64), np.eye(40, dtype=np.int64)[:4] * 3]), [17], 1),
}


@functools.lru_cache(maxsize=None)
def row_case(key):
    """the model, the device's own moment tables of a weighted measure, NMAX rows and the reference on them"""
    import outerbase_amd as ob
    name, make_terms, noise, q = ROW_CASES[key]
    mdl = model(name)
    kinds, om_o, om_d = mdl["kinds"], mdl["om_o"], mdl["om_d"]
    d = len(kinds)
    terms = np.ascontiguousarray(make_terms(mdl), dtype=np.int64)
    rng = np.random.default_rng(len(key))
    x = sample_x(rng, NMAX, kinds)
    nodes, w = sample_x(rng, 40, kinds), some_zero_weights(rng, 40, d)
    Theta = theta_of(terms, q, 5 + len(key))
    t = ob.obmod._Terms(om_d, terms)
    mom = ob.input_moments(om_d, t, nodes, w)
    ref = X.reference_dx_of(om_o, x)
    Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, om_o, x, terms))
    f = R.moments(ref, terms, Theta, noise, mom.mean, mom.cov, Cc, grad=True)
    return dict(mdl=mdl, terms=terms, t=t, noise=noise, q=q, x=x, Theta=Theta, mom=mom, ref=ref, C=Cc, f=f,
                lay=ob.conditional_layout(om_d, t, noise))


def ratios(res, f, n):
    return {"M": E.worst_ratio(res.mean, f["M"][:n], f["tol_M"][:n]),
            "W": E.worst_ratio(res.var, f["W"][:n], f["tol_W"][:n]),
            "dM": E.worst_ratio(res.grad_mean, f["dM"][:n], f["tol_dM"][:n]),
            "dW": E.worst_ratio(res.grad_var, f["dW"][:n], f["tol_dW"][:n])}


@pytest.mark.parametrize("route", ["lds", "generic"])
@pytest.mark.parametrize("key", list(ROW_CASES))
def test_row_pass_against_extended_reference(key, route, monkeypatch):
    import outerbase_amd as ob
    if route == "generic":
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    c = row_case(key)
    om_d, f = c["mdl"]["om_d"], c["f"]
    gof, tuples = R.groups_of(c["terms"], c["noise"])
    assert c["lay"]["n_groups"] == len(tuples) and np.array_equal(c["lay"]["group_of"], gof)
    if key == "d8 level 0 on E":
        assert len(tuples) == 1 and np.all(E._f64(f["W"]) > 0)
    if key == "d8 G = p":
        assert len(tuples) == len(c["terms"])
    if key in ("d12 9-11 factors", "d40 beyond the LDS tile"):
        assert not c["lay"]["fused"]
    elif route == "lds":
        assert c["lay"]["fused"]
    worst = {}
    for n in NS:
        res = ob.conditional_moments(om_d, c["t"], c["Theta"], c["mom"], c["noise"], c["x"][:n], grad=True)
        assert res.mean.shape == (n, c["q"]) and res.grad_var.shape == (n, len(res.control_dims), c["q"])
        for k, v in ratios(res, f, n).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("%s (%s, p=%d, G=%d, C=%.3g): err/tolerance %s" % (
        key, route, len(c["terms"]), len(tuples), c["C"], ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) < 1


def run_raw(c, n, chunk_rows=0, want=(True, True, True, True)):
    """obhip_conditional_moments_dev on NaN-filled buffers; want: which of mean, var, gradmean, gradvar are asked for"""
    torch, call, dev = _dev()
    t, q = c["t"], c["q"]
    ctrl = R.control_dims(t.d, c["noise"])
    de = _u32(c["noise"])
    dx = torch.from_numpy(np.ascontiguousarray(c["x"][:n][:, ctrl].T)).to(dev)
    dth = torch.from_numpy(np.ascontiguousarray(c["Theta"].T)).to(dev)
    shapes = [(q, n), (q, n), (q, len(ctrl), n), (q, len(ctrl), n)]
    bufs = [torch.full(s, NAN, dtype=torch.float64, device=dev) if w else None for s, w in zip(shapes, want)]
    call("obhip_conditional_moments_dev", c["mdl"]["om_d"]._h, t._h, dth.data_ptr(), q, de.ctypes.data, de.size,
         c["mom"].mean_dev.data_ptr(), c["mom"].cov_dev.data_ptr(), dx.data_ptr(), n, chunk_rows,
         *[None if b is None else b.data_ptr() for b in bufs])
    torch.cuda.synchronize()
    return [None if b is None else b.cpu().numpy() for b in bufs]


@pytest.mark.parametrize("key", ["d3 p300 all but one", "d8 p300 interleaved", "d40 beyond the LDS tile"])
def test_chunked_call_and_second_call_give_the_same_bits(key, monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    c = row_case(key)
    whole, again, chunked = run_raw(c, 200), run_raw(c, 200), run_raw(c, 200, chunk_rows=128)
    for a, b, ch in zip(whole, again, chunked):
        assert np.all(np.isfinite(a))
        assert np.array_equal(a, b)
        assert np.array_equal(a, ch)


def test_each_output_alone_has_the_bits_of_all_together(monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    c = row_case("d8 p300 interleaved")
    full = run_raw(c, 65)
    for i in range(4):
        want = tuple(j == i for j in range(4))
        alone = run_raw(c, 65, want=want)
        assert np.array_equal(alone[i], full[i])
        assert all(alone[j] is None for j in range(4) if j != i)
    assert all(b is None for b in run_raw(c, 65, want=(False,) * 4))       # nothing asked for: nothing done


def test_a_row_that_is_not_finite_gets_nan_and_its_neighbours_nothing():
    c = dict(row_case("d8 p129 last"))
    full = run_raw(c, 65)
    x = c["x"].copy()
    x[3, 2] = NAN
    c["x"] = x
    bad = run_raw(c, 65)
    for a, b in zip(full, bad):
        assert np.all(np.isnan(b[..., 3]))
        keep = np.arange(65) != 3
        assert np.array_equal(a[..., keep], b[..., keep])


# ---- cross-checks against the entries that exist -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cross_case(name):
    import outerbase_amd as ob
    mdl = golden_model(name)
    kinds, terms, om_d = mdl["kinds"], mdl["terms"], mdl["om_d"]
    d = len(kinds)
    rng = np.random.default_rng(17 + d)
    nodes, w = sample_x(rng, 50, kinds), some_zero_weights(rng, 50, d)
    Theta = theta_of(terms, 3, 23 + d)
    t = ob.obmod._Terms(om_d, terms)
    mom = ob.input_moments(om_d, t, nodes, w)
    return dict(mdl=mdl, kinds=kinds, terms=terms, t=t, nodes=nodes, w=w, Theta=Theta, mom=mom, d=d)


def _ref_on(c, x, noise, grad=False):
    om_o = c["mdl"]["om_o"]
    ref = X.reference_dx_of(om_o, x)
    Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, om_o, x, c["terms"]))
    return R.moments(ref, c["terms"], c["Theta"], noise, c["mom"].mean, c["mom"].cov, Cc, grad=grad), Cc


@pytest.mark.parametrize("name,dim", [("mixed_d3", 1), ("mat25_d8", 5)])
def test_one_control_dimension_is_the_main_effect_and_the_law_of_total_variance(name, dim):
    """S = {dim}.  On a grid M is obhip_main_effect_dev's curve (the mean added back); at the nodes of the
    dimension sum_i w^_i W_i = V - V1_dim of obhip_sobol_dev.  Each within the sum of the two sides' tolerances:
    the reference's for this side; for the other the same C . bound and sum of magnitudes with the gamma of its
    own summation (p + d + L + 4 for the curve), and the tolerances of sobol_ref for V and V1."""
    import outerbase_amd as ob
    c = cross_case(name)
    om_d, d = c["mdl"]["om_d"], c["d"]
    noise = [l for l in range(d) if l != dim]
    p, L = len(c["terms"]), int(c["mom"].levels[dim])
    grid = np.sort(sample_x(np.random.default_rng(130), 130, c["kinds"])[:, dim])
    x = np.tile(c["nodes"][:1], (130, 1))
    x[:, dim] = grid
    res = ob.conditional_moments(om_d, c["t"], c["Theta"], c["mom"], noise, grid[:, None])
    sob = ob.sobol(om_d, c["t"], c["Theta"], c["mom"])
    curve = ob.main_effects(om_d, c["t"], c["Theta"], c["mom"], dim, grid) + sob.mean[None, :]
    f, Cc = _ref_on(c, x, noise)
    tol_other = Cc * f["bnd_M"] + E.gamma(p + d + L + 4) * (f["abs_M"] + np.abs(sob.mean)[None, :])
    r1 = E.worst_ratio(res.mean, np.asarray(curve, dtype=ld), f["tol_M"] + tol_other)
    # the law of total variance at the nodes
    xn = np.tile(c["nodes"][:1], (len(c["nodes"]), 1))
    xn[:, dim] = c["nodes"][:, dim]
    resn = ob.conditional_moments(om_d, c["t"], c["Theta"], c["mom"], noise, xn)
    fn, _ = _ref_on(c, xn, noise)
    wn = S.normalised_weights(c["w"], len(c["nodes"]), d)[:, dim]
    fs = S.formulas(c["terms"], c["Theta"], c["mom"].mean, c["mom"].cov)
    got = wn @ np.asarray(resn.var, dtype=ld)
    want = np.asarray(sob.var, dtype=ld) - np.asarray(sob.first_var[dim], dtype=ld)
    tol = E._f64(wn) @ fn["tol_W"] + fs["tol_V"] + fs["tol_V1"][dim]
    r2 = E.worst_ratio(got, want, tol)
    print("%s S = {%d}: main effect %.3g, law of total variance %.3g of the tolerance" % (name, dim, r1, r2))
    assert r1 < 1 and r2 < 1


@pytest.mark.parametrize("name,di,dj", [("mixed_d3", 0, 2), ("mat25_d8", 2, 5)])
def test_two_control_dimensions_are_the_interaction_surface(name, di, dj):
    """S = {di, dj}: M on a grid is obhip_interaction_effect_dev's surface E[f | x_i, x_j]"""
    import outerbase_amd as ob
    c = cross_case(name)
    torch, call, dev = _dev()
    om_d, d, q = c["mdl"]["om_d"], c["d"], c["Theta"].shape[1]
    noise = [l for l in range(d) if l not in (di, dj)]
    rng = np.random.default_rng(9)
    gi, gj = sample_x(rng, 9, c["kinds"])[:, di].copy(), sample_x(rng, 11, c["kinds"])[:, dj].copy()
    s2 = ob.sobol2(om_d, c["t"], c["Theta"], c["mom"])
    dzi, dzj = torch.from_numpy(gi).to(dev), torch.from_numpy(gj).to(dev)
    out = torch.full((q, 9, 11), NAN, dtype=torch.float64, device=dev)
    call("obhip_interaction_effect_dev", om_d._h, c["t"]._h, di, dj, s2.G.data_ptr(), q, dzi.data_ptr(), 9,
         dzj.data_ptr(), 11, out.data_ptr())
    torch.cuda.synchronize()
    surf = out.cpu().numpy().transpose(1, 2, 0).reshape(99, q)
    x = np.tile(c["nodes"][:1], (99, 1))
    x[:, di], x[:, dj] = np.repeat(gi, 11), np.tile(gj, 9)
    res = ob.conditional_moments(om_d, c["t"], c["Theta"], c["mom"], noise, x)
    f, Cc = _ref_on(c, x, noise)
    p, LL = len(c["terms"]), int(c["mom"].levels[di] * c["mom"].levels[dj])
    tol_other = Cc * f["bnd_M"] + E.gamma(p + d + LL + 4) * f["abs_M"]
    r = E.worst_ratio(res.mean, np.asarray(surf, dtype=ld), f["tol_M"] + tol_other)
    print("%s S = {%d, %d}: err/tolerance %.3g" % (name, di, dj, r))
    assert r < 1


def test_mean_and_variance_over_five_by_five_noise_nodes_through_predict_product():
    """the independent route: predict_product on the rows times the 25 pairs of noise nodes, reduced in long double
    with the weights of the measure; tolerance: the reference's plus, for the other side, C . bound + gamma_{p+d+29}
    on the same sums (25 more summands), the second moment carrying twice the relative error of a value"""
    import outerbase_amd as ob
    c = cross_case("mixed_d3")
    om_d, d = c["mdl"]["om_d"], c["d"]
    noise, ctrl = [0, 2], [1]
    rng = np.random.default_rng(4)
    nodes = sample_x(rng, 5, c["kinds"])
    w = rng.uniform(0.2, 1.0, (5, d))
    mom = ob.input_moments(om_d, c["t"], nodes, w)
    x = sample_x(rng, 65, c["kinds"])
    res = ob.conditional_moments(om_d, c["t"], c["Theta"], mom, noise, x)
    rows, idx = S.grid_rows(nodes[:, noise])
    wn = S.normalised_weights(w, 5, d)
    wr = wn[idx[:, 0], 0] * wn[idx[:, 1], 2]
    pred = np.asarray(ob.predict_product(om_d, c["t"], c["Theta"], x[:, ctrl], rows, noise), dtype=ld)   # na x nb x q
    mean = np.einsum("b,abj->aj", wr, pred)
    var = np.einsum("b,abj->aj", wr, (pred - mean[:, None, :]) ** 2)
    cc = dict(c)
    cc["mom"] = mom
    f, Cc = _ref_on(cc, x, noise)
    p = len(c["terms"])
    tol_m = f["tol_M"] + Cc * f["bnd_M"] + E.gamma(p + d + 29) * f["abs_M"]
    # |f| <= sum of magnitudes on every node pair: a relative error e of the values is one of 2 e + e^2 of their
    # centred squares, measured against the second moment of the magnitudes
    B, bB = X.reference_dx_of(c["mdl"]["om_o"], _expand(x, rows, noise, d)).getmat(c["terms"])
    aTh = np.abs(c["Theta"])
    aF = (np.abs(E._f64(B)) @ aTh).reshape(65, 25, -1)
    bF = (E._f64(bB) @ aTh).reshape(65, 25, -1)
    wrf = E._f64(wr)
    tol_v = f["tol_W"] + 4 * np.einsum("b,abj->aj", wrf, (Cc * bF + E.gamma(p + d + 29) * aF) * aF)
    r1, r2 = E.worst_ratio(res.mean, mean, tol_m), E.worst_ratio(res.var, var, tol_v)
    print("5 x 5 noise nodes through predict_product: mean %.3g, variance %.3g of the tolerance" % (r1, r2))
    assert r1 < 1 and r2 < 1


def _expand(x, rows, noise, d):
    """the na nb full-width rows of the pairs (row of x, row of the noise grid), a slow"""
    full = np.repeat(x, len(rows), axis=0)
    full[:, noise] = np.tile(rows, (len(x), 1))
    return full


def test_multifit_conditional_is_the_module_function_in_raw_units():
    import outerbase_amd as ob
    c = cross_case("mixed_d3")
    om_d, q = c["mdl"]["om_d"], c["Theta"].shape[1]
    rng = np.random.default_rng(5)
    meansd = np.stack([rng.standard_normal(q), rng.uniform(0.5, 3.0, q), np.ones(q)], axis=1)
    mf = ob.MultiFit(om_d, c["t"], c["Theta"], meansd, np.ones(len(c["terms"])), 0.0, 6.0)
    x = sample_x(rng, 65, c["kinds"])
    res = mf.conditional(x, [0, 2], c["nodes"], c["w"], grad=True)
    base = ob.conditional_moments(om_d, c["t"], c["Theta"], c["mom"], [0, 2], x[:, [1]], grad=True)
    cent, sca = meansd[:, 0], meansd[:, 1]
    assert np.array_equal(res.control_dims, [1]) and np.array_equal(base.control_dims, [1])
    assert np.array_equal(res.mean, cent[None, :] + sca[None, :] * base.mean)
    assert np.array_equal(res.var, base.var * (sca * sca)[None, :])
    assert np.array_equal(res.grad_mean, base.grad_mean * sca[None, None, :])
    assert np.array_equal(res.grad_var, base.grad_var * (sca * sca)[None, None, :])
    plain = mf.conditional(x, [0, 2], c["nodes"], c["w"])
    assert plain.grad_mean is None and plain.grad_var is None and np.array_equal(plain.mean, res.mean)


# ---- the refusals -------------------------------------------------------------------------------------------
def test_every_refusal_returns_before_the_device_and_writes_nothing():
    from outerbase_amd import ObhipError
    from outerbase_amd._lib import lib
    torch, call, dev = _dev()
    c = row_case("d3 p127 first")
    t, om_d, q, n = c["t"], c["mdl"]["om_d"], 1, 65
    dth = torch.from_numpy(np.ascontiguousarray(c["Theta"].T)).to(dev)
    dx = torch.from_numpy(np.ascontiguousarray(c["x"][:n, 1:].T)).to(dev)
    out = [torch.full((4 * n,), NAN, dtype=torch.float64, device=dev) for _ in range(4)]
    dm, dc = c["mom"].mean_dev, c["mom"].cov_dev

    def moments(**kw):
        a = dict(m=om_d._h, t=t._h, th=dth.data_ptr(), q=q, de=_u32([0]), dm=dm.data_ptr(), dc=dc.data_ptr(),
                 x=dx.data_ptr(), n=n, chunk=0)
        a.update(kw)
        de = a["de"]
        return lib.obhip_conditional_moments_dev(a["m"], a["t"], a["th"], a["q"], None if de is None else de.ctypes.data,
                                                 0 if de is None else de.size, a["dm"], a["dc"], a["x"], a["n"],
                                                 a["chunk"], *[o.data_ptr() for o in out])
    bad = {"null model": dict(m=None), "null terms": dict(t=None), "null Theta": dict(th=None),
           "null tables": dict(dm=None), "null cov": dict(dc=None), "null xs": dict(x=None), "null dims_e": dict(de=None),
           "empty dims_e": dict(de=_u32([])), "all dimensions": dict(de=_u32([0, 1, 2])),
           "unsorted": dict(de=_u32([2, 0])), "repeated": dict(de=_u32([1, 1])), "out of range": dict(de=_u32([3])),
           "chunk_rows 100": dict(chunk=100), "chunk_rows 64": dict(chunk=64), "q = 0": dict(q=0),
           "q above 65535": dict(q=65536), "more than 2^40 rows": dict(n=(1 << 40) + 1)}
    for what, kw in bad.items():
        assert moments(**kw) == 1, what                                          # OBHIP_ERR_INVALID
    assert all(bool(torch.all(torch.isnan(o))) for o in out)                      # nothing written
    assert moments(n=0) == 0 and all(bool(torch.all(torch.isnan(o))) for o in out)   # n = 0: a no-op
    # the tables entry and the layout share the checks of the dimensions
    mE = torch.full((8,), NAN, dtype=torch.float64, device=dev)
    for de in (_u32([]), _u32([0, 1, 2]), _u32([2, 0]), _u32([3])):
        assert lib.obhip_conditional_tables_dev(t._h, de.ctypes.data, de.size, dm.data_ptr(), dc.data_ptr(),
                                                mE.data_ptr(), mE.data_ptr()) == 1
        assert lib.obhip_conditional_layout(t._h, de.ctypes.data, de.size, None, None, None, None) == 1
    assert lib.obhip_conditional_tables_dev(t._h, _u32([0]).ctypes.data, 1, dm.data_ptr(), dc.data_ptr(), None,
                                            mE.data_ptr()) == 1
    assert bool(torch.all(torch.isnan(mE)))
    with pytest.raises(ValueError):
        import outerbase_amd as ob
        ob.conditional_moments(om_d, t, c["Theta"], c["mom"], [0], c["x"][:5], chunk_rows=100)
    with pytest.raises(ValueError):
        ob.conditional_moments(om_d, t, c["Theta"], c["mom"], [0, 1, 2], c["x"][:5])
    with pytest.raises(ObhipError):                                              # the Python side raises what the library refuses
        call("obhip_conditional_layout", None, _u32([0]).ctypes.data, 1, None, None, None, None)
    assert moments() == 0                                                        # and the library goes on


def limit_models():
    """name -> (device model, terms, noise dimensions, word of the message): term sets beyond the level limit of the
    Sobol passes, beyond their dimension limit, and with noise tables beyond the LDS of a workgroup (3 x 8 x 2 x 60^2
    bytes > 160 KB); the last one is within it once only one of the two wide dimensions is noise"""
    import outerbase_amd as ob

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
    return {"level 256 on E": (lvl, np.array([[0, 0], [256, 1]]), [0], b"255"),
            "level 256 on S": (lvl, np.array([[0, 0], [256, 1]]), [1], b"255"),
            "noise tables beyond the LDS": (big, np.array([[0, 0, 0], [59, 59, 1]]), [0, 1], b"LDS"),
            "256 dimensions": (d256, t256, [0], b"255 dimensions")}


@pytest.mark.parametrize("name", ["level 256 on E", "level 256 on S", "noise tables beyond the LDS", "256 dimensions"])
def test_limits_of_the_sobol_passes_refuse_through_every_entry(name):
    """the level, d and LDS limits reach the entries through cond_setup alone: each is OBHIP_ERR_INVALID from the
    layout, the tables and the moments entry, with the NaN-filled outputs left as they were.  p > 2^24 cannot be built
    through an entry at a size a test can afford (2^24 + 1 terms); tests/conditional_plan_check.cpp walks that
    refusal on the plan."""
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    torch, call, dev = _dev()
    om, terms, noise, word = limit_models()[name]
    t = ob.obmod._Terms(om, np.ascontiguousarray(terms, dtype=np.int64))
    de = _u32(noise)
    G = C.c_uint64(77)
    buf = [torch.full((4096,), NAN, dtype=torch.float64, device=dev) for _ in range(6)]
    tab = torch.zeros(1 << 17, dtype=torch.float64, device=dev)
    assert lib.obhip_conditional_layout(t._h, de.ctypes.data, de.size, C.byref(G), None, None, None) == 1
    assert word in lib.obhip_last_error() and G.value == 77
    assert lib.obhip_conditional_tables_dev(t._h, de.ctypes.data, de.size, tab.data_ptr(), tab.data_ptr(),
                                            buf[0].data_ptr(), buf[1].data_ptr()) == 1
    assert word in lib.obhip_last_error()
    assert lib.obhip_conditional_moments_dev(om._h, t._h, tab.data_ptr(), 1, de.ctypes.data, de.size, tab.data_ptr(),
                                             tab.data_ptr(), tab.data_ptr(), 5, 0, *[b.data_ptr() for b in buf[2:]]) == 1
    assert word in lib.obhip_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.all(torch.isnan(b))) for b in buf)


def test_one_wide_noise_dimension_is_within_the_lds_and_its_tables_are_right():
    """the term set of the LDS refusal with only one of its 60-level dimensions as noise: 3 x 8 x 3601 bytes of LDS,
    more than the 64 KB a kernel has without asking; the tables against the reference"""
    import outerbase_amd as ob
    om, terms, _, _ = limit_models()["noise tables beyond the LDS"]
    t = ob.obmod._Terms(om, np.ascontiguousarray(terms, dtype=np.int64))
    rng = np.random.default_rng(60)
    m, Cv = S.random_tables(rng, [60, 60, 2])
    pm, pc = S.pack_tables(m, Cv)
    assert ob.conditional_layout(om, t, [0])["n_groups"] == 2
    mE, K = run_tables(t, [0], pm, pc, 2)
    wm, wK, tm, tK = R.group_tables([[0], [59]], [m[0]], [Cv[0]])
    assert E.worst_ratio(mE, wm, tm) < 1 and E.worst_ratio(K, wK, tK) < 1 and np.array_equal(K, K.T)


def test_host_buffer_entries_and_python_tables_give_the_device_entries_bits():
    """obhip_conditional_tables and obhip_conditional_moments (xs with a leading dimension, two of the four outputs
    NULL) and sensitivity.conditional_tables against the _dev entries"""
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    c = row_case("d8 p129 last")
    t, om_d, q, n, ldx = c["t"], c["mdl"]["om_d"], c["q"], 65, 70
    de = _u32(c["noise"])
    ctrl = R.control_dims(t.d, c["noise"])
    G = c["lay"]["n_groups"]
    pm, pc = c["mom"].mean_dev.cpu().numpy(), c["mom"].cov_dev.cpu().numpy()
    mE_d, K_d = run_tables(t, c["noise"], pm, pc, G)
    mE_p, K_p = ob.conditional_tables(om_d, t, c["mom"], c["noise"])
    mE_h, K_h = np.full(G, NAN), np.full((G, G), NAN)
    assert lib.obhip_conditional_tables(t._h, de.ctypes.data, de.size, pm.ctypes.data, pc.ctypes.data,
                                        mE_h.ctypes.data, K_h.ctypes.data) == 0
    for a, b in ((mE_p, mE_d), (K_p, K_d), (mE_h, mE_d), (K_h, K_d)):
        assert np.array_equal(a, b)
    full = run_raw(c, n)
    xs = np.full((len(ctrl), ldx), NAN)
    xs[:, :n] = c["x"][:n][:, ctrl].T
    Th = np.ascontiguousarray(c["Theta"].T)
    var, gm = np.full((q, n), NAN), np.full((q, len(ctrl), n), NAN)
    assert lib.obhip_conditional_moments(om_d._h, t._h, Th.ctypes.data, q, de.ctypes.data, de.size, pm.ctypes.data,
                                         pc.ctypes.data, xs.ctypes.data, n, ldx, 0, None, var.ctypes.data,
                                         gm.ctypes.data, None) == 0
    assert np.array_equal(var, full[1]) and np.array_equal(gm, full[2])
