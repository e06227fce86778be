"""Second-order and total-interaction variances and interaction surfaces on the GPU (obhip_sobol2_dev,
obhip_interaction_effect_dev and what is built on them) against the long-double reference of
tests/sobol2_ref.py.

Stage 2 (sums on random float64 tables): every V2, VT2 and entry of G within its own gamma . sum |summands|.
End to end: device tables, then device sums, against long-double sums of long-double tables; allowance eight
times the float64 restatement's own error on the same case.  Every test prints err / tolerance.

TW = 128 is the pair kernel's term-tile width, RC = 2 its response chunk, T = 5 the dimensions per block of
its output triangle (d = 5 | 6 and 10 | 11 add a block), 8 and 24 the dimensions whose row offsets it keeps in
registers (d = 8 | 9, 24 | 25; d = 40 takes the others from memory)."""
import ctypes as C
import functools

import numpy as np
import pytest

import extended_ref as E
import sobol2_ref as S2
import sobol_ref as S
from conftest import knots_for, sample_x
from test_sobol2_host import PAIR2_CASES, pair2_tables
from test_sobol_host import golden_model, reference_of, some_zero_weights, theta_of

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 7
ld = np.longdouble


def _dev():
    import torch
    from outerbase_amd._lib import call
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return torch, call, dev


# ---- stage 2: the sums on random tables -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair2_case(p, d, q):
    import outerbase_amd as ob
    c = pair2_tables(p, d, q)
    kinds = ["mat25"] * d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    return dict(c, om=om, t=ob.obmod._Terms(om, c["terms"]))


def run_sobol2(t, Theta, pm, pc, with_G=True):
    """obhip_sobol2_dev on NaN-filled buffers with PAD doubles behind the outputs -> (out, G, padding untouched)"""
    torch, call, dev = _dev()
    q, d = Theta.shape[1], t.d
    npairs, nG, wsb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    call("obhip_sobol2_layout", t._h, C.byref(npairs), C.byref(nG))
    call("obhip_sobol2_workspace_bytes", t.p, d, q, C.byref(wsb))
    npairs, nG = npairs.value, nG.value
    ws = torch.full((wsb.value // 8,), NAN, dtype=torch.float64, device=dev)
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    dm, dc = torch.from_numpy(pm).to(dev), torch.from_numpy(pc).to(dev)
    out = torch.full((q * 2 * npairs + PAD,), NAN, dtype=torch.float64, device=dev)
    G = torch.full((q * nG + PAD,), NAN, dtype=torch.float64, device=dev) if with_G else None
    call("obhip_sobol2_dev", t._h, dth.data_ptr(), q, dm.data_ptr(), dc.data_ptr(), out.data_ptr(),
         None if G is None else G.data_ptr(), ws.data_ptr(), wsb.value)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    clean = bool(np.all(np.isnan(out[q * 2 * npairs:])))
    g = None
    if G is not None:
        g = G.cpu().numpy()
        clean = clean and bool(np.all(np.isnan(g[q * nG:])))
        g = g[:q * nG].reshape(q, nG)
    return out[:q * 2 * npairs].reshape(q, 2 * npairs), g, clean


@pytest.mark.parametrize("p,d,q", PAIR2_CASES)
def test_pair_sums_on_random_tables(p, d, q):
    c = pair2_case(p, d, q)
    f2 = c["f2"]
    npairs = d * (d - 1) // 2
    pm, pc = S.pack_tables(c["m"], c["Cv"])
    out, g, clean = run_sobol2(c["t"], c["Theta"], pm, pc)
    out2, g2, clean2 = run_sobol2(c["t"], c["Theta"], pm, pc)
    out3, _, clean3 = run_sobol2(c["t"], c["Theta"], pm, pc, with_G=False)
    assert clean and clean2 and clean3                                           # the padding is untouched
    assert np.array_equal(out, out2) and np.array_equal(g, g2)                   # the same bits on every call
    assert np.array_equal(out, out3)                                             # with and without d_G
    assert out.shape == (q, 2 * npairs)
    if d == 1:
        assert out.size == 0 and g.size == 0                                     # no pairs: nothing written
        return
    assert len(set(c["levels"])) > 1 or p == 1
    got = dict(V2=out[:, :npairs].T, VT2=out[:, npairs:].T)
    r = {k: E.worst_ratio(got[k], f2[k], f2["tol_" + k]) for k in ("V2", "VT2")}
    want_G, tol_G = S2.pack_G(f2["G"]), S2.pack_G(f2["tol_G"])
    r["G"] = E.worst_ratio(g, want_G, tol_G)
    print("p=%d d=%d q=%d: err/tolerance %s" % (p, d, q, ", ".join("%s %.3g" % kv for kv in r.items())))
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(g))
    assert max(r.values()) < 1


def test_sobol_dev_returns_the_same_bits_around_a_sobol2_call():
    from test_gpu_sobol import run_sobol
    c = pair2_case(300, 20, 5)
    pm, pc = S.pack_tables(c["m"], c["Cv"])
    before, g_before = run_sobol(c["t"], c["Theta"], pm, pc)
    run_sobol2(c["t"], c["Theta"], pm, pc)
    after, g_after = run_sobol(c["t"], c["Theta"], pm, pc)
    assert np.array_equal(before, after) and np.array_equal(g_before, g_after)
    f = c["f"]
    got = dict(mu=after[:, 0], V=after[:, 1], V1=after[:, 2:2 + 20].T, VT=after[:, 2 + 20:].T)
    assert max(E.worst_ratio(got[k], f[k], f["tol_" + k]) for k in got) < 1


# ---- end to end ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e_case2(name):
    import ob_oracle as O
    mdl = golden_model(name)
    kinds, terms, om_o = mdl["kinds"], mdl["terms"], mdl["om_o"]
    d = len(kinds)
    rng = np.random.default_rng(7 + d)
    n = 200
    nodes, w = sample_x(rng, n, kinds), some_zero_weights(rng, n, d)
    Theta = theta_of(terms, 5, 11 + d)
    levels = S.levels_of(terms)
    ref = reference_of(om_o, nodes)
    m, Cv = S.tables_from_bases([ref.getbase(l)[0] for l in range(d)], levels, w)
    b = O.OuterBase(om_o, nodes)
    m64, C64 = S.tables_from_bases([b.getbase(l + 1) for l in range(d)], levels, w, dtype=np.float64)
    return dict(mdl=mdl, nodes=nodes, w=w, Theta=Theta, levels=levels, f=S.formulas(terms, Theta, m, Cv),
                f2=S2.formulas2(terms, Theta, m, Cv), f2_64=S2.formulas2(terms, Theta, m64, C64, dtype=np.float64))


@pytest.mark.parametrize("name", ["mixed_d3", "mat25_d8"])
def test_sobol2_end_to_end(name):
    """per entry the scale is the stage-2 tolerance (gamma . sum |summands|); the float64 restatement's worst
    err / scale is measured here, and the device is allowed eight times that"""
    import outerbase_amd as ob
    c = e2e_case2(name)
    mdl, f, f2, f64 = c["mdl"], c["f"], c["f2"], c["f2_64"]
    d = len(c["levels"])
    mom = ob.input_moments(mdl["om_d"], mdl["terms"], c["nodes"], c["w"])
    res = ob.sobol2(mdl["om_d"], mdl["terms"], c["Theta"], mom)
    got = dict(V2=res.second_var, VT2=res.total_interaction_var)
    r64 = max(E.worst_ratio(f64[k], f2[k], f2["tol_" + k]) for k in got)
    rdev = max(E.worst_ratio(got[k], f2[k], f2["tol_" + k]) for k in got)
    print("%s end to end: float64 restatement %.3g, device %.3g of the scale; device / restatement %.3g" % (
        name, r64, rdev, rdev / r64))
    assert rdev <= 8 * r64
    assert np.array_equal(res.pairs, f2["pairs"])
    i, j = res.pairs[:, 0], res.pairs[:, 1]
    V = E._f64(f["V"])[None, :]
    assert np.all(np.abs(res.second - E._f64(f2["V2"]) / V) < 1e-9)
    assert np.all(np.abs(res.total_interaction - E._f64(f2["VT2"]) / V) < 1e-9)
    assert np.all(np.abs(res.closed_var / V - E._f64(f["V1"][i] + f["V1"][j] + f2["V2"]) / V) < 1e-9)
    assert np.all(res.second <= res.total_interaction + 1e-12) and np.all(res.second >= -1e-12)
    for mat, flat in ((res.second_var_mat, res.second_var), (res.total_interaction_var_mat, res.total_interaction_var),
                      (res.second_mat, res.second), (res.total_interaction_mat, res.total_interaction)):
        assert mat.shape == (d, d, c["Theta"].shape[1])
        assert np.array_equal(mat[i, j], flat) and np.array_equal(mat[j, i], flat)
        assert np.all(np.isnan(mat[np.arange(d), np.arange(d)]))


# ---- the interaction surface ---------------------------------------------------------------------------------
def surface_reference(c, res1, res2, mom, di, dj, zi, zj):
    """the interaction surface (both main effects and mu taken off) in long double from G, g and mu as the device
    returned them, and its tolerance C . bound + gamma . sum |summands| per part: the conditional mean
    gamma_{L_i L_j + L_i + 2}, a main effect gamma_{L + 2}, four more roundings for the differences"""
    mdl, levels = c["mdl"], c["levels"]
    lo, hi = min(di, dj), max(di, dj)
    pairs = [tuple(r) for r in res2.pairs]
    o = pairs.index((lo, hi))
    sizes = [levels[a] * levels[b] for a, b in pairs]
    goff = int(np.sum(sizes[:o]))
    G = res2.G.cpu().numpy()[:, goff:goff + sizes[o]].reshape(-1, levels[lo], levels[hi])    # q x L_lo x L_hi
    if di > dj:
        G = G.transpose(0, 2, 1)
    gall = res1.g.cpu().numpy()
    parts = []
    for dim, z in ((di, zi), (dj, zj)):
        x = np.tile(c["nodes"][:1], (len(z), 1))
        x[:, dim] = z
        ref = reference_of(mdl["om_o"], x)
        Cc = E.constant_from_oracle_ratio(S.oracle_getbase_ratio(ref, mdl["om_o"], x, levels))
        L, off = levels[dim], int(levels[:dim].sum())
        R, bR = (a[:, :L] for a in ref.getbase(dim))
        parts.append((R, np.abs(E._f64(R)), E._f64(bR), gall[:, off:off + L].T, Cc))
    (Ri, aRi, bRi, gi, Ci), (Rj, aRj, bRj, gj, Cj) = parts
    Cc = max(Ci, Cj)
    mu = np.asarray(res1.mean, dtype=ld)
    Gl, aG = np.asarray(G, dtype=ld), np.abs(G)
    cond = np.einsum("at,qts,bs->abq", Ri, Gl, Rj)
    mi, mj = Ri @ np.asarray(gi, dtype=ld), Rj @ np.asarray(gj, dtype=ld)
    want = cond - mi[:, None, :] - mj[None, :, :] + mu[None, None, :]
    a_cond = np.einsum("at,qts,bs->abq", aRi, aG, aRj)
    a_mi, a_mj = aRi @ np.abs(gi), aRj @ np.abs(gj)
    Li, Lj = levels[di], levels[dj]
    tol = (Cc * (np.einsum("at,qts,bs->abq", bRi, aG, aRj) + np.einsum("at,qts,bs->abq", aRi, aG, bRj))
           + E.gamma(Li * Lj + Li + 2) * a_cond
           + (Cc * (bRi @ np.abs(gi)) + E.gamma(Li + 2) * a_mi)[:, None, :]
           + (Cc * (bRj @ np.abs(gj)) + E.gamma(Lj + 2) * a_mj)[None, :, :]
           + E.gamma(4) * (a_cond + a_mi[:, None, :] + a_mj[None, :, :] + 2 * np.abs(res1.mean)[None, None, :]))
    return want, tol, dict(G=G, gi=gi, gj=gj, aRj=aRj, Rj=Rj)


@pytest.mark.parametrize("name,di,dj", [("mixed_d3", 0, 2), ("mat25_d8", 5, 2), ("mixed_d3", 1, 2)])
def test_interaction_surface(name, di, dj):
    """13 x 17 grid points (221 threads: one block partly filled; dim_i > dim_j reads G transposed)"""
    import outerbase_amd as ob
    c = e2e_case2(name)
    mdl = c["mdl"]
    mom = ob.input_moments(mdl["om_d"], mdl["terms"], c["nodes"], c["w"])
    res1 = ob.sobol(mdl["om_d"], mdl["terms"], c["Theta"], mom)
    res2 = ob.sobol2(mdl["om_d"], mdl["terms"], c["Theta"], mom)
    pts = sample_x(np.random.default_rng(13 * 17), 17, mdl["kinds"])
    zi, zj = np.sort(pts[:13, di]), np.sort(pts[:, dj])
    surf = ob.interaction_effects(mdl["om_d"], mdl["terms"], c["Theta"], mom, di, dj, zi, zj)
    assert surf.shape == (13, 17, c["Theta"].shape[1])
    want, tol, _ = surface_reference(c, res1, res2, mom, di, dj, zi, zj)
    r = E.worst_ratio(surf, want, tol)
    print("%s interaction surface of dimensions %d, %d: err/tolerance %.3g" % (name, di, dj, r))
    assert r < 1
    assert np.array_equal(surf, ob.interaction_effects(mdl["om_d"], mdl["terms"], c["Theta"], mom, di, dj, zi, zj))
    back = ob.interaction_effects(mdl["om_d"], mdl["terms"], c["Theta"], mom, dj, di, zj, zi)
    assert E.worst_ratio(back.transpose(1, 0, 2), want, tol) < 1


def test_interaction_surface_has_zero_mean_over_either_axis():
    """on the measure's own nodes the weighted mean of the surface over x_i (or x_j) vanishes.  With the exact
    means m* of the nodes, G, g, mu as the device returned them and m the device's table, the mean over x_i at
    z'_b is  sum_{t,s} G[t,s] (m* - m)[t] psi_{j,s}(z'_b) - sum_t g_i[t] (m* - m)[t]  +  (G^T m - g_j) psi_j  +
    (mu - g_i^T m), so the tolerance is: tol_m of stage 1 times |G psi_j| + |g_i|; the stage-2 tolerances of g_j, G
    and mu on the device's own tables (and gamma_{L_i + 1} for G^T m, gamma_{L_i + 1} for g_i^T m); the weighted
    mean of the surface's own tolerance and gamma_{n+2} sum w |surface| for the mean itself."""
    import outerbase_amd as ob
    c = e2e_case2("mixed_d3")
    mdl, levels, nodes, w = c["mdl"], c["levels"], c["nodes"][:17], c["w"][:17]
    terms, Theta = mdl["terms"], c["Theta"]
    mom = ob.input_moments(mdl["om_d"], terms, nodes, w)
    res1 = ob.sobol(mdl["om_d"], terms, Theta, mom)
    res2 = ob.sobol2(mdl["om_d"], terms, Theta, mom)
    ref = reference_of(mdl["om_o"], nodes)
    Cc = E.constant_from_oracle_ratio(S.oracle_getbase_ratio(ref, mdl["om_o"], nodes, levels))
    _, (tol_m, _) = S.ref_tables(ref, levels, w, Cc)
    f = S.formulas(terms, Theta, mom.mean, mom.cov)
    f2 = S2.formulas2(terms, Theta, mom.mean, mom.cov)
    wn = E._f64(S.normalised_weights(w, 17, len(levels)))
    worst = 0.0
    for di, dj in ((0, 1), (0, 2), (1, 2), (2, 0)):
        zi, zj = nodes[:, di], nodes[:, dj]
        surf = ob.interaction_effects(mdl["om_d"], terms, Theta, mom, di, dj, zi, zj)      # 17 x 17 x q
        _, tol, x = surface_reference(dict(c, nodes=nodes), res1, res2, mom, di, dj, zi, zj)
        o = [tuple(r) for r in f2["pairs"]].index((min(di, dj), max(di, dj)))
        tG = f2["tol_G"][o] if di < dj else f2["tol_G"][o].transpose(1, 0, 2)               # L_i x L_j x q
        aG, mi = np.abs(x["G"]), np.abs(mom.mean[di])                                      # q x L_i x L_j
        Li = levels[di]
        Gpsi = np.abs(np.einsum("qts,bs->tbq", x["G"], E._f64(x["Rj"])))                    # L_i x 17 x q
        t_tab = np.einsum("t,tbq->bq", tol_m[di], Gpsi) + (tol_m[di] @ np.abs(x["gi"]))[None, :]
        t_gj = (f["tol_g"][dj] + np.einsum("tsq,t->sq", tG, mi) + E.gamma(Li + 1) * np.einsum("qts,t->sq", aG, mi))
        t_mu = f["tol_mu"] + f["tol_g"][di].T @ mi + E.gamma(Li + 1) * (np.abs(x["gi"]).T @ mi)
        t_all = (t_tab + x["aRj"] @ t_gj + t_mu[None, :] + np.einsum("a,abq->bq", wn[:, di], tol)
                 + E.gamma(17 + 2) * np.einsum("a,abq->bq", wn[:, di], np.abs(surf)))
        mean = np.einsum("a,abq->bq", wn[:, di], surf)
        r = float(np.max(np.abs(mean) / t_all))
        worst = max(worst, r)
        assert np.max(np.abs(surf)) > 1e3 * np.max(np.abs(mean))                            # a surface, not zeros
    print("weighted mean of the interaction surface over x_i: |mean| / tolerance %.3g" % worst)
    assert worst < 1


# ---- the Python layer ------------------------------------------------------------------------------------------
def test_multifit_sobol2_is_the_module_function_in_raw_units():
    import outerbase_amd as ob
    c = e2e_case2("mixed_d3")
    mdl, q = c["mdl"], c["Theta"].shape[1]
    rng = np.random.default_rng(5)
    meansd = np.stack([rng.standard_normal(q), rng.uniform(0.5, 3.0, q), np.ones(q)], axis=1)
    t = ob.obmod._Terms(mdl["om_d"], mdl["terms"])
    mf = ob.MultiFit(mdl["om_d"], t, c["Theta"], meansd, np.ones(len(mdl["terms"])), 0.0, 6.0)
    res = mf.sobol2(c["nodes"], c["w"])
    mom = ob.input_moments(mdl["om_d"], t, c["nodes"], c["w"])
    base = ob.sobol2(mdl["om_d"], t, c["Theta"], mom)
    s2 = (meansd[:, 1] * meansd[:, 1])[None, :]
    assert np.array_equal(res.pairs, base.pairs)
    assert np.array_equal(res.second_var, base.second_var * s2)
    assert np.array_equal(res.total_interaction_var, base.total_interaction_var * s2)
    assert np.array_equal(res.closed_var, base.closed_var * s2)
    assert np.array_equal(res.var, base.var * s2[0])
    assert np.array_equal(res.second, base.second) and np.array_equal(res.total_interaction, base.total_interaction)
    assert np.array_equal(res.second_var_mat[0, 2], base.second_var_mat[0, 2] * s2[0])
    gi, gj = np.linspace(0.1, 0.9, 7), np.linspace(0.2, 0.8, 4)
    assert np.array_equal(mf.interaction_effects(0, 2, gi, gj, c["nodes"], c["w"]),
                          ob.interaction_effects(mdl["om_d"], t, c["Theta"], mom, 0, 2, gi, gj) * meansd[:, 1][None, None, :])


def test_zero_coefficients_give_zero_variances_and_nan_shares():
    import outerbase_amd as ob
    c = e2e_case2("mixed_d3")
    mdl = c["mdl"]
    mom = ob.input_moments(mdl["om_d"], mdl["terms"], c["nodes"])
    res = ob.sobol2(mdl["om_d"], mdl["terms"], np.zeros((len(mdl["terms"]), 3)), mom)
    assert res.second_var.shape == (3, 3) and np.all(res.second_var == 0) and np.all(res.total_interaction_var == 0)
    assert np.all(res.closed_var == 0)
    assert np.all(np.isnan(res.second)) and np.all(np.isnan(res.total_interaction))
    assert np.all(res.G.cpu().numpy() == 0)
