"""Shapley effects on the GPU (obhip_shapley_dev and what is built on it) against the long-double reference of
tests/shapley_ref.py.

Stage 2 (sums on random float64 tables): every effect within its own gamma . sum |summands| of route (a), the
column sums beside obhip_sobol_dev's V.  End to end: device tables, then device sums, against long-double sums of
long-double tables; allowance eight times the float64 restatement's own error on the same case.  Every test prints
err / tolerance.

TW = 128 is the pair kernel's term-tile width; it keeps 8, 24 or 40 player slots in registers (d = 8 | 9, 24 | 25)
with 2, 2 or 1 responses per chunk, reads d - 40 dimensions per pair from memory beyond d = 40, and takes 40
players at most."""
import ctypes as C
import functools

import numpy as np
import pytest

import extended_ref as E
import shapley_ref as SH
import sobol_ref as S
from conftest import knots_for, sample_x
from test_shapley_host import ALL_STAGE2, double_rule, stage2_case
from test_sobol_host import golden_model, reference_of, some_zero_weights, theta_of

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 7
HOST_ENTRY = {(129, 9, 5, "default"), (300, 10, 1, "even odd")}      # the cases that also run obhip_shapley
RATIOS = []


def _dev():
    import torch
    from outerbase_amd._lib import call
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return torch, call, dev


def ids_of(groups, d):
    if groups is None:
        return None
    ids = np.empty(d, dtype=np.int32)
    for g, dims in enumerate(groups):
        ids[dims] = g
    return ids


@functools.lru_cache(maxsize=None)
def terms_of(p, d, q):
    import outerbase_amd as ob
    c = stage2_case(p, d, q, "default")
    kinds = ["mat25"] * d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    return ob.obmod._Terms(om, c["terms"])


def run_shapley(t, groups, Theta, pm, pc, P):
    """obhip_shapley_dev on NaN-filled buffers with PAD doubles behind the output -> (out q x P, padding untouched)"""
    from outerbase_amd._lib import lib
    torch, call, dev = _dev()
    q, d = Theta.shape[1], t.d
    ids = ids_of(groups, d)
    wsb = C.c_uint64(0)
    call("obhip_shapley_workspace_bytes", t.p, d, q, C.byref(wsb))
    ws = torch.full((max(1, wsb.value // 8),), NAN, dtype=torch.float64, device=dev)
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    dm, dc = torch.from_numpy(pm).to(dev), torch.from_numpy(pc).to(dev)
    out = torch.full((q * P + PAD,), NAN, dtype=torch.float64, device=dev)
    rc = lib.obhip_shapley_dev(t._h, None if ids is None else ids.ctypes.data, dth.data_ptr(), q, dm.data_ptr(),
                               dc.data_ptr(), out.data_ptr(), ws.data_ptr(), wsb.value)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    return rc, out[:q * P].reshape(q, P), bool(np.all(np.isnan(out[q * P:])))


def sobol_V(t, Theta, pm, pc):
    from test_gpu_sobol import run_sobol
    out, _ = run_sobol(t, Theta, pm, pc)
    return out[:, 1]


# ---- stage 2: the sums on random tables -----------------------------------------------------------------
@pytest.mark.parametrize("p,d,q,name", ALL_STAGE2)
def test_effects_on_random_tables(p, d, q, name):
    from outerbase_amd._lib import call
    c = stage2_case(p, d, q, name)
    sh, f, t = c["sh"], c["f"], terms_of(p, d, q)
    P = len(sh["players"])
    pm, pc = S.pack_tables(c["m"], c["Cv"])
    rc, out, clean = run_shapley(t, c["groups"], c["Theta"], pm, pc, P)
    rc2, out2, clean2 = run_shapley(t, c["groups"], c["Theta"], pm, pc, P)
    assert rc == 0 and rc2 == 0 and clean and clean2                               # the padding is untouched
    assert np.array_equal(out, out2)                                               # the same bits on every call
    assert np.all(np.isfinite(out))
    if name in ("default", "identity"):                                            # None and the identity partition
        other = None if name == "identity" else [[l] for l in range(d)]
        rc3, out3, _ = run_shapley(t, other, c["Theta"], pm, pc, P)
        assert rc3 == 0 and np.array_equal(out, out3)
    if (p, d, q, name) in HOST_ENTRY:
        ids = ids_of(c["groups"], d)
        host = np.full((q, P), NAN)
        th = np.ascontiguousarray(c["Theta"].T)
        call("obhip_shapley", t._h, None if ids is None else ids.ctypes.data, th.ctypes.data, q, pm.ctypes.data,
             pc.ctypes.data, host.ctypes.data)
        assert np.array_equal(host, out)
    r = E.worst_ratio(out.T, sh["Sh"], sh["tol_Sh"])
    V = sobol_V(t, c["Theta"], pm, pc)
    rV = float(np.max(np.abs(out.sum(axis=1) - V) / (sh["tol_Sh"].sum(axis=0) + f["tol_V"])))
    RATIOS.append((r, rV, "p=%d d=%d q=%d %s (P=%d, G=%d)" % (p, d, q, name, P, sh["G"])))
    print("p=%d d=%d q=%d %s: P=%d G=%d, err/tolerance %.3g, |column sum - V of sobol_dev| / tolerances %.3g" % (
        p, d, q, name, P, sh["G"], r, rV))
    assert r < 1 and rV < 1


@pytest.fixture(scope="module", autouse=True)
def report_worst_first():
    """after the module: the ratios of the stage-2 cases, worst first"""
    yield
    for r, rV, label in sorted(RATIOS, reverse=True):
        print("err/tolerance %.3g, sum against V %.3g: %s" % (r, rV, label))


def test_more_than_forty_players_are_refused_with_the_output_untouched():
    from outerbase_amd._lib import lib
    c = stage2_case(128, 44, 2, "forty players")
    t = terms_of(128, 44, 2)
    pm, pc = S.pack_tables(c["m"], c["Cv"])
    rc, out, clean = run_shapley(t, None, c["Theta"], pm, pc, 44)                  # 44 dimensions, 44 players
    assert rc == 1 and b"players" in lib.obhip_last_error()
    assert np.all(np.isnan(out)) and clean


# ---- end to end ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e_case(name):
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
    groups = [None, [[0, d - 1]] + [[l] for l in range(1, d - 1)]]
    G = [(len(SH.players_of(d, g)) + 1) // 2 for g in groups]
    return dict(mdl=mdl, nodes=nodes, w=w, Theta=Theta, groups=groups,
                sh=[SH.shapley(terms, Theta, m, Cv, g) for g in groups],
                sh64=[SH.shapley(terms, Theta, m64, C64, g, dtype=np.float64, rule=double_rule(k))
                      for g, k in zip(groups, G)])


@pytest.mark.parametrize("name", ["mixed_d3", "mat25_d8"])
def test_shapley_end_to_end(name):
    """per entry the scale is the stage-2 tolerance (gamma . sum |summands|); the float64 restatement's worst
    err / scale is measured here, and the device is allowed eight times that"""
    import outerbase_amd as ob
    c = e2e_case(name)
    mdl = c["mdl"]
    mom = ob.input_moments(mdl["om_d"], mdl["terms"], c["nodes"], c["w"])
    first = ob.sobol(mdl["om_d"], mdl["terms"], c["Theta"], mom)
    for groups, sh, sh64 in zip(c["groups"], c["sh"], c["sh64"]):
        res = ob.shapley(mdl["om_d"], mdl["terms"], c["Theta"], mom, groups=groups)
        r64 = E.worst_ratio(sh64["Sh"], sh["Sh"], sh["tol_Sh"])
        rdev = E.worst_ratio(res.effect_var, sh["Sh"], sh["tol_Sh"])
        print("%s end to end, %d players: float64 restatement %.3g, device %.3g of the scale; device / restatement "
              "%.3g" % (name, len(sh["players"]), r64, rdev, rdev / r64))
        assert rdev <= 8 * r64
        assert res.players == sh["players"] and res.effect_var.shape == (len(sh["players"]), c["Theta"].shape[1])
        assert np.array_equal(res.var, res.effect_var.sum(axis=0))
        assert np.all(np.abs(res.var / first.var - 1) < 1e-9)
        assert np.all(np.abs(res.effect.sum(axis=0) - 1) < 1e-12)
        assert np.all(np.abs(res.effect - E._f64(sh["Sh"] / sh["Sh"].sum(axis=0)[None, :])) < 1e-9)
        if groups is None:
            assert np.all(first.first_var <= res.effect_var * (1 + 1e-9))
            assert np.all(res.effect_var <= first.total_var * (1 + 1e-9))


# ---- the Python layer ------------------------------------------------------------------------------------------
def test_multifit_shapley_is_the_module_function_in_raw_units():
    """a small fit: n = 200, d = 3, q = 2"""
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    rng = np.random.default_rng(5)
    x = sample_x(rng, 200, mdl["kinds"])
    y = np.stack([np.sin(3 * x[:, 0]) + x[:, 1] * x[:, 2], 40.0 + 7.0 * np.cos(2 * x[:, 1]) * x[:, 0]], axis=1)
    y = y + 0.01 * rng.standard_normal(y.shape)
    mf = ob.fit_newton_multi(mdl["om_d"], mdl["terms"], x, y)
    for groups in (None, [[0, 2], [1]]):
        res = mf.shapley(x, groups=groups)
        mom = ob.input_moments(mdl["om_d"], mf._t, x)
        base = ob.shapley(mdl["om_d"], mf._t, mf.coeff, mom, groups=groups)
        s2 = (mf.y_sca * mf.y_sca)[None, :]
        assert res.effect_var.shape == ((3 if groups is None else 2), 2)
        assert np.array_equal(res.effect_var, base.effect_var * s2) and np.array_equal(res.var, base.var * s2[0])
        assert np.array_equal(res.effect, base.effect) and res.players == base.players
        sob = mf.sobol(x)
        assert np.all(np.abs(res.var / sob.var - 1) < 1e-9)


def test_zero_coefficients_give_zero_effects_and_nan_shares():
    import outerbase_amd as ob
    c = e2e_case("mixed_d3")
    mdl = c["mdl"]
    mom = ob.input_moments(mdl["om_d"], mdl["terms"], c["nodes"])
    res = ob.shapley(mdl["om_d"], mdl["terms"], np.zeros((len(mdl["terms"]), 3)), mom)
    assert res.effect_var.shape == (3, 3) and np.all(res.effect_var == 0) and np.all(res.var == 0)
    assert np.all(np.isnan(res.effect))
