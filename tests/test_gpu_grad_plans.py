"""Every plan and kernel variant of the hyper-gradient products (csrc/kernels_grad.hip, grad_views.cpp,
kernels_grad_dense.hip, kernels_grad_d3.hip) held per entry to the extended-precision instrument.

Each shape of grad_plan_ref.CASES is named for what it makes the library run; the test reads the
library's own report of what it will launch (obhip_grad_plan_info: the plan, the k_tmm_d3 groups with W,
NU, blocks and row splits, the dense kernel and its passes) and asserts the variant from it before it
compares anything, so no shape relies on a guess about the device.  The eight products -- getmat_gradhyp,
matmul_gradhyp, matmul_gradhyp_dot, tmatmul_gradhyp, sqmm_gradhyp, sqtmm_gradhyp with a signed weight,
sqcolsums_gradhyp, residvar_gradhyp -- are each held to  C x propagated bound + gamma_k x sum |summands|
(extended_ref.py), the float64 oracle's figures printed beside the device's.  test_grad_plan_host.py shows
on the host that these very shapes see the defects such kernels can have."""
import ctypes as C

import numpy as np
import pytest

import extended_ref as E
import grad_plan_ref as G
from conftest import knots_for, make_pair
from test_gpu_extended import Report
from test_grad_plan_host import PRODUCTS, reference

pytestmark = pytest.mark.gpu


def device_model(r, m):
    """the device model on the data the reference was computed from (the oracle's rotation)"""
    _, om_d = make_pair(r["kinds"], knots_for(r["kinds"], m), share_rotation=True)
    rot, bv, _ = om_d.rotation()
    rotg, lbvg = om_d.rotation_grad()
    om = r["om"]
    assert np.array_equal(rot, om.rotmat) and np.array_equal(rotg, om.rotmat_gradhyp)
    assert np.array_equal(bv, om.basisvar) and np.array_equal(lbvg, om.logbasisvar_gradhyp)
    return om_d


def check_variant(name, r, info):
    """the report against what the case is named for, and against the grouping restated in grad_plan_ref"""
    c = G.CASES[name]
    e, n = c["expect"], c["n"]
    groups, dense = info["groups"], info["dense"]
    print("%s | plan %s, %d groups %s, dense %s" % (name, info["plan"], len(groups), [
        (g["nh"], g["W"], g["Mu"], g["p"], g["NU"], g["pblocks"], g["nsplit"], g["tps"]) for g in groups], dense))
    if "plan" in e:
        assert info["plan"] == e["plan"], (name, info["plan"])
    for key, field in (("nu", "NU"), ("pblocks", "pblocks"), ("p_pad", "p_pad"), ("W", "W"), ("nh", "nh")):
        if key in e:
            assert {g[field] for g in groups} == e[key], (name, key, groups)
    if "nhseq" in e:
        assert [g["nh"] for g in groups] == e["nhseq"], (name, groups)
    if "groups" in e:
        assert len(groups) >= e["groups"], (name, groups)
    if "ngroups" in e:
        assert len(groups) == e["ngroups"], (name, groups)
    if "d3split" in e:
        assert {(g["nsplit"], g["tps"]) for g in groups} == {e["d3split"]}, (name, groups)
    if "kernel" in e:
        assert dense is not None and dense["kernel"] == e["kernel"], (name, dense)
    for key in ("W2", "Mu"):
        if key in e:
            assert dense[key] == e[key], (name, key, dense)
    if "Mu_range" in e:
        assert e["Mu_range"][0] <= dense["Mu"] <= e["Mu_range"][1], (name, dense)
    if "passes" in e:
        assert dense["passes"] == e["passes"], (name, dense)
    if "densesplit" in e:
        assert (dense["nsplit"], dense["tps"]) == e["densesplit"], (name, dense)
    if "fallback" in e:
        assert info["view_groups"] > 0 and info["view_groups_per_hyp"] == e["fallback"], (name, info)
    assert info["nhyp"] == r["ref"].nhyp and info["ntiles"] == (n + 63) // 64
    # the grouping and the geometry restated on the host (what the staged defects were run on)
    mine = G.d3_groups(r["terms"], [E.NUMHYP[k] for k in r["kinds"]])
    if groups:
        assert mine is not None and len(mine) == len(groups), (name, mine)
        for g, q in zip(groups, mine):
            assert g["members"] == [h0 for _, h0 in q["members"]], (name, g, q)
            assert (g["nh"], g["W"], g["Mu"], g["p"]) == (q["nh"], q["W"], q["Mu"], q["p"]), (name, g, q)
            geo = G.d3_geometry(q, n, info["cus"])
            assert all(g[k] == geo[k] for k in ("p_pad", "pblocks", "nsplit", "tps")) and g["NU"] == geo["nu"], (g, geo)
    elif not e.get("env"):
        assert mine is None, name


def device_products(bd, terms, a, v):
    return {
        "getmat_gradhyp": bd.getmat_gradhyp(terms), "matmul_gradhyp": bd.matmul_gradhyp(terms, a),
        "matmul_gradhyp_dot": bd.matmul_gradhyp_dot(terms, a, v), "tmatmul_gradhyp": bd.tmatmul_gradhyp(terms, v),
        "sqmm_gradhyp": bd.sqmm_gradhyp(terms, a), "sqtmm_gradhyp": bd.sqtmm_gradhyp(terms, v),
        "sqcolsums_gradhyp": bd.sqcolsums_gradhyp(terms), "residvar_gradhyp": bd.residvar_gradhyp(terms),
    }


# the shapes whose likelihood also forms both contractions in one sweep: every W2 x NH x NU of k_tmm_d3, two blocks
# along the terms, two row splits, groups of both widths in one term set
SWEPT = [name for name in G.CASES if name.startswith("nu")] + ["group closes on nh"]


@pytest.mark.parametrize("name", list(G.CASES))
def test_every_plan_and_variant_against_the_instrument(name, monkeypatch):
    """the variant asserted from the library's report, then the eight products per entry (module docstring);
    where named in SWEPT, MODE 3 of the fused pass as well (one_sweep)"""
    import outerbase_amd as ob
    r = reference(name)
    c = G.CASES[name]
    for key, val in c["expect"].get("env", {}).items():
        monkeypatch.setenv(key, val)
    om_d = device_model(r, c["m"])
    bd = ob.outerbase(om_d, r["x"])
    terms = ob.obmod._Terms(om_d, r["terms"])
    info = bd.grad_plan_info(terms)
    check_variant(name, r, info)
    got = device_products(bd, terms, r["a"], r["v"])
    assert bd.grad_plan_info(terms) == info                # the report is of what ran: the products changed nothing in it
    rep = Report(name + " C = %.3g" % r["C"])
    for q in PRODUCTS:
        want = r["want"][q]
        assert np.shape(got[q]) == np.shape(want), q
        rep.check(q, got[q], want, r["tol"][q], r["oracle"][q])
    if name in SWEPT:
        one_sweep(name, r, om_d, rep)
    rep.done()


def _launches(scope):
    from outerbase_amd import _lib
    cnt, ms = C.c_uint64(0), C.c_double(0)
    _lib.call("obhip_profile_get", scope, C.byref(cnt), C.byref(ms))
    return cnt.value


def one_sweep(name, r, om_d, rep):
    """k_tmm_d3 MODE 3 (grad_dual_dev): lpdfvec(loglik_gauss, logpr_gauss) with the marginal adjustment asks
    for gradhyp and diaghessgradhyp in one update, and the likelihood forms both in one sweep.  The same
    likelihood on its own forms them singly (MODE 1, MODE 2) from the same residuals in the same order of
    summation: bit for bit.  diaghessgradhyp = e^{-2 sigma} sqcolsums_gradhyp also against the instrument."""
    import outerbase_amd as ob
    from outerbase_amd import _lib
    terms, x, n, p = r["terms"], r["x"], r["n"], r["p"]
    rng = np.random.default_rng(G.SEED[name] + 3)
    y, coeff = rng.standard_normal(n), 0.05 * rng.standard_normal(p)
    sigma, rho = -1.1, 4.0
    ngroups = len(ob.outerbase(om_d, x).grad_plan_info(terms)["groups"])
    assert ngroups >= 1

    lik = ob.loglik_gauss(om_d, terms, y, x)
    lp = ob.lpdfvec(lik, ob.logpr_gauss(om_d, terms))
    lp.updatepara([sigma, rho])
    lp.compute_gradhyp = lp.compute_gradpara = True
    _lib.call("obhip_profile_reset")
    _lib.call("obhip_profile_enable", 1)
    lp.update(coeff)
    swept = _launches(b"tmm_d3")
    dual = (np.array(lik.gradhyp), np.array(lik.diaghessgradhyp()))
    after = _launches(b"tmm_d3")
    _lib.call("obhip_profile_enable", 0)
    # one launch per group for both contractions, and the accessor answers from what the sweep left
    assert swept == ngroups and after == swept, (swept, after, ngroups)

    alone = ob.loglik_gauss(om_d, terms, y, x)
    alone.updatepara([sigma])
    alone.compute_gradhyp = True
    _lib.call("obhip_profile_reset")
    _lib.call("obhip_profile_enable", 1)
    alone.update(coeff)
    single = (np.array(alone.gradhyp), np.array(alone.diaghessgradhyp()))
    singly = _launches(b"tmm_d3")
    _lib.call("obhip_profile_enable", 0)
    assert singly == 2 * ngroups, (singly, ngroups)
    assert np.array_equal(dual[0], single[0]) and np.array_equal(dual[1], single[1])
    e2 = np.exp(np.longdouble(-2.0 * sigma))
    want = r["want"]["sqcolsums_gradhyp"]
    # (two more roundings: the exponential and the product with it)
    rep.check("one sweep diaghessgradhyp", dual[1], want * e2,
              float(e2) * (r["tol"]["sqcolsums_gradhyp"] + 4 * E.U * np.abs(np.asarray(want, dtype=np.float64))),
              r["oracle"]["sqcolsums_gradhyp"] * float(e2))
