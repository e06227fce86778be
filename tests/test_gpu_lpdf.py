"""The model layer (csrc/lpdf.cpp over vec_ops.h, kernels_misc.hip and the grad_*_dev entries) held to its long
double restatement tests/lpdf_ref.py: every quantity of loglik_gauss / loglik_std / loglik_gda / logpr_gauss and
of the pair with its marginal adjustment, at the shapes where the n-vector sums change path, on both sides of
the switches the layer takes, through call orders that cross its caches, and sharded over simulated ranks.

Everywhere: worst_ratio(device, want, C b + s) <= 1 over every entry, C measured per case from the float64
oracle (eight times the largest of its err / bound on the entries of B and dB and of the C it needs on any
quantity, at most 2e-13; lpdf_worker.constant / walk_constant), device and oracle ratios printed side by side.

The host references are memoised per case (lpdf_worker, functools.lru_cache).  After every optcg the coefficients
are held to the stopping criterion and, for the one-noise-level likelihoods, to the long double solve of the normal
equations (lpdf_worker.hold_optcg); after optnewton to that solve by the Newton residual bound (check_newton)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lpdf_ref as LR
import lpdf_worker as W
import posterior_ref as PR

pytestmark = pytest.mark.gpu

# p through spread_terms: the constant term alone, 3, 40, 130; n around the 256-row block of every n-vector
# kernel; more terms than rows included
SHAPES = W.SHAPES


# ---- A. every quantity, every likelihood ---------------------------------------------------------------------------
@pytest.mark.parametrize("hypname", ["short", "default"])
@pytest.mark.parametrize("p,n", SHAPES)
def test_every_quantity_of_every_object(hypname, p, n):
    W.check_all_objects(W.small(hypname, p, n), ("pr", "lik") if (p + n) % 2 else ("lik", "pr"))


@pytest.mark.parametrize("n,ymean", [(1, 0.0), (2, 0.0), (257, 0.0), (257, 1e6), (513, 1e6)])
def test_para0(n, ymean):
    """para0 = log(0.01 var(y)) (half of it for loglik_gda), y far from zero included; a single row has no
    variance: NaN, and the object works once updatepara has given it a noise level"""
    q = W.small("short", 3, n, ymean)
    om_d, lik = W.make(q, "loglik_gauss")
    _, lg = W.make(q, "loglik_gda", om_d)
    if n == 1:
        assert np.isnan(lik.para0[0]) and np.isnan(lg.para0[0])
        lik.updatepara([q.sigma])
        Cc, _ = W.constant(q)
        W.hold(q.name + " after updatepara", W.read(lik, q.g, q.coeff), W.ref_lik(q), Cc, W.oracle_lik(q))
        return
    want, wg = LR.para0_gauss(q.case.y), LR.para0_gda(q.case.y)
    W.hold(q.name + " para0", {"para0": lik.para0}, {"para0": want[None]}, 0.0)
    W.hold(q.name + " para0 gda", {"para0": lg.para0}, {"para0": LR.cat(wg[None], LR.exact(np.zeros(1)))}, 0.0)
    assert np.array_equal(lik.para, lik.para0)


def test_response_far_from_zero():
    """y = 1e6 + N(0, 1): val, gradients and para0 where yhat - y is a million times the noise"""
    q = W.small("short", 40, 257, 1e6)
    W.check_all_objects(q)


@pytest.fixture(scope="module")
def edge_16641():
    """65 . 256 + 1 rows: the first n at which a lane of k_vsum2 adds two partials"""
    return W.edge(65 * 256 + 1)


@pytest.fixture(scope="module")
def edge_262401():
    """1025 . 256 + 1 rows: k_vsum1, k_vcolsum1, k_wdot1 and k_sum2_stage1 all take a second grid-stride trip
    with a ragged last block (the one slow reference of the module: nine chunks in long double)"""
    return W.edge(1025 * 256 + 1)


def check_edge(q):
    assert q.case.p == 12 and q.case.nhyp == 3
    W.check_all_objects(q)
    om_d, lik = W.make(q, "loglik_gauss")
    W.hold(q.name + " para0", {"para0": lik.para0}, {"para0": LR.para0_gauss(q.case.y)[None]}, 0.0)


def test_row_edge_where_a_lane_adds_two_partials(edge_16641):
    check_edge(edge_16641)


def test_row_edge_where_every_sum_takes_a_second_trip(edge_262401):
    check_edge(edge_262401)


# ---- B. both sides of the path switches ----------------------------------------------------------------------------
@pytest.mark.parametrize("d3", ["0", None])
def test_gradient_plan_switch_read_per_call(monkeypatch, d3):
    """OBHIP_GRAD_D3 = 0 / unset: grad_mm_dot_dev + grad_tmm_host, or the Fused plan that fills dhg_cache"""
    if d3 is None:
        monkeypatch.delenv("OBHIP_GRAD_D3", raising=False)
    else:
        monkeypatch.setenv("OBHIP_GRAD_D3", d3)
    W.check_all_objects(W.small("short", 40, 257))
    W.check_all_objects(W.small("default", 130, 257))


def test_process_wide_switches_in_child_processes():
    """OBHIP_UPDATE_FUSED=0 (a static of LoglikGauss::update), OBHIP_FORCE_GENERIC=1, OBHIP_HM3=0: one child process
    per setting, one at a time, each under its own time limit; the first non-zero status or time limit ends the
    loop, so that nothing more starts on the device after a child that went wrong"""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lpdf_worker.py")
    for switch in ("OBHIP_UPDATE_FUSED=0", "OBHIP_FORCE_GENERIC=1", "OBHIP_HM3=0"):
        k, v = switch.split("=")
        env = dict(os.environ)
        env[k] = v
        r = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=300)
        print(switch)
        print(r.stdout[-6000:])
        assert r.returncode == 0, (switch, r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
        assert "lpdf worker ok" in r.stdout, switch


@pytest.mark.parametrize("d,maxlev,want_mu", [(26, 5, 131), (16, 6, 97)])
def test_term_sets_outside_and_inside_the_fused_products_lds_domain(d, maxlev, want_mu):
    """131 used columns: hessmult takes the fused product, update() falls back to the separate passes; 97: both fused"""
    import outerbase_amd as ob
    q = W.lds(d, maxlev)
    lik = W.check_without_gradients(q)
    assert 1 + int(ob.obmod._Terms(lik.om, q.case.terms).maxlevels().sum()) == want_mu


def test_views_too_wide_for_the_fused_gradient_kernel():
    W.check_all_objects(W.wide())


# ---- C. call order: named sequences ----------------------------------------------------------------------------------
def test_optcg_then_diaghess_comes_from_the_preconditioners_sums():
    W.check_optcg_then_diaghess(W.small("short", 40, 257))


def test_updateom_after_optcg_does_not_serve_the_old_sums():
    """optcg caches the preconditioner's sqcolsums in the likelihood; new hyper-parameters + updateom must drop them"""
    q = W.small("short", 40, 257)
    lp, lik, om_d = W.check_optcg_then_diaghess(q)
    hyp2 = np.asarray(q.case.om.hyp) + np.array([0.05, -0.04, 0.03, 0.02, -0.05, 0.04])
    om2 = W.oracle_model(PR.KINDS, PR.NKNOTS, hyp2)
    om_d.updatehyp(hyp2)
    W.share_rotation(om2, om_d)
    lp.updateom()
    q2 = W.at(q, om=om2, coeff=lp.coeff)
    Cc, _ = W.constant(q2)
    W.hold("updateom after optcg: lik", {"diaghess": lik.diaghess(), "diaghessgradpara": lik.diaghessgradpara()},
           W.ref_lik(q2), Cc, W.oracle_lik(q2))
    W.hold("updateom after optcg: pair", W.read(lp, q.g, q2.coeff), W.ref_pair(q2), Cc, W.oracle_pair(q2))


def test_updateterms_to_the_same_number_of_terms():
    """other levels, the same p: every cache keyed by size alone would survive"""
    import outerbase_amd as ob
    q = W.small("short", 40, 257)
    om_d, lik = W.make(q, "loglik_gauss")
    lp = ob.lpdfvec(W.make(q, "logpr_gauss", om_d)[1], lik)
    lp.updatepara([q.rho, q.sigma])
    Cc, _ = W.constant(q)
    W.hold("before updateterms", W.read(lp, q.g, q.coeff), W.ref_pair(q), Cc, W.oracle_pair(q))
    terms2 = PR.spread_terms(q.case.om, 80, 5)[40:]
    assert not np.array_equal(np.sort(terms2, axis=0), np.sort(q.case.terms, axis=0))
    lp.updateterms(terms2)
    q2 = W.at(q, terms=terms2)
    C2, _ = W.constant(q2)
    W.hold("after updateterms: pair", W.read(lp, q.g, q.coeff), W.ref_pair(q2), C2, W.oracle_pair(q2))
    W.hold("after updateterms: lik", W.read(lik, q.g), W.ref_lik(q2), C2, W.oracle_lik(q2))


def test_gda_diaghessgradhyp_between_an_update_and_a_hessmult():
    """diaghessgradhyp borrows the residual vector as scratch: what is read after it is still the current state"""
    q = W.small("short", 40, 257)
    Cc, _ = W.constant(q)
    _, lg = W.make(q, "loglik_gda")
    lg.updatepara([q.sigma, q.lam])
    lg.compute_gradhyp = lg.compute_gradpara = True
    lg.update(q.coeff)
    got = {"diaghessgradhyp": lg.diaghessgradhyp(), "hessmult": lg.hessmult(q.g), "val": lg.val, "grad": lg.grad,
           "gradhyp": lg.gradhyp, "gradpara": lg.gradpara}
    W.hold("gda update -> diaghessgradhyp -> hessmult", got, W.ref_gda(q), Cc, W.oracle_gda(q))
    W.hold("gda ... -> update again", W.read(lg, q.g, q.coeff), W.ref_gda(q), Cc, W.oracle_gda(q))


def test_update_gradhyp_twice_with_the_gradient_plan_flipped_between(monkeypatch):
    import outerbase_amd as ob
    q = W.small("short", 40, 257)
    Cc, _ = W.constant(q)
    om_d, lik = W.make(q, "loglik_gauss")
    lp = ob.lpdfvec(W.make(q, "logpr_gauss", om_d)[1], lik)
    lp.updatepara([q.rho, q.sigma])
    monkeypatch.delenv("OBHIP_GRAD_D3", raising=False)
    W.hold("plan unset", W.read(lp, q.g, q.coeff), W.ref_pair(q), Cc, W.oracle_pair(q))
    monkeypatch.setenv("OBHIP_GRAD_D3", "0")
    W.hold("plan 0", W.read(lp, q.g, q.coeff), W.ref_pair(q), Cc, W.oracle_pair(q))
    lp.updatepara([q.rho, q.sigma])          # redohess with the other plan
    W.hold("plan 0, rebuilt", W.read(lp, q.g, q.coeff), W.ref_pair(q), Cc, W.oracle_pair(q))
    monkeypatch.delenv("OBHIP_GRAD_D3")
    lp.updatepara([q.rho, q.sigma])
    W.hold("plan unset, rebuilt", W.read(lp, q.g, q.coeff), W.ref_pair(q), Cc, W.oracle_pair(q))


# ---- D. the row-sharded likelihood over simulated ranks ---------------------------------------------------------------
@pytest.mark.parametrize("ranks", [1, 3])
def test_sharded_likelihood_equals_the_row_weighted_reference(ranks):
    """N simulated ranks all hold these rows: every sum over rows times N, n_total = N n, para0 of all rows"""
    import outerbase_amd as ob
    q = W.small("short", 40, 257)
    Cc, _ = W.constant(q, ranks)
    comm = W.sim_comm(ranks)
    try:
        om_d = W.device_model(q.case.om)
        for kind in ("loglik_gauss", "loglik_std"):
            _, lik = W.make(q, kind, om_d)
            lik.set_comm(comm)
            W.hold("sim(%d) %s para0" % (ranks, kind), {"para0": lik.para0},
                   {"para0": LR.para0_gauss(q.case.y, ranks)[None]}, 0.0)
            assert np.array_equal(lik.para, lik.para0)
            lik.updatepara([q.sigma])
            got, want = W.read(lik, q.g, q.coeff), W.ref_lik(q, ranks)
            if kind == "loglik_std":
                got["hess"], want = lik.hess(), W.ref_lik(q, ranks, True)
            W.hold("sim(%d) %s" % (ranks, kind), got, want, Cc, W.oracle_lik(q, ranks))
        for order in (("pr", "lik"), ("lik", "pr")):
            parts = {"pr": W.make(q, "logpr_gauss", om_d)[1], "lik": W.make(q, "loglik_gauss", om_d)[1]}
            lp = ob.lpdfvec(parts[order[0]], parts[order[1]])
            lp.set_comm(comm)
            lp.updatepara([{"pr": q.rho, "lik": q.sigma}[k] for k in order])
            W.hold("sim(%d) lpdfvec(%s, %s)" % ((ranks,) + order), W.read(lp, q.g, q.coeff), W.ref_pair(q, order, ranks),
                   Cc, W.oracle_pair(q, order, ranks))
        # optcg under the communicator, then the likelihood's diaghess from the preconditioner's sums
        lp.optcg(1e-8, 200)
        s = LR.Session(q.case.om, q.case.x, q.case.y, q.case.terms, "gauss", order, ranks)
        s.updatepara([{"pr": q.rho, "lik": q.sigma}[k] for k in order])
        W.hold_optcg("sim(%d) optcg" % ranks, s, lp.coeff, 1e-8, lp.cgiters, 200, Cc)
        q2 = W.at(q, coeff=lp.coeff)
        lik = parts["lik"]
        W.hold("sim(%d) optcg -> lik.diaghess" % ranks,
               {"diaghess": lik.diaghess(), "diaghessgradpara": lik.diaghessgradpara()}, W.ref_lik(q2, ranks), Cc,
               W.oracle_lik(q2, ranks))
        got = dict(val=lp.val, grad=lp.grad, gradhyp=lp.gradhyp, gradpara=lp.gradpara, diaghess=lp.diaghess())
        W.hold("sim(%d) optcg -> pair" % ranks, got, W.ref_pair(q2, order, ranks), Cc, W.oracle_pair(q2, order, ranks))
    finally:
        free_later(comm)


_comms = []


def free_later(comm):
    """the objects of a test may outlive its body (garbage collection): communicators go at module teardown"""
    _comms.append(comm)


def teardown_module(module):
    import gc
    gc.collect()
    while _comms:
        W.free_comm(_comms.pop())


def test_loglik_gda_refuses_a_communicator_and_stays_usable():
    from outerbase_amd._lib import ObhipError
    q = W.small("short", 40, 257)
    Cc, _ = W.constant(q)
    _, lg = W.make(q, "loglik_gda")
    comm = W.sim_comm(3)
    try:
        with pytest.raises(ObhipError) as e:
            lg.set_comm(comm)
        assert e.value.code == 1                           # OBHIP_ERR_INVALID
        lg.updatepara([q.sigma, q.lam])
        W.hold("gda after the refused set_comm", W.read(lg, q.g, q.coeff), W.ref_gda(q), Cc, W.oracle_gda(q))
    finally:
        free_later(comm)


def test_what_was_read_before_set_comm_is_not_served_after_it():
    """diaghess() and update(gradhyp) taken on one rank's rows, then the communicator: the same reads must be the
    all-ranks values (the cached sqcolsums and the cached diaghessgradhyp sums belong to the old sharding)"""
    import outerbase_amd as ob
    q = W.small("short", 40, 257)
    ranks = 3
    C1, _ = W.constant(q)
    Cn, _ = W.constant(q, ranks)
    om_d, lik = W.make(q, "loglik_gauss")
    lp = ob.lpdfvec(W.make(q, "logpr_gauss", om_d)[1], lik)
    lp.updatepara([q.rho, q.sigma])
    W.hold("before set_comm: pair", W.read(lp, q.g, q.coeff), W.ref_pair(q), C1, W.oracle_pair(q))
    W.hold("before set_comm: lik", W.read(lik, q.g), W.ref_lik(q), C1, W.oracle_lik(q))
    comm = W.sim_comm(ranks)
    try:
        lp.set_comm(comm)
        W.hold("after set_comm: lik", W.read(lik, q.g), W.ref_lik(q, ranks), Cn, W.oracle_lik(q, ranks))
        W.hold("after set_comm: pair", W.read(lp, q.g, q.coeff), W.ref_pair(q, ("pr", "lik"), ranks), Cn,
               W.oracle_pair(q, ("pr", "lik"), ranks))
    finally:
        free_later(comm)


@pytest.mark.parametrize("ranks", [1, 3])
def test_sharded_pair_with_the_full_adjustment(ranks):
    """lpdfvec(loglik_std, logpr_gauss) under the communicator through optnewton: the Hessian, the coefficients and
    the full-Hessian adjustment of the rows weighted by N"""
    w = W.Walker("std", 0)
    comm = W.sim_comm(ranks)
    try:
        w.lp.set_comm(comm)
        w.s.N = ranks
        w.title = "sim(%d) std" % ranks
        para = [-0.8, 4.0]
        w.lp.updatepara(para)
        w.s.updatepara(para)
        w.apply(0, {"name": "optnewton", "draw": 3})
        w.apply(1, {"name": "update", "draw": 4, "flags": [True, True, True, True]})
    finally:
        free_later(comm)


# ---- C. call order: the random walk and the sequences that involve optnewton -------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "std", "gda"])
@pytest.mark.parametrize("seed", range(8))
def test_random_call_order(kind, seed):
    """lpdfvec(logpr_gauss, loglik_gauss), lpdfvec(loglik_std, logpr_gauss), lpdfvec(logpr_gauss, loglik_gda): 12
    seeded steps over updatepara / updatehyp + updateom / updateterms (same p, other p) / update under every flag
    combination / domarg / optnewton / optcg / hessmult / the diaghess family on the pair and on the likelihood
    alone (/ dodiag); after every step everything the Session says is defined is compared, and the walk stops at the
    first failing step"""
    W.run_walk(kind, seed)


@pytest.mark.parametrize("kind", ["gauss", "std", "gda"])
def test_the_same_walk_twice_gives_the_same_bits(kind):
    a, b = W.run_walk(kind, 1), W.run_walk(kind, 1)
    assert len(a) == len(b) and len(a) > 50
    for i, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v, equal_nan=True), i


def newton_walker():
    w = W.Walker("std", 2)
    para = [-0.6, 3.0]
    w.lp.updatepara(para)
    w.s.updatepara(para)
    w.apply(0, {"name": "optnewton", "draw": 11})
    assert w.s.fullhess and w.lp.fullhess
    return w


def test_optnewton_then_update_keeps_the_full_adjustment():
    w = newton_walker()
    w.apply(1, {"name": "update", "draw": 12, "flags": [True, True, True, True]})
    # the two adjustments differ by far more than any tolerance: the diagonal one must not have come back
    H = w.lp.hess()
    full = w.s.pair(w.s.coeff, H)
    w.s.fullhess = False
    diag = w.s.pair(w.s.coeff)
    w.s.fullhess = True
    assert abs(float(full["val"].v - diag["val"].v)) > 1e6 * float(LR.tol(full["val"], w.C))
    # and it survives a rebuild: updatepara, then update
    w.apply(2, {"name": "updatepara", "draw": 13})
    w.apply(3, {"name": "update", "draw": 14, "flags": [True, True, True, True]})


def test_optnewton_then_optcg_drops_the_full_adjustment():
    w = newton_walker()
    w.apply(1, {"name": "optcg", "draw": 15})
    assert not w.s.fullhess and not w.lp.fullhess
    w.apply(2, {"name": "update", "draw": 16, "flags": [True, True, True, True]})


# ---- E. predictors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "std", "std full", "gda", "gda nodiag"])
def test_predictors(kind):
    """pred_gauss, predr_std (diagonal, and full after optnewton) and pred_gda at 1, 63 and 257 new rows: mean and
    variance after an updatepara + update that changes them; a predictor snapshots the lpdf at creation, so the
    earlier one still answers with the earlier state"""
    import outerbase_amd as ob
    base = kind.split()[0]
    w = W.Walker(base, 3)
    s, lp = w.s, w.lp
    if kind == "gda nodiag":
        w.lik.dodiag = False
        s.set_doda(False)
    rng = np.random.default_rng(77)

    def state(i):
        para = W.draw_para(rng, base, s.order)
        lp.updatepara(para)
        s.updatepara(para)
        if kind == "std full":
            w.apply(i, {"name": "optnewton", "draw": 20 + i})
        else:
            w.apply(i, {"name": "update", "draw": 20 + i, "flags": [True, True, False, False]})
        H = lp.hess() if kind == "std full" else None
        D = s.pair(s.coeff, H)["diaghess"]
        pred = ob.predictor(lp)
        wants = {}
        for nnew in (1, 63, 257):
            xnew = PR.inside_rows(nnew, 300 + nnew)
            wants[nnew] = (xnew, LR.predict(s.case, xnew, s.coeff, s.para["lik"], base, D, H, s.doda))
        return pred, wants

    def check(what, pred, wants):
        for nnew, (xnew, want) in wants.items():
            pred.update(xnew)
            W.hold("%s %s nnew %d" % (kind, what, nnew), {"mean": pred.mean(), "var": pred.var()}, want, w.C)

    p1, w1 = state(0)
    check("first", p1, w1)
    p2, w2 = state(1)
    check("second", p2, w2)
    assert float(np.max(np.abs(w1[63][1]["var"].v - w2[63][1]["var"].v))) > 1e6 * float(np.max(LR.tol(w2[63][1]["var"], w.C)))
    check("first again", p1, w1)
