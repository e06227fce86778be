"""The instrument of test_gpu_lpdf.py proved on the host (no GPU): lpdf_ref against the float64 oracle with the
oracle's own max(err / bound) as the measured C, its gradients against difference quotients of its own value
in long double, and row weight N against the rows physically repeated."""
import functools

import numpy as np
import pytest

import extended_ref as E
import lpdf_ref as LR
import posterior_ref as PR
from extended_ref import ld

# (hyp, p, n, seed): the kinds and knots of posterior_ref at the default scales and at the short ones; more
# terms than rows, the constant term alone and a single row are in
CASES = {"default p40 n257": (None, 40, 257, 1), "short p40 n257": (PR.HYP_SHORT, 40, 257, 2),
         "short p130 n65": (PR.HYP_SHORT, 130, 65, 3), "default p3 n20": (None, 3, 20, 4),
         "short p1 n2": (PR.HYP_SHORT, 1, 2, 5), "default p40 n1": (None, 40, 1, 6)}


@functools.lru_cache(maxsize=None)
def case_of(name):
    hyp, p, n, seed = CASES[name]
    om = PR.oracle_model(hyp)
    rng = np.random.default_rng(700 + seed)
    x = PR.inside_rows(n, 40 + seed)
    terms = PR.spread_terms(om, p, seed)
    y = rng.standard_normal(n)
    extra = dict(coeff=0.1 * rng.standard_normal(p), g=rng.standard_normal(p), sigma=float(rng.uniform(-2, 0.5)),
                 rho=float(rng.uniform(1, 6)), lam=float(rng.uniform(-1, 1)))
    return LR.Case(om, x, y, terms), extra


def show(title, r64, worst):
    print("%s" % title)
    for k in sorted(worst):
        print("   %-22s oracle err/bound %.2e   oracle err/tol %.3f" % (k, r64.get(k, 0.0), worst[k]))


def case_constant(case, sets):
    """C of a case as lpdf_worker.constant takes it: eight times the largest of the oracle's max(err / bound) on the
    entries of B and dB and of the C it needs on every quantity (lpdf_ref.oracle_need), none above the cap"""
    r64 = dict(LR.entry_ratio(case))
    for title, got64, want in sets:
        for k, v in LR.oracle_need(got64, want).items():
            r64[title + " " + k] = v
    for k, v in r64.items():
        assert v <= E.C_CAP, ("the oracle alone would need more than the cap", k, v)
    return LR.constant_of(r64)[0]


def hold_oracle(title, got64, want, C):
    """the oracle passes EVERY entry of every quantity at the case's C"""
    worst = LR.ratios(got64, want, C)
    show(title + "  (C = %.2e)" % C, LR.oracle_ratio(got64, want), worst)
    assert set(worst) == set(k for k in want if k in got64)
    for k, v in worst.items():
        assert v <= 1.0, (title, k, v)


@pytest.mark.parametrize("name", list(CASES))
def test_every_function_against_the_float64_oracle(name):
    E.require_extended()
    case, q = case_of(name)
    lik = LR.loglik_gauss(case, q["coeff"], q["sigma"], q["g"])
    pr = LR.logpr_gauss(case, q["coeff"], q["rho"], q["g"])
    para = [q["sigma"], q["lam"]]
    sets = [(name + " loglik_gauss", LR.oracle_loglik_gauss(case, q["coeff"], q["sigma"], q["g"]), lik),
            (name + " margadj_diag", LR.oracle_margadj_diag(case, q["sigma"], q["rho"]), LR.margadj_diag(lik, pr))]
    sets += [(name + " loglik_gda doda=%d" % doda, LR.oracle_loglik_gda(case, q["coeff"], para, q["g"], doda),
              LR.loglik_gda(case, q["coeff"], para, q["g"], doda)) for doda in (True, False)]
    C = case_constant(case, sets)
    for title, got64, want in sets:
        hold_oracle(title, got64, want, C)
    # the prior holds no design matrix: its tolerance is the rounding allowance alone
    hold_oracle(name + " logpr_gauss", LR.oracle_logpr_gauss(case, q["coeff"], q["rho"], q["g"]), pr, 0.0)


@pytest.mark.parametrize("hypname", ["short", "default"])
def test_the_oracle_alone_passes_every_entry_of_every_gpu_case(hypname):
    """the cases of test_gpu_lpdf.py (lpdf_worker): with the C measured from it the oracle is within the tolerance
    on every entry of every quantity of every object, so that a device failure there is the device's"""
    import lpdf_worker as W
    cases = [W.small(hypname, p, n) for p, n in W.SHAPES]
    if hypname == "short":
        cases += [W.small("short", 40, 257, 1e6), W.edge(65 * 256 + 1), W.wide()]
    for q in cases:
        C, r64 = W.constant(q)
        worst = W.oracle_passes(q, C)
        print("%-22s C %.2e  largest oracle ratio %.2e  worst err / tol %s" % (
            q.name, C, max(r64.values()), " ".join("%s %.2f" % kv for kv in worst.items())))
        assert max(worst.values()) <= 1.0, (q.name, worst)


@pytest.mark.parametrize("d,maxlev", [(26, 5), (16, 6)])
def test_the_oracle_alone_passes_the_term_sets_of_the_lds_limits(d, maxlev):
    import lpdf_worker as W
    want, got64, C = W.ref_without_gradients(W.lds(d, maxlev))
    worst = LR.ratios(got64, want, C)
    print("lds d%d C %.2e %s" % (d, C, worst))
    assert set(worst) == set(want) and max(worst.values()) <= 1.0


@pytest.mark.parametrize("kind", ["gauss", "std", "gda"])
@pytest.mark.parametrize("seed", [0, 1])
def test_session_against_the_oracle_from_scratch_after_every_step(kind, seed):
    """12 seeded random steps of the walk test_gpu_lpdf.py takes, with the float64 oracle recomputed from scratch at
    the state the Session holds in the device's place: the Session's arithmetic at every state it passes through
    (the oracle shares the Session's state, so its cache RULES are not what this proves: the next test does)"""
    import lpdf_worker as W
    assert len(W.walk_steps(seed, kind)) == 12
    W.host_walk(kind, seed)


@pytest.mark.parametrize("kind", ["gauss", "gda"])
@pytest.mark.parametrize("seed", range(4))
def test_session_rules_against_the_harness_state_machine(kind, seed):
    """the same walks beside oracle/ob_harness.py's LpdfVec, which keeps its own caches: the Session's rules for
    what is defined, and of which state, against an independent holder of them (no optnewton there: the rule of
    the full adjustment is left to the named GPU sequences, whose two adjustments differ by far more than any
    tolerance)"""
    import lpdf_worker as W
    W.harness_walk(kind, seed)


def test_the_walks_reach_every_step_of_the_alphabet():
    import lpdf_worker as W
    for kind in ("gauss", "std", "gda"):
        seen = {st["name"] for seed in range(8) for st in W.walk_steps(seed, kind)}
        want = {"updatepara", "updateom", "updateterms_same", "updateterms_other", "update", "domarg", "optcg",
                "hessmult", "reads"} | ({"optnewton"} if kind == "std" else set()) | ({"doda"} if kind == "gda" else set())
        assert seen == want, (kind, want - seen)


def test_full_adjustment_and_predictors_against_the_float64_oracle():
    """the full-Hessian adjustment and the three predictors (mean, variance; predr_std diagonal and full; pred_gda
    with its residual variance at the new rows) on the H both sides hold"""
    import math
    import ob_oracle as O
    import lpdf_worker as W
    q = W.small("short", 40, 257)
    case, sig, rho = q.case, q.sigma, q.rho
    C, _ = W.constant(q)
    G, _ = O.gram(O.OuterBase(case.om, case.x), case.terms)
    H = math.exp(-2 * sig) * G + np.diag(O.prior_prec(case.om, case.terms, rho))
    for N in (1, 3):
        HN = math.exp(-2 * sig) * N * G + np.diag(O.prior_prec(case.om, case.terms, rho))
        hold_oracle("margadj_full N=%d" % N, LR.oracle_margadj_full(case, HN, sig, rho, N),
                    LR.margadj_full(case, HN, sig, rho, N), C)
    D = W.ref_pair(q)["diaghess"]
    D64 = W.oracle_pair(q)["diaghess"]
    for nnew in (1, 63, 257):
        xnew = PR.inside_rows(nnew, 300 + nnew)
        mean = O.predict_mean(case.om, case.terms, q.coeff, xnew)
        bn = O.OuterBase(case.om, xnew)
        e0 = math.exp(2 * sig)
        hold_oracle("pred_gauss %d" % nnew, {"mean": mean, "var": O.predict_var_gauss(case.om, case.terms, D64, sig, xnew)},
                    LR.predict(case, xnew, q.coeff, [sig], "gauss", D), C)
        hold_oracle("predr_std diag %d" % nnew, {"mean": mean, "var": O.ob_sqmm(bn, case.terms, D64) + e0},
                    LR.predict(case, xnew, q.coeff, [sig], "std", D), C)
        hold_oracle("predr_std full %d" % nnew, {"mean": mean, "var": O.predict_var_std(case.om, case.terms, H, sig, xnew)},
                    LR.predict(case, xnew, q.coeff, [sig], "std", D, H), C)
        rv = O.ob_residvar(bn, case.terms)
        for doda in (True, False):
            var = O.ob_sqmm(bn, case.terms, 1.0 / D64) + e0 + (math.exp(2 * q.lam) * rv if doda else 0.0)
            hold_oracle("pred_gda %d doda=%d" % (nnew, doda), {"mean": mean, "var": var},
                        LR.predict(case, xnew, q.coeff, [sig, q.lam], "gda", D, None, doda), C)
    v0 = LR.predict(case, xnew, q.coeff, [sig], "gauss", None)["var"]
    assert np.all(v0.v == np.exp(2 * ld(sig)))


def test_hess_of_loglik_std_against_the_float64_oracle():
    import math
    import ob_oracle as O
    case, q = case_of("short p40 n257")
    want = LR.loglik_gauss(case, q["coeff"], q["sigma"], hess=True)
    G, _ = O.gram(O.OuterBase(case.om, case.x), case.terms)
    got64 = {"hess": math.exp(-2 * q["sigma"]) * G}
    hold_oracle("hess", got64, {"hess": want["hess"]}, case_constant(case, [("", got64, {"hess": want["hess"]})]))
    # diaghess is the diagonal of hess
    assert np.array_equal(np.diagonal(want["hess"].v), want["diaghess"].v)


def test_para0_against_the_float64_oracle_and_far_from_zero():
    import ob_oracle as O
    rng = np.random.default_rng(5)
    for n, mean in ((2, 0.0), (257, 0.0), (257, 1e6), (513, 1e6)):
        y = mean + rng.standard_normal(n)
        want = LR.para0_gauss(y)
        got = O.default_sigma(y)
        r = E.worst_ratio(np.array([got]), want.v[None], LR.tol(want, 0.0)[None])
        print("para0 n %d mean %g: oracle err/tol %.3f tol %.2e" % (n, mean, r, float(LR.tol(want, 0.0))))
        assert r <= 1.0
        # the one-pass form sum y^2 - n mean^2 loses eps (mean / sd)^2: the tolerance must not let it through
        if mean:
            onepass = np.log(0.01 * (np.sum(y * y) - n * np.mean(y) ** 2) / (n - 1))
            assert abs(onepass - float(want.v)) > float(LR.tol(want, 0.0))
        g = LR.para0_gda(y)
        assert abs(0.5 * got - float(g.v)) <= float(LR.tol(g, 0.0))
    assert np.isnan(LR.para0_gauss(np.array([1.5])).v)


# ---- the restatement's gradients are the gradients of its own value ------------------------------------------
def small_case():
    om = PR.oracle_model(PR.HYP_SHORT)
    rng = np.random.default_rng(11)
    return LR.Case(om, PR.inside_rows(40, 12), rng.standard_normal(40), PR.spread_terms(om, 12, 13)), rng


def central(f, z, h=1e-6):
    """central differences of the scalar f at the long double point z"""
    z = np.asarray(z, dtype=ld)
    out = np.empty(len(z), dtype=ld)
    for k in range(len(z)):
        e = np.zeros(len(z), dtype=ld)
        e[k] = ld(h)
        out[k] = (f(z + e) - f(z - e)) / (2 * ld(h))
    return out


def close(got, want, rel=1e-10):
    got, want = np.asarray(got, dtype=ld).ravel(), np.asarray(want, dtype=ld).ravel()
    assert float(np.max(np.abs(got - want))) <= rel * float(np.max(np.abs(want))), (got, want)


def test_grad_and_gradpara_are_difference_quotients_of_val():
    """central differences in long double, h = 1e-6: truncation ~ h^2 (the values are quadratic or smooth in
    coeff and para), rounding ~ eps_ld / h = 1e-13; 1e-10 relative to the largest entry"""
    case, rng = small_case()
    c0 = 0.1 * rng.standard_normal(case.p)
    sigma, rho, lam = -0.7, 3.5, 0.3
    # coefficients are exact float64 inputs of the restatement: step them as long doubles through the same code
    close(LR.loglik_gauss(case, c0, sigma)["grad"].v, central(lambda c: LR.loglik_gauss(case, c, sigma)["val"].v, c0))
    close(LR.logpr_gauss(case, c0, rho)["grad"].v, central(lambda c: LR.logpr_gauss(case, c, rho)["val"].v, c0))
    for doda in (True, False):
        close(LR.loglik_gda(case, c0, [sigma, lam], doda=doda)["grad"].v,
              central(lambda c: LR.loglik_gda(case, c, [sigma, lam], doda=doda)["val"].v, c0))
        close(LR.loglik_gda(case, c0, [sigma, lam], doda=doda)["gradpara"].v,
              central(lambda z: LR.loglik_gda(case, c0, z, doda=doda)["val"].v, [sigma, lam]))
    close(LR.loglik_gauss(case, c0, sigma)["gradpara"].v,
          central(lambda z: LR.loglik_gauss(case, c0, z[0])["val"].v, [sigma]))
    close(LR.logpr_gauss(case, c0, rho)["gradpara"].v, central(lambda z: LR.logpr_gauss(case, c0, z[0])["val"].v, [rho]))

    # the pair with its diagonal adjustment, both orders of the members
    def pair(z, order):
        lik, pr = LR.loglik_gauss(case, c0, z[order.index("lik")]), LR.logpr_gauss(case, c0, z[order.index("pr")])
        return LR.lpdfvec_diag([(k, lik if k == "lik" else pr) for k in order])
    for order, z0 in ((["pr", "lik"], [rho, sigma]), (["lik", "pr"], [sigma, rho])):
        close(pair(z0, order)["gradpara"].v, central(lambda z: pair(z, order)["val"].v, z0))
    # the diaghess family: derivatives of diaghess by the parameters
    close(LR.loglik_gda(case, c0, [sigma, lam])["diaghessgradpara"].v[3],
          central(lambda z: LR.loglik_gda(case, c0, z)["diaghess"].v[3], [sigma, lam]))
    close(LR.loglik_gauss(case, c0, sigma)["diaghessgradpara"].v[3],
          central(lambda z: LR.loglik_gauss(case, c0, z[0])["diaghess"].v[3], [sigma]))


def test_gradhyp_is_a_difference_quotient_of_val_through_the_eigen_solver():
    """the rotation is rebuilt by the float64 eigen-solver at hyp +- step: the criterion the suite uses for
    this quotient (test_lpdfvec_marginal_adjustment_diagonal_form): step 1e-4 along a random direction, levels
    <= 7, 1e-3"""
    import ob_oracle as O
    kinds = ["mat25pow", "mat25", "mat25"]
    rng = np.random.default_rng(31)

    def model(hyp=None):
        om = O.OuterMod()
        om.setcovfs(kinds)
        if hyp is not None:
            om.hyp_set(hyp)
        om.setknot(O.bench_knots(kinds, 20))
        return om
    om0 = model()
    x, y = O.synth_xy(42, 0, 200, kinds)
    y = (y - y.mean()) / y.std(ddof=1)
    terms = om0.selectterms(40)
    assert terms.max() <= 7
    coeff = 0.05 * rng.standard_normal(40)
    rho, sigma, lam = 4.5, -1.1, 0.2
    hd = rng.random(len(om0.hyp)) - 0.5

    def values(om):
        case = LR.Case(om, x, y, terms)
        lik, pr = LR.loglik_gauss(case, coeff, sigma), LR.logpr_gauss(case, coeff, rho)
        return {"lik": lik, "pr": pr, "pair": LR.lpdfvec_diag([("pr", pr), ("lik", lik)]),
                "gda": LR.loglik_gda(case, coeff, [sigma, lam])}
    v0 = values(om0)
    vp, vm = values(model(om0.hyp + 1e-4 * hd)), values(model(om0.hyp - 1e-4 * hd))
    for k in v0:
        fd = float(vp[k]["val"].v - vm[k]["val"].v) / 2e-4
        an = float(v0[k]["gradhyp"].v @ hd)
        print("gradhyp of %s: quotient %.8e analytic %.8e" % (k, fd, an))
        assert abs(fd - an) < 1e-3 * abs(fd)


# ---- row weight ------------------------------------------------------------------------------------------------
def test_row_weight_equals_the_rows_repeated():
    """N simulated ranks = the rows physically repeated N times, to long double rounding (the two differ in the
    order of the long double sums only)"""
    case, q = case_of("short p40 n257")
    N = 3
    rep = LR.Case(case.om, np.tile(case.x, (N, 1)), np.tile(case.y, N), case.terms)
    a = LR.loglik_gauss(case, q["coeff"], q["sigma"], q["g"], N=N, hess=True)
    b = LR.loglik_gauss(rep, q["coeff"], q["sigma"], q["g"], hess=True)
    for k in a:
        err = float(np.max(np.abs(a[k].v - b[k].v)))
        assert err <= 1e-16 * float(np.max(np.abs(b[k].v))), (k, err)
        # and the tolerances of the two forms agree to a rounding of the product by N
        ta, tb = LR.tol(a[k], 1e-13), LR.tol(b[k], 1e-13)
        assert np.all(ta >= tb * (1 - 1e-12)) and np.all(ta <= 1.5 * tb + 1e-300), k
    pa, pb = LR.para0_gauss(case.y, N), LR.para0_gauss(np.tile(case.y, N))
    assert abs(float(pa.v - pb.v)) <= 1e-17 * abs(float(pb.v))
    # the oracle on the repeated rows passes the weighted reference
    got64 = LR.oracle_loglik_gauss(case, q["coeff"], q["sigma"], q["g"], N=N)
    hold_oracle("row weight 3", got64, a, case_constant(case, [("", got64, a)]))


def test_chunked_rows_equal_the_rows_at_once(monkeypatch):
    case, q = case_of("default p3 n20")
    whole = LR.loglik_gda(case, q["coeff"], [q["sigma"], q["lam"]], q["g"])
    monkeypatch.setattr(LR, "CHUNK", 7)
    parts = LR.loglik_gda(LR.Case(case.om, case.x, case.y, case.terms), q["coeff"], [q["sigma"], q["lam"]], q["g"])
    for k in whole:
        assert float(np.max(np.abs(whole[k].v - parts[k].v))) <= 1e-17 * float(np.max(np.abs(whole[k].v))), k
        assert np.allclose(LR.tol(whole[k], 1e-13), LR.tol(parts[k], 1e-13), rtol=1e-9, atol=0), k
