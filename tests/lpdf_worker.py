"""What test_gpu_lpdf.py shares with the child processes it starts for the process-wide switches of the model
layer (OBHIP_UPDATE_FUSED is read once per process, OBHIP_FORCE_GENERIC and OBHIP_HM3 where a launch is planned):
the cases, their memoised host references (lpdf_ref) with the C measured from the float64 oracle, the readers
of the device objects and the comparison that prints device and oracle ratios side by side.

Run as a program it checks every quantity of the three likelihoods, the prior and the pair on the n = 257,
p = 40 case and the optcg -> diaghess sequence under whatever switches its environment sets, and exits 0 / 1."""
import ctypes as C
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import extended_ref as E       # noqa: E402
import lpdf_ref as LR          # noqa: E402
import posterior_ref as PR     # noqa: E402

HYPS = {"short": PR.HYP_SHORT, "default": None}
EDGE_KINDS = ["mat25pow", "mat25"]
# (p, n) of the d = 4 cases, the whole product: p through spread_terms (the constant term alone, 3, 40, 130), n
# around the 256-row block of every n-vector kernel, more terms than rows included
SHAPES = [(p, n) for p in (1, 3, 40, 130) for n in (1, 2, 255, 256, 257, 513)]


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- models ---------------------------------------------------------------------------------------------------
def oracle_model(kinds, nknots, hyp=None):
    import ob_oracle as O
    om = O.OuterMod()
    om.setcovfs(kinds)
    if hyp is not None:
        om.hyp_set(np.asarray(hyp, dtype=np.float64))
    om.setknot(O.bench_knots(kinds, nknots))
    return om


def share_rotation(om_o, om_d):
    """the device model takes the oracle's eigen-decomposition: both sides hold the same rotation"""
    om_d.set_rotation(om_o.rotmat, om_o.basisvar, om_o.maxlevel)
    om_d.set_rotation_grad(om_o.rotmat_gradhyp, om_o.logbasisvar_gradhyp)


def device_model(om_o):
    import outerbase_amd as ob
    om_d = ob.outermod()
    ob.setcovfs(om_d, om_o.kinds)
    om_d.updatehyp(om_o.hyp)
    ob.setknot(om_d, [np.asarray(om_o.knots_of(k)) for k in range(om_o.d)])
    share_rotation(om_o, om_d)
    return om_d


# ---- cases ----------------------------------------------------------------------------------------------------
class Q:
    """one case: the lpdf_ref.Case, the inputs of every call and the oracle's C"""


@functools.lru_cache(maxsize=None)
def small(hypname, p, n, ymean=0.0):
    """the d = 4 model of posterior_ref (all three covariance families) on n rows and p spread terms"""
    q = Q()
    q.name = "%s p%d n%d%s" % (hypname, p, n, " far" if ymean else "")
    om = oracle_model(PR.KINDS, PR.NKNOTS, HYPS[hypname])
    rng = np.random.default_rng(1000 * p + n)
    q.case = LR.Case(om, PR.inside_rows(n, 7 * n + p), ymean + rng.standard_normal(n), PR.spread_terms(om, p, p + n))
    fill(q, rng)
    return q


@functools.lru_cache(maxsize=None)
def edge(n):
    """the row-count edges: d = 2, 12 knots, p = 12, three hyper-parameters"""
    q = Q()
    q.name = "edge n%d" % n
    om = oracle_model(EDGE_KINDS, 12)
    rng = np.random.default_rng(n)
    x = PR.inside_rows(n, n, EDGE_KINDS)
    q.case = LR.Case(om, x, np.sin(3 * x[:, 0]) * x[:, 1] + 0.3 * rng.standard_normal(n), om.selectterms(12))
    fill(q, rng)
    return q


def random_terms(rng, p, d, maxlev, max_nnz):
    """terms with a controlled number of non-zero levels, the constant first (as test_gpu_parity.random_terms)"""
    t = np.zeros((p, d), dtype=np.int64)
    for k in range(1, p):
        nnz = int(rng.integers(1, max_nnz + 1))
        dims = rng.choice(d, size=nnz, replace=False)
        t[k, dims] = rng.integers(1, maxlev + 1, size=nnz)
    return t


@functools.lru_cache(maxsize=None)
def wide():
    """a term of nine factors: its views are beyond the 8 column slots of the fused gradient kernel, the older
    per-hyper-parameter passes answer (test_views_too_wide_for_the_fused_kernel_take_the_older_passes)"""
    q = Q()
    q.name = "wide views"
    kinds = ["mat25"] * 10
    om = oracle_model(kinds, 10)
    rng = np.random.default_rng(9)
    terms = random_terms(rng, 120, 10, 3, 9)
    terms[1, :9] = 1
    x = PR.inside_rows(200, 9, kinds)
    q.case = LR.Case(om, x, rng.standard_normal(200), terms)
    fill(q, rng)
    return q


@functools.lru_cache(maxsize=None)
def lds(d, maxlev):
    """the term sets of test_fused_hessian_product_between_its_two_lds_limits: 1 + d maxlev used columns, inside
    (97) or outside (131) what the fused product keeps in LDS for its update() form"""
    q = Q()
    q.name = "lds d%d" % d
    kinds = ["mat25"] * d
    om = oracle_model(kinds, 20)
    rng = np.random.default_rng(d)
    n, p = 700, 3000
    x = PR.inside_rows(n, d, kinds)
    terms = random_terms(rng, p, d, maxlev, 4)
    for l in range(d):                      # every level of every dimension is used somewhere
        terms[1 + l * maxlev:1 + (l + 1) * maxlev, :] = 0
        terms[1 + l * maxlev:1 + (l + 1) * maxlev, l] = np.arange(1, maxlev + 1)
    q.case = LR.Case(om, x, rng.standard_normal(n), terms)
    fill(q, rng)
    q.coeff, q.g = q.coeff / 10, q.g / 50
    return q


@functools.lru_cache(maxsize=None)
def ref_without_gradients(q):
    """(want, the oracle's answers, C) of loglik_gauss where n x p x nhyp is too much for the host: everything
    that needs no dB"""
    want = LR.loglik_gauss(q.case, q.coeff, q.sigma, q.g, grads=False)
    got64 = LR.oracle_loglik_gauss(q.case, q.coeff, q.sigma, q.g, grads=False)
    r64 = dict(LR.entry_ratio(q.case, grads=False))
    r64.update(LR.oracle_need(got64, want))
    assert max(r64.values()) <= E.C_CAP, r64
    return want, got64, LR.constant_of(r64)[0]


def check_without_gradients(q):
    want, got64, Cc = ref_without_gradients(q)
    _, lik = make(q, "loglik_gauss")
    lik.updatepara([q.sigma])
    lik.compute_gradpara = True
    lik.update(q.coeff)
    got = dict(val=lik.val, grad=lik.grad, gradpara=lik.gradpara, hessmult=lik.hessmult(q.g), diaghess=lik.diaghess(),
               diaghessgradpara=lik.diaghessgradpara(), sqcolsums=lik.ob.sqcolsums(q.case.terms))
    hold(q.name + " loglik_gauss", got, want, Cc, got64)
    return lik


def fill(q, rng):
    p = q.case.p
    q.coeff, q.g = 0.1 * rng.standard_normal(p), rng.standard_normal(p)
    q.sigma, q.rho, q.lam = float(rng.uniform(-2, 0.5)), float(rng.uniform(1, 6)), float(rng.uniform(-1, 1))


@functools.lru_cache(maxsize=None)
def constant(q, N=1):
    """(C, {quantity: the oracle's ratio}) of the case: the oracle's max(err / bound) on the entries of B and dB
    (lpdf_ref.entry_ratio) and the C it needs on every quantity built on them (lpdf_ref.oracle_need: the
    likelihoods, the pair with its adjustment); eight times the largest, at most the cap -- and no ratio alone
    may need more than the cap"""
    r64 = dict(LR.entry_ratio(q.case))
    for k, v in LR.oracle_need(oracle_lik(q, N), ref_lik(q, N)).items():
        r64["lik " + k] = v
    for order in (("pr", "lik"), ("lik", "pr")):
        for k, v in LR.oracle_need(oracle_pair(q, order, N), ref_pair(q, order, N)).items():
            r64["pair " + k] = max(v, r64.get("pair " + k, 0.0))
    if N == 1:
        for doda in (True, False):
            for k, v in LR.oracle_need(oracle_gda(q, doda), ref_gda(q, doda)).items():
                r64["gda%d %s" % (doda, k)] = v
    for k, v in r64.items():
        assert v <= E.C_CAP, ("the oracle alone would need more than the cap", q.name, k, v)
    return LR.constant_of(r64)[0], r64


def oracle_passes(q, Cc):
    """{object: the oracle's worst err / tolerance over every entry of every quantity} at the case's C"""
    sets = {"lik": (oracle_lik(q), ref_lik(q), Cc), "pr": (oracle_pr(q), ref_pr(q), 0.0),
            "gda1": (oracle_gda(q, True), ref_gda(q, True), Cc), "gda0": (oracle_gda(q, False), ref_gda(q, False), Cc),
            "pair": (oracle_pair(q), ref_pair(q), Cc),
            "pair'": (oracle_pair(q, ("lik", "pr")), ref_pair(q, ("lik", "pr")), Cc)}
    return {k: max(LR.ratios(got64, want, c).values()) for k, (got64, want, c) in sets.items()}


@functools.lru_cache(maxsize=None)
def ref_lik(q, N=1, hess=False):
    return LR.loglik_gauss(q.case, q.coeff, q.sigma, q.g, N=N, hess=hess)


@functools.lru_cache(maxsize=None)
def oracle_lik(q, N=1):
    return LR.oracle_loglik_gauss(q.case, q.coeff, q.sigma, q.g, N=N)


@functools.lru_cache(maxsize=None)
def ref_pr(q):
    return LR.logpr_gauss(q.case, q.coeff, q.rho, q.g)


@functools.lru_cache(maxsize=None)
def oracle_pr(q):
    return LR.oracle_logpr_gauss(q.case, q.coeff, q.rho, q.g)


@functools.lru_cache(maxsize=None)
def ref_gda(q, doda=True):
    return LR.loglik_gda(q.case, q.coeff, [q.sigma, q.lam], q.g, doda)


@functools.lru_cache(maxsize=None)
def oracle_gda(q, doda=True):
    return LR.oracle_loglik_gda(q.case, q.coeff, [q.sigma, q.lam], q.g, doda)


def with_hessmult(d, a, b):
    d["hessmult"] = a["hessmult"] + b["hessmult"]
    return d


@functools.lru_cache(maxsize=None)
def ref_pair(q, order=("pr", "lik"), N=1, domarg=True):
    parts = {"lik": ref_lik(q, N), "pr": ref_pr(q)}
    return with_hessmult(LR.lpdfvec_diag([(k, parts[k]) for k in order], domarg), parts["lik"], parts["pr"])


@functools.lru_cache(maxsize=None)
def oracle_pair(q, order=("pr", "lik"), N=1, domarg=True):
    lik, pr = oracle_lik(q, N), oracle_pr(q)
    parts = {"lik": lik, "pr": pr}
    out = {k: lik[k] + pr[k] for k in ("val", "grad", "gradhyp", "diaghess", "hessmult")}
    out["gradpara"] = np.concatenate([parts[k]["gradpara"] for k in order])
    if domarg:
        m = LR.oracle_margadj_diag(q.case, q.sigma, q.rho, N)
        out["val"] += m["val"]
        out["gradhyp"] = out["gradhyp"] + m["gradhyp"]
        out["gradpara"] = out["gradpara"] + np.concatenate([m["gradpara_" + k] for k in order])
        out["diaghessgradhyp"] = lik["diaghessgradhyp"] + pr["diaghessgradhyp"]
        out["diaghessgradpara"] = np.concatenate([parts[k]["diaghessgradpara"] for k in order], axis=1)
    return out


# ---- the device objects and what is read from them ---------------------------------------------------------------
def make(q, kind, om_d=None):
    """(om_d, object) of kind loglik_gauss | loglik_std | loglik_gda | logpr_gauss on the case's data"""
    import outerbase_amd as ob
    om_d = om_d or device_model(q.case.om)
    if kind == "logpr_gauss":
        return om_d, ob.logpr_gauss(om_d, q.case.terms)
    return om_d, getattr(ob, kind)(om_d, q.case.terms, q.case.y, q.case.x)


def read(obj, g=None, update=None, family=True):
    """every quantity the object gives at its current state, under lpdf_ref's names; update: coefficients to
    call update() with first (all four flags set)"""
    out = {}
    if update is not None:
        obj.compute_val = obj.compute_grad = obj.compute_gradhyp = obj.compute_gradpara = True
        obj.update(update)
        out.update(val=obj.val, grad=obj.grad, gradhyp=obj.gradhyp, gradpara=obj.gradpara)
    if g is not None:
        out["hessmult"] = obj.hessmult(g)
    out["diaghess"] = obj.diaghess()
    if family:
        out["diaghessgradhyp"] = obj.diaghessgradhyp()
        out["diaghessgradpara"] = obj.diaghessgradpara()
    return out


def read_basis(lik, terms, gda=False):
    """the products the likelihood's outerbase gives directly"""
    if gda:
        return {"residvar": lik.ob.residvar(terms), "residvar_gradhyp": lik.ob.residvar_gradhyp(terms)}
    return {"sqcolsums": lik.ob.sqcolsums(terms), "sqcolsums_gradhyp": lik.ob.sqcolsums_gradhyp(terms)}


def sim_comm(ranks):
    from outerbase_amd._lib import call
    comm = C.c_void_p()
    call("obhip_comm_init_sim", C.byref(comm), ranks)
    return comm


def free_comm(comm):
    from outerbase_amd._lib import lib
    lib.obhip_comm_destroy(comm)


# ---- the comparison -------------------------------------------------------------------------------------------
def hold(title, got, want, Cc, got64=None):
    """worst_ratio(device, want, C b + s) <= 1 for every quantity the device gave (every entry of it), device
    and oracle ratios printed side by side; every quantity read must have a reference"""
    missing = [k for k in got if k not in want]
    assert not missing, (title, "no reference for", missing)
    dev = LR.ratios(got, want, Cc)
    orc = LR.ratios(got64, want, Cc) if got64 is not None else {}
    bad = []
    for k in sorted(dev):
        o = "%.3f" % orc[k] if k in orc else "-"
        print("%-44s %-20s device %.3f  oracle %s  (C %.2e)" % (title, k, dev[k], o, Cc))
        if not dev[k] <= 1.0:
            bad.append((k, dev[k]))
    assert not bad, (title, bad)
    return dev


def check_all_objects(q, pair_order=("pr", "lik")):
    """every quantity of loglik_gauss, loglik_std, logpr_gauss, loglik_gda (doda on and off) and the pair with
    its diagonal adjustment on one case"""
    import outerbase_amd as ob
    Cc, _ = constant(q)
    terms = q.case.terms
    om_d = device_model(q.case.om)
    for kind in ("loglik_gauss", "loglik_std"):
        _, lik = make(q, kind, om_d)
        lik.updatepara([q.sigma])
        got = read(lik, q.g, q.coeff)
        got.update(read_basis(lik, terms))
        want = ref_lik(q)
        if kind == "loglik_std" and q.case.n * q.case.p * q.case.p <= 1 << 21:
            got["hess"] = lik.hess()
            want = ref_lik(q, 1, True)
        hold(q.name + " " + kind, got, want, Cc, oracle_lik(q))
    _, pr = make(q, "logpr_gauss", om_d)
    pr.updatepara([q.rho])
    hold(q.name + " logpr_gauss", read(pr, q.g, q.coeff), ref_pr(q), 0.0, oracle_pr(q))
    for doda in (True, False):
        _, lg = make(q, "loglik_gda", om_d)
        if not doda:
            lg.dodiag = False
        lg.updatepara([q.sigma, q.lam])
        got = read(lg, None, q.coeff)
        got["hessmult"] = lg.hessmult(q.g)
        got.update(read_basis(lg, terms, True))
        hold(q.name + " loglik_gda doda=%d" % doda, got, ref_gda(q, doda), Cc, oracle_gda(q, doda))
    parts = {"pr": make(q, "logpr_gauss", om_d)[1], "lik": make(q, "loglik_gauss", om_d)[1]}
    lp = ob.lpdfvec(parts[pair_order[0]], parts[pair_order[1]])
    lp.domarg = True
    lp.updatepara([{"pr": q.rho, "lik": q.sigma}[k] for k in pair_order])
    hold(q.name + " lpdfvec(%s, %s)" % pair_order, read(lp, q.g, q.coeff), ref_pair(q, pair_order), Cc,
         oracle_pair(q, pair_order))


def check_optcg_then_diaghess(q):
    """optcg leaves the preconditioner's sqcolsums to the likelihood: diaghess / diaghessgradpara read after it,
    and everything of the pair at the device's own coefficients"""
    import outerbase_amd as ob
    Cc, _ = constant(q)
    om_d, lik = make(q, "loglik_gauss")
    lp = ob.lpdfvec(make(q, "logpr_gauss", om_d)[1], lik)
    lp.updatepara([q.rho, q.sigma])
    lp.optcg(1e-8, 200)
    s = LR.Session(q.case.om, q.case.x, q.case.y, q.case.terms, "gauss", ("pr", "lik"))
    s.updatepara([q.rho, q.sigma])
    hold_optcg(q.name + " optcg", s, lp.coeff, 1e-8, lp.cgiters, 200, Cc)
    q2 = at(q, coeff=lp.coeff)
    want = ref_lik(q2)
    hold(q.name + " optcg -> lik.diaghess", {"diaghess": lik.diaghess(), "diaghessgradpara": lik.diaghessgradpara()},
         want, Cc, oracle_lik(q2))
    got = dict(val=lp.val, grad=lp.grad, gradhyp=lp.gradhyp, gradpara=lp.gradpara, diaghess=lp.diaghess(),
               diaghessgradhyp=lp.diaghessgradhyp(), diaghessgradpara=lp.diaghessgradpara())
    hold(q.name + " optcg -> pair", got, ref_pair(q2), Cc, oracle_pair(q2))
    return lp, lik, om_d


def at(q, **changes):
    """the case with other inputs (coefficients, parameters, terms, model): a new memo key"""
    r = Q()
    r.__dict__.update(q.__dict__)
    case = q.case
    if "terms" in changes or "om" in changes:
        case = LR.Case(changes.pop("om", case.om), case.x, case.y, changes.pop("terms", case.terms))
    r.case = case
    r.__dict__.update(changes)
    r.name = q.name + "*"
    return r


# ---- call order: the step alphabet, the device walker and the oracle at a Session's state -------------------------
WALK_N, WALK_P = 257, 40
CG_TOL, CG_MAXIT = 1e-8, 100
FLAG_NAMES = ("val", "grad", "gradhyp", "gradpara")


def walk_steps(seed, kind, nsteps=12):
    """seeded random steps over the alphabet; pure data, so the host test and the device walk the same sequences"""
    rng = np.random.default_rng(100 * seed + {"gauss": 1, "std": 2, "gda": 3}[kind])
    names = ["updatepara", "updateom", "updateterms_same", "updateterms_other", "update", "update", "domarg",
             "optnewton" if kind == "std" else "optcg", "optcg", "hessmult", "reads"] + (["doda"] if kind == "gda" else [])
    out = []
    for _ in range(nsteps):
        name = names[int(rng.integers(len(names)))]
        st = {"name": name, "draw": int(rng.integers(1 << 30))}
        if name == "update":
            st["flags"] = [bool(b) for b in rng.integers(0, 2, 4)]
        out.append(st)
    return out


def draw_para(rng, kind, order):
    lik = [float(rng.uniform(-2, 0.5))] + ([float(rng.uniform(-1, 1))] if kind == "gda" else [])
    pr = [float(rng.uniform(1, 6))]
    return (pr + lik) if order[0] == "pr" else (lik + pr)


def walk_start(kind, seed):
    """(Session, hyp0, rng-free inputs) of a walk: the d = 4 model at the short scales, n = 257, p = 40"""
    om = oracle_model(PR.KINDS, PR.NKNOTS, PR.HYP_SHORT)
    rng = np.random.default_rng(5000 + seed)
    x = PR.inside_rows(WALK_N, 900 + seed)
    y = rng.standard_normal(WALK_N)
    order = ("lik", "pr") if kind == "std" else ("pr", "lik")
    return LR.Session(om, x, y, PR.spread_terms(om, WALK_P, seed), kind, order)


def step_inputs(s, st):
    """the inputs a step needs besides the Session's state, from the step's own draw"""
    rng = np.random.default_rng(st["draw"])
    name = st["name"]
    if name == "updatepara" or name == "doda":
        return {"para": draw_para(rng, s.kind, s.order)}
    if name == "updateom":
        hyp = np.asarray(PR.HYP_SHORT) + 0.1 * (rng.random(6) - 0.5)
        return {"om": oracle_model(PR.KINDS, PR.NKNOTS, hyp)}
    if name == "updateterms_same":
        return {"terms": PR.spread_terms(s.om, 2 * s.case.p, st["draw"] % 1000)[s.case.p:]}
    if name == "updateterms_other":
        p = int(rng.choice([q for q in (24, 40, 56) if q != s.case.p]))
        return {"terms": PR.spread_terms(s.om, p, st["draw"] % 1000)}
    if name in ("update", "hessmult", "reads", "optcg", "optnewton", "domarg"):
        return {"coeff": 0.1 * rng.standard_normal(s.case.p), "g": rng.standard_normal(s.case.p)}
    raise ValueError(name)


def oracle_state(s, coeff, H=None, g=None):
    """the float64 oracle from scratch at the Session's state, under the pair's names"""
    case, order = s.case, s.order
    sig, rho = s.para["lik"][0], s.para["pr"][0]
    if s.kind == "gda":
        lik = LR.oracle_loglik_gda(case, coeff, s.para["lik"], g, s.doda)
    else:
        lik = LR.oracle_loglik_gauss(case, coeff, sig, g, s.N)
    pr = LR.oracle_logpr_gauss(case, coeff, rho, g)
    parts = {"lik": lik, "pr": pr}
    out = {k: lik[k] + pr[k] for k in ("val", "grad", "gradhyp", "diaghess")}
    if g is not None:
        out["hessmult"] = lik["hessmult"] + pr["hessmult"]
    out["gradpara"] = np.concatenate([parts[k]["gradpara"] for k in order])
    if s.domarg:
        if s.fullhess:
            m = LR.oracle_margadj_full(case, H, sig, rho, s.N)
        else:
            D = out["diaghess"]
            dD = lik["diaghessgradhyp"] + pr["diaghessgradhyp"]
            m = {"val": -0.5 * np.sum(np.log(D)), "gradhyp": -0.5 * np.sum(dD / D[:, None], axis=0),
                 "gradpara_lik": -0.5 * np.sum(lik["diaghessgradpara"] / D[:, None], axis=0),
                 "gradpara_pr": -0.5 * np.sum(pr["diaghessgradpara"] / D[:, None], axis=0)}
        out["val"] = out["val"] + m["val"]
        out["gradhyp"] = out["gradhyp"] + m["gradhyp"]
        out["gradpara"] = out["gradpara"] + np.concatenate([m["gradpara_" + k] for k in order])
        out["diaghessgradhyp"] = lik["diaghessgradhyp"] + pr["diaghessgradhyp"]
        out["diaghessgradpara"] = np.concatenate([parts[k]["diaghessgradpara"] for k in order], axis=1)
    return out


def oracle_hess(s):
    import math
    import ob_oracle as O
    G, _ = O.gram(O.OuterBase(s.om, np.tile(s.x, (s.N, 1))), s.terms)
    return math.exp(-2 * s.para["lik"][0]) * G + np.diag(O.prior_prec(s.om, s.terms, s.para["pr"][0]))


def walk_constant(s):
    """C while the Session's case stands: eight times the oracle's max(err / bound) on the entries of B and dB"""
    r = LR.entry_ratio(s.case)
    assert max(r.values()) <= E.C_CAP, r
    return LR.constant_of(r)[0]


class Walker:
    """the device objects beside a Session: every step is applied to both, and after it everything the Session
    says is defined is read from the device and compared"""

    def __init__(self, kind, seed, log=None):
        import outerbase_amd as ob
        self.s = s = walk_start(kind, seed)
        self.om_d = device_model(s.om)
        cls = {"gauss": ob.loglik_gauss, "std": ob.loglik_std, "gda": ob.loglik_gda}[kind]
        self.lik = cls(self.om_d, s.terms, s.y, s.x)
        self.pr = ob.logpr_gauss(self.om_d, s.terms)
        parts = {"lik": self.lik, "pr": self.pr}
        self.lp = ob.lpdfvec(parts[s.order[0]], parts[s.order[1]])
        self.C = walk_constant(s)
        self.title = "%s seed %d" % (kind, seed)
        self.log = [] if log is None else log       # every number read from the device, for the bit comparison

    def H(self):
        """the device's total Hessian while the full adjustment is in force (the H both sides hold), held to `hess`"""
        s = self.s
        if not (s.kind == "std" and s.domarg and s.fullhess):
            return None
        H = self.lp.hess()
        hold(self.title + " hess", {"hess": H}, {"hess": s.pair_parts(np.zeros(s.case.p))["hess"]}, self.C)
        self.log.append(H.copy())
        return H

    def hold(self, what, got, want, got64=None):
        for k in sorted(got):
            self.log.append(np.array(got[k], dtype=np.float64, copy=True))
        hold(self.title + " " + what, got, want, self.C, got64)

    def after_update(self, what, want, H):
        lp = self.lp
        got = {k: getattr(lp, k) for k in want}
        self.hold(what, got, want, oracle_state(self.s, self.s.coeff, H))

    def compare_reads(self, what, g, H):
        s, lp, lik = self.s, self.lp, self.lik
        po, lo = s.reads(g, H)
        coeff = s.coeff if s.coeff is not None else np.zeros(s.case.p)
        got = {k: (lp.hessmult(g) if k == "hessmult" else getattr(lp, k)()) for k in po}
        self.hold(what + " pair", got, po, oracle_state(s, coeff, H, g))
        got = {k: (lik.hessmult(g) if k == "hessmult" else getattr(lik, k)()) for k in lo}
        self.hold(what + " lik", got, lo)
        if s.kind == "gda":
            s.std_built = True         # the likelihood's diaghess family runs buildstd

    def apply(self, i, st):
        s, lp = self.s, self.lp
        name, inp = st["name"], step_inputs(self.s, st)
        what = "step %d %s" % (i, name)
        if name == "updatepara":
            lp.updatepara(inp["para"])
            s.updatepara(inp["para"])
        elif name == "doda":
            self.lik.dodiag = not s.doda
            s.set_doda(not s.doda)
            lp.updatepara(inp["para"])
            s.updatepara(inp["para"])
        elif name == "updateom":
            self.om_d.updatehyp(inp["om"].hyp)
            share_rotation(inp["om"], self.om_d)
            lp.updateom()
            s.updateom(inp["om"])
            self.C = walk_constant(s)
        elif name.startswith("updateterms"):
            lp.updateterms(inp["terms"])
            s.updateterms(inp["terms"])
            self.C = walk_constant(s)
        elif name == "domarg":
            lp.domarg = not s.domarg
            s.set_domarg(not s.domarg)
        elif name == "update":
            for k, v in zip(FLAG_NAMES, st["flags"]):
                setattr(lp, "compute_" + k, v)
                s.flags[k] = v
            lp.update(inp["coeff"])
            s.built = True                      # (buildhess has run: the device's H is the current one)
            H = self.H()
            self.after_update(what + " flags %s" % "".join(str(int(b)) for b in st["flags"]), s.update(inp["coeff"], H), H)
        elif name in ("optcg", "optnewton"):
            if name == "optcg":
                lp.optcg(CG_TOL, CG_MAXIT)
                hold_optcg(self.title + " " + what, s, lp.coeff, CG_TOL, lp.cgiters, CG_MAXIT, self.C)
            else:
                self.check_newton(what)
            s.fullhess = name == "optnewton"
            s.built = True
            H = self.H()
            self.after_update(what, s.after_opt(lp.coeff, name == "optnewton", H), H)
            for k in FLAG_NAMES:
                assert getattr(lp, "compute_" + k) == s.flags[k], (what, k)
        g = step_inputs(s, dict(st, name="reads"))["g"]
        self.compare_reads(what + " then", g, self.H())

    def check_newton(self, what):
        """optnewton: the device's coefficients against the long double solve of the normal equations, by the Newton
        residual bound of the solver (chol_ref.solve_bound) carried through inv(H) together with the tolerances
        of H and r themselves; the quantities are then evaluated at the device's OWN coefficients"""
        import chol_ref as CR
        s, lp = self.s, self.lp
        lp.optnewton()
        th = lp.coeff
        Hp, rp = s.newton_system()
        L = PR.cholesky_ld(_f64(Hp.v))
        want = PR.forward_ld(L.T[::-1, ::-1], PR.forward_ld(L, rp.v[:, None])[::-1])[::-1, 0]
        H64 = _f64(Hp.v)
        Lhat = np.linalg.cholesky(H64)
        tol = np.abs(np.linalg.inv(H64)) @ (CR.solve_bound(Lhat, th) + LR.tol(Hp, self.C) @ np.abs(th) + LR.tol(rp, self.C))
        r = E.worst_ratio(th, want, tol)
        print("%-44s %-20s device %.3f" % (self.title + " " + what, "coeff", r))
        assert r <= 1.0, (what, "coeff", r)


def host_walk(kind, seed, nsteps=12):
    """the same steps with the float64 oracle, recomputed from scratch at the Session's state, in the device's place
    (CPU only).  The oracle is told the state (parameters, flags, fullhess, domarg, doda) by the Session itself, so
    this proves the Session's ARITHMETIC at every state it passes through -- the full adjustment, every flag
    combination, the reads -- not its cache rules; harness_walk holds the rules against an independent state
    machine.  Returns the worst ratio."""
    s = walk_start(kind, seed)
    worst = 0.0

    def held(what, want, got64):
        nonlocal worst
        r = LR.ratios(got64, want, Cc)
        assert set(r) == set(want), (what, set(want) - set(r))
        print("%-10s seed %d %-34s %s" % (kind, seed, what, " ".join("%s %.2f" % kv for kv in sorted(r.items()))))
        worst = max([worst] + list(r.values()))
        assert worst <= 1.0, (kind, seed, what, r)

    Cc = walk_constant(s)
    for i, st in enumerate(walk_steps(seed, kind, nsteps)):
        name, inp = st["name"], step_inputs(s, st)
        what = "step %d %s" % (i, name)
        if name == "updatepara":
            s.updatepara(inp["para"])
        elif name == "doda":
            s.set_doda(not s.doda)
            s.updatepara(inp["para"])
        elif name == "updateom":
            s.updateom(inp["om"])
        elif name.startswith("updateterms"):
            s.updateterms(inp["terms"])
        elif name == "domarg":
            s.set_domarg(not s.domarg)
        if name in ("updateom", "updateterms_same", "updateterms_other"):
            Cc = walk_constant(s)
        H = None
        if name == "update":
            s.flags.update(zip(FLAG_NAMES, st["flags"]))
            H = oracle_hess(s) if s.kind == "std" and s.domarg and s.fullhess else None
            held(what, s.update(inp["coeff"], H), oracle_state(s, inp["coeff"], H))
        elif name in ("optcg", "optnewton"):
            s.fullhess = name == "optnewton"
            H = oracle_hess(s) if s.kind == "std" and s.domarg and s.fullhess else None
            coeff = inp["coeff"]
            if name == "optnewton":
                Hp, rp = s.newton_system()
                coeff = np.linalg.solve(oracle_hess(s), _f64(rp.v))
            held(what, s.after_opt(coeff, name == "optnewton", H), oracle_state(s, coeff, H))
        H = oracle_hess(s) if s.kind == "std" and s.domarg and s.fullhess else None
        po, lo = s.reads(inp.get("g", np.ones(s.case.p)), H)
        coeff = s.coeff if s.coeff is not None else np.zeros(s.case.p)
        got64 = oracle_state(s, coeff, H, inp.get("g", np.ones(s.case.p)))
        held(what + " reads", po, {k: got64[k] for k in po})
        if s.kind == "gda":
            s.std_built = True
    return worst


def harness_walk(kind, seed, nsteps=12):
    """The same steps with the float64 state machine of oracle/ob_harness.py (LpdfVec over LogprGauss and
    LoglikGauss | LoglikGda, with its own redohess / buildhess caches, its own buildstd and its own optcg loop on
    its own model object) in the device's place: an INDEPENDENT holder of the reference's cache rules, where
    host_walk's oracle is told the state by the Session itself.  What the harness has cached is read as it stands
    (its val / grad / gradhyp / gradpara after update, its diaghessv, its members' observation standard deviations in
    hessmult), so a Session that called something defined which a state change had left stale, or expected the
    value of another state, disagrees with it.  The harness has no optnewton and no full Hessian (the rule that
    optnewton's adjustment stays and optcg drops it is not covered here: kinds gauss and gda only), and the device's
    rule that a change of domarg rebuilds is applied to it by hand."""
    import ob_harness as HN
    assert kind in ("gauss", "gda")
    s = walk_start(kind, seed)
    hom = oracle_model(PR.KINDS, PR.NKNOTS, PR.HYP_SHORT)
    hlik = (HN.LoglikGauss if kind == "gauss" else HN.LoglikGda)(hom, s.terms, s.y, s.x)
    hpr = HN.LogprGauss(hom, s.terms)
    parts = {"lik": hlik, "pr": hpr}
    hp = HN.LpdfVec(parts[s.order[0]], parts[s.order[1]])
    Cc = walk_constant(s)
    worst = 0.0

    def held(what, want, got64):
        nonlocal worst
        r = LR.ratios(got64, want, Cc)
        assert set(r) == set(want), (what, set(want) - set(r))
        print("%-10s seed %d %-34s %s" % (kind, seed, what, " ".join("%s %.2f" % kv for kv in sorted(r.items()))))
        worst = max([worst] + list(r.values()))
        assert worst <= 1.0, (kind, seed, what, r)

    for i, st in enumerate(walk_steps(seed, kind, nsteps)):
        name, inp = st["name"], step_inputs(s, st)
        what = "step %d %s" % (i, name)
        if name in ("updatepara", "doda"):
            if name == "doda":
                hlik.doda = not hlik.doda
                s.set_doda(not s.doda)
            hp.updatepara(inp["para"])
            s.updatepara(inp["para"])
        elif name == "updateom":
            hom.hyp_set(inp["om"].hyp)
            hp.updateom()
            s.updateom(inp["om"])
            Cc = walk_constant(s)
        elif name.startswith("updateterms"):
            hp.updateterms(inp["terms"])
            s.updateterms(inp["terms"])
            Cc = walk_constant(s)
        elif name == "domarg":
            hp.domarg = not hp.domarg
            hp.redohess = True
            s.set_domarg(not s.domarg)
        elif name == "update":
            s.flags.update(zip(FLAG_NAMES, st["flags"]))
            hp.update(inp["coeff"], want_gradhyp=True)
            want = s.update(inp["coeff"])
            held(what, want, {k: getattr(hp, k) for k in want})
        elif name == "optcg":
            hp.optcg(CG_TOL, CG_MAXIT)
            want = s.after_opt(hp.coeff, False)
            held(what, want, {k: getattr(hp, k) for k in want})
        g = inp.get("g", np.ones(s.case.p))
        po, lo = s.reads(g)
        got = {}
        if "hessmult" in po:
            got["hessmult"] = hp.hessmult(g)
        if "diaghess" in po:
            got["diaghess"] = hp.diaghessv
        held(what + " reads", {k: po[k] for k in got}, got)
        if kind == "gda":
            hlik.buildstd()                    # (the likelihood's diaghess family of the device runs buildstd)
            s.std_built = True
        held(what + " lik", {k: lo[k] for k in ("diaghess", "diaghessgradhyp", "diaghessgradpara")},
             {"diaghess": hlik.diaghess(), "diaghessgradhyp": hlik.diaghessgradhyp(),
              "diaghessgradpara": hlik.diaghessgradpara()})
    return worst


def hold_fuzz_case(om_o, x, y, terms, coeff, sigma, rho, para_gda, lp, lps, lg, dhg_gda):
    """test_gpu_parity.test_random_lpdf_level_quantities beside its flat tolerances: the same device objects against
    lpdf_ref, device and oracle ratios side by side -- lp = lpdfvec(logpr_gauss, loglik_gauss) after update(coeff),
    lps = lpdfvec(loglik_std, logpr_gauss) after optnewton, lg = loglik_gda after update(coeff)"""
    s1 = LR.Session(om_o, x, y, terms, "gauss", ("pr", "lik"))
    s1.updatepara([rho, sigma])
    s2 = LR.Session(om_o, x, y, terms, "std", ("lik", "pr"))
    s2.updatepara([sigma, rho])
    s2.fullhess = True
    H, theta = lps.hess(), lps.coeff
    names = ("val", "grad", "gradhyp", "gradpara")
    sets = [("diagonal adjustment", {k: getattr(lp, k) for k in names}, {k: s1.pair(coeff)[k] for k in names},
             oracle_state(s1, coeff)),
            ("full adjustment", {k: getattr(lps, k) for k in names}, {k: s2.pair(theta, H)[k] for k in names},
             oracle_state(s2, theta, H)),
            ("loglik_gda", dict(val=lg.val, grad=lg.grad, gradhyp=lg.gradhyp, gradpara=lg.gradpara, diaghessgradhyp=dhg_gda),
             LR.loglik_gda(s1.case, coeff, para_gda), LR.oracle_loglik_gda(s1.case, coeff, para_gda))]
    r64 = dict(LR.entry_ratio(s1.case))
    for title, _, want, got64 in sets:
        for k, v in LR.oracle_need(got64, want).items():
            r64[title + " " + k] = v
    assert max(r64.values()) <= E.C_CAP, r64
    Cc = LR.constant_of(r64)[0]
    hold("fuzz hess", {"hess": H}, {"hess": s2.pair_parts(np.zeros(len(coeff)))["hess"]}, Cc)
    for title, got, want, got64 in sets:
        hold("fuzz " + title, got, want, Cc, got64)


def hold_optcg(title, s, theta, cgtol, iters, maxit, Cc):
    """What optcg(cgtol, maxit) left at the Session's state, held to the criterion it was given (fit.cpp:71-73: the
    loop ends at the first iterate with  grad^T (grad / m) < tol,  m = the pair's diaghess, grad the gradient of the
    pair without its adjustment):

      * it stopped by that criterion, not by running out of iterations;
      * the long double gradient g at the device's coefficients meets it: sum g_k^2 / m_k < tol, with the tolerance
        of that sum as a float64 result (first order: 2 |g_k| tol(g_k) / m_k + g_k^2 tol(m_k) / m_k^2);
      * for the one-noise-level likelihoods the objective is quadratic, theta - theta* = inv(H) g for the long double
        solve theta* of the normal equations (posterior_ref.cholesky_ld), and the criterion bounds every |g_k| by
        sqrt(tol m_k): |theta - theta*| <= |inv(H)| (sqrt(tol m) + tol(H) |theta| + tol(r)), the tolerances of H
        and r as check_newton carries them.  (The restatement of loglik_gda has no hess(): the criterion alone
        is held there.)"""
    theta = _f64(theta)
    assert iters < maxit, (title, "optcg ran out of iterations", iters)
    parts = s.pair_parts(theta)
    g, m = parts["grad"], parts["diaghess"]
    gv, mv = _f64(g.v), _f64(m.v)
    num = float(np.sum(gv * gv / mv))
    slack = float(np.sum(2 * np.abs(gv) * LR.tol(g, Cc) / mv + gv * gv * LR.tol(m, Cc) / (mv * mv)))
    print("%-44s %-20s sum g^2/m %.3e (+- %.1e) against tol %.1e after %d iterations" % (title, "criterion", num, slack,
                                                                                      cgtol, iters))
    assert num <= cgtol + slack, (title, "criterion", num, cgtol, slack)
    if s.kind == "gda":
        return
    z = np.zeros(s.case.p)
    lik0 = LR.loglik_gauss(s.case, z, s.para["lik"][0], None, s.N, hess=True, grads=False)
    pr0 = s.pr(z)
    Hp = lik0["hess"] + LR.Pair(np.diag(pr0["diaghess"].v), 0.0, np.diag(np.broadcast_to(pr0["diaghess"].s, (s.case.p,))))
    rp = lik0["grad"] + pr0["grad"]
    L = PR.cholesky_ld(_f64(Hp.v))
    want = PR.forward_ld(L.T[::-1, ::-1], PR.forward_ld(L, rp.v[:, None])[::-1])[::-1, 0]
    H64 = _f64(Hp.v)
    tol = np.abs(np.linalg.inv(H64)) @ (np.sqrt(cgtol * _f64(m.v)) + LR.tol(Hp, Cc) @ np.abs(theta) + LR.tol(rp, Cc))
    r = E.worst_ratio(theta, want, tol)
    print("%-44s %-20s device %.3f" % (title, "coeff", r))
    assert r <= 1.0, (title, "coeff against the long double solve", r)


def run_walk(kind, seed, nsteps=12):
    """the walk; stops at the first failing step (an AssertionError leaves)"""
    w = Walker(kind, seed)
    for i, st in enumerate(walk_steps(seed, kind, nsteps)):
        w.apply(i, st)
    return w.log


def main():
    q = small("short", 40, 257)
    check_all_objects(q)
    check_optcg_then_diaghess(q)
    print("lpdf worker ok")
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main())
    except AssertionError as e:
        print("FAILED:", e)
        sys.exit(1)
