"""The acquisition picks on the device (csrc/acquire.cpp, kernels_acquire.hip) against the long-double explicit
refits of tests/acquire_ref.py, at the smallest shapes at which each part can go wrong:

    d3 p=5 m=1 k=1                       one row, one pick
    d3 p=5 m=63 / 64 / 65, k=12          the predictor's 64-row tile edge
    d3 p=5 m=255 / 256 / 257, k=3        k_acq_update's 256-row workgroup edge
    d3 p=5 m=66 000 k=2                  more than 256 partial pairs: k_acq_pick's strided loop
    d8 p=67 m=65 k=65 and k=70           candidates run out: n_picked = 65, success
    d5 p=130 m=129 k=12; m=1000 k=12     several workgroups, twelve downdates
    d=40 p=357, 198 used columns, m=65 k=3        beyond the star and tile predictors' comfort
    mat25 x 20, p=2500, levels <= 12, m=300 k=3   the pass is k_star_predict

Every case but the last runs the four criteria x {believer, constant} x both directions, on the predictor's own
route and again under OBHIP_FORCE_GENERIC; the two must return the same picks.  The conditions of the cases (top two
scores more than 1000 allowances apart, 8 r < C_CAP) are asserted on the reference alone by test_acquire_host.py and
again here before the device is looked at.  score, all m of score0, mean and var are held to the allowances of
acquire_ref.py, C eight times the float64 restatement's own err / bound on the same case; every check prints
err / tolerance.  Output buffers are padded and the padding must stay as it was.

The star case: the long-double factorisation at p = 2500 does not fit a few seconds, so that case is held to the
generic route of the same call (equal picks, values within the sum of the two routes' allowances taken with
C = C_CAP) and both routes to the float64 restatement on the oracle's B, within the same."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import acquire_ref as A
import extended_ref as E
from test_acquire_host import built, cfg_index, model

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 3
KEYS = ("index", "score", "score0", "mean", "var")


def posterior_of(om_d, terms, c):
    import outerbase_amd as ob
    return ob.Posterior.from_hessian(om_d, terms, c.H, c.sigma)


def dev_acquire(post, c, cfg, k, skip=None):
    """obhip_acquire_dev into padded buffers; the padding must come back untouched"""
    import torch
    from outerbase_amd._lib import call
    from outerbase_amd.design import ACQUISITIONS, LIES, _dev_cols, _stream
    dev = _stream()
    f64 = torch.float64
    dx = _dev_cols(c.xcand, dev)
    dth = torch.from_numpy(c.theta).to(dev)
    sk = c.skip if skip is None else np.asarray(skip) != 0
    dk = torch.from_numpy(np.ascontiguousarray(sk, dtype=np.uint8)).to(dev) if sk.any() else None
    index = torch.full((k + PAD,), -7, dtype=torch.int64, device=dev)
    score = torch.full((k + PAD,), NAN, dtype=f64, device=dev)
    score0, mean, var = (torch.full((c.m + PAD,), NAN, dtype=f64, device=dev) for _ in range(3))
    params = (C.c_double * 4)(cfg.best, cfg.xi, cfg.kappa, cfg.level)
    n = C.c_uint64(0)
    call("obhip_acquire_dev", post._h, dth.data_ptr(), dx.data_ptr(), c.m, ACQUISITIONS[cfg.criterion], params,
         int(cfg.maximize), LIES[cfg.lie], cfg.lie_value, None if dk is None else dk.data_ptr(), k, index.data_ptr(),
         score.data_ptr(), score0.data_ptr(), mean.data_ptr(), var.data_ptr(), C.byref(n))
    torch.cuda.synchronize()
    n = n.value
    index, score, score0, mean, var = (a.cpu().numpy() for a in (index, score, score0, mean, var))
    assert np.all(index[n:] == -7) and np.all(np.isnan(score[n:])), "index / score written beyond n_picked"
    for a in (score0, mean, var):
        assert np.all(np.isnan(a[c.m:])), "score0 / mean / var written beyond their end"
    return dict(index=index[:n], score=score[:n], score0=score0[:c.m], mean=mean[:c.m], var=var[:c.m], n_picked=n)


def set_route(monkeypatch, generic):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)


def check(label, b, got, gaps=True, exempt=()):
    """the conditions on the reference, then picks, then values"""
    c, st, picks = b["c"], b["st"], b["picks"]
    assert 8 * b["r"] < E.C_CAP, label
    if gaps:
        gap = A.gap_ratio(st, b["C"], exempt)
        assert gap > 1000, "%s: the top two scores are %.3g allowances apart: choose another seed" % (label, gap)
    assert got["n_picked"] == len(picks), label
    assert list(got["index"]) == picks, label
    w = A.ratios(got, st, b["C"])
    line = "acquire | %s: C %.3g (float64 restatement err/bound %.3g); device err/tolerance %s" % (
        label, b["C"], b["r"], ", ".join("%s %.3g" % kv for kv in w.items()))
    print(line)
    assert max(w.values()) < 1, line
    for key in ("score0", "mean", "var"):
        assert np.all(np.isnan(got[key][~c.finite])), key


ROUTES = {}


def run_case(label, b, k, generic, monkeypatch, **kw):
    """one route of one call; the second route to arrive is compared with the first: the same picks"""
    set_route(monkeypatch, generic)
    with posterior_of(b["om_d"], b["terms"], b["c"]) as post:
        got = dev_acquire(post, b["c"], b["cfg"], k)
    check("%s %r %s" % (label, b["cfg"], "generic" if generic else "own route"), b, got, **kw)
    other = ROUTES.setdefault((label, repr(b["cfg"])), (generic, got))
    if other[0] != generic:
        assert list(other[1]["index"]) == list(got["index"]), "the two routes pick differently"
    return got


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("ci", range(16))
@pytest.mark.parametrize("name,p,m,k,seed", A.SHAPES)
def test_picks_and_values_against_explicit_refits(name, p, m, k, seed, ci, generic, monkeypatch):
    b = built(name, p, m, k, seed, ci)
    assert len(b["picks"]) == min(k, m)                              # k = 70 of 65: n_picked = 65
    run_case("%s p=%d m=%d k=%d" % (name, p, m, k), b, k, generic, monkeypatch)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("ci", range(16))
def test_term_set_with_198_used_columns(ci, generic, monkeypatch):
    name, p, m, k, seed = A.WIDE
    b = built(name, p, m, k, seed, ci)
    run_case("wide d=40 p=%d used=198 m=%d k=%d" % (b["c"].p, m, k), b, k, generic, monkeypatch)


# ---- the star case ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def star_case():
    from conftest import knots_for
    from test_gpu_star import make_pair, share_info
    kinds = ["mat25"] * 20
    om_o, om_d = make_pair(kinds, knots_for(kinds, 40))
    terms = om_o.selectterms(3 * 2500)
    terms = np.ascontiguousarray(terms[terms.max(1) <= 12][:2500])
    assert len(terms) == 2500
    info = share_info(om_d, terms)
    assert 9 <= info["nswf"] <= 16 and info["nleft"] <= 192             # k_star's domain: the pass is k_star_predict
    c = A.seeded_case(om_o, terms, 300, 94)
    return c, om_d, terms, A.configs_of(c)


@pytest.mark.parametrize("crit", A.CRITERIA)
def test_star_predictor_pass_against_the_generic_route_and_the_float64_restatement(crit, monkeypatch):
    c, om_d, terms, cfgs = star_case()
    cfg = cfgs[cfg_index(crit, A.CONSTANT, False)]
    want = A.recurrence64(c, cfg, 3, bounds=True)
    assert want["n_picked"] == 3
    got = {}
    with posterior_of(om_d, terms, c) as post:
        for generic in (False, True):
            set_route(monkeypatch, generic)
            got[generic] = dev_acquire(post, c, cfg, 3)
    assert list(got[False]["index"]) == list(got[True]["index"]) == list(want["index"])
    st = want["states"]
    both = {key: float(np.max(np.abs(got[False][key] - got[True][key]) / (
        E.C_CAP * (st[3]["bound_mu"] if key == "mean" else st[3]["bound_d"])))) for key in ("mean", "var")}
    both["score0"] = float(np.max(np.abs(got[False]["score0"] - got[True]["score0"]) / (E.C_CAP * st[0]["bound_score"] + st[0]["rest_score"])))
    w = {generic: A.ratios(got[generic], st, E.C_CAP) for generic in (False, True)}
    print("acquire | star p=2500 m=300 k=3 %r: err / allowance (C = C_CAP) against the float64 restatement: own route %s, "
          "generic %s; one route against the other %s" % (cfg, w[False], w[True], both))
    assert max(both.values()) < 2                                       # the sum of the two routes' allowances
    assert max(max(v.values()) for v in w.values()) < 2


# ---- semantics --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def semantic(variant, ci):
    name, p, m, k, seed = A.SEMANTICS
    om_o, om_d, terms = model(name, p)
    from conftest import sample_x
    base = A.seeded_case(om_o, terms, m, seed)
    cfg = A.configs_of(base)[ci]
    xc, skip, extra = base.xcand.copy(), None, {}

    def case_of(xc, skip=None):
        c = A.seeded_case(om_o, terms, len(xc), seed, xcand=xc, skip=skip)
        c.theta, c.rhs0 = base.theta, base.rhs0
        return c
    if variant == "twin":                  # 300 rows: two workgroups of k_acq_update (rows 0-255 | 256-299)
        xc = np.concatenate([xc, sample_x(np.random.default_rng(seed + 7), 300 - m, om_o.kinds)])
        first = A.states(case_of(xc), cfg, None, 1)[0]
        w = first[0]                       # the best row of step 0 twice, bit for bit: its copy stands in the other
        twin = 256 + (w + 17) % 44 if w < 256 else (w + 17) % 64      # workgroup and at another place of its 64-row tile
        assert twin % 64 != w % 64 and (twin < 256) != (w < 256)
        xc[twin] = xc[w]
        extra = dict(lo=min(w, twin), hi=max(w, twin))
    else:
        first = A.states(base, cfg, None, 5)[0]
    if variant == "skip":                  # every winner of the plain run is skipped
        skip = np.zeros(m, dtype=bool)
        skip[first] = True
    elif variant == "nan":                 # the best candidate loses a coordinate
        xc[first[0], 1] = NAN
    c = case_of(xc, skip)
    picks, ystar, st = A.states(c, cfg, None, k)
    Cc, r = A.constant_of(c, cfg, st, picks)
    return dict(c=c, cfg=cfg, picks=picks, ystar=ystar, st=st, C=Cc, r=r, om_d=om_d, terms=terms, first=first, **extra)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("crit", A.CRITERIA)
def test_semantics(crit, generic, monkeypatch):
    set_route(monkeypatch, generic)
    route = "generic" if generic else "own route"
    ci = cfg_index(crit, A.CONSTANT, False)
    k = A.SEMANTICS[3]
    # two bit-identical candidates tie, the lower index is picked, and their outputs are the same bits
    b = semantic("twin", ci)
    lo, hi = b["lo"], b["hi"]
    assert b["picks"][0] == lo
    with posterior_of(b["om_d"], b["terms"], b["c"]) as post:
        got = dev_acquire(post, b["c"], b["cfg"], k)
    check("twin rows %s %s" % (crit, route), b, got, exempt=(hi,))
    assert got["index"][0] == lo
    for key in ("score0", "mean", "var"):
        assert np.array_equal(got[key][lo:lo + 1], got[key][hi:hi + 1]), key
    # with every winner skipped the runners-up come back
    b = semantic("skip", ci)
    assert not set(b["first"]) & set(b["picks"])
    with posterior_of(b["om_d"], b["terms"], b["c"]) as post:
        check("winners skipped %s %s" % (crit, route), b, dev_acquire(post, b["c"], b["cfg"], k))
        # all rows skipped: nothing is picked and the index / score padding is untouched
        none = dev_acquire(post, b["c"], b["cfg"], k, skip=np.ones(b["c"].m))
        assert none["n_picked"] == 0 and len(none["index"]) == 0
    # a candidate with a NaN coordinate is never picked, its outputs are NaN, the others are not disturbed
    b = semantic("nan", ci)
    assert b["first"][0] not in b["picks"] and not b["c"].finite[b["first"][0]]
    with posterior_of(b["om_d"], b["terms"], b["c"]) as post:
        check("nan row %s %s" % (crit, route), b, dev_acquire(post, b["c"], b["cfg"], k))


@pytest.mark.parametrize("generic", [False, True])
def test_underflow_of_ei_and_the_range_of_pi(generic, monkeypatch):
    set_route(monkeypatch, generic)
    name, p, m, k, seed = A.SEMANTICS
    b = built(name, p, m, k, seed, cfg_index(A.EI, A.BELIEVER, False))
    c = b["c"]
    mu0, sd0 = E._f64(b["st"][0]["mu"]), np.sqrt(E._f64(b["st"][0]["d"]))
    far = float(mu0.min() - 100.0 * sd0.max())                    # u < -100 everywhere: Phi and phi underflow
    with posterior_of(b["om_d"], b["terms"], c) as post:
        got = dev_acquire(post, c, A.Config(A.EI, best=far), 2)
        assert np.all(got["score0"] == 0.0) and list(got["index"]) == [0, 1] and np.all(got["score"] == 0.0)
        for best in (far, float(np.median(mu0)), float(mu0.max() + 100.0 * sd0.max())):
            pi = dev_acquire(post, c, A.Config(A.PI, best=best, lie=A.CONSTANT, lie_value=best), 3)
            assert np.all((pi["score0"] >= 0.0) & (pi["score0"] <= 1.0)) and np.all((pi["score"] >= 0.0) & (pi["score"] <= 1.0))


# ---- against the library itself ---------------------------------------------------------------------------
def test_believer_against_condition_and_predict():
    """the believer's variances are those of condition() on the picked rows, and its means are the predictor's"""
    import outerbase_amd as ob
    b = built("d5", 130, 129, 12, 90, cfg_index(A.LCB, A.BELIEVER, False))
    c, last = b["c"], b["st"][-1]
    with posterior_of(b["om_d"], b["terms"], c) as post:
        res = post.acquire(c.xcand, c.theta, k=12, criterion="lcb")
        assert list(res.index) == b["picks"] and res.n_picked == 12 and res.criterion == "lcb"
        with post.condition(c.xcand[res.index]) as cond:
            refit = cond.var(c.xcand)
    tol = b["C"] * last["bound_d"]
    r1, r2 = E.worst_ratio(refit, last["d"], tol), E.worst_ratio(res.var, last["d"], tol)
    r12 = float(np.max(np.abs(refit - res.var) / (2 * tol)))
    mean = ob.obmod._terms_of(b["om_d"], b["terms"])
    from outerbase_amd._lib import call, ptr
    x, pm = np.asfortranarray(c.xcand), np.empty(c.m)
    call("obhip_predict", b["om_d"]._h, mean._h, ptr(c.theta), ptr(x), c.m, c.m, ptr(pm), None, c.sigma, None)
    tm = b["C"] * b["st"][0]["bound_mu"]
    rm = float(np.max(np.abs(pm - res.mean) / (2 * tm)))
    print("acquire | believer: var refit by condition() err/tolerance %.3g, downdates %.3g, one against the other %.3g; "
          "mean against obhip_predict %.3g" % (r1, r2, r12, rm))
    assert r1 < 1 and r2 < 1 and r12 < 1 and rm < 1


def test_constant_liar_against_a_refit_with_the_fantasised_rows():
    """A NewtonAccumulator refit with the picked rows added at the lie.  The accumulator standardises over the rows
    it holds, so the lie is the centre of the real rows (0 in their standardised units): the fantasies then leave
    the centre where it is and only stretch the scale, y'_std = (sca / sca') [y_std; 0], and the refit's prediction
    times sca' / sca is, in the standardised units of the real rows, the mean the downdates left."""
    import ob_oracle as O
    import outerbase_amd as ob
    from conftest import sample_x
    from outerbase_amd._lib import call, ptr
    om_o, om_d, terms = model("d8", 67)
    rng = np.random.default_rng(43)
    x = sample_x(rng, 90, om_o.kinds)
    y = rng.standard_normal(90) * 3.0 + 7.0
    xc = sample_x(rng, 65, om_o.kinds)
    sigma, rho, k, p = math.log(0.1), 1.0, 5, len(terms)
    best = float(np.float32(-0.5))
    t = ob.obmod._terms_of(om_d, terms)
    xf = np.asfortranarray(xc)
    with ob.NewtonAccumulator(om_d, terms, 1) as acc:
        acc.add(x, y[:, None])
        fit = acc.fit(sigma, rho)
        theta = np.ascontiguousarray(fit.coeff[:, 0])
        cen, sca = float(fit.y_cent[0]), float(fit.y_sca[0])
        s = acc.state()
        with acc.posterior(sigma, rho) as post:
            res = post.acquire(xc, theta, k=k, criterion="ei", best=best, lie="constant", lie_value=0.0)
            assert res.n_picked == k
            raw = post.acquire(xc, theta, k=k, criterion="ei", best=cen + sca * best, lie="constant", lie_value=cen,
                               xi=0.0, response=0)
            lcb = post.acquire(xc, theta, k=k, criterion="lcb"), post.acquire(xc, theta, k=k, criterion="lcb", response=0)
            pi = post.acquire(xc, theta, k=k, criterion="pi", best=best), post.acquire(xc, theta, k=k, criterion="pi",
                                                                                       best=cen + sca * best, response=0)
        acc.add(xc[res.index], np.full((k, 1), cen))
        fit2 = acc.fit(sigma, rho)
        assert abs(float(fit2.y_cent[0]) - cen) <= 4 * E.U * abs(cen)
        th2, pm = np.ascontiguousarray(fit2.coeff[:, 0]), np.empty(65)
        call("obhip_predict", om_d._h, t._h, ptr(th2), ptr(xf), 65, 65, ptr(pm), None, sigma, None)
        refit = pm * (float(fit2.y_sca[0]) / sca)
    G = np.zeros((p, p))
    G[np.triu_indices(p)] = s["tri"]
    G = G + np.triu(G, 1).T
    H = math.exp(-2 * sigma) * G + np.diag(O.prior_prec(om_o, terms, rho))
    c = A.make_case(om_o, terms, H, sigma, theta, xc)
    cfg = A.Config(A.EI, best=best, lie=A.CONSTANT, lie_value=0.0)
    picks, ystar, st = A.states(c, cfg, list(res.index), k)
    Cc, r = A.constant_of(c, cfg, st, picks)
    got = dict(index=res.index, score=res.score, score0=res.score0, mean=res.mean, var=res.var, n_picked=k)
    w = A.ratios(got, st, Cc)
    # the device within its allowance, the refit (another float64 route without a measured constant) within C_CAP's
    rr = float(np.max(np.abs(refit - res.mean) / ((Cc + E.C_CAP) * st[-1]["bound_mu"])))
    print("acquire | constant liar on an accumulator's posterior: C %.3g; err/tolerance %s; mean against the refit %.3g"
          % (Cc, w, rr))
    assert max(w.values()) < 1 and rr < 1
    # response=0: raw units in, raw units out, the same picks; PI has no unit
    assert list(raw.index) == list(res.index) and list(pi[0].index) == list(pi[1].index) and list(lcb[0].index) == list(lcb[1].index)
    u8 = 8 * E.U
    assert np.all(np.abs(raw.mean - (cen + sca * res.mean)) <= u8 * (abs(cen) + sca * np.abs(res.mean)))
    assert np.all(np.abs(raw.var - sca ** 2 * res.var) <= u8 * sca ** 2 * res.var)
    assert np.all(np.abs(lcb[1].mean - (cen + sca * lcb[0].mean)) <= u8 * (abs(cen) + sca * np.abs(lcb[0].mean)))
    assert np.all(np.abs(lcb[1].score0 - (sca * lcb[0].score0 - cen)) <= u8 * (abs(cen) + sca * np.abs(lcb[0].score0)))
    # best = cen + sca * best_std is rounded on the way out and on the way back in: t moves by dt, EI by at most
    # Phi dt <= dt and PI by at most phi / sd dt <= 0.4 dt / sd
    dt = 4 * E.U * (abs(cen) / sca + abs(best))
    sd0 = np.sqrt(E._f64(st[0]["d"]))
    assert np.all(np.abs(raw.score0 - sca * res.score0) <= sca * (dt + u8 * np.abs(res.score0)))
    assert np.all(np.abs(pi[1].score0 - pi[0].score0) <= 0.4 * dt / sd0 + u8 * pi[0].score0)


def test_two_calls_return_the_same_bits():
    for ci in (cfg_index(A.EI, A.CONSTANT, False), cfg_index(A.STRADDLE, A.BELIEVER, True)):
        b = built("d5", 130, 1000, 12, 91, ci)
        with posterior_of(b["om_d"], b["terms"], b["c"]) as post:
            one, two = dev_acquire(post, b["c"], b["cfg"], 12), dev_acquire(post, b["c"], b["cfg"], 12)
        for key in KEYS:
            assert np.array_equal(one[key], two[key], equal_nan=True), key


def test_select_is_what_it_was_and_refused_calls_change_nothing():
    import torch
    from outerbase_amd._lib import lib
    b = built("d3", 5, 63, 12, 82, 0)
    c = b["c"]
    with posterior_of(b["om_d"], b["terms"], c) as post:
        with pytest.raises(ValueError):
            post.select(c.xcand, 2, criterion="ei")
        a = torch.full((64,), NAN, dtype=torch.float64, device="cuda")
        n = C.c_uint64(77)
        x = torch.from_numpy(np.ascontiguousarray(c.xcand.T)).cuda()
        par = (C.c_double * 4)(NAN, 0.0, 1.96, 0.0)
        f = lib.obhip_acquire_dev
        args = (post._h, a.data_ptr(), x.data_ptr(), c.m, 0, par, 0, 0, 0.0, None, 3, a.data_ptr(), a.data_ptr(),
                a.data_ptr(), a.data_ptr(), a.data_ptr(), C.byref(n))
        assert f(*args) == 1                                              # best is NaN
        torch.cuda.synchronize()
        assert n.value == 77 and bool(torch.isnan(a).all())
