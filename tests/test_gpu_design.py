"""The sequential design on the device (csrc/design.cpp, kernels_design.hip) against the long-double
explicit refits of tests/design_ref.py, at the smallest shapes at which the step can go wrong: p = 5 (one
partial 4-term step of the matrix instruction), 67 and 130; m = 1, 63, 64, 65, 129 around the 64-row tile
and 1000 (16 workgroups through the partial argmax); k = 1 and 12, k = m = 65 (every candidate taken) and
k = 70 of 65 (n_picked = 65); a d = 40 term set with 198 used columns in the tile.  Every case runs on
the fused kernel and again under OBHIP_FORCE_GENERIC (predictor to scratch, k_design_update), and the two
must return the same picks.

Before the device is looked at, every case asserts ON THE REFERENCE ALONE that the top two scores of every
step differ by more than 1000 allowances: only then are the picks determined, and then the device must
return the reference's picks, all of them.  Scores, all m variances and the trace are held to
C x (summands) x (magnitudes) of design_ref.py, C eight times the float64 restatement's own err / bound on
the same case; every check prints err / tolerance.  Output buffers are padded and the padding must stay
as it was."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import design_ref as D
import extended_ref as E
from test_sobol_host import d5_model, golden_model

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 3
CRITERIA = [D.MAXVAR, D.IMSE]


@functools.lru_cache(maxsize=None)
def model(name, p):
    mdl = {"d3": lambda: golden_model("mixed_d3"), "d8": lambda: golden_model("ref_basic_d8"), "d5": d5_model}[name]()
    terms = np.ascontiguousarray(mdl["om_o"].selectterms(p))
    assert len(terms) == p
    return mdl["om_o"], mdl["om_d"], terms


@functools.lru_cache(maxsize=None)
def wide_model():
    from test_gpu_predict_grad import wide
    kinds, om_o, om_d, terms, used, _ = wide()
    assert used == 198
    return om_o, om_d, np.ascontiguousarray(terms)


# (model, p, m, k asked for, seed)
SHAPES = [("d3", 5, 1, 1, 21), ("d3", 5, 63, 12, 22), ("d8", 67, 64, 12, 23), ("d8", 67, 65, 65, 24),
          ("d8", 67, 65, 70, 24), ("d5", 130, 129, 12, 25), ("d5", 130, 1000, 12, 26), ("d5", 130, 65, 1, 27)]


@functools.lru_cache(maxsize=None)
def built(name, p, m, k, seed, criterion, variant=None):
    """case, the reference along its own picks, C of the case -- computed once, shared by the fused and the
    unfused run and left unchanged"""
    om_o, om_d, terms = wide_model() if name == "wide" else model(name, p)
    kw = {}
    if variant is not None:
        from conftest import sample_x
        xc = sample_x(np.random.default_rng(seed), m, om_o.kinds)
        base = D.seeded_case(om_o, terms, m, criterion, seed, xcand=xc)
        first = D.states(base, None, 5)[0]
        if variant == "twin":                       # the best candidate twice, bit for bit, its copy in another
            xc[1 if first[0] >= 64 else 100] = xc[first[0]]   # workgroup of the fused kernel (rows 0-63 | 64-127)
        elif variant == "zero weights":             # what would be picked first is excluded
            kw["weights"] = np.ones(m)
            kw["weights"][first] = 0.0
        elif variant == "replace":                  # one candidate a million times the rest, replicates allowed
            kw["weights"] = np.ones(m)
            kw["weights"][7] = 1e6
            kw["replace"] = True
        elif variant == "nan":                      # the best candidate loses a coordinate
            xc[first[0], 1] = NAN
        kw["xcand"] = xc
    c = D.seeded_case(om_o, terms, m, criterion, seed, **kw)
    picks, st = D.states(c, None, k)
    Cc, r = D.constant_of(c, st, picks)
    return dict(c=c, picks=picks, st=st, C=Cc, r=r, om_d=om_d, terms=terms, first=None if variant is None else first)


def posterior_of(b):
    import outerbase_amd as ob
    return ob.Posterior.from_hessian(b["om_d"], b["terms"], b["c"].H, b["c"].sigma)


def dev_select(post, c, k):
    """obhip_design_select_dev into padded buffers; the padding must come back untouched"""
    import torch
    from outerbase_amd._lib import call
    from outerbase_amd.design import CRITERIA as CODE, _dev_cols, _stream
    dev = _stream()
    f64 = torch.float64
    imse = c.criterion == D.IMSE
    dx = _dev_cols(c.xcand, dev)
    dr = _dev_cols(c.xref, dev) if imse else None
    du = torch.from_numpy(c.u).to(dev) if imse else None
    dw = torch.from_numpy(c.w).to(dev)
    index = torch.full((k + PAD,), -7, dtype=torch.int64, device=dev)
    score = torch.full((k + PAD,), NAN, dtype=f64, device=dev)
    var = torch.full((c.m + PAD,), NAN, dtype=f64, device=dev)
    trace = torch.full((k + 1 + PAD,), NAN, dtype=f64, device=dev)
    n = C.c_uint64(0)
    call("obhip_design_select_dev", post._h, dx.data_ptr(), c.m, CODE[c.criterion], None if dr is None else dr.data_ptr(),
         c.r, None if du is None else du.data_ptr(), dw.data_ptr(), k, int(c.replace), index.data_ptr(),
         score.data_ptr(), var.data_ptr(), trace.data_ptr(), C.byref(n))
    torch.cuda.synchronize()
    n = n.value
    index, score, var, trace = (a.cpu().numpy() for a in (index, score, var, trace))
    assert np.all(index[n:] == -7) and np.all(np.isnan(score[n:])), "index / score written beyond n_picked"
    assert np.all(np.isnan(var[c.m:])) and np.all(np.isnan(trace[n + 1:])), "var / trace written beyond their end"
    return dict(index=index[:n], score=score[:n], var=var[:c.m], trace=trace[:n + 1], n_picked=n, num=None)


def set_route(monkeypatch, generic):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)


def check(label, b, got, gaps=True):
    """picks, then values"""
    c, st, picks = b["c"], b["st"], b["picks"]
    if gaps:
        gap = D.gap_ratio(st, b["C"])
        assert gap > 1000, "%s: the top two scores are %.3g allowances apart: choose another seed" % (label, gap)
    assert got["n_picked"] == len(picks), label
    assert list(got["index"]) == picks, label
    w = D.ratios(got, st, b["C"])
    line = "design | %s: C %.3g (float64 restatement err/bound %.3g); device err/tolerance %s" % (
        label, b["C"], b["r"], ", ".join("%s %.3g" % kv for kv in w.items()))
    print(line)
    assert max(w.values()) < 1, line
    assert np.all(np.isnan(got["var"][~c.finite]))


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("criterion", CRITERIA)
@pytest.mark.parametrize("name,p,m,k,seed", SHAPES)
def test_picks_and_values_against_explicit_refits(name, p, m, k, seed, criterion, generic, monkeypatch):
    set_route(monkeypatch, generic)
    b = built(name, p, m, k, seed, criterion)
    assert len(b["picks"]) == min(k, m)                              # k = 70 of 65: n_picked = 65
    with posterior_of(b) as post:
        got = dev_select(post, b["c"], k)
    check("%s p=%d m=%d k=%d %s %s" % (name, p, m, k, criterion, "unfused" if generic else "fused"), b, got)


@pytest.mark.parametrize("generic", [False, True])
def test_term_set_with_198_used_columns(generic, monkeypatch):
    set_route(monkeypatch, generic)
    b = built("wide", 0, 65, 3, 31, D.MAXVAR)
    with posterior_of(b) as post:
        got = dev_select(post, b["c"], 3)
    check("wide d=40 p=%d used=198 m=65 k=3 %s" % (b["c"].p, "unfused" if generic else "fused"), b, got)


@pytest.mark.parametrize("criterion", CRITERIA)
def test_against_the_library_itself(criterion):
    """conditioning on the picked rows through the Gram path gives the variances the downdates left; and the
    handle's variance is obhip_predict_std's without the noise"""
    import outerbase_amd as ob
    from outerbase_amd._lib import call, ptr
    b = built("d5", 130, 129, 12, 25, criterion)
    c, last = b["c"], b["st"][-1]
    with posterior_of(b) as post:
        res = post.select(c.xcand, 12, criterion=criterion, reference=getattr(c, "xref", None),
                          ref_weights=getattr(c, "u", None))
        assert list(res.index) == b["picks"]
        with post.condition(c.xcand[res.index]) as cond:
            refit = cond.var(c.xcand)
            gain = cond.logdet - post.logdet
        tol = b["C"] * last["bound_d"]
        r1, r2 = E.worst_ratio(refit, last["d"], tol), E.worst_ratio(res.var, last["d"], tol)
        r12 = float(np.max(np.abs(refit - res.var) / (2 * tol)))
        print("design | %s: refit by condition() err/tolerance %.3g, downdates %.3g, one against the other %.3g" % (
            criterion, r1, r2, r12))
        assert r1 < 1 and r2 < 1 and r12 < 1
        if criterion == D.MAXVAR:                   # greedy D-optimality: the trace is the growth of log det H
            assert abs(gain - res.trace[-1]) <= b["C"] * last["bound_trace"] + 4 * E.U * c.p * abs(post.logdet)
        v0, v1 = post.var(c.xcand), post.var(c.xcand, noise=True)
        x = np.asfortranarray(c.xcand)
        mean, std = np.empty(c.m), np.full(c.m, NAN)
        t = ob.obmod._terms_of(b["om_d"], b["terms"])
        theta, H = np.zeros(c.p), np.asfortranarray(c.H)                 # named: alive until the call returns
        call("obhip_predict_std", b["om_d"]._h, t._h, ptr(theta), ptr(H), ptr(x), c.m, c.m, ptr(mean), c.sigma, ptr(std))
        nu = math.exp(2 * c.sigma)
        assert np.array_equal(v1, std)                                # the same kernels on the same H
        assert np.all(np.abs(v0 - (std - nu)) <= 4 * E.U * (v0 + nu))
        assert abs(post.logdet - float(b["st"][0]["logdet"])) <= 64 * E.U * c.p * max(abs(post.logdet), c.p)


def test_accumulator_route_forms_the_hessian_of_the_solve():
    """acc.posterior(sigma, rho) against from_hessian of the exported state: the same variances"""
    import ob_oracle as O
    import outerbase_amd as ob
    from conftest import sample_x
    om_o, om_d, terms = model("d8", 67)
    rng = np.random.default_rng(41)
    x = sample_x(rng, 90, om_o.kinds)
    Y = rng.standard_normal((90, 2)) * np.array([1.0, 50.0]) + np.array([0.0, 7.0])
    xnew = sample_x(rng, 65, om_o.kinds)
    sigma, rho = math.log(0.1), 1.0
    with ob.NewtonAccumulator(om_d, terms, 2) as acc:
        acc.add(x, Y)
        s = acc.state()
        p = len(terms)
        G = np.zeros((p, p))
        G[np.triu_indices(p)] = s["tri"]
        G = G + np.triu(G, 1).T
        H = math.exp(-2 * sigma) * G + np.diag(O.prior_prec(om_o, terms, rho))
        c = D.make_case(om_o, terms, H, sigma, xnew, D.MAXVAR)
        _, st = D.states(c, [], 0)
        Cc, r = D.constant_of(c, st, [])
        tol = Cc * st[0]["bound_d"]
        with acc.posterior(sigma, rho) as pa, ob.Posterior.from_hessian(om_d, terms, H, sigma) as ph:
            va, vh = pa.var(xnew), ph.var(xnew)
            fit = acc.fit(sigma, rho)
            assert np.array_equal(pa.meansd[:, :2], np.stack([fit.y_cent, fit.y_sca], axis=1))
            assert pa.meansd[1, 1] > 10 * pa.meansd[0, 1]            # raw-unit variances: var * meansd[j, 1] ** 2
            ra, rh = E.worst_ratio(va, st[0]["d"], tol), E.worst_ratio(vh, st[0]["d"], tol)
            rr = float(np.max(np.abs(va - vh) / (2 * tol)))
            print("design | accumulator route p=%d: C %.3g (err/bound %.3g); err/tolerance acc %.3g, from_hessian %.3g, "
                  "one against the other %.3g" % (p, Cc, r, ra, rh, rr))
            assert ra < 1 and rh < 1 and rr < 1
            assert abs(pa.logdet - ph.logdet) <= 64 * E.U * p * max(abs(ph.logdet), p)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("criterion", CRITERIA)
def test_semantics(criterion, generic, monkeypatch):
    set_route(monkeypatch, generic)
    route = "unfused" if generic else "fused"
    # two bit-identical candidates tie and the lower index is picked
    b = built("d5", 130, 129, 3, 51, criterion, "twin")
    lo, hi = sorted([b["first"][0], 1 if b["first"][0] >= 64 else 100])
    assert b["picks"][0] == lo and hi not in b["picks"]                 # the twin is spent with it
    with posterior_of(b) as post:
        check("twin rows %s %s" % (criterion, route), b, dev_select(post, b["c"], 3), gaps=False)
    # rows of weight 0 are never picked
    b = built("d5", 130, 129, 5, 52, criterion, "zero weights")
    assert not set(b["first"]) & set(b["picks"])
    with posterior_of(b) as post:
        check("zero weights %s %s" % (criterion, route), b, dev_select(post, b["c"], 5))
    # with replacement a row may be picked again; after one pick its variance is d nu / (nu + d)
    b = built("d5", 130, 129, 3, 53, criterion, "replace")
    assert b["picks"] == [7, 7, 7]
    with posterior_of(b) as post:
        got = dev_select(post, b["c"], 3)
        check("replace %s %s" % (criterion, route), b, got)
        one = dev_select(post, b["c"], 1)
    d0, nu = b["st"][0]["d"][7], b["c"].nu
    assert abs(float(one["var"][7] - d0 * nu / (nu + d0))) <= b["C"] * b["st"][1]["bound_d"][7]
    # a candidate with a NaN coordinate is never picked and does not disturb the others
    b = built("d5", 130, 129, 5, 54, criterion, "nan")
    assert b["first"][0] not in b["picks"]
    with posterior_of(b) as post:
        check("nan row %s %s" % (criterion, route), b, dev_select(post, b["c"], 5))


@pytest.mark.parametrize("criterion", CRITERIA)
def test_two_calls_return_the_same_bits(criterion):
    b = built("d5", 130, 1000, 12, 26, criterion)
    with posterior_of(b) as post:
        one, two = dev_select(post, b["c"], 12), dev_select(post, b["c"], 12)
    for key in ("index", "score", "var", "trace"):
        assert np.array_equal(one[key], two[key]), key


def test_refused_calls_change_nothing_and_bad_reference_weights_are_numeric_errors():
    import torch
    from outerbase_amd._lib import lib
    b = built("d3", 5, 63, 12, 22, D.IMSE)
    c = b["c"]
    with posterior_of(b) as post:
        a = torch.full((64,), NAN, dtype=torch.float64, device="cuda")
        n = C.c_uint64(77)
        x = torch.from_numpy(np.ascontiguousarray(c.xcand.T)).cuda()
        f = lib.obhip_design_select_dev
        assert f(post._h, x.data_ptr(), c.m, 1, None, 0, None, None, 3, 0, a.data_ptr(), a.data_ptr(), a.data_ptr(),
                 a.data_ptr(), C.byref(n)) == 1
        assert f(post._h, x.data_ptr(), c.m, 0, None, 0, None, None, 0, 0, a.data_ptr(), a.data_ptr(), a.data_ptr(),
                 a.data_ptr(), C.byref(n)) == 1
        torch.cuda.synchronize()
        assert n.value == 77 and bool(torch.isnan(a).all())
        for bad in (-0.5, NAN, float("inf")):
            u = c.u.copy()
            u[3] = bad
            with pytest.raises(Exception) as e:
                post.select(c.xcand, 3, criterion="imse", reference=c.xref, ref_weights=u)
            assert getattr(e.value, "code", None) == 5
        with pytest.raises(Exception) as e:
            post.select(c.xcand, 3, criterion="imse", reference=c.xref, ref_weights=np.zeros(c.r))
        assert getattr(e.value, "code", None) == 5
    import outerbase_amd as ob
    with pytest.raises(ob.ObhipError) as e:                              # not positive definite
        ob.Posterior.from_hessian(b["om_d"], b["terms"], -np.eye(c.p), c.sigma)
    assert e.value.code == 5
