"""The acquisition picks over several responses on the device (csrc/acquire_multi.cpp, kernels_acquire_multi.hip)
against the long-double explicit refits of tests/acquire_multi_ref.py, at the smallest shapes that cross the kernels'
seams: the d = 5, p = 130 term set with m = 300 candidates (two 256-row workgroups of k_macq_update, the second one
ragged, five 64-row predictor tiles) and k = 5, and m = 1 and m = 257.

The conditions of the cases (constant not capped, the top two scores of every step more than one allowance apart, every
believed-feasibility decision further from its limit than the mean's allowance) are asserted on the reference alone by
test_acquire_multi_host.py and again here before the device is looked at, so the picks must be EQUAL at every step;
score, all m of score0 and pof0, the m x q means, var, the final front and the incumbent are held to the allowances of
acquire_multi_ref.py, C eight times the float64 restatement's own err / bound on the same case.  Every check prints
err / tolerance.  Output buffers are padded and the padding must stay as it was."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import acquire_multi_ref as M
import acquire_ref as A
import extended_ref as E
from test_acquire_host import model
from test_acquire_multi_host import built, conditions, main_built, mcase

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 3
CRIT = {M.CEI: 0, M.CPI: 1, M.POF: 2, M.EHVI: 3}


def posterior_of(om_d, terms, c):
    import outerbase_amd as ob
    return ob.Posterior.from_hessian(om_d, terms, c.H, c.sigma)


def dev_multi(post, mc, cfg, k, skip=None, xcand=None, expect=0):
    """obhip_acquire_multi_dev into padded buffers; the padding must come back untouched.  front and best SIGNED.
    expect=1: the call must be refused and every output must come back as it went in"""
    import torch
    from outerbase_amd._lib import lib
    from outerbase_amd.design import LIES, _dev_cols, _stream
    dev = _stream()
    f64 = torch.float64
    c, q = mc.c, cfg.q
    x = c.xcand if xcand is None else xcand
    m = len(x)
    dx = _dev_cols(x, dev)
    dth = torch.from_numpy(np.ascontiguousarray(mc.Theta.T)).to(dev)
    sk = c.skip if skip is None else np.asarray(skip) != 0
    dk = torch.from_numpy(np.ascontiguousarray(sk, dtype=np.uint8)).to(dev) if sk.any() else None
    index = torch.full((k + PAD,), -7, dtype=torch.int64, device=dev)
    score = torch.full((k + PAD,), NAN, dtype=f64, device=dev)
    score0, pof0, var = (torch.full((m + PAD,), NAN, dtype=f64, device=dev) for _ in range(3))
    mean = torch.full((q * m + PAD,), NAN, dtype=f64, device=dev)
    F0 = len(cfg.front)
    fout = np.full(2 * (F0 + k) + PAD, NAN)
    roles = np.ascontiguousarray(cfg.role, dtype=np.int32)
    signs, limits, lv = (np.ascontiguousarray(v, dtype=np.float64) for v in (cfg.g, cfg.limits(), cfg.lie_value))
    fr = np.ascontiguousarray(cfg.front)
    n, nf, bo = C.c_uint64(99), C.c_uint64(98), C.c_double(97.0)
    rc = lib.obhip_acquire_multi_dev(post._h, dth.data_ptr(), q, dx.data_ptr(), m, CRIT[cfg.criterion], roles.ctypes.data,
                                     signs.ctypes.data, limits.ctypes.data, cfg.xi, fr.ctypes.data if F0 else None, F0,
                                     LIES[cfg.lie], lv.ctypes.data, None if dk is None else dk.data_ptr(), k,
                                     index.data_ptr(), score.data_ptr(), score0.data_ptr(), pof0.data_ptr(), mean.data_ptr(),
                                     var.data_ptr(), fout.ctypes.data, C.byref(nf), C.byref(bo), C.byref(n))
    torch.cuda.synchronize()
    assert rc == expect, lib.obhip_last_error()
    index, score, score0, pof0, mean, var = (a.cpu().numpy() for a in (index, score, score0, pof0, mean, var))
    if expect:
        assert (n.value, nf.value, bo.value) == (99, 98, 97.0) and np.all(index == -7) and np.all(np.isnan(fout))
        assert all(np.all(np.isnan(a)) for a in (score, score0, pof0, mean, var)), "a refused call wrote an output"
        return lib.obhip_last_error()
    n = n.value
    assert np.all(index[n:] == -7) and np.all(np.isnan(score[n:])), "index / score written beyond n_picked"
    for a in (score0, pof0, var):
        assert np.all(np.isnan(a[m:])), "score0 / pof0 / var written beyond their end"
    assert np.all(np.isnan(mean[q * m:]))
    F = nf.value if cfg.criterion == M.EHVI else 0
    assert np.all(np.isnan(fout[2 * F:])), "front written beyond n_front"
    front = fout[:2 * F].reshape(-1, 2) * np.array([cfg.g[j] for j in cfg.objs[:2]]) if F else np.zeros((0, 2))
    best = cfg.g[cfg.objs[0]] * bo.value if cfg.criterion in (M.CEI, M.CPI) else None
    return dict(index=index[:n], score=score[:n], score0=score0[:m], pof0=pof0[:m], mean=mean[:q * m].reshape(q, m).T.copy(),
                var=var[:m], front=front, best=best, n_picked=n)


def same_bits(a, b):
    """two results of dev_multi agree bit for bit (NaN with NaN; best may be None)"""
    for key in a:
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, key
        else:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key


def set_route(monkeypatch, generic):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)


def check(label, b, got, exempt=()):
    """the conditions on the reference, then picks, then values"""
    c, cfg, st, picks = b["mc"].c, b["cfg"], b["st"], b["picks"]
    conditions(label, b, len(picks), exempt)
    assert got["n_picked"] == len(picks), label
    assert list(got["index"]) == picks, label
    w = M.ratios(got, st, cfg, b["C"])
    line = "acquire_multi | %s: C %.3g (float64 restatement err/bound %.3g); device err/tolerance %s" % (
        label, b["C"], b["r"], ", ".join("%s %.3g" % kv for kv in w.items()))
    print(line)
    assert max(w.values()) < 1, line
    for key in ("score0", "pof0", "var"):
        assert np.all(np.isnan(got[key][~c.finite])), key
    return w


def run_built(b, k, generic=False, monkeypatch=None, **kw):
    if monkeypatch is not None:
        set_route(monkeypatch, generic)
    with posterior_of(b["om_d"], b["terms"], b["mc"].c) as post:
        return dev_multi(post, b["mc"], b["cfg"], k, **kw)


# ---- 1. picks and values against explicit refits -----------------------------------------------------------
@pytest.mark.parametrize("q", (1, 2, 4))
@pytest.mark.parametrize("lie", A.LIES)
@pytest.mark.parametrize("criterion", M.CRITERIA)
def test_picks_and_values_against_explicit_refits(criterion, lie, q):
    b = main_built(q, criterion, lie)
    if b is None:
        assert criterion == M.EHVI and q == 1                     # two objectives need two responses
        return
    check(repr(b["cfg"]), b, run_built(b, M.SHAPE[3]))


@pytest.mark.parametrize("criterion", [M.CEI, M.EHVI])
def test_generic_predictor_route(criterion, monkeypatch):
    """the predictor's route is the only thing OBHIP_FORCE_GENERIC changes: the same picks, values within the allowances"""
    b = main_built(4, criterion, A.CONSTANT)
    own = run_built(b, M.SHAPE[3], False, monkeypatch)
    gen = run_built(b, M.SHAPE[3], True, monkeypatch)
    check("%r generic" % b["cfg"], b, gen)
    assert list(own["index"]) == list(gen["index"])


@pytest.mark.parametrize("m", [1, 257])
@pytest.mark.parametrize("criterion", [M.CEI, M.EHVI])
def test_one_row_and_one_row_past_a_workgroup(criterion, m):
    name, p, _, k = M.SHAPE
    b = built(name, p, m, k, M.SEED + 50 + m, 2, criterion, A.CONSTANT)
    assert len(b["picks"]) == min(k, m)
    check("m=%d %r" % (m, b["cfg"]), b, run_built(b, k))


# ---- 2. fronts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F0", [0, 1, 7])
def test_initial_fronts(F0):
    b = main_built(2, M.EHVI, A.BELIEVER, F0=F0)
    assert len(b["cfg"].front) == F0
    check("F0=%d %r" % (F0, b["cfg"]), b, run_built(b, M.SHAPE[3]))


@functools.lru_cache(maxsize=None)
def messy_front_case():
    """the front of the F0 = 3 call with a dominated point, a duplicate and a point outside the box added, shuffled"""
    base = main_built(2, M.EHVI, A.BELIEVER)
    cfg0 = base["cfg"]
    f = np.array(cfg0.front)
    g = np.array([cfg0.g[j] for j in cfg0.objs])
    worse = f[0] + g * 0.25                                             # dominated by point 0 (worse in both signed coordinates)
    outside = np.array(cfg0.ref) + g * 0.5
    front = np.array([worse, f[0], outside, f[1], f[0], f[2]])
    cfg = M.MConfig(M.EHVI, 2, objs=cfg0.objs, maximize=cfg0.maximize, ref=cfg0.ref, front=front, lie=cfg0.lie, lie_value=cfg0.lie_value)
    return base, cfg


def test_front_with_a_dominated_point_a_duplicate_and_a_point_outside_the_box():
    """the host normalises it to the front of the clean call: every output carries the clean call's bits"""
    base, cfg = messy_front_case()
    k = M.SHAPE[3]
    assert [(p[0], p[1]) for p in M.pareto(cfg.points0, cfg.r)] == [(p[0], p[1]) for p in M.pareto(base["cfg"].points0, cfg.r)]
    assert len(M.pareto(cfg.points0, cfg.r)) < 6
    with posterior_of(base["om_d"], base["terms"], base["mc"].c) as post:
        clean = dev_multi(post, base["mc"], base["cfg"], k)
        messy = dev_multi(post, base["mc"], cfg, k)
    check("clean front", base, clean)
    same_bits(clean, messy)


def test_believer_picks_extend_the_front_and_knock_a_point_out():
    """the reference does both within one call (asserted on the reference), and the device's final front agrees"""
    found = None
    for F0 in (3, 7, 1):
        for q in (2, 4):
            b = main_built(q, M.EHVI, A.BELIEVER, F0=F0)
            grew = lost = False
            for s0, s1 in zip(b["st"][:-1], b["st"][1:]):
                a, c = {(p[0], p[1]) for p in s0["front"]}, {(p[0], p[1]) for p in s1["front"]}
                grew, lost = grew or bool(c - a), lost or bool(a - c)
            if grew and lost and found is None:
                found = b
    assert found is not None, "no committed call extends the front and knocks a point out: choose another seed"
    w = check("front moves %r" % found["cfg"], found, run_built(found, M.SHAPE[3]))
    assert "front" in w


def test_front_at_capacity_and_beyond():
    """F0 + k = 2048 with m = 64: synthetic front points far from the means (a staircase far on the good side of the
    first objective would dominate everything, so it stands far on its poor side, inside a far reference point);
    F0 + k = 2049 is refused"""
    name, p, _, _ = M.SHAPE
    mc, om_d, terms = mcase(name, p, 64, M.SEED + 9, 2)
    base = M.config_of(mc, M.EHVI, A.BELIEVER, F0=0)
    g = np.array([base.g[j] for j in base.objs])
    k, F0 = 2, 2046
    i = np.arange(F0, dtype=np.float64)
    signed = np.column_stack([40.0 + i / 64, 80.0 - i / 64])            # undominated among themselves, exact in float64
    ref = g * np.array([100.0, 100.0])

    def cfg_of(F):
        return M.MConfig(M.EHVI, 2, objs=base.objs, maximize=base.maximize, ref=ref, front=(signed * g)[:F], lie=A.BELIEVER)
    cfg = cfg_of(F0)
    assert len(M.pareto(cfg.points0, cfg.r)) == F0
    with posterior_of(om_d, terms, mc.c) as post:
        got = dev_multi(post, mc, cfg, k)
        msg = dev_multi(post, mc, M.MConfig(M.EHVI, 2, objs=base.objs, maximize=base.maximize, ref=ref,
                                            front=np.concatenate([signed * g, [[39.0 * g[0], 90.0 * g[1]]]]), lie=A.BELIEVER), k, expect=1)
    assert b"2048" in msg
    # The means are of order one: every candidate dominates the whole staircase, and the first believer pick empties the
    # front.  Every row times 2047 strips is beyond mpmath in a few seconds: the reference evaluates the rows near the
    # top (the picks among them) and leaves the others at the float64 restatement's value, so score0 and pof0 are held
    # to the sum of the two float64 routes' allowances there, the picked scores and everything else to one
    want = M.recurrence64(mc, cfg, k)
    assert list(got["index"]) == list(want["index"]) and got["n_picked"] == k
    picks, _, st = M.states(mc, cfg, list(want["index"]), k, full0=False)
    assert [s["best"] for s in st[:-1]] == picks
    Cc, r = M.constant_of(mc, cfg, st, picks)
    assert 8 * r < E.C_CAP and M.gap_ratio(st, Cc) > 1
    w = M.ratios(got, st, cfg, Cc)
    print("acquire_multi | capacity F0=%d k=%d: C %.3g; device err/tolerance %s" % (F0, k, Cc, w))
    assert max(v for key, v in w.items() if key not in ("score0", "pof0")) < 1 and w["score0"] < 2 and w["pof0"] < 2
    assert len(got["front"]) == len(st[-1]["front"]) <= 2


# ---- 3. the switch in mid-batch ---------------------------------------------------------------------------
def test_cei_without_an_incumbent_switches_in_mid_batch():
    found = None
    for q in (2, 4):
        for lie in A.LIES:
            b = main_built(q, M.CEI, lie, best=False)
            feas = [s["feasible"] for s in b["st"][:-1]]
            if True in feas[:-1] and found is None:
                found = b
    assert found is not None, "no committed call has a believed-feasible pick before its last: choose another seed"
    b = found
    got = run_built(b, M.SHAPE[3])
    check("no incumbent %r" % b["cfg"], b, got)
    assert np.array_equal(got["score0"], got["pof0"], equal_nan=True)                   # bit for bit: base = 1
    first = [s["feasible"] for s in b["st"][:-1]].index(True)
    later = b["st"][first + 1]
    assert math.isfinite(float(later["incumbent"])) and math.isinf(float(b["st"][first]["incumbent"]))
    assert math.isfinite(got["best"])
    j = b["picks"][first + 1]                                                           # constrained EI on the new incumbent:
    assert float(later["raw"][j]) < float(later["pof"][j]) or float(later["pof"][j]) == 0   # EI of order sd < 1 times pof


def test_incumbent_stays_infinite_when_no_pick_is_believed_feasible():
    b0 = main_built(2, M.CEI, A.BELIEVER, best=False)
    mc, cfg0 = b0["mc"], b0["cfg"]
    mu = mc.c.Bo @ mc.Theta
    cfg = M.MConfig(M.CEI, 2, objs=[0], maximize=[True], constraints=[(1, "<=", float(np.float32(mu[:, 1].min() - mu[:, 1].std())))],
                    best=None, xi=cfg0.xi, lie=A.BELIEVER)
    k = M.SHAPE[3]
    picks, _, st = M.states(mc, cfg, None, k)
    assert not any(s["feasible"] for s in st[:-1])
    Cc, r = M.constant_of(mc, cfg, st, picks)
    b = dict(b0, cfg=cfg, st=st, picks=picks, C=Cc, r=r)
    got = run_built(b, k)
    check("never feasible", b, got)
    assert got["best"] == math.inf                                       # signed: +inf, no feasible run to the end


# ---- 4. bit identities --------------------------------------------------------------------------------------
def single_acquire(post, c, theta, criterion, best, xi, maximize, lie, lie_value, k):
    from test_gpu_acquire import dev_acquire
    cfg = A.Config(criterion, best=best, xi=xi, maximize=maximize, lie=lie, lie_value=lie_value)
    keep = c.theta
    try:
        c.theta = theta
        return dev_acquire(post, c, cfg, k)
    finally:
        c.theta = keep


@pytest.mark.parametrize("lie", A.LIES)
@pytest.mark.parametrize("criterion,single", [(M.CEI, A.EI), (M.CPI, A.PI)])
def test_one_response_without_constraints_is_acquire_bit_for_bit(criterion, single, lie):
    b = main_built(1, criterion, lie)
    mc, cfg = b["mc"], b["cfg"]
    assert not cfg.cons and cfg.maximize == [True]
    k = M.SHAPE[3]
    with posterior_of(b["om_d"], b["terms"], mc.c) as post:
        multi = dev_multi(post, mc, cfg, k)
        again = dev_multi(post, mc, cfg, k)
        one = single_acquire(post, mc.c, mc.Theta[:, 0].copy(), single, cfg.best, cfg.xi, True, lie, float(cfg.lie_value[0]), k)
    for key in ("index", "score", "score0", "var"):
        assert np.array_equal(multi[key], one[key], equal_nan=True), key
    assert np.array_equal(multi["mean"][:, 0], one["mean"], equal_nan=True)
    same_bits(multi, again)                                                             # two calls: the same bits


def test_pof_of_one_constraint_is_pi_at_step_zero_and_two_calls_agree():
    """one response, so that the means are the one-response predictor's on both sides (with q > 1 they come from the
    multi-response predictor, another kernel and other bits)"""
    b = main_built(4, M.EHVI, A.BELIEVER)
    mc = b["mc"]
    j, lim = 1, b["cfg"].constraints[0][2]
    one_col = M.make_case(mc.c, mc.Theta[:, [j]].copy())
    cfg = M.MConfig(M.POF, 1, constraints=[(0, "<=", lim)])
    with posterior_of(b["om_d"], b["terms"], mc.c) as post:
        multi = dev_multi(post, one_col, cfg, 1)
        one = single_acquire(post, mc.c, mc.Theta[:, j].copy(), A.PI, lim, 0.0, False, A.BELIEVER, 0.0, 1)
        e1, e2 = dev_multi(post, mc, b["cfg"], 3), dev_multi(post, mc, b["cfg"], 3)
    assert np.array_equal(multi["score0"], one["score0"], equal_nan=True)
    assert np.array_equal(multi["pof0"], one["score0"], equal_nan=True)
    assert list(multi["index"]) == list(one["index"]) and np.array_equal(multi["score"], one["score"])
    same_bits(e1, e2)


@pytest.mark.parametrize("criterion", [M.CEI, M.EHVI])
def test_twin_rows_in_two_workgroups_tie_and_the_lower_index_wins(criterion):
    b = main_built(4, criterion, A.BELIEVER)
    mc, cfg = b["mc"], b["cfg"]
    w = b["picks"][0]
    twin = 256 + (w + 17) % 44 if w < 256 else (w + 17) % 64
    assert twin % 64 != w % 64 and (twin < 256) != (w < 256)
    x = mc.c.xcand.copy()
    x[twin] = x[w]
    with posterior_of(b["om_d"], b["terms"], mc.c) as post:
        got = dev_multi(post, mc, cfg, 2, xcand=x)
    assert got["score0"][w] == got["score0"][twin] and got["pof0"][w] == got["pof0"][twin]
    assert np.array_equal(got["mean"][w], got["mean"][twin]) and got["var"][w] == got["var"][twin]
    assert got["index"][0] == min(w, twin)


# ---- 5. semantics ---------------------------------------------------------------------------------------------
def test_skip_nan_and_nothing_eligible():
    b = main_built(2, M.CEI, A.BELIEVER)
    mc, cfg, picks = b["mc"], b["cfg"], b["picks"]
    m = mc.m
    x = mc.c.xcand.copy()
    x[picks[1], 2] = NAN
    skip = np.zeros(m, dtype=bool)
    skip[picks[0]] = True
    with posterior_of(b["om_d"], b["terms"], mc.c) as post:
        got = dev_multi(post, mc, cfg, 5, skip=skip, xcand=x)
        assert got["n_picked"] == 5 and picks[0] not in got["index"] and picks[1] not in got["index"]
        assert np.isnan(got["score0"][picks[1]]) and np.isnan(got["mean"][picks[1]]).all() and np.isfinite(got["score0"][picks[0]])
        few = np.ones(m, dtype=bool)
        few[[7, 260]] = False
        got = dev_multi(post, mc, cfg, 5, skip=few)
        assert got["n_picked"] == 2 and sorted(got["index"]) == [7, 260]              # fewer picks, no error
        got = dev_multi(post, mc, cfg, 5, skip=np.ones(m, dtype=bool))
        assert got["n_picked"] == 0


def test_scores_at_rows_conditioned_on_heavily_approach_the_sd_zero_branch():
    """A posterior conditioned 4000 times on each of three rows: sd there is about sqrt(nu / 4000).  score0 of a call on
    it is finite everywhere, and at those rows within E|HVI(y) - HVI(ms)| of the sd = 0 branch's value HVI(ms):
    HVI falls by at most (r2 - min(y2, ms2))+ per unit of y1 and likewise for y2, the coordinates are independent and
    E|y - ms| = E(ms - y)+ x 2 = sd sqrt(2 / pi) x .., so the distance is at most
    0.8 sd ((r1 - ms1)+ + (r2 - ms2)+ + 1.6 sd).  That the branch itself returns HVI(ms) is the host file's; a
    candidate whose downdated d is exactly <= 0 cannot be arranged from outside."""
    b = main_built(2, M.EHVI, A.BELIEVER)
    mc, cfg = b["mc"], b["cfg"]
    rows = b["picks"][:3]
    with posterior_of(b["om_d"], b["terms"], mc.c) as post:
        with post.condition(np.repeat(mc.c.xcand[rows], 4000, axis=0)) as heavy:
            got = dev_multi(heavy, mc, cfg, 1)
    assert np.all(np.isfinite(got["score0"])) and np.all(got["score0"] >= 0) and np.all(got["pof0"] == 1.0)
    front = [(float(p[0]), float(p[1])) for p in M.pareto(cfg.points0, cfg.r)]
    nu = math.exp(2 * mc.c.sigma)
    for i in rows:
        sd = math.sqrt(max(got["var"][i], 0.0))
        assert sd < 1.5 * math.sqrt(nu / 4000)
        y = (cfg.g[cfg.objs[0]] * got["mean"][i, cfg.objs[0]], cfg.g[cfg.objs[1]] * got["mean"][i, cfg.objs[1]])
        want = M.hvi(front, cfg.r, y)
        tol = 0.8 * sd * (max(cfg.r[0] - y[0], 0.0) + max(cfg.r[1] - y[1], 0.0) + 1.6 * sd)
        print("row %d: sd %.3g, score0 %.6g, HVI(ms) %.6g, distance / bound %.3g" % (i, sd, got["score0"][i], want, abs(got["score0"][i] - want) / tol))
        assert abs(got["score0"][i] - want) <= tol


def test_raw_units_round_trip_with_meansd():
    import outerbase_amd as ob
    b = main_built(4, M.EHVI, A.CONSTANT)
    mc, cfg = b["mc"], b["cfg"]
    b2 = main_built(4, M.CEI, A.CONSTANT)
    meansd = np.array([[1.5, 2.0, 40.0], [-3.0, 0.5, 40.0], [0.25, 4.0, 40.0], [10.0, 1.25, 40.0]])
    cen, sca = meansd[:, 0], meansd[:, 1]
    raw = lambda j, v: cen[j] + sca[j] * v
    k = M.SHAPE[3]
    for bb in (b, b2):
        cf = bb["cfg"]
        kw = dict(k=k, objective=cf.objs[0] if len(cf.objs) == 1 else tuple(cf.objs), maximize=cf.maximize,
                  lie=cf.lie, constraints=cf.constraints, xi=cf.xi)
        kr = dict(kw, constraints=[(j, op, raw(j, lim)) for j, op, lim in cf.constraints], lie_value=[raw(j, v) for j, v in enumerate(cf.lie_value)])
        kw["lie_value"] = list(cf.lie_value)
        if cf.criterion == M.EHVI:
            kw.update(ref=cf.ref, front=cf.front)
            kr.update(ref=[raw(j, v) for j, v in zip(cf.objs, cf.ref)], front=np.column_stack([raw(j, cf.front[:, a]) for a, j in enumerate(cf.objs)]))
            unit = sca[cf.objs[0]] * sca[cf.objs[1]]
        else:
            kw.update(best=cf.best)
            kr.update(best=raw(cf.objs[0], cf.best), xi=cf.xi * sca[cf.objs[0]])
            unit = sca[cf.objs[0]]
        with posterior_of(bb["om_d"], bb["terms"], mc.c) as post:
            std = post.acquire_multi(mc.c.xcand, mc.Theta, **kw)
            post.meansd = meansd
            got = post.acquire_multi(mc.c.xcand, mc.Theta, **kr)
        assert isinstance(std, ob.AcquireMultiResult) and std.criterion == cf.criterion
        assert list(std.index) == bb["picks"] == list(got.index)                       # the picks do not move
        assert np.allclose(got.score, unit * std.score, rtol=1e-9, atol=0) and np.allclose(got.score0, unit * std.score0, rtol=1e-9, atol=1e-300)
        assert np.allclose(got.pof0, std.pof0, rtol=1e-9, atol=1e-300)
        assert np.allclose(got.mean, cen + sca * std.mean, rtol=1e-9, atol=1e-9) and np.allclose(got.var, std.var, rtol=1e-9)
        assert np.array_equal(got.scale, sca) and np.array_equal(std.scale, np.ones(4))
        if cf.criterion == M.EHVI:
            assert got.front.shape == std.front.shape and np.allclose(got.front, cen[cf.objs] + sca[cf.objs] * std.front, rtol=1e-9, atol=1e-9)
        else:
            assert np.isclose(got.best, raw(cf.objs[0], std.best), rtol=1e-9)


# ---- 6. untouched neighbours --------------------------------------------------------------------------------
def test_refused_calls_change_nothing_and_the_neighbours_return_what_they_returned():
    b = main_built(2, M.CEI, A.BELIEVER)
    mc, cfg = b["mc"], b["cfg"]
    c = mc.c

    class Bad:
        """cfg with one field replaced"""
        def __init__(self, **kw):
            self.__dict__.update(cfg.__dict__)
            self._limits = cfg.limits()
            self.__dict__.update(kw)

        def limits(self):
            return self._limits
    two = M.MConfig(M.EHVI, 2, objs=[0, 1], maximize=[True, False], ref=[0.0, 0.0])
    with posterior_of(b["om_d"], b["terms"], c) as post:
        before = single_acquire(post, c, mc.Theta[:, 0].copy(), A.EI, cfg.best, cfg.xi, True, A.BELIEVER, 0.0, 3)
        sel = post.select(c.xcand, 3)
        assert b"q must be" in dev_multi(post, mc, Bad(q=0), 3, expect=1)
        wide = M.make_case(c, np.zeros((c.p, 17)))
        assert b"q must be" in dev_multi(post, wide, Bad(q=17, role=np.zeros(17), g=np.ones(17), _limits=np.zeros(17), lie_value=np.zeros(17)), 3, expect=1)
        assert b"takes 1 objectives" in dev_multi(post, mc, Bad(role=np.array([0, 0])), 3, expect=1)       # two objectives with CEI
        for bad in (NAN, math.inf):
            bt = Bad(criterion=M.EHVI, role=two.role, g=two.g, _limits=np.array([bad, 0.0]), objs=[0, 1], front=np.zeros((0, 2)))
            assert b"reference point" in dev_multi(post, mc, bt, 3, expect=1)
        from outerbase_amd._lib import lib
        roles, signs, lim = np.array([0, 1], dtype=np.int32), cfg.g.copy(), cfg.limits()
        n = C.c_uint64(5)
        assert lib.obhip_acquire_multi_dev(post._h, 1, 2, 1, c.m, 0, roles.ctypes.data, signs.ctypes.data, lim.ctypes.data, 0.0, None, 0,
                                           0, None, None, 3, None, None, None, None, None, None, None, None, None, C.byref(n)) == 1
        assert b"null outputs" in lib.obhip_last_error() and n.value == 5
        after = single_acquire(post, c, mc.Theta[:, 0].copy(), A.EI, cfg.best, cfg.xi, True, A.BELIEVER, 0.0, 3)
        sel2 = post.select(c.xcand, 3)
        good = dev_multi(post, mc, cfg, 3)
    for key in before:
        assert np.array_equal(np.asarray(before[key]), np.asarray(after[key]), equal_nan=True), key
    assert np.array_equal(sel.index, sel2.index) and np.array_equal(sel.score, sel2.score) and np.array_equal(sel.var, sel2.var)
    assert list(good["index"]) == b["picks"][:3]
    # and acquire's own reference still describes it
    cfg1 = A.Config(A.EI, best=cfg.best, xi=cfg.xi, maximize=True)
    keep = c.theta
    c.theta, c.rhs0 = mc.Theta[:, 0].copy(), mc.rhs0[:, 0].copy()
    try:
        picks, _, st = A.states(c, cfg1, None, 3)
        Cc, r = A.constant_of(c, cfg1, st, picks)
        assert list(before["index"]) == picks and max(A.ratios(before, st, Cc).values()) < 1
    finally:
        c.theta = keep
        c.rhs0 = np.array(c.H, dtype=np.longdouble) @ np.array(keep, dtype=np.longdouble)
