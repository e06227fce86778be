"""The matrix-free PCG (obhip_fit_cg, obhip_fit_cg_dev, lpdfvec.optcg: fit_cg_dev_impl and k_cg_* of
csrc/api.cpp) against the long double loop of tests/pcg_ref.py on the device's OWN design matrix
(getmat; pinned per entry in test_gpu_extended.py), so that what is compared is the loop and the
products as the loop uses them: every schedule (OBHIP_CG_REFRESH = 1, 2, 3, 5, unset = 16), every stop
path and the shapes of pcg_ref.CASES, each of which reaches another path:

  small      batched, cg_iter_regs, k_hm2             six        batched, k_hm2 with six factors
  rows17000  host in the loop, speculative product    p1...p1025 lane / element edges of cg_iter_regs
  p4096      last size in registers                   p4097      strided loops, no speculation, k_cg_q
  star300    k_star<OP_HESS> batched                  star2000   k_star<OP_HESS>, host in the loop
  small under OBHIP_FORCE_GENERIC: two-kernel product + k_cg_q; small through obhip_comm_init_sim(1 | 4):
  the sharded branch; OBHIP_HM3=0 and OBHIP_HESSMULT_FUSED=0 (read once per process): child processes.

Per run: the iteration count (the reference's, = maxit where the cap ends the loop), theta against the
long double iterate of that count, diagH, val_out against the long double value AT the returned
theta.  Bound on theta: max(32 err64, 1e-12), relative in the max norm, err64 = the float64 loop's own
distance from the long double iterate (same matrix, same count).

Measured on one MI355X: distance of the device's theta from the long double iterate under the default
schedule, per cap (tol = 0) and for the case's converging tolerance; `all R` = the largest distance over
every schedule and cap of the case, `err64` = the largest err64 of the case.  (-s prints every figure of
a run.)  Host round trips over 33 iterations: 14 on the batched shapes, 40 to 42 on the others.

case / cap                          1      5      7      8      9     15     16     17     31     32     33   conv (iters)  all R   err64
small                           4e-16  5e-16  5e-16  4e-16  4e-16  4e-16  4e-16  2e-16  3e-16  2e-16  3e-16    9e-17 (19)   2e-15   5e-16
six                             5e-16      -      -  6e-16      -      -  6e-16  3e-16      -      -      -    8e-17 (33)   6e-16   7e-16
rows17000                       4e-16      -      -  3e-16      -      -  2e-14  5e-14      -      -      -    2e-13 (20)   6e-13   3e-13
p1                              6e-17      -      -  6e-17      -      -  6e-17  6e-17      -      -      -    6e-17 ( 1)   6e-17   2e-16
p1023                           3e-16      -      -  7e-16      -      -  7e-16  4e-16      -      -      -    9e-16 (21)   9e-16   9e-16
p1024                           4e-16      -      -  6e-16      -      -  5e-16  4e-16      -      -      -    2e-16 (21)   6e-16   5e-16
p1025                           3e-16      -      -  5e-16      -      -  5e-16  3e-16      -      -      -    9e-17 (21)   1e-15   4e-16
p4096                           7e-16      -      -  3e-15      -      -  3e-15  3e-15      -      -      -    9e-14 (34)   1e-13   2e-13
p4097                           1e-15  3e-15  3e-15  3e-15  3e-15  4e-15  4e-15  3e-15  1e-15  2e-15  3e-15    5e-15 (35)   2e-14   7e-15
star300                         4e-16  2e-15  2e-15  2e-15  2e-15  2e-15  2e-15  2e-15  3e-16  4e-16  8e-16    1e-15 (34)   5e-15   2e-14
star2000                        2e-16      -      -  4e-16      -      -  3e-16  2e-16      -      -      -    1e-16 (24)   4e-16   4e-16
small generic                   3e-16      -      -  3e-16      -      -  5e-16  1e-16      -      -      -    2e-16 (19)   5e-16   5e-16
small sim(1)                    4e-16      -      -  4e-16      -      -  4e-16  2e-16      -      -      -    9e-17 (19)   4e-16   5e-16
small sim(4)                    5e-16      -      -  6e-16      -      -  6e-16  3e-16      -      -      -    1e-16 (20)   6e-16   3e-15
small OBHIP_HM3=0               4e-16  5e-16  5e-16  4e-16  4e-16  4e-16  4e-16  2e-16  3e-16  2e-16  3e-16    9e-17 (19)   2e-15   5e-16
star300 OBHIP_HM3=0             4e-16  2e-15  2e-15  3e-15  3e-15  3e-15  3e-15  2e-15  2e-15  3e-15  4e-15    6e-15 (34)   1e-14   2e-14
small OBHIP_HESSMULT_FUSED=0    4e-16  3e-16  3e-16  3e-16  3e-16  3e-16  4e-16  2e-16  1e-16  1e-16  2e-16    2e-16 (19)   7e-16   5e-16
star300 OBHIP_HESSMULT_FUSED=0  4e-16  2e-15  2e-15  2e-15  2e-15  2e-15  2e-15  2e-15  6e-16  1e-15  2e-15    2e-15 (34)   1e-14   2e-14
"""
import contextlib
import ctypes as C
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import pcg_ref as R
from conftest import knots_for, make_pair

pytestmark = pytest.mark.gpu

LD = np.longdouble
SCHEDULES = ("1", "2", "3", "5", None)          # OBHIP_CG_REFRESH (read per call); None = unset = 16
_cache = {}
MEASURED = {}                                    # (label, what, maxit) -> (device distance, err64)


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def host_syncs():
    from outerbase_amd._lib import call
    c = C.c_uint64(0)
    call("obhip_profile_get", b"host_syncs", C.byref(c), None)
    return c.value


def share_info(om_d, terms):
    import outerbase_amd as ob
    from outerbase_amd._lib import call, ptr
    info = np.zeros(11, dtype=np.uint64)
    tt = ob.obmod._Terms(om_d, terms)
    call("obhip_terms_share_tables", tt._h, ptr(info), None, None, None, None)
    return dict(p_pad=int(info[0]), nswf=int(info[7]))


class Problem:
    """a design matrix with its response and parameters, the device objects and the reference runs"""

    def __init__(self, case, om_d, bd, tt, terms, y, Bd, prec, rows=1):
        self.case, self.om_d, self.bd, self.tt, self.terms, self.y = case, om_d, bd, tt, terms, y
        self.sigma, self.rho, self.tol = case["sigma"], case["rho"], case["tol"]
        self.prec, self.rows = prec, rows
        # the sharded form: `rows` virtual ranks hold the same rows, the problem is the rows repeated
        self.B = Bd if rows == 1 else np.tile(Bd, (rows, 1))
        self.B_ld = self.B.astype(LD)
        self.yy = y if rows == 1 else np.tile(y, rows)
        self._runs = {}

    def ref(self, tol, maxit, dtype=LD, coeff0=None, sigma=None, y=None):
        """the guarded loop: long double on the reference's schedule, float64 on the library's"""
        key = (tol, maxit, dtype, None if coeff0 is None else np.asarray(coeff0).tobytes(), sigma, y is not None)
        if key not in self._runs:
            self._runs[key] = R.pcg_ref(self.B_ld if dtype is LD else self.B, self.yy if y is None else y,
                                        self.sigma if sigma is None else sigma, self.prec, tol, maxit,
                                        coeff0=coeff0, guards=True, refresh=1 if dtype is LD else 16, dtype=dtype)
        return self._runs[key]

    def value_at(self, theta, sigma=None, y=None):
        """(long double value at theta, |float64 value - it|, the magnitudes that cancel in it)"""
        sg = self.sigma if sigma is None else sigma
        yy = self.yy if y is None else y
        v_ld, _, parts = R.evaluate(self.B_ld, yy, sg, self.prec, theta)
        v_64, _, _ = R.evaluate(self.B, yy, sg, self.prec, theta, dtype=np.float64)
        return v_ld, abs(float(LD(v_64) - v_ld)), float(parts)

    def fit(self, tol, maxit, theta0=None, want_val=True, sigma=None, y=None, comm=None, dev=False):
        """obhip_fit_cg (obhip_fit_cg_dev with dev or a communicator) -> (theta, iters, diagH, val, host syncs)"""
        from outerbase_amd._lib import call, ptr
        p = len(self.prec)
        th = np.zeros(p) if theta0 is None else np.array(theta0, dtype=np.float64)
        dh, its, val = np.empty(p), C.c_uint64(0), C.c_double(math.nan)
        yv = np.ascontiguousarray(self.y if y is None else y)
        sg = self.sigma if sigma is None else sigma
        if comm is None and not dev:
            s0 = host_syncs()
            call("obhip_fit_cg", self.bd._h, self.tt._h, self.om_d._h, ptr(yv), sg, self.rho, tol, maxit, ptr(th),
                 C.byref(its), ptr(dh), C.byref(val) if want_val else None)
            return th, its.value, dh, val.value, host_syncs() - s0
        import torch
        dy, dth = torch.from_numpy(yv).cuda(), torch.from_numpy(th).cuda()
        ddh = torch.empty(p, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s0 = host_syncs()
        call("obhip_fit_cg_dev", self.bd._h, self.tt._h, self.om_d._h, dy.data_ptr(), sg, self.rho, tol, maxit,
             dth.data_ptr(), C.byref(its), ddh.data_ptr(), C.byref(val) if want_val else None, comm)
        s1 = host_syncs()
        torch.cuda.synchronize()
        return dth.cpu().numpy(), its.value, ddh.cpu().numpy(), val.value, s1 - s0


def capped(run, maxit):
    """the run with tol = 0 cut at maxit: with tol = 0 no tolerance test ever holds, so the iterates
    do not depend on the cap"""
    k = min(maxit, run.iters)
    stop = "maxit" if maxit < run.iters or (maxit == run.iters and run.stop == "maxit") else run.stop
    return SimpleNamespace(iters=k, theta=run.iterates[k], m=run.m, stop=stop)


def problem(name, rows=1):
    if (name, rows) not in _cache:
        import outerbase_amd as ob
        case = R.CASES[name]
        if (name, 1) in _cache:
            q = _cache[(name, 1)]
            _cache[(name, rows)] = Problem(case, q.om_d, q.bd, q.tt, q.terms, q.y, q.B, q.prec, rows)
            return _cache[(name, rows)]
        om_o, om_d = make_pair(case["kinds"], knots_for(case["kinds"], case["knots"]))
        terms = R.case_terms(case, om_d)
        x, y = R.case_xy(case)
        bd = ob.outerbase(om_d, x)
        tt = ob.obmod._Terms(om_d, terms)
        Bd = bd.getmat(terms)
        prec = R.case_prec(case, om_d, terms)
        q = Problem(case, om_d, bd, tt, terms, y, Bd, prec)
        q.x = x
        _cache[(name, 1)] = q
        if rows != 1:
            return problem(name, rows)
    return _cache[(name, rows)]


def check_run(q, label, tol, maxit, got, ref, f64, want_val=True):
    """one device run against the long double run of the same arguments"""
    th, its, dh, val, _ = got
    assert f64.iters == ref.iters, (label, maxit, "float64 and long double references disagree")
    assert its == ref.iters, (label, tol, maxit, its, ref.iters)
    if tol == 0.0 and ref.stop == "maxit":
        assert its == maxit
    err64 = R.relmax(f64.theta, ref.theta)
    dist = R.relmax(th, ref.theta)
    MEASURED[(label, tol, maxit)] = (dist, err64)
    print("pcg %-22s tol %-7g maxit %-4d iters %-3d dist %.2e err64 %.2e" % (label, tol, maxit, its, dist, err64))
    assert dist <= max(32 * err64, 1e-12), (label, tol, maxit, dist, err64)
    # m = e^{-2 sigma} colsums(B^2) + prec (fit.cpp:51)
    assert R.relmax(dh, ref.m) < 1e-11, (label, maxit)
    if want_val:
        v_ld, d64, parts = q.value_at(th)
        bound = max(32 * d64, 1e-13 * parts)
        assert abs(float(LD(val) - v_ld)) <= bound, (label, tol, maxit, val, float(v_ld), bound)


def check_problem(q, label, ladder, schedules=SCHEDULES, comm=None, batched=None, converge=True):
    """the ladder of caps with tol = 0 and the converging run, under every schedule"""
    case = q.case
    last = max(ladder)
    ld0, f0 = q.ref(0.0, last), q.ref(0.0, last, np.float64)
    for sched in schedules:
        lab = label if sched is None else "%s R=%s" % (label, sched)
        with env("OBHIP_CG_REFRESH", sched):
            for maxit in ladder:
                ref, f64 = capped(ld0, maxit), capped(f0, maxit)
                got = q.fit(0.0, maxit, comm=comm)
                check_run(q, lab, 0.0, maxit, got, ref, f64)
                if maxit in (16, 17):
                    # 16 ends on a refresh (no further update() for the value), 17 on a recurrence step;
                    # the same call again, and without the value: the same bits
                    again = q.fit(0.0, maxit, comm=comm)
                    noval = q.fit(0.0, maxit, want_val=False, comm=comm)
                    assert np.array_equal(got[0], again[0]) and got[1] == again[1] and got[3] == again[3]
                    assert np.array_equal(got[0], noval[0]) and got[1] == noval[1]
                    assert np.array_equal(got[2], again[2])
            if converge:
                ref, f64 = q.ref(q.tol, 400), q.ref(q.tol, 400, np.float64)
                got = q.fit(q.tol, 400, comm=comm)
                check_run(q, lab, q.tol, 400, got, ref, f64)
                again = q.fit(q.tol, 400, comm=comm)
                assert np.array_equal(got[0], again[0]) and got[1] == again[1] and got[3] == again[3]
    # witness of the refresh: the step after a refresh iteration starts from an evaluated gradient, not
    # from the recurrence's, so from there on the bits differ from a schedule that never refreshes (and
    # the iterates agree to rounding: both lie within the bound above).  A batch that ran across its
    # refresh iteration would give the same bits.
    if ld0.stop == "maxit":
        for sched in schedules:
            at = 16 if sched is None else int(sched)
            if at < 2 or at + 1 > last:
                continue
            with env("OBHIP_CG_REFRESH", sched):
                with_refresh = q.fit(0.0, at + 1, comm=comm)
            with env("OBHIP_CG_REFRESH", "1000000"):
                never = q.fit(0.0, at + 1, comm=comm)
            assert with_refresh[1] == never[1] == at + 1
            assert not np.array_equal(with_refresh[0], never[0]), (label, sched)
    # the conditions of the case, on the device's matrix
    if converge:
        ref = q.ref(q.tol, 400)
        ok, worst = R.stop_margin_ok(ref.trace, q.tol)
        assert ok, (label, worst)
        if case["window"]:
            assert 18 <= ref.iters <= 60 and ref.stop == "next", (label, ref.iters)
    # witness of the schedule (default refresh): host round trips of the call itself, y / theta / diagH
    # already in HBM, over 33 iterations (two refresh iterations; a handful of round trips belong to the
    # set-up of any call, so a short run tells nothing)
    if batched is not None and ld0.stop == "maxit":
        with env("OBHIP_CG_REFRESH", None):
            th, its, _, _, syncs = q.fit(0.0, 33, want_val=False, comm=comm, dev=True)
        assert its == 33
        print("pcg %-22s host syncs %d for %d iterations" % (label, syncs, its))
        if batched:
            assert syncs < its / 2, (label, syncs, its)
        else:
            assert syncs >= its, (label, syncs, its)
    return ld0


def check_shape(name):
    """the case's shape lies where its row of the table says: batch limit, padding, star kernel"""
    q = problem(name)
    case = q.case
    info = share_info(q.om_d, q.terms)
    assert info["p_pad"] == R.p_pad_of(case["p"])
    small = R.n_pad_of(case["n"]) * info["p_pad"] <= R.BATCH_LIMIT
    assert small == (name not in ("rows17000", "star2000"))
    if name == "rows17000":
        assert R.n_pad_of(case["n"]) * info["p_pad"] == 17024 * 256
    if name.startswith("star") or name == "p4096":
        assert 9 <= info["nswf"] <= 16                                  # k_star's domain (test_gpu_star.py)
    if name in ("p4096", "p4097", "star300", "star2000"):
        assert q.terms.max() <= 12
    # batched = small and the Hessian product can be enqueued ahead; p = 4097 is beyond one workgroup's
    # terms for k_hm2 / k_star (no speculation), so the host stays in the loop
    assert case["batched"] == (small and case["p"] <= 4096)
    return q


@pytest.mark.parametrize("name", list(R.CASES))
def test_pcg_against_long_double_loop(name):
    q = check_shape(name)
    check_problem(q, name, q.case["ladder"], batched=q.case["batched"])


def test_pcg_without_lds_tile():
    """OBHIP_FORCE_GENERIC (read per call): the two-kernel product and k_cg_q under the register step
    kernel; nothing can be enqueued ahead, so the host looks once per iteration"""
    q = problem("small")
    with env("OBHIP_FORCE_GENERIC", "1"):
        check_problem(q, "small generic", R.LADDER_SHORT, batched=False)


@pytest.mark.parametrize("ranks", [1, 4])
def test_pcg_sharded_over_virtual_ranks(ranks):
    """obhip_comm_init_sim(N): the `many` branch (no HmThen, an all-reduce, k_cg_q) is the loop on the
    rows repeated N times with ntot = N n"""
    from outerbase_amd._lib import call, lib
    q = problem("small", rows=ranks)
    comm = C.c_void_p()
    call("obhip_comm_init_sim", C.byref(comm), ranks)
    try:
        assert q.B.shape[0] == ranks * q.case["n"]
        check_problem(q, "small sim(%d)" % ranks, R.LADDER_SHORT, comm=comm, batched=False)
    finally:
        lib.obhip_comm_destroy(comm)


def test_pcg_through_lpdfvec_and_warm_starts():
    """lpdfvec.optcg: cold, then warm from its own result after sigma moved by 0.3 (updatepara); the
    same through obhip_fit_cg with theta in / out"""
    import outerbase_amd as ob
    q = problem("small")
    lik = ob.loglik_gauss(q.om_d, q.terms, q.y, q.x)
    pr = ob.logpr_gauss(q.om_d, q.terms)
    lp = ob.lpdfvec(lik, pr)
    lp.updatepara([q.sigma, q.rho])
    assert lik.para[0] == q.sigma and pr.para[0] == q.rho
    cold = q.ref(q.tol, 400)
    lp.optcg(q.tol, 400)
    assert lp.cgiters == cold.iters
    th0 = lp.coeff
    err64 = R.relmax(q.ref(q.tol, 400, np.float64).theta, cold.theta)
    assert R.relmax(th0, cold.theta) <= max(32 * err64, 1e-12)
    assert R.relmax(lp.totdiaghess, cold.m) < 1e-11
    sig2 = q.sigma + 0.3
    warm, warm64 = q.ref(q.tol, 400, coeff0=th0, sigma=sig2), q.ref(q.tol, 400, np.float64, coeff0=th0, sigma=sig2)
    ok, worst = R.stop_margin_ok(warm.trace, q.tol)
    assert ok and warm.iters == warm64.iters and warm.iters >= 5, (worst, warm.iters)
    bound = max(32 * R.relmax(warm64.theta, warm.theta), 1e-12)
    lp.updatepara([sig2, q.rho])
    lp.optcg(q.tol, 400)
    assert lp.cgiters == warm.iters
    dist = R.relmax(lp.coeff, warm.theta)
    print("pcg warm start through lpdfvec: iters %d dist %.2e bound %.2e" % (warm.iters, dist, bound))
    assert dist <= bound
    for sched in SCHEDULES:
        with env("OBHIP_CG_REFRESH", sched):
            th, its, dh, val, _ = q.fit(q.tol, 400, theta0=th0, sigma=sig2)
        assert its == warm.iters, sched
        assert R.relmax(th, warm.theta) <= bound, sched
        assert R.relmax(dh, warm.m) < 1e-11
        v_ld, d64, parts = q.value_at(th, sigma=sig2)
        assert abs(float(LD(val) - v_ld)) <= max(32 * d64, 1e-13 * parts)


def test_pcg_edges():
    """zero response, a warm start at the exact solution, the rounding floor, overflow of e^{-2 sigma}:
    the outcome of the guarded reference loop"""
    import outerbase_amd as ob
    q = problem("small")
    p = len(q.prec)
    # y = 0: !(num > 0) before any step
    zero = np.zeros_like(q.y)
    ref = q.ref(q.tol, 50, y=zero)
    assert ref.iters == 0 and ref.stop == "num"
    for sched in ("1", None):
        with env("OBHIP_CG_REFRESH", sched):
            th, its, dh, val, _ = q.fit(q.tol, 50, y=zero)
        assert its == 0 and not th.any() and np.all(np.isfinite(dh)) and math.isfinite(val)
        v_ld, d64, parts = q.value_at(th, y=zero)
        assert abs(float(LD(val) - v_ld)) <= max(32 * d64, 1e-13 * parts)
    # at the exact solution valdiff still opens at 10: the one step of the reference
    want = R.dense_solve(q.B, q.y, q.sigma, q.prec)
    th0 = want.astype(np.float64)
    ref, f64 = q.ref(q.tol, 50, coeff0=th0), q.ref(q.tol, 50, np.float64, coeff0=th0)
    assert ref.iters == f64.iters == 1
    th, its, _, _, _ = q.fit(q.tol, 50, theta0=th0)
    assert its == 1 and np.all(np.isfinite(th))
    assert R.relmax(th, want) <= max(32 * R.relmax(f64.theta, want), 1e-12)
    # tol = 0: the loop ends on the floor, at the solution
    ref, f64 = q.ref(0.0, 5000), q.ref(0.0, 5000, np.float64)
    assert ref.stop == f64.stop == "floor"
    for sched in SCHEDULES:
        with env("OBHIP_CG_REFRESH", sched):
            th, its, _, val, _ = q.fit(0.0, 5000)
        assert 33 < its < 5000 and np.all(np.isfinite(th)) and math.isfinite(val), (sched, its)
        dist = R.relmax(th, want)
        print("pcg floor R=%s: iters %d (reference %d, float64 %d) dist from the solve %.2e" %
              (sched, its, ref.iters, f64.iters, dist))
        assert dist <= max(32 * R.relmax(f64.theta, want), 1e-12), sched
    # sigma = -400: e^{800} = inf, m and grad both non-finite (fit.cpp:53-56): arithmetic on infinities
    ref = R.pcg_ref(q.B, q.y, -400.0, q.prec, q.tol, 50, guards=True, dtype=np.float64)
    assert not ref.finite and ref.iters == 0
    th, its, _, val, _ = q.fit(q.tol, 50, sigma=-400.0)
    assert its == 0 and not th.any() and val == -math.inf
    start = np.linspace(-1.0, 1.0, p)
    th, its, _, val, _ = q.fit(q.tol, 50, sigma=-400.0, theta0=start)
    assert its == 0 and np.array_equal(th, start) and val == -math.inf
    lik = ob.loglik_gauss(q.om_d, q.terms, q.y, q.x)
    lp = ob.lpdfvec(lik, ob.logpr_gauss(q.om_d, q.terms))
    lp.updatepara([-400.0, q.rho])
    lp.optcg(q.tol, 50)
    assert lp.cgiters == 0 and lp.val == -math.inf


def test_pcg_under_process_wide_switches():
    """OBHIP_HM3=0 (k_hm2 where the star kernel would run) and OBHIP_HESSMULT_FUSED=0 (nothing
    speculative: k_hm_tl or two kernels) are read once per process: one child each, one after the other,
    none started after a failure"""
    here = os.path.dirname(os.path.abspath(__file__))
    for var in ("OBHIP_HM3", "OBHIP_HESSMULT_FUSED"):
        envp = dict(os.environ)
        envp.pop("OBHIP_CG_REFRESH", None)
        envp[var] = "0"
        r = subprocess.run([sys.executable, os.path.join(here, "pcg_paths_worker.py"), var], env=envp,
                           capture_output=True, text=True, timeout=600)
        print(r.stdout)
        assert r.returncode == 0, var + "\n" + r.stdout[-3000:] + r.stderr[-4000:]
        assert "pcg paths ok " + var in r.stdout
