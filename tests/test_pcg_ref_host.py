"""tests/pcg_ref.py checks itself, and the cases of its table, on the oracle's design matrix
(ob_getmat): every case small enough for the CPU (p < 2000; tests/test_gpu_pcg.py repeats the
conditions on the device's own matrix for all of them).

- the long double loop, the float64 loop and oracle/ob_oracle.py::fit_cg (which shares no text with
  pcg_ref) count the same iterations;
- with tol = 0 and enough iterations the loop ends at the long double dense solve;
- the reference's schedule (R = 1) and the library's (R = 16) give the same count and the same
  iterates up to long double rounding;
- no evaluated stop test of a case sits on its threshold (pcg_ref.stop_margin_ok), and the
  converging cases stop in 18...60 iterations, one of them beyond 32 -- so that the refresh
  iterations 16 and 32 of the library's schedule are crossed.
"""
import numpy as np
import pytest

import pcg_ref as R

LD = np.longdouble
HOST_CASES = [k for k, c in R.CASES.items() if c["host"]]
_cache = {}


def host_case(name):
    """(case, B of the oracle, y, prec) and the runs shared by the tests, computed once"""
    if name not in _cache:
        import ob_oracle as O
        case = R.CASES[name]
        om = O.OuterMod()
        om.setcovfs(case["kinds"])
        om.setknot(O.bench_knots(case["kinds"], case["knots"]))
        terms = R.case_terms(case, om)
        x, y = R.case_xy(case)
        bo = O.OuterBase(om, x)
        B = O.ob_getmat(bo, terms)
        prec = R.case_prec(case, om, terms)
        d = dict(case=case, om=om, bo=bo, terms=terms, x=x, y=y, B=B, prec=prec)
        a = (B, y, case["sigma"], prec, case["tol"], 400)
        d["ld"] = R.pcg_ref(*a, guards=True)
        d["ld16"] = R.pcg_ref(*a, guards=True, refresh=16)
        d["f64"] = R.pcg_ref(*a, guards=True, dtype=np.float64)
        d["f64_16"] = R.pcg_ref(*a, guards=True, refresh=16, dtype=np.float64)
        _cache[name] = d
    return _cache[name]


def test_case_table_is_complete_and_small_cases_run_here():
    assert set(HOST_CASES) == {"small", "six", "rows17000", "p1", "p1023", "p1024", "p1025"}
    for name, c in R.CASES.items():
        assert c["host"] == (c["p"] < 2000), name
        # which side of the batch limit the shape lies on (fit_cg_dev_impl: n_pad * p_pad <= 2^22)
        small = R.n_pad_of(c["n"]) * R.p_pad_of(c["p"]) <= R.BATCH_LIMIT
        assert small == (name not in ("rows17000", "star2000")), name
        assert set(c["ladder"]) <= set(R.LADDER_FULL) and {16, 17} <= set(c["ladder"])
    assert R.n_pad_of(17000) * R.p_pad_of(200) == 17024 * 256 > R.BATCH_LIMIT


@pytest.mark.parametrize("name", HOST_CASES)
def test_counts_agree_with_the_oracle(name):
    """long double, float64, both schedules, with and without the guards, and O.fit_cg"""
    import ob_oracle as O
    d = host_case(name)
    c = d["case"]
    want = d["ld"].iters
    assert d["ld16"].iters == d["f64"].iters == d["f64_16"].iters == want
    if name == "p1":
        # one step solves it; the reference then divides rounding noise by rounding noise and goes
        # on, the guarded loop ends on the floor
        assert want == 1 and d["ld"].stop == "floor"
        return
    th_o, it_o, m_o = O.fit_cg(d["bo"], d["terms"], d["y"], sigma=c["sigma"], rho=c["rho"], tol=c["tol"],
                               maxit=400)
    assert it_o == want
    plain = R.pcg_ref(d["B"], d["y"], c["sigma"], d["prec"], c["tol"], 400, dtype=np.float64)
    assert plain.iters == want and plain.stop == "tol"
    # (the two restatements run the same arithmetic in float64, in other summation orders)
    assert R.relmax(th_o, plain.theta) < 1e-9 and R.relmax(m_o, plain.m) < 1e-13
    assert R.relmax(plain.theta, d["f64"].theta) == 0.0       # the guards change nothing on the way


@pytest.mark.parametrize("name", HOST_CASES)
def test_no_stop_test_on_its_threshold_and_refresh_crossed(name):
    d = host_case(name)
    c = d["case"]
    ok, worst = R.stop_margin_ok(d["ld"].trace, c["tol"])
    assert ok, (name, worst)
    ok16, worst16 = R.stop_margin_ok(d["ld16"].trace, c["tol"])
    assert ok16, (name, worst16)
    if c["window"]:
        assert 18 <= d["ld"].iters <= 60, (name, d["ld"].iters)
        assert d["ld"].stop == "next"
    # the maxit ladder runs with tol = 0: nothing but the cap may end those runs before 33 (p = 1
    # ends on the floor after one step, by 1e-28 against rounding noise of 1e-32)
    free = R.pcg_ref(d["B"], d["y"], c["sigma"], d["prec"], 0.0, 33, guards=True, dtype=np.float64)
    if name == "p1":
        assert free.iters == 1 and free.stop == "floor"
        assert float(free.trace[-1][0] / free.trace[0][0]) < 1e-30
    else:
        assert free.iters == 33 and free.stop == "maxit"
        nums = np.array([float(t[0] / free.trace[0][0]) for t in free.trace])    # the 33 opening tests
        assert len(nums) == 33 and nums.min() > 1e-26          # two digits clear of the floor


def test_one_case_crosses_the_second_refresh():
    assert max(host_case(n)["ld"].iters for n in HOST_CASES if R.CASES[n]["window"]) > 32


@pytest.mark.parametrize("name", HOST_CASES)
def test_schedules_agree_in_long_double(name):
    """R = 1 and R = 16: same count, same iterates.  Both loops round in long double, and a rounding
    error is amplified by the loop alike in either format; err64 (float64 loop against long double)
    measures that amplification per iterate, so the bound is the device tests' bound scaled by the ratio
    of the formats' unit roundoffs: max(32 err64, 1e-12) eps_ld / eps64."""
    d = host_case(name)
    assert d["ld"].iters == d["ld16"].iters
    ratio = float(np.finfo(LD).eps) / R.EPS64
    for k in range(1, d["ld"].iters + 1):
        err64 = R.relmax(d["f64_16"].iterates[k], d["ld"].iterates[k])
        got = R.relmax(d["ld16"].iterates[k], d["ld"].iterates[k])
        assert got <= max(32 * err64, 1e-12) * ratio, (name, k, got, err64)
    assert abs(float(d["ld16"].val - d["ld"].val)) <= 1e-15 * abs(float(d["ld"].val))


@pytest.mark.parametrize("name", ["small", "p1", "p1025"])
def test_converges_to_the_dense_solve(name):
    """tol = 0: the guarded loop runs to the rounding floor and ends at the solution of
    (e2 B^T B + diag(prec)) theta = e2 B^T y"""
    d = host_case(name)
    c = d["case"]
    want = R.dense_solve(d["B"], d["y"], c["sigma"], d["prec"])
    for refresh in (1, 16):
        r = R.pcg_ref(d["B"], d["y"], c["sigma"], d["prec"], 0.0, 5000, guards=True, refresh=refresh)
        # (p = 1 under the recurrence: the gradient after the one step is exactly 0)
        assert r.stop in ("floor", "num") and r.iters < 5000
        # num = |grad|^2 in the M^-1 norm has dropped by 1e-28: the error by 1e-14 in that norm,
        # times the square root of the preconditioned condition number (at most 1e3 here)
        assert R.relmax(r.theta, want) < 1e-11, (name, refresh)
        v, g, _ = R.evaluate(d["B"], d["y"], c["sigma"], d["prec"], want)
        assert float(r.val) <= float(v) + 1e-15 * abs(float(v))          # the solve maximises val
        assert float(np.max(np.abs(g))) <= 1e-15 * float(np.max(np.abs(d["ld"].m * want)))


def test_edges_of_the_guarded_loop():
    d = host_case("small")
    c = d["case"]
    B, y, prec = d["B"], d["y"], d["prec"]
    # zero response: the reference divides 0 by 0, the guarded loop takes no step
    r = R.pcg_ref(B, 0 * y, c["sigma"], prec, c["tol"], 50, guards=True)
    assert r.iters == 0 and r.stop == "num" and not r.theta.any() and np.isfinite(float(r.val))
    plain = R.pcg_ref(B, 0 * y, c["sigma"], prec, c["tol"], 3)
    assert not np.all(np.isfinite(plain.theta.astype(float)))
    # e^{-2 sigma} overflows in float64: m and grad both non-finite, fit.cpp:53-56
    r = R.pcg_ref(B, y, -400.0, prec, c["tol"], 50, guards=True, dtype=np.float64)
    assert not r.finite and r.iters == 0 and r.val == -np.inf and not r.theta.any()
    # warm start at the solution: valdiff opens at 10, so one step is taken (fit.cpp:69-73)
    want = R.dense_solve(B, y, c["sigma"], prec)
    r = R.pcg_ref(B, y, c["sigma"], prec, c["tol"], 50, coeff0=want.astype(np.float64), guards=True)
    assert r.iters == 1 and R.relmax(r.theta, want) < 1e-15
    # warm start after a change of sigma: converges to the new solve
    r = R.pcg_ref(B, y, c["sigma"] + 0.3, prec, c["tol"], 400, coeff0=d["ld"].theta, guards=True)
    assert 5 <= r.iters < d["ld"].iters + 5
    want = R.dense_solve(B, y, c["sigma"] + 0.3, prec)
    assert R.relmax(r.theta, want) < 1e-4
    # the sharded form: the rows four times over with ntot = 4 n is the same problem as e2 * 4
    r4 = R.pcg_ref(np.tile(B, (4, 1)), np.tile(y, 4), c["sigma"], prec, 0.0, 8, guards=True)
    r1 = R.pcg_ref(B, y, c["sigma"] - 0.5 * np.log(LD(4)), prec, 0.0, 8, guards=True)
    assert R.relmax(r4.theta, r1.theta) < 1e-17
