"""lpdf::optcg (src/fit.cpp:37-96) for lpdfvec(logpr_gauss, loglik_gauss), restated in plain NumPy
on a dense design matrix B (n x p) that the caller hands in: likelihood and prior of
loglik_gauss.cpp:110-157 and logpr_gauss.cpp:101-115.  Everything runs in np.longdouble; dtype =
np.float64 runs the same text in double.  Nothing here is shared with oracle/ob_oracle.py::fit_cg.

Two switches restate what the library does differently from the reference:

refresh=R   R = 1 evaluates value and gradient with update() in every iteration (fit.cpp:78).
            R > 1 advances them by the recurrence grad -= alpha q, val += alpha g.p - alpha^2 p.q / 2
            (exact for this quadratic objective) and evaluates only when (k + 1) % R == 0.
guards=True the library's documented departures: the rounding floor num <= 1e-28 num0 (num0 = the
            first num), !(num > 0), !(denom > 0), and the look-ahead stop (the opening test of the
            next iteration, taken right after the step: same count, the Hessian product of a
            converged iterate is not formed).  The non-finite exit of fit.cpp:53-56 (m AND grad both
            non-finite) is the reference's own and holds either way.

CASES is the table of shapes that tests/test_pcg_ref_host.py and tests/test_gpu_pcg.py both read.
"""
import math
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)


def prior_logsd(prec, dtype=LD):
    """sum(log(coeffsd * sca)) of logpr_gauss.cpp:101 from the precisions 1 / (coeffsd sca)^2"""
    return -(np.log(np.asarray(prec, dtype=dtype)).sum()) / dtype(2)


def evaluate(B, y, sigma, prec, coeff, ntot=None, dtype=LD):
    """(val, grad, parts) of lpdfvec::update at coeff: loglik_gauss.cpp:117-126 + logpr_gauss.cpp:98-106.
    parts = the magnitudes that cancel in val."""
    B = np.asarray(B, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    prec = np.asarray(prec, dtype=dtype)
    c = np.asarray(coeff, dtype=dtype)
    n = dtype(B.shape[0] if ntot is None else ntot)
    with np.errstate(all="ignore"):
        e2 = np.exp(dtype(-2) * dtype(sigma))
        r = B @ c - y
        ss = (r * r).sum()
        pen = (c * c * prec).sum()
        logsd = prior_logsd(prec, dtype)
        val = -e2 * ss / dtype(2) - n * dtype(sigma) - pen / dtype(2) - logsd
        grad = B.T @ (-e2 * r) - c * prec
        parts = e2 * ss / dtype(2) + abs(n * dtype(sigma)) + pen / dtype(2) + abs(logsd)
    return val, grad, parts


def pcg_ref(B, y, sigma, prec, tol, maxit, coeff0=None, refresh=1, guards=False, ntot=None,
            dtype=LD):
    """The loop.  Returns a namespace with
    theta      the result
    iterates   [coeff0, iterate after step 1, ...] (len = iters + 1)
    iters      the iteration count as the reference counts it (k of fit.cpp:71 when the loop ends)
    m          the preconditioner e^{-2 sigma} colsums(B^2) + prec
    val        the value at theta, truly evaluated (-inf after the non-finite exit)
    finite     False when the loop left through fit.cpp:53-56
    trace      per opening test that was evaluated: (num, denom, valdiff, val); the look-ahead's
               test is recorded with denom = nan
    stop       'tol', 'maxit', 'floor', 'num', 'denom', 'next' or 'nonfinite'"""
    B = np.asarray(B, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    prec = np.asarray(prec, dtype=dtype)
    p = B.shape[1]
    coeff = np.zeros(p, dtype=dtype) if coeff0 is None else np.array(coeff0, dtype=dtype)
    tol = dtype(tol)
    half = dtype(1) / dtype(2)
    out = SimpleNamespace(iterates=[coeff.copy()], trace=[], finite=True, stop="maxit")
    with np.errstate(all="ignore"):
        e2 = np.exp(dtype(-2) * dtype(sigma))

        def update(c):
            v, g, _ = evaluate(B, y, sigma, prec, c, ntot, dtype)
            return v, g

        def hessmult(v):                                  # loglik_gauss.cpp:137-145 + logpr_gauss.cpp:113-115
            return e2 * (B.T @ (B @ v)) + prec * v

        val, grad = update(coeff)
        m = e2 * (B * B).sum(0) + prec                    # fit.cpp:51
        out.m = m
        if not np.all(np.isfinite(m)) and not np.all(np.isfinite(grad)):   # fit.cpp:53-56
            out.theta, out.iters, out.val = coeff, 0, dtype(-np.inf)
            out.finite, out.stop = False, "nonfinite"
            return out
        rm = grad / m
        pv = rm.copy()
        q = hessmult(pv)
        valdiff = dtype(10)
        num0 = None
        k = 0
        while k < maxit:                                  # fit.cpp:71
            num = (grad * rm).sum()
            denom = (q * pv).sum()
            out.trace.append((num, denom, valdiff, val))
            if num < tol and valdiff < tol:               # fit.cpp:73
                out.stop = "tol"
                break
            if guards:
                if num0 is None:
                    num0 = num
                if not num > 0:
                    out.stop = "num"
                    break
                if num <= dtype(1e-28) * num0:
                    out.stop = "floor"
                    break
                if not denom > 0:
                    out.stop = "denom"
                    break
            alpha = num / denom
            gp = (grad * pv).sum()
            coeff = coeff + alpha * pv
            valo = val
            if (k + 1) % refresh == 0:
                val, grad = update(coeff)                 # fit.cpp:78
            else:
                val = val + (alpha * gp - half * alpha * alpha * denom)
                grad = grad - alpha * q
            valdiff = val - valo
            rm = grad / m
            num2 = -((alpha * q) * rm).sum()
            beta = num2 / num
            pv = rm + beta * pv
            k += 1
            out.iterates.append(coeff.copy())
            if guards and k < maxit:
                nxt = (grad * rm).sum()
                if nxt < tol and valdiff < tol:
                    out.trace.append((nxt, dtype(np.nan), valdiff, val))
                    out.stop = "next"
                    break
            q = hessmult(pv)
        out.theta, out.iters = coeff, k
        out.val = update(coeff)[0]
    return out


def dense_solve(B, y, sigma, prec, ntot=None):
    """theta of (e2 B^T B + diag(prec)) theta = e2 B^T y in long double: Cholesky by hand (NumPy's
    linalg has no long double), then one step of refinement"""
    B = np.asarray(B, dtype=LD)
    y = np.asarray(y, dtype=LD)
    prec = np.asarray(prec, dtype=LD)
    e2 = np.exp(LD(-2) * LD(sigma))
    H = e2 * (B.T @ B) + np.diag(prec)
    rhs = e2 * (B.T @ y)
    p = H.shape[0]
    L = np.zeros_like(H)
    for j in range(p):
        d = H[j, j] - (L[j, :j] * L[j, :j]).sum()
        L[j, j] = np.sqrt(d)
        if j + 1 < p:
            L[j + 1:, j] = (H[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]

    def solve(b):
        z = np.zeros(p, dtype=LD)
        for j in range(p):
            z[j] = (b[j] - (L[j, :j] * z[:j]).sum()) / L[j, j]
        x = np.zeros(p, dtype=LD)
        for j in range(p - 1, -1, -1):
            x[j] = (z[j] - (L[j + 1:, j] * x[j + 1:]).sum()) / L[j, j]
        return x
    th = solve(rhs)
    return th + solve(rhs - H @ th)


def relmax(a, b):
    """max |a - b| / max |b|, in long double"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(LD(1e-300), np.max(np.abs(b))))


def stop_margin_ok(trace, tol):
    """no evaluated stop test sits on its threshold: num / tol and valdiff / tol are at least
    max(1e-6, 1e3 eps64 |val| / tol) away from 1 (a refreshed valdiff is a difference of two full
    evaluations).  -> (ok, the smallest distance seen minus its margin)"""
    tol = LD(tol)
    worst = math.inf
    for num, _, valdiff, val in trace:
        margin = max(1e-6, float(1e3 * EPS64 * abs(val) / tol))
        for v in (num, valdiff):
            worst = min(worst, float(abs(v / tol - 1)) - margin)
    return worst >= 0.0, worst


LADDER_FULL = (1, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)
LADDER_SHORT = (1, 8, 16, 17)
BATCH_LIMIT = 1 << 22          # n_pad * p_pad up to which eight iterations are enqueued per host look
TILE_ROWS = 64                 # rows per tile of the basis store (n_pad)

# terms: "select" = selectterms(p); "cap12" = selectterms(3 p) without terms beyond level 12 in any
# dimension, the first p of them (still downward-closed; tests/test_gpu_star.py).
# window: the converging count must lie in 18...60; host: small enough for the CPU test.
CASES = {
    "small": dict(kinds=["mat25"] * 8, knots=40, n=500, p=100, seed=11, sigma=-2.0, rho=2.0, tol=5e-8,
                  terms="select", ladder=LADDER_FULL, window=True, host=True, batched=True),
    "six": dict(kinds=["mat25pow"] * 8, knots=40, n=1000, p=256, seed=12, sigma=-3.0, rho=8.0, tol=4e-10,
                terms="select", ladder=LADDER_SHORT, window=True, host=True, batched=True),
    "rows17000": dict(kinds=["mat25"] * 8, knots=40, n=17000, p=200, seed=13, sigma=-2.0, rho=2.0, tol=1e-6, xpow=1.35,
                      terms="select", ladder=LADDER_SHORT, window=True, host=True, batched=False),
    "p1": dict(kinds=["mat25"] * 4, knots=40, n=130, p=1, seed=14, sigma=-2.0, rho=2.0, tol=1e-8,
               terms="select", ladder=LADDER_SHORT, window=False, host=True, batched=True),
    "p1023": dict(kinds=["mat25"] * 4, knots=40, n=130, p=1023, seed=15, sigma=-2.0, rho=2.0, tol=5e-8,
                  terms="select", ladder=LADDER_SHORT, window=True, host=True, batched=True),
    "p1024": dict(kinds=["mat25"] * 4, knots=40, n=130, p=1024, seed=36, sigma=-2.0, rho=2.0, tol=3e-8,
                  terms="select", ladder=LADDER_SHORT, window=True, host=True, batched=True),
    "p1025": dict(kinds=["mat25"] * 4, knots=40, n=130, p=1025, seed=17, sigma=-2.0, rho=2.0, tol=2e-8,
                  terms="select", ladder=LADDER_SHORT, window=True, host=True, batched=True),
    "p4096": dict(kinds=["mat25"] * 20, knots=40, n=300, p=4096, seed=18, sigma=-1.5, rho=0.5, tol=1e-6,
                  terms="cap12", ladder=LADDER_SHORT, window=True, host=False, batched=True),
    "p4097": dict(kinds=["mat25"] * 20, knots=40, n=300, p=4097, seed=19, sigma=-1.5, rho=0.5, tol=1e-6,
                  terms="cap12", ladder=LADDER_FULL, window=True, host=False, batched=False),
    "star300": dict(kinds=["mat25"] * 20, knots=40, n=300, p=2500, seed=20, sigma=-1.5, rho=0.5, tol=1e-6,
                    terms="cap12", ladder=LADDER_FULL, window=True, host=False, batched=True),
    "star2000": dict(kinds=["mat25"] * 20, knots=40, n=2000, p=2500, seed=21, sigma=-1.5, rho=0.5, tol=1e-6,
                     terms="cap12", ladder=LADDER_SHORT, window=True, host=False, batched=False),
}


def p_pad_of(p):
    """terms padded to whole workgroups of 256 lanes (obhip_terms::p_pad)"""
    return (p + 255) // 256 * 256


def n_pad_of(n):
    return (n + TILE_ROWS - 1) // TILE_ROWS * TILE_ROWS


def case_terms(case, om):
    """the case's term set from om.selectterms (oracle or device model: the same lattice walk)"""
    p = case["p"]
    if case["terms"] == "select":
        return np.asarray(om.selectterms(p), dtype=np.int64)
    t = np.asarray(om.selectterms(3 * p), dtype=np.int64)
    t = t[t.max(1) <= 12][:p]
    assert len(t) == p
    return t


def case_xy(case):
    """inputs in (0.02, 0.98)^d and a smooth response with noise, from the case's seed"""
    rng = np.random.default_rng(case["seed"])
    n, d = case["n"], len(case["kinds"])
    x = 0.02 + 0.96 * rng.random((n, d)) ** case.get("xpow", 1.0)   # xpow > 1: rows crowd towards 0.02
    w = rng.standard_normal(d) / np.sqrt(np.arange(1, d + 1))
    y = np.sin(3.0 * (x @ w)) + (x[:, 0] - 0.5) * (x[:, d - 1] - 0.5) + 0.05 * rng.standard_normal(n)
    y = 0.3 + (y - y.mean()) / y.std(ddof=1)     # (off centre: the constant term has something to fit)
    return x, y


def case_prec(case, om, terms):
    """logpr_gauss::diaghess (logpr_gauss.cpp:122-124): 1 / (coeffsd e^rho)^2, coeffsd^2 = getvar(terms)"""
    sd = np.sqrt(np.asarray(om.getvar(terms), dtype=np.float64)) * math.exp(case["rho"])
    return 1.0 / (sd * sd)
