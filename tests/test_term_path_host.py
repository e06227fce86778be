"""The term-count instrument of tests/term_path_ref.py itself, the plan of csrc/term_path_plan.h and the refusals of
the new entries (no GPU):

  - the reference against direct fits at n = 40, p = 24, step 1: a refit without each row in turn (leave-one-out),
    the dense N(0, nu I + B_k inv(P_k) B_k^T) log density (evidence) and a direct solve of every prefix (theta_k,
    mean_k, v_k);
  - as a CONDITION of every case test_gpu_term_path.py runs on the device: the float64 LAPACK route, which factors
    every prefix on its own, stays within the tolerance, and the leave-one-out cases keep max h <= 0.9;
  - a float64 restatement of the kernel's scheme (one factor, ascending columns, checkpoints, 128-row tiles, groups
    of 64) stays within it and each of five staged faults lands above it;
  - tests/term_path_check.cpp walks the plan as a program of its own, under the address and undefined-behaviour
    sanitizers;
  - what the entries refuse without a device."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import extended_ref as E
import posterior_ref as P
import term_path_ref as T

ld = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against direct fits --------------------------------------------------------------------------
def _solve_ld(A, b):
    L = P.cholesky_ld(A)
    y = P.forward_ld(L, b)
    return P.forward_ld(L.T[::-1, ::-1], y[::-1])[::-1]


def test_reference_against_direct_fits():
    """n = 40, p = 24, step 1, q = 2, sigma = log 0.3, rho = 2.  B is the oracle's float64 design matrix taken as
    exact (bB = 0), H = e^{-2 sigma} B^T B + diag(prec) rounded to float64 -- what ref_path is given -- so the
    identities hold up to that rounding: a relative perturbation u of H moves every quantity by at most about
    cond(H) u of its magnitude; allowed: 64 cond(H) u of the largest magnitude of the quantity, nothing else."""
    import ob_oracle as O
    E.require_extended()
    n, p, q, sigma, rho = 40, 24, 2, math.log(0.3), 2.0
    om = P.oracle_model()
    terms = np.asarray(om.selectterms(p), dtype=np.int64)
    x = P.inside_rows(n, 3)
    Bo = O.ob_getmat(O.OuterBase(om, x), terms)
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((n, q))
    prec = O.prior_prec(om, terms, rho)
    B, Yl, precl = np.asarray(Bo, dtype=ld), np.asarray(Y, dtype=ld), np.asarray(prec, dtype=ld)
    e2, nu = np.exp(-2 * ld(sigma)), np.exp(2 * ld(sigma))
    Hl = e2 * (B.T @ B) + np.diag(precl)
    H = E._f64(Hl)
    H = 0.5 * (H + H.T)
    G = E._f64(e2 * (B.T @ Yl))
    Gl = np.asarray(G, dtype=ld)
    allow = 64 * np.linalg.cond(H) * E.U
    yty = E._f64((Yl * Yl).sum(axis=0))
    hold = T.ref_path(H, None, False, B, np.zeros((n, p)), G, Y, sigma, 1, False)
    loo = T.ref_path(H, None, False, B, np.zeros((n, p)), G, Y, sigma, 1, True)
    ev, _ = T.ref_evidence(H, None, False, G, prec, yty, n, sigma, 1)
    _, _, thetas = T.ref_coef(H, None, False, G, 1, ks_theta=tuple(range(1, p + 1)))
    assert hold["ks"] == list(range(1, p + 1))
    worst = 0.0

    def close(got, want, what):
        nonlocal worst
        err = float(np.max(np.abs(E._f64(np.asarray(got, dtype=ld) - np.asarray(want, dtype=ld)))))
        mag = float(np.max(np.abs(E._f64(want))))
        worst = max(worst, err / mag)
        assert err <= allow * mag, (what, err, mag)

    for c, k in enumerate(hold["ks"]):
        Bk, Hk = B[:, :k], np.asarray(H, dtype=ld)[:k, :k]
        theta = _solve_ld(Hk, Gl[:k])
        close(thetas[k][0][:k], theta, "theta_%d" % k)
        assert not np.any(thetas[k][0][k:])
        mean = Bk @ theta
        Sk = _solve_ld(Hk, Bk.T)                                       # inv(H_k) B_k^T
        v = np.einsum("ik,ki->i", Bk, Sk)
        close(hold["mean"][c], mean, "mean_%d" % k)
        close(hold["v"][c], v, "v_%d" % k)
        r = Yl - mean
        s2 = nu + v
        close(hold["scores"][c, :, 0], (r * r).sum(axis=0), "sse_%d" % k)
        close(hold["scores"][c, :, 1], (r * r).sum(axis=0), "spe_%d hold-out" % k)
        lpd = (-(T.LOG2PI + np.log(s2))[:, None] / 2 - r * r / s2[:, None] / 2).sum(axis=0)
        close(hold["scores"][c, :, 2], lpd, "lpd_%d hold-out" % k)
        close(hold["sumv"][c], v.sum(), "sumv_%d" % k)
        # a refit without each row in turn
        spe, lpl = np.zeros(q, dtype=ld), np.zeros(q, dtype=ld)
        for i in range(n):
            b = Bk[i]
            Hm = Hk - e2 * np.outer(b, b)
            gm = Gl[:k] - e2 * np.outer(b, Yl[i])
            th = _solve_ld(Hm, gm)
            e = Yl[i] - b @ th
            s2i = nu + b @ _solve_ld(Hm, b[:, None])[:, 0]
            spe += e * e
            lpl += -(T.LOG2PI + np.log(s2i)) / 2 - e * e / s2i / 2
        close(loo["scores"][c, :, 1], spe, "PRESS_%d" % k)
        close(loo["scores"][c, :, 2], lpl, "loo lpd_%d" % k)
        close(loo["scores"][c, :, 0], (r * r).sum(axis=0), "sse_%d loo" % k)
        # the evidence: y ~ N(0, nu I + B_k inv(P_k) B_k^T)
        Cov = nu * np.eye(n, dtype=ld) + (Bk / precl[None, :k]) @ Bk.T
        Lc = P.cholesky_ld(Cov)
        w = P.forward_ld(Lc, Yl)
        dens = -(ld(n) / 2) * T.LOG2PI - np.log(np.diagonal(Lc)).sum() - (w * w).sum(axis=0) / 2
        close(ev[c], dens, "evidence_%d" % k)
    print("term path | reference against direct fits, n = 40, p = 24, every prefix: worst relative difference %.3g "
          "(allowed %.3g = 64 cond(H) u, cond(H) = %.3g)" % (worst, allow, np.linalg.cond(H)))


# ---- the condition of every device case ---------------------------------------------------------------------------
def _check_route(label, c):
    ratios = T.score_ratios(c["h64"]["scores"], c["h64"]["sumv"], c)
    print("term path | %s: float64 route err/bound %.3g (probe %.3g), C %.3g, err/tol %s"
          % (label, c["r"], c["r_probe"], c["C"], {k: "%.3g" % v for k, v in ratios.items()}))
    assert 8 * max(c["r"], c["r_probe"]) < E.C_CAP
    assert max(ratios.values()) <= 1.0, ratios
    assert np.all(np.isfinite(E._f64(c["ref"]["scores"])))


@pytest.mark.parametrize("p,n,step", T.HOLD_CASES)
def test_float64_route_is_within_the_hold_out_tolerance(p, n, step):
    _check_route("hold-out p=%d n=%d step=%d" % (p, n, step), T.hold_case(p, n, step))


@pytest.mark.parametrize("q", T.HOLD_Q)
def test_float64_route_with_several_responses(q):
    _check_route("hold-out p=129 n=130 step=16 q=%d" % q, T.hold_case(129, 130, 16, q))


@pytest.mark.parametrize("p,step", T.LOO_CASES)
@pytest.mark.parametrize("q", T.LOO_Q)
def test_float64_route_is_within_the_leave_one_out_tolerance(p, step, q):
    c = T.loo_case(p, step, q)
    _check_route("loo p=%d step=%d q=%d" % (p, step, q), c)
    print("term path | loo p=%d: max h %.3g" % (p, c["ref"]["hmax"]))
    assert 0.0 < c["ref"]["hmax"] <= 0.9


def test_float64_route_of_the_coefficients_and_the_evidence():
    """U, Theta_k at k in (1, 64, 65, p) and the evidence at every checkpoint, p = 385 on the real Hessian (every
    prefix factored on its own in the reference): the float64 route -- ONE LAPACK factor, nested -- is within the
    rest (there is no design matrix in either, so no C)"""
    c = T.real(385)
    H, G, p = c["H"], c["G"], 385
    ks = (1, 64, 65, p)
    u, ru, thetas = T.ref_coef(H, None, False, G, 64, ks_theta=ks, backward=True)
    L64 = np.linalg.cholesky(H)
    u64 = np.linalg.solve(L64, G)
    assert E.worst_ratio(u64, u, ru) <= 1.0
    for k in ks:
        th64 = np.zeros_like(G)
        th64[:k] = np.linalg.solve(L64[:k, :k].T, u64[:k])
        assert E.worst_ratio(th64, thetas[k][0], thetas[k][1]) <= 1.0, k
    prec = np.exp(-np.linspace(0.0, 9.0, p))
    yty = np.array([1499.0, 1499.0, 1499.0])
    want, rest = T.ref_evidence(H, None, False, G, prec, yty, 1500, c["sigma"], 64, backward=True)
    got = T.host_evidence64(H, G, prec, yty, 1500, c["sigma"], 64)
    r = E.worst_ratio(got, want, rest)
    print("term path | evidence p=385 step=64: float64 route err/rest %.3g" % r)
    assert r <= 1.0


# ---- the failures the chosen inputs must be able to see -------------------------------------------------------------
def test_staged_failures_land_above_the_tolerance():
    """the scheme of k_term_path in float64 on the leave-one-out case p = 385, step 64, q = 3, 300 rows (three row
    tiles, four column tiles, nu = 0.01): clean it is within the tolerance; each staged fault is above it in at
    least one of sse, spe, lpd, sumv"""
    c = T.loo_case(385, 64, 3)
    run = lambda fault: T.score_ratios(*T.scheme64(c["H"], c["Bo"], c["G"], c["Y"], c["sigma"], 64, True, fault), c)
    clean = run(None)
    assert max(clean.values()) <= 1.0, clean
    for fault in (("tile", 2, 1), "early", "u_short", "restart", "h_nu"):
        ratios = run(fault)
        print("term path | staged %s: err/tol %s (clean %.3g)" % (fault, {k: "%.3g" % v for k, v in ratios.items()},
                                                                  max(clean.values())))
        assert max(ratios.values()) > 1.0, fault


def test_staged_failures_in_hold_out_mode():
    """the same in hold-out mode on the dyadic Hessian, p = 385, n = 130 (two row tiles), step 16"""
    c = T.hold_case(385, 130, 16)
    run = lambda fault: T.score_ratios(*T.scheme64(c["H"], c["Bo"], c["G"], c["Y"], 0.0, 16, False, fault), c)
    assert max(run(None).values()) <= 1.0
    for fault in (("tile", 20, 1), "early", "u_short", "restart"):
        assert max(run(fault).values()) > 1.0, fault


# ---- the plan -----------------------------------------------------------------------------------------------------
def test_plan_walked_by_a_program_of_its_own(tmp_path):
    # any host C++17 compiler will do: the program is plain C++ (the ROCm tree brings clang++ where g++ is missing)
    found = [shutil.which(c) for c in ("g++", "c++", "clang++")] + \
        [c for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(c)]
    found = [c for c in found if c]
    assert found, "no host C++ compiler: the only walk of the plan cannot run"
    gxx = found[0]
    exe = str(tmp_path / "term_path_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "term_path_check.cpp"), "-o", exe], check=True)
    result = subprocess.run([exe], capture_output=True, text=True)
    assert result.stderr == "", result.stderr
    assert result.returncode == 0, result.stdout
    last = result.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000, result.stdout


def test_plan_header_is_plain_cpp():
    with open(os.path.join(ROOT, "outerbase_amd", "csrc", "term_path_plan.h")) as f:
        plain, frame = f.read().split("#if defined(__HIPCC__)")
    assert [ln.split()[1] for ln in plain.splitlines() if ln.startswith("#include")] == \
        ["<algorithm>", "<cstdint>", '"row_chunks.h"']
    assert "#include" not in frame and "getenv" not in plain + frame


def test_checkpoints_of_the_reference_and_the_layout_entry_agree():
    from outerbase_amd._lib import call
    for p in (1, 15, 16, 17, 129, 385):
        for step in (1, 7, 16, 129, 1000):
            K, used, scratch = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            call("obhip_term_path_layout", p, 3, step, 300, 0, C.byref(K), C.byref(used), C.byref(scratch))
            ks = T.checkpoints(p, step)
            assert K.value == len(ks) and ks[-1] == p and all(b > a for a, b in zip(ks, ks[1:]))
            assert used.value % 128 == 0 and used.value >= 128
            pp, E_ = (p + 127) // 128 * 128, K.value * 10
            assert scratch.value == 8 * (384 * pp + 3 * E_ + E_)      # Z of 300 rows padded, 3 tiles, 1 group


# ---- the tie rule of TermPathResult.best (host arithmetic) ------------------------------------------------------------
def test_best_takes_the_lowest_size_on_a_tie():
    import outerbase_amd as ob
    sizes = np.array([16, 32, 48, 64])
    ev = np.array([[1.0, 0.0], [3.0, 2.0], [3.0, 2.0], [2.0, 3.0]])
    res = ob.TermPathResult(None, None, None, None, sizes, ev, None, 0.0, 6.0, False)
    assert res.best() == 32 and res.best(response=0) == 32 and res.best(response=1) == 64
    res.spe = np.array([[2.0, 5.0], [1.0, 4.0], [1.0, 4.0], [1.0, 6.0]])
    res.lpd = -res.spe
    assert res.best("spe") == 32 and res.best("lpd") == 32 and res.best("spe", response=0) == 32
    with pytest.raises(ValueError):
        res.best("rmse")


# ---- refusals that need no device -------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    from outerbase_amd._lib import ObhipError, lib
    K = C.c_uint64(0)
    buf = (C.c_double * 8)()
    a = C.addressof(buf)

    def refused(name, *args):
        rc = getattr(lib, name)(*args)
        assert rc == 1, (name, rc)                                     # OBHIP_ERR_INVALID
        assert lib.obhip_last_error()

    refused("obhip_term_path_layout", 0, 1, 1, 0, 0, C.byref(K), None, None)
    refused("obhip_term_path_layout", 65536, 1, 1, 0, 0, C.byref(K), None, None)
    refused("obhip_term_path_layout", 8, 0, 1, 0, 0, C.byref(K), None, None)
    refused("obhip_term_path_layout", 8, 65535, 1, 0, 0, C.byref(K), None, None)
    refused("obhip_term_path_layout", 8, 1, 0, 0, 0, C.byref(K), None, None)
    refused("obhip_term_path_layout", 8, 1, 1, 10, 100, C.byref(K), None, None)
    refused("obhip_term_path_layout", 8, 1, 1, (1 << 40) + 1, 0, C.byref(K), None, None)
    assert K.value == 0                                                # a refused call writes nothing
    assert lib.obhip_term_path_layout(8, 1, 3, 0, 0, None, None, None) == 0
    refused("obhip_normal_acc_rhs_dev", None, None, 0.0, a, a)
    refused("obhip_posterior_path_coef_dev", None, a, 1, a)
    refused("obhip_posterior_path_theta_dev", None, a, 1, 1, a)
    refused("obhip_posterior_path_evidence", None, a, 1, a, a, 10, 1, a)
    refused("obhip_posterior_path_scores_dev", None, a, 1, a, 1, a, 1, None, 1, 0, 0, a, a)
    assert lib.obhip_abi_version() == 5
    assert ObhipError is not None
