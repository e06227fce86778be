"""The Cholesky solve (csrc/kernels_chol.hip, launch_newton_solve) per entry against tests/chol_ref.py: the factor
L^ the call leaves in d_G and the solution theta^, through obhip_newton_solve_dev and
obhip_newton_multi_solve_dev, under every schedule the kernel has -- 1, 2, 4 and 8 panels per pass, the
128 x 128 update tiles forced on every strip and trailing update (OBHIP_CHOL_T64=0), and the by-rows-left
schedule (8 -> 4 -> 2 panels inside one factorisation) brought down to p = 3137 with OBHIP_CHOL_M8=2048
OBHIP_CHOL_M4=1024, plus the shipped thresholds' 4 -> 2 transition at p = 4160.

  exact case   the dyadic H = L0 L0^T: |L^ - L0| <= C x (first-order bound of the factor under theorem 10.3)
  real case    e^{-2 sigma} B^T B + diag(prec) of the oracle's B: |L^ L^^T - H| <= C gamma(p + 1) |L^| |L^|^T
  both         |H theta^ - r| <= C_s gamma(3 p + 1) |L^| |L^|^T |theta^|, every column of the batched solve too

C and C_s are eight times the worse of two float64 host routes on the same matrix, at most 1 (chol_ref's
docstring; test_chol_ref_host.py holds both routes to 8 x ratio < 1 on every case used here and stages the
failures these cases must be able to see).  The matrix that was factorised is known exactly: the library is
called with sigma = 0 on a G the host scaled, and d_diagH -- the bits k_form_hessian also wrote to the
diagonal -- is read back; in the exact case it must equal diag(H) bit for bit (rho = 100 makes every prior
precision vanish against the diagonal), in the real case the reference's H takes its diagonal from it.

The switches are read once per process: one child process (chol_exact_worker.py) per environment, which
only loads, calls and writes back.  Behind every workspace lies a sentinel-filled tail that must come back
untouched.  Every check prints one line -- the rows of the table in DESIGN.md section 6."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chol_ref as R

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chol_exact_worker.py")


def teardown_module():
    """the cached cases hold L0 and its bound at every size (0.7 GB): not for the rest of the session"""
    R.exact_case.cache_clear()
    R.multi_constants.cache_clear()


def _over(ratio, C):
    """err / tolerance from err / bound and the constant; C = 0 (p = 1: both routes exact) allows nothing"""
    if C > 0:
        return ratio / C
    return 0.0 if ratio == 0 else float("inf")


def _npd_matrix(col):
    H, _ = R.dyadic_hessian(R.NPD_P, 800)
    H[col, col] = -1e15           # indefinite whatever the prior adds to the diagonal
    return H


@pytest.mark.parametrize("name", list(R.ENVIRONMENTS))
def test_factor_and_solution_per_entry(name, tmp_path):
    """One environment of chol_ref.ENVIRONMENTS (the table of the module's docstring in rows):

      default            exact 1, 63, 64, 65, 129, 449, 1217 (one panel per pass) and 4160 (4 -> 2 panels at
                         the shipped thresholds); real 257, 705
      panels2/4/8        the sizes of the older schedule test (a pass ending inside a panel, right behind one,
                         mid-pass); real 705 and the not-positive-definite report at 8 panels
      panels2/4/8_t128   the same on 128 x 128 tiles, plus sizes that leave 1, 127, 128 and 129 rows to an
                         update (chol_ref.RAGGED_SIZES says which size gives which); real 705 and the batched
                         solve (q = 3, p = 1217) at 8 panels
      t128               the not-positive-definite report on 128 x 128 tiles
      by_rows_left       exact 3072, 3137: three passes of 8 panels, three of 4, then 2 down to a one-row last
                         panel; the batched solve (q = 3) at 3137
      by_rows_left_t128  exact 3137 on 128 x 128 tiles

    Not positive definite (p = 700): the bad pivot in the first block (column 5), a mid-pass panel (200) and
    the last ragged block (699); the error names the 64-column block and nothing faults."""
    env, exact, real, multi, npd, seconds = R.ENVIRONMENTS[name]
    d = str(tmp_path)
    jobs, info = [], {}

    def add(jname, kind, p, G, Rq, terms, rho):
        np.save(os.path.join(d, jname + "_G.npy"), np.ascontiguousarray(G))
        np.save(os.path.join(d, jname + "_R.npy"), np.ascontiguousarray(Rq))
        if terms is not None:
            np.save(os.path.join(d, jname + "_terms.npy"), terms)
        jobs.append(dict(name=jname, kind=kind, p=p, q=int(Rq.shape[0]), rho=rho, G=jname + "_G.npy",
                         R=jname + "_R.npy", terms=None if terms is None else jname + "_terms.npy"))

    for p in exact:
        c = R.exact_case(p)
        add("exact%d" % p, "solve", p, R.exact_hessian(c), c["r"][None, :], None, R.EXACT_RHO)
    for p in real:
        parts = R.real_parts(p)
        add("real%d" % p, "solve", p, parts["G"], parts["r"][None, :], parts["terms"], R.REAL_RHO)
    for case, p, q in multi:
        assert case == "exact"
        c = R.exact_case(p)
        info["multi%d" % p] = R.multi_rhs(p, q)
        add("multi%d" % p, "multi", p, R.exact_hessian(c), info["multi%d" % p], None, R.EXACT_RHO)
    for col in npd:
        add("npd%d" % col, "npd", R.NPD_P, _npd_matrix(col), R.rhs_of(R.NPD_P), None, 2.0)
    jobs.sort(key=lambda j: j["p"])       # ascending: the child stops at the first error
    with open(os.path.join(d, "jobs.json"), "w") as f:
        json.dump(jobs, f)
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("OBHIP_CHOL_")}
    child_env.update(env)
    run = subprocess.run([sys.executable, WORKER, d], env=child_env, capture_output=True, text=True, timeout=seconds)
    assert run.returncode == 0, "exit %d after %r\n%s" % (run.returncode, run.stdout[-300:], run.stderr[-2000:])
    assert [ln.split()[1] for ln in run.stdout.splitlines() if ln.startswith("done")] == [j["name"] for j in jobs]

    def out(jname, what):
        return np.load(os.path.join(d, "%s_%s.npy" % (jname, what)))

    worst = {}
    for j in jobs:
        guard = out(j["name"], "guard")
        assert guard.size == 4096 and np.all(guard == 0xA5), "%s: the call wrote behind its workspace" % j["name"]
    for p in exact:
        c, jn = R.exact_case(p), "exact%d" % p
        H = R.exact_hessian(c)
        assert np.array_equal(out(jn, "diag"), np.diagonal(H)), "p = %d: d_diagH is not diag(H) bit for bit" % p
        Lh, th = out(jn, "L"), out(jn, "theta")[0]
        rl, rs = R.factor_ratio_exact(Lh, c["L0"], c["bound"]), R.solve_ratio(H, c["r"], Lh, th)
        worst[jn] = (_over(rl, c["C"]), _over(rs, c["Cs"]))
        print("chol | %s exact p=%d: %s; device err/bound L %.3g theta %.3g, err/tolerance L %.3g theta %.3g"
              % (name, p, R.describe(c), rl, rs, *worst[jn]))
    for p in real:
        jn = "real%d" % p
        parts, diag = R.real_parts(p), out(jn, "diag")
        # G_kk + prec_k with the DEVICE model's prior precision (its own eigen-solver: not the oracle's bits), a
        # float64 sum of a positive term -- whatever it is, it is what was factorised, and the reference takes it
        assert np.all(np.isfinite(diag)) and np.all(diag >= np.diagonal(parts["G"])), "p = %d: d_diagH" % p
        want = np.diagonal(parts["G"]) + parts["prec"]
        print("chol | %s real p=%d: d_diagH against the oracle's G_kk + prec_k: %.3g relative"
              % (name, p, float(np.max(np.abs(diag - want) / want))))
        c = R.real_case(p, diag)
        Lh, th = out(jn, "L"), out(jn, "theta")[0]
        rl, rs = R.factor_residual_ratio(Lh, c["H"]), R.solve_ratio(c["H"], c["r"], Lh, th)
        worst[jn] = (_over(rl, c["C"]), _over(rs, c["Cs"]))
        print("chol | %s real p=%d: %s; device err/bound L %.3g theta %.3g, err/tolerance L %.3g theta %.3g"
              % (name, p, R.describe(c), rl, rs, *worst[jn]))
    for case, p, q in multi:
        c, jn = R.exact_case(p), "multi%d" % p
        H, Rq = R.exact_hessian(c), info[jn]
        assert np.array_equal(out(jn, "diag"), np.diagonal(H))
        Lh, Th = out(jn, "L"), out(jn, "theta")
        rl = R.factor_ratio_exact(Lh, c["L0"], c["bound"])
        Cs = R.multi_constants(p, q)
        rs = [R.solve_ratio(H, Rq[k], Lh, Th[k]) for k in range(q)]
        worst[jn] = (_over(rl, c["C"]), max(_over(rs[k], Cs[k]) for k in range(q)))
        print("chol | %s batched exact p=%d q=%d: C %.3g C_s per column %s; device err/bound L %.3g theta %s, "
              "err/tolerance L %.3g theta %.3g" % (name, p, q, c["C"], " ".join("%.3g" % v for v in Cs), rl,
                                                   " ".join("%.3g" % v for v in rs), *worst[jn]))
    for col in npd:
        with open(os.path.join(d, "npd%d_msg.txt" % col)) as f:
            msg = f.read()
        print("chol | %s not positive definite at column %d: %s" % (name, col, msg))
        assert "not positive definite" in msg and "column %d)" % (col // 64 * 64) in msg, msg
    bad = {k: v for k, v in worst.items() if not (v[0] <= 1.0 and v[1] <= 1.0)}
    assert not bad, "above tolerance (err/tolerance of L, of theta): %s" % bad
