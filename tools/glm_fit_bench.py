"""What an IRLS iteration costs next to the Gaussian one-step fit, at d=20, n=1e6, p=4096.

One process, one basis.  Timed with device events, --reps times after a warm-up of each:
  (a) obhip_fit_newton_multi_dev (q = 1) with the design matrix staged anew (a GLM fit before it has
      invalidated the staged one: what an IRLS iteration has to do as well) and with the matrix found staged;
  (b) obhip_fit_glm_dev with maxit = 1 (one iteration) and to convergence (tol 1e-8), binomial and Poisson;
  (c) obhip_glm_rows_dev alone, in GB/s of the 8 x 8 bytes per row it reads and writes.
One profiled fit of each family gives the per-scope times (obhip_profile_get); the summary reports
iteration / Gaussian step and, above 1.10, the scopes the difference falls on.  Writes one JSON (--out).

  python tools/glm_fit_bench.py [--rows 1000000 --p 4096 --d 20 --reps 3]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCOPES = ["glm_rows", "glm_rows_trial", "materialize_B", "gram", "tmm", "mm", "cholesky", "backsolve", "form_hessian"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "glm_fit_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib, obmod
    from outerbase_amd.glm import GlmInfo
    call, lib = _lib.call, _lib.lib
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import ob_oracle as O
    n, p, d, f64 = args.rows, args.p, args.d, torch.float64
    kinds = ["mat25"] * d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, O.bench_knots(kinds, args.knots))
    t = obmod._terms_of(om, om.selectterms(p))
    dev = torch.device("cuda", 0)
    x = torch.empty((d, n), dtype=f64, device=dev)
    ysyn = torch.empty(n, dtype=f64, device=dev)
    kk = np.zeros(d, dtype=np.int32)
    call("obhip_synth_xy_dev", 7, 0, n, d, kk.ctypes.data, x.data_ptr(), ysyn.data_ptr())
    f = (ysyn - ysyn.mean()) / ysyn.std()
    torch.manual_seed(3)
    trials = torch.randint(1, 6, (n,), device=dev).to(f64)
    yb = torch.binomial(trials, torch.sigmoid(1.5 * f)) / trials
    off = torch.log(0.5 + 3.5 * torch.rand(n, dtype=f64, device=dev))
    yp = torch.poisson(torch.exp(0.8 * f + 1.0 + off))
    basis = C.c_void_p()
    call("obhip_basis_create_dev", C.byref(basis), om._h, x.data_ptr(), n, t.maxlevels().ctypes.data)
    wsb, wsg = C.c_uint64(0), C.c_uint64(0)
    call("obhip_glm_workspace_bytes", p, n, C.byref(wsb))
    call("obhip_newton_multi_workspace_bytes", p, 1, C.byref(wsg))
    ws = torch.empty(max(wsb.value, wsg.value), dtype=torch.uint8, device=dev)
    H = torch.empty((p, p), dtype=f64, device=dev)
    g, th, dh = (torch.empty(p, dtype=f64, device=dev) for _ in range(3))
    eta = torch.empty(n, dtype=f64, device=dev)
    sigma, rho = math.log(0.01), 6.0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def gauss():
        call("obhip_fit_newton_multi_dev", None, basis, t._h, om._h, f.data_ptr(), 1, n, sigma, rho, H.data_ptr(),
             g.data_ptr(), th.data_ptr(), dh.data_ptr(), None, 0, ws.data_ptr(), wsg.value)

    def glm(family, y, a, o, maxit):
        info = GlmInfo()
        call("obhip_fit_glm_dev", basis, t._h, om._h, family, y.data_ptr(), None if a is None else a.data_ptr(),
             None if o is None else o.data_ptr(), sigma, rho, 1e-8, maxit, H.data_ptr(), th.data_ptr(), dh.data_ptr(),
             eta.data_ptr(), C.byref(info), ws.data_ptr(), wsb.value)
        return info

    def scopes(fn):
        call("obhip_profile_enable", 1)
        call("obhip_profile_reset")
        fn()
        torch.cuda.synchronize()
        out = {}
        for name in SCOPES:
            cnt, ms = C.c_uint64(0), C.c_double(0.0)
            call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
            if cnt.value:
                out[name] = {"launches": cnt.value, "ms": ms.value}
        call("obhip_profile_enable", 0)
        return out

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}

    fams = {"binomial": (1, yb, trials, None), "poisson": (2, yp, None, off)}
    res = {"config": {"d": d, "n": n, "p": p, "knots": args.knots, "reps": args.reps},
           "source_hash": lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0), "families": {}}
    glm(1, yb, trials, None, 1)       # warm-up of both; leaves no staged matrix behind
    gauss()
    torch.cuda.synchronize()
    restaged, staged = [], []
    for _ in range(args.reps):
        glm(1, yb, trials, None, 1)
        restaged.append(timed(gauss)[0])
        staged.append(timed(gauss)[0])
    res["gaussian_step"] = {"staged_anew": stats(restaged), "found_staged": stats(staged)}
    glm(1, yb, trials, None, 1)
    res["gaussian_step"]["scopes_staged_anew"] = scopes(gauss)
    Tg = statistics.median(restaged)
    for name, (fam, y, a, o) in fams.items():
        one, whole, its = [], [], []
        for _ in range(args.reps):
            one.append(timed(lambda: glm(fam, y, a, o, 1))[0])
            ms, info = timed(lambda: glm(fam, y, a, o, 25))
            whole.append(ms)
            its.append((int(info.iterations), int(info.halvings), int(info.converged)))
        sc = scopes(lambda: glm(fam, y, a, o, 25))
        per_it = [w / i[0] for w, i in zip(whole, its)]
        res["families"][name] = {"one_iteration": stats(one), "whole_fit": stats(whole), "per_iteration": stats(per_it),
                                 "iterations_halvings_converged": its, "scopes_of_a_whole_fit": sc}
        print("%-8s one iteration %.1f ms, whole fit %.1f ms in %d iterations (%d halvings): %.1f ms per iteration; "
              "Gaussian step %.1f ms staged anew, %.1f ms found staged"
              % (name, statistics.median(one), statistics.median(whole), its[0][0], its[0][1], statistics.median(per_it),
                 Tg, statistics.median(staged)), flush=True)
    # the row pass alone
    n_pad = (n + 63) // 64 * 64
    sc_in = torch.rand(n_pad, dtype=f64, device=dev)
    outs = [torch.empty(n_pad, dtype=f64, device=dev) for _ in range(4)]
    sums = torch.empty(3, dtype=f64, device=dev)
    etain = 0.8 * f
    rows = {}
    for name, (fam, y, a, o) in fams.items():
        def rp():
            call("obhip_glm_rows_dev", fam, n, etain.data_ptr(), None, 0.0, y.data_ptr(), None if a is None else a.data_ptr(),
                 None, sigma, sc_in.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                 outs[3].data_ptr(), sums.data_ptr())
        rp()
        v = [timed(rp)[0] for _ in range(args.reps + 2)][2:]
        nbytes = 8.0 * n * (8 if a is not None else 7)
        rows[name] = dict(stats(v), GB_per_s=nbytes / (statistics.median(v) * 1e-3) / 1e9)
    res["row_pass"] = rows
    call("obhip_basis_destroy", basis)
    summ = {"gaussian_step_staged_anew_ms": Tg, "gaussian_step_found_staged_ms": statistics.median(staged)}
    gs = res["gaussian_step"]["scopes_staged_anew"]
    for name, r in res["families"].items():
        ratio = r["per_iteration"]["median_ms"] / Tg
        summ[name + "_iteration_over_gaussian_step"] = ratio
        summ[name + "_row_pass_GB_per_s"] = rows[name]["GB_per_s"]
        if ratio > 1.10:
            k = r["iterations_halvings_converged"][0][0]
            extra = {s: v["ms"] / k - gs.get(s, {"ms": 0.0})["ms"] for s, v in r["scopes_of_a_whole_fit"].items()}
            summ[name + "_excess_ms_per_iteration_by_scope"] = dict(sorted(extra.items(), key=lambda kv: -kv[1]))
    res["summary"] = summ
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(summ))


if __name__ == "__main__":
    main()
