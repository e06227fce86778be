"""What gradient rows cost next to value rows in the streaming fit, at the headline terms (d=20 mat25, p=4096).

One process.  After a warm-up of both, --reps times in turn (device events around each call):
  (a) obhip_normal_acc_add_dev of n L value rows (basis build + staging + Gram + fold): NewtonAccumulator.add
  (b) obhip_normal_acc_add_grad_dev of n rows with L = d differentiated dimensions: the same Gram flops and the
      same staged bytes
and, on its own, the staging kernel through obhip_design_dx_dev on --stage-rows rows (its write rate, beside
the 5.0-5.3 TB/s of k_materialize_tl).  With --borehole the test RMSE of the fit on 1000
rows of the Borehole function with and without its analytic gradient rows (information, not a gate).
Writes one JSON (--out).

  python tools/grad_obs_bench.py [--rows 10000 100000 --p 4096 --d 20 --reps 5]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def borehole(u):
    """(y, dy/du) of the Borehole function on the unit cube (8 inputs)"""
    import numpy as np
    lo = np.array([0.05, 100.0, 63070.0, 990.0, 63.1, 700.0, 1120.0, 9855.0])
    hi = np.array([0.15, 50000.0, 115600.0, 1110.0, 116.0, 820.0, 1680.0, 12045.0])
    v = lo + (hi - lo) * u
    rw, r, Tu, Hu, Tl, Hl, L, Kw = v.T
    lr = np.log(r / rw)
    den = lr * (1 + 2 * L * Tu / (lr * rw * rw * Kw) + Tu / Tl)
    num = 2 * math.pi * Tu * (Hu - Hl)
    y = num / den
    # den = lr + 2 L Tu / (rw^2 Kw) + lr Tu / Tl
    c = 2 * L * Tu / (rw * rw * Kw)
    dden = np.stack([-(1 + Tu / Tl) / rw - 2 * c / rw, (1 + Tu / Tl) / r, c / Tu + lr / Tl, 0 * r, -lr * Tu / (Tl * Tl),
                     0 * r, c / L, -c / Kw], axis=1)
    dnum = np.stack([0 * r, 0 * r, 2 * math.pi * (Hu - Hl), 2 * math.pi * Tu, 0 * r, -2 * math.pi * Tu, 0 * r, 0 * r], axis=1)
    dy = (dnum * den[:, None] - num[:, None] * dden) / (den * den)[:, None]
    return y, dy * (hi - lo)[None, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--stage-rows", type=int, default=4096)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--borehole", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "grad_obs_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib
    from outerbase_amd.driver import HotPath
    call = _lib.call
    d, p, L = args.d, args.p, args.d
    kinds = ["mat25"] * d

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}

    res = {"config": {"d": d, "p": p, "L": L, "knots": args.knots, "reps": args.reps, "kinds": "mat25 x d"},
           "source_hash": _lib.lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0), "runs": []}
    dims = np.arange(d, dtype=np.uint32)
    for n in args.rows:
        a = HotPath(kinds, args.knots, p, n * L)
        a.setup()
        torch.cuda.synchronize()
        dev, f64 = a.x.device, torch.float64
        xv, yv = a.x, a.y.reshape(1, -1).contiguous()                     # n L value rows
        xg = a.x[:, :n].contiguous()                                       # n gradient rows
        g = torch.randn((1, L, n), dtype=f64, device=dev)
        acc = ob.NewtonAccumulator(a.om, a.terms, 1)
        acc._need()
        caps = a.t.maxlevels()

        def run_values(sign=1):
            basis = C.c_void_p()
            call("obhip_basis_create_dev", C.byref(basis), a.om._h, xv.data_ptr(), n * L, caps.ctypes.data)
            try:
                call("obhip_normal_acc_add_dev", acc._h, basis, yv.data_ptr(), n * L, sign)
                torch.cuda.synchronize()
            finally:
                call("obhip_basis_destroy", basis)

        def run_grads(sign=1):
            call("obhip_normal_acc_add_grad_dev", acc._h, xg.data_ptr(), n, dims.ctypes.data, L, None, g.data_ptr(), n, sign)

        run_values(), run_grads()
        torch.cuda.synchronize()
        tv, tg = [], []
        for _ in range(args.reps):
            tv.append(timed(run_values))
            tg.append(timed(run_grads))
        acc.close()
        a.close()
        A, B = statistics.median(tv), statistics.median(tg)
        res["runs"].append({"gradient_rows": n, "value_rows": n * L, "add_value_rows": stats(tv), "add_grad_rows": stats(tg),
                            "grad_over_values": B / A, "grad_over_values_min": min(tg) / max(tv),
                            "grad_over_values_max": max(tg) / min(tv),
                            "gram_fp64_flops_per_s_grad": 2.0 * n * L * p * (p + 1) / 2 / (B * 1e-3)})
        print(json.dumps(res["runs"][-1]))
        del a, acc, xv, yv, xg, g
        torch.cuda.empty_cache()

    # the staging kernel alone
    n = args.stage_rows
    a = HotPath(kinds, args.knots, p, n)
    a.setup()
    out = torch.empty((L, n, p), dtype=torch.float64, device=a.x.device)

    def run_stage():
        call("obhip_design_dx_dev", a.om._h, a.t._h, a.x.data_ptr(), n, dims.ctypes.data, L, None, out.data_ptr(), p)

    run_stage()
    torch.cuda.synchronize()
    ts = [timed(run_stage) for _ in range(args.reps)]
    S = statistics.median(ts)
    res["staging"] = {"rows": n, "design_dx": stats(ts), "bytes_written": 8.0 * n * L * p,
                      "write_bytes_per_s": 8.0 * n * L * p / (S * 1e-3),
                      "write_bytes_per_s_min": 8.0 * n * L * p / (max(ts) * 1e-3),
                      "write_bytes_per_s_max": 8.0 * n * L * p / (min(ts) * 1e-3),
                      "fused_kernel": not os.environ.get("OBHIP_FORCE_GENERIC")}
    print(json.dumps(res["staging"]))
    a.close()

    if args.borehole:
        k8 = ["mat25"] * 8
        om = ob.outermod()
        ob.setcovfs(om, k8)
        ob.setknot(om, [np.linspace(0.0, 1.0, args.knots)] * 8)
        terms = om.selectterms(1024)
        rng = np.random.default_rng(1)
        u, ut = 0.02 + 0.96 * rng.random((1000, 8)), 0.02 + 0.96 * rng.random((5000, 8))
        y, dy = borehole(u)
        yt, _ = borehole(ut)
        plain = ob.fit_newton_multi(om, terms, u, y)
        withg = ob.fit_newton_grad(om, terms, u, y, dy)
        rm = lambda f: float(np.sqrt(np.mean((f.predict(ut)[:, 0] - yt) ** 2)))
        res["borehole"] = {"rows": 1000, "test_rows": 5000, "p": 1024, "sd_y": float(np.std(yt)),
                           "rmse_values_only": rm(plain), "rmse_with_gradients": rm(withg)}
        print(json.dumps(res["borehole"]))

    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
