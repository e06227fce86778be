"""What a Hessian-vector product of q responses costs beside the vector-Jacobian product, at d = 20
mat25, p = 4096 (selectterms), n = 1e5 new rows, q in {1, 16, 64}.

One process.  After one fit (coefficients of one response; the q columns are scaled copies -- the
time does not depend on the values) and a warm-up of all three legs, --reps times in turn per q
(device events around each leg):
  (a) obhip_predict_vjp_multi_dev, VJP only           -- the first-derivative kernel, the yardstick
  (b) obhip_predict_hvp_multi_dev, HVP only
  (c) obhip_predict_hvp_multi_dev, HVP + JVP + VJP + means
A central difference of the VJP costs 2 x (a) and keeps half the digits: the HVP is held against
that.  Median and min-max per leg and b / a, c / a.  Writes one JSON (--out).

  timeout -k 10 900 python tools/predict_hvp_bench.py [--rows 100000 --p 4096 --d 20 --reps 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--q", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--out", default=os.path.join("profiles", "predict_hvp_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from outerbase_amd import _lib
    from outerbase_amd.driver import HotPath
    call = _lib.call
    kinds = ["mat25"] * args.d
    n, d, p = args.rows, args.d, args.p

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}

    a = HotPath(kinds, args.knots, p, n)
    a.setup()
    a.step()
    torch.cuda.synchronize()
    dev, f64 = a.x.device, torch.float64
    om, t, x = a.om._h, a.t._h, a.xnew.data_ptr()
    rng = np.random.default_rng(1)
    V = torch.from_numpy(rng.standard_normal((d, n))).to(dev)
    per_q, layout = {}, {}
    for q in args.q:
        mu, rows, lds, fused = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(-1)
        call("obhip_predict_hvp_layout", t, q, C.byref(mu), C.byref(rows), C.byref(lds), C.byref(fused))
        layout[str(q)] = {"used_columns": mu.value, "tile_rows": rows.value, "lds_bytes": lds.value,
                          "fused_kernel": bool(fused.value) and not os.environ.get("OBHIP_FORCE_GENERIC")}
        Theta = (a.theta[None, :] * torch.from_numpy(rng.uniform(0.5, 2.0, q)).to(dev)[:, None]).contiguous()
        W = torch.from_numpy(rng.standard_normal((q, n))).to(dev)
        mean = torch.empty((q, n), dtype=f64, device=dev)
        jvp = torch.empty((q, n), dtype=f64, device=dev)
        out = torch.empty((d, n), dtype=f64, device=dev)
        hvp = torch.empty((d, n), dtype=f64, device=dev)

        def run_a():
            call("obhip_predict_vjp_multi_dev", om, t, Theta.data_ptr(), q, x, n, W.data_ptr(), n, None, out.data_ptr())

        def run_b():
            call("obhip_predict_hvp_multi_dev", om, t, Theta.data_ptr(), q, x, n, W.data_ptr(), n, V.data_ptr(), None,
                 None, None, hvp.data_ptr())

        def run_c():
            call("obhip_predict_hvp_multi_dev", om, t, Theta.data_ptr(), q, x, n, W.data_ptr(), n, V.data_ptr(),
                 mean.data_ptr(), out.data_ptr(), jvp.data_ptr(), hvp.data_ptr())

        legs = (run_a, run_b, run_c)
        for fn in legs:
            fn()
        torch.cuda.synchronize()
        times = [[] for _ in legs]
        for _ in range(args.reps):
            for v, fn in zip(times, legs):
                v.append(timed(fn))
        ta, tb, tc = times
        per_q[str(q)] = {"a_vjp_multi": stats(ta), "b_hvp_only": stats(tb), "c_hvp_jvp_vjp_mean": stats(tc),
                         "b_over_a": statistics.median(tb) / statistics.median(ta),
                         "c_over_a": statistics.median(tc) / statistics.median(ta),
                         "b_below_two_a": bool(statistics.median(tb) < 2 * statistics.median(ta))}
        del Theta, W, mean, jvp, out, hvp
    res = {"config": {"d": d, "n": n, "p": p, "knots": args.knots, "reps": args.reps, "kinds": "mat25 x d"},
           "source_hash": _lib.lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0),
           "layout": layout, "q": per_q}
    a.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({q: {k: (round(v["median_ms"], 3) if isinstance(v, dict) else v) for k, v in r.items()}
                      for q, r in per_q.items()}))


if __name__ == "__main__":
    main()
