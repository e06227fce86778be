"""What the Jacobian and the vector-Jacobian product of q responses cost, at d = 20 mat25, p = 4096
(selectterms), n = 1e5 new rows, q in {1, 3, 16, 32, 64}.

One process.  After one fit (coefficients of one response; the q columns are scaled copies -- the
time does not depend on the values) and a warm-up of all four legs, --reps times in turn per q
(device events around each leg):
  (a) q calls of obhip_predict_grad_dev             -- the per-response route, what MultiFit.predict_grad did
  (b) obhip_predict_jac_multi_dev, means + Jacobian -- one fused kernel per chunk of 64 responses
  (c) obhip_predict_vjp_multi_dev, means + VJP      -- the same kernel, the Jacobian never written
  (d) obhip_predict_multi_dev, means only           -- for scale
Median and min-max per leg, and the separation the feature is held to at q = 16 and q = 64:
max(b) < min(a) and max(c) <= max(b).  Writes one JSON (--out).

  timeout -k 10 900 python tools/predict_jac_bench.py [--rows 100000 --p 4096 --d 20 --reps 5]
"""
import argparse
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
    ap.add_argument("--q", type=int, nargs="+", default=[1, 3, 16, 32, 64])
    ap.add_argument("--out", default=os.path.join("profiles", "predict_jac_bench.json"))
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
    terms = np.asarray(a.terms)
    nnz = (terms > 0).sum(1)
    used = 1 + sum(len(np.unique(terms[:, l][terms[:, l] > 0])) for l in range(d))
    width = int(nnz.max()) + int(nnz.max()) % 2

    def lds_bytes(nqb):      # predict_jac_lds of csrc/kernels_predict_jac.hip
        return ((2 * used - 1 + d) * 65 + 16 * nqb * 65 + 8 * 64 + 64) * 8

    budget = 160 * 1024      # kLdsBudget of csrc/obhip_internal.h
    fused = lds_bytes(1) <= budget and width >= 2 and not os.environ.get("OBHIP_FORCE_GENERIC")
    nqb_max = max([b for b in (1, 2, 4) if lds_bytes(b) <= budget], default=0)
    rng = np.random.default_rng(1)
    per_q = {}
    for q in args.q:
        Theta = (a.theta[None, :] * torch.from_numpy(rng.uniform(0.5, 2.0, q)).to(dev)[:, None]).contiguous()
        W = torch.from_numpy(rng.standard_normal((q, n))).to(dev)
        mean = torch.empty((q, n), dtype=f64, device=dev)
        jac = torch.empty((q, d, n), dtype=f64, device=dev)
        out = torch.empty((d, n), dtype=f64, device=dev)

        def run_a():
            for j in range(q):
                call("obhip_predict_grad_dev", om, t, Theta[j].data_ptr(), x, n, mean[j].data_ptr(), jac[j].data_ptr(),
                     None, a.sigma, None, None)

        def run_b():
            call("obhip_predict_jac_multi_dev", om, t, Theta.data_ptr(), q, x, n, mean.data_ptr(), jac.data_ptr())

        def run_c():
            call("obhip_predict_vjp_multi_dev", om, t, Theta.data_ptr(), q, x, n, W.data_ptr(), n, mean.data_ptr(),
                 out.data_ptr())

        def run_d():
            call("obhip_predict_multi_dev", om, t, Theta.data_ptr(), q, x, n, mean.data_ptr(), None, a.sigma, None)

        legs = (run_a, run_b, run_c, run_d)
        for fn in legs:
            fn()
        torch.cuda.synchronize()
        times = [[] for _ in legs]
        for _ in range(args.reps):
            for v, fn in zip(times, legs):
                v.append(timed(fn))
        ta, tb, tc, td = times
        per_q[str(q)] = {"a_grad_per_response": stats(ta), "b_jac_multi": stats(tb), "c_vjp_multi": stats(tc),
                         "d_predict_multi": stats(td),
                         "b_over_a": statistics.median(tb) / statistics.median(ta),
                         "c_over_b": statistics.median(tc) / statistics.median(tb),
                         "b_below_a": bool(max(tb) < min(ta)), "c_not_above_b": bool(max(tc) <= max(tb))}
        del Theta, W, mean, jac, out
    res = {"config": {"d": d, "n": n, "p": p, "knots": args.knots, "reps": args.reps, "kinds": "mat25 x d"},
           "source_hash": _lib.lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0),
           "terms": {"used_columns": int(used), "factors_total": int(nnz.sum()), "max_factors": int(nnz.max()),
                     "fused_kernel": bool(fused), "lds_bytes_nqb_max": lds_bytes(nqb_max) if nqb_max else None,
                     "response_blocks_per_launch": nqb_max},
           "q": per_q}
    a.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({q: {k: (round(v["median_ms"], 3) if isinstance(v, dict) else v) for k, v in r.items()}
                      for q, r in per_q.items()}))


if __name__ == "__main__":
    main()
