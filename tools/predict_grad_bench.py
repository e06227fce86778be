"""What the input gradients cost next to the predictor, at BASELINE configs[2] (d=20, n=1e6, p=4096).

One process.  After one fit (coefficients, diagonal Hessian) and a warm-up of all three, --reps times
in turn (device events around each call):
  (a) obhip_predict_dev, mean only                      -- the predictor as it was
  (b) obhip_predict_grad_dev, mean + gradient
  (c) obhip_predict_grad_dev, mean + gradient + variance + variance gradient
One-sided finite differences through (a) cost (d + 1) x (a) per gradient, central ones 2 d x (a):
the ratio (b) / (a) is reported against both.  Bytes are what the kernel must move (x in, results
out); flops are those of the contraction alone (term products and their sums: the dense pass and
one pass per dimension view), the basis evaluation not counted.  Writes one JSON (--out).

  python tools/predict_grad_bench.py [--rows 1000000 --p 4096 --d 20 --reps 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "predict_grad_bench.json"))
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
    cv = 1.0 / a.diagH
    mean = torch.empty(n, dtype=f64, device=dev)
    var = torch.empty(n, dtype=f64, device=dev)
    grad = torch.empty((d, n), dtype=f64, device=dev)
    gradvar = torch.empty((d, n), dtype=f64, device=dev)
    om, t, th, x = a.om._h, a.t._h, a.theta.data_ptr(), a.xnew.data_ptr()

    def run_a():
        call("obhip_predict_dev", om, t, th, x, n, mean.data_ptr(), None, a.sigma, None)

    def run_b():
        call("obhip_predict_grad_dev", om, t, th, x, n, mean.data_ptr(), grad.data_ptr(), None, a.sigma, None, None)

    def run_c():
        call("obhip_predict_grad_dev", om, t, th, x, n, mean.data_ptr(), grad.data_ptr(), cv.data_ptr(), a.sigma,
             var.data_ptr(), gradvar.data_ptr())

    for fn in (run_a, run_b, run_c):
        fn()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(args.reps):
        ta.append(timed(run_a))
        tb.append(timed(run_b))
        tc.append(timed(run_c))

    terms = np.asarray(a.terms)
    nnz = (terms > 0).sum(1)
    used = 1 + sum(len(np.unique(terms[:, l][terms[:, l] > 0])) for l in range(d))
    # multiplies of the products plus one multiply-add (2 flops) per summand
    flops_dense = float(np.sum(np.maximum(nnz - 1, 0) + 2))
    flops_views = float(np.sum(nnz * (np.maximum(nnz - 2, 0) + 1 + 2)))
    flops_b = n * (flops_dense + flops_views)
    flops_c = n * (flops_dense + np.sum(nnz >= 0) * 2.0 + flops_views + 4.0 * np.sum(nnz))
    bytes_b = 8.0 * n * (d + 1 + d)
    bytes_c = 8.0 * n * (d + 2 + 2 * d)
    A, B, Cc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
    res = {"config": {"d": d, "n": n, "p": p, "knots": args.knots, "reps": args.reps, "kinds": "mat25 x d"},
           "source_hash": _lib.lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0),
           "terms": {"used_columns": int(used), "factors_total": int(nnz.sum()), "max_factors": int(nnz.max()),
                     "fused_kernel": bool(2 * used + d + 31 <= 320 and nnz.max() <= 8
                                          and not os.environ.get("OBHIP_FORCE_GENERIC"))},
           "a_predict_mean": stats(ta), "b_grad": stats(tb), "c_grad_var": stats(tc),
           "summary": {"b_over_a": B / A, "b_over_a_min": min(tb) / max(ta), "b_over_a_max": max(tb) / min(ta),
                       "c_over_a": Cc / A, "one_sided_differences": d + 1, "central_differences": 2 * d,
                       "b_below_d_plus_1_a": bool(max(tb) / min(ta) < d + 1),
                       "b_bytes_per_s": bytes_b / (B * 1e-3), "c_bytes_per_s": bytes_c / (Cc * 1e-3),
                       "b_contraction_fp64_flops_per_s": flops_b / (B * 1e-3),
                       "c_contraction_fp64_flops_per_s": float(flops_c) / (Cc * 1e-3)}}
    a.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"]))


if __name__ == "__main__":
    main()
