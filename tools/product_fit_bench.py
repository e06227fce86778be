"""What a full grid of training data costs through NewtonAccumulator.add_product next to the existing route --
the same pairs expanded to full-width rows and added with obhip_normal_acc_add_dev -- at the headline model
(d = 20 mat25, selectterms p = 4096), dims_b = the last 8 dimensions, na = 10^3, nb = 10^3, 10^4, 10^5.

One process, one response; inputs from obhip_synth_xy_dev, everything stays on the device.  Per nb:
  add_product            obhip_normal_acc_add_product_dev into an empty accumulator (reset before every repetition);
  add_product + refit    the same followed by obhip_normal_acc_solve_dev;
  parts                  one more repetition with the library's profiling scopes on: the two stagings, the two
                         Grams, the GEMM, the dot, the moments pass and the fold, by their ProfScope names.
At nb = --rows-nb (10^3: 10^6 pairs) only, alternating with the above in the same process:
  rows + refit           the pairs expanded to rows (on the device, outside the timing), basis of the rows,
                         obhip_normal_acc_add_dev, obhip_normal_acc_solve_dev.
The row route of 10^7 and 10^8 pairs is NOT run.  Timings are device events around the calls after a warm-up of
the same work; --reps repetitions, median, min, max and all values are written (--out) with the command line.
No speed-up is asserted.

  timeout -k 10 900 python tools/product_fit_bench.py [--na 1000 --nb 1000,10000,100000 --p 4096 --reps 5]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARTS = ["product_fit_moments", "materialize_side_a", "materialize_side_b", "product_fit_gram_a", "product_fit_gram_b",
         "product_fit_gemm", "product_rhs_dot", "product_fit_fold"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--na", type=int, default=1000)
    ap.add_argument("--nb", default="1000,10000,100000")
    ap.add_argument("--rows-nb", type=int, default=1000, help="the nb at which the expanded-row route runs as well")
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--nb-dims", type=int, default=8)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "product_fit_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib
    from outerbase_amd.driver import KIND_ID, bench_knots
    call = _lib.call
    kinds = ["mat25"] * args.d
    nbs = [int(v) for v in args.nb.split(",")]
    na, p, d, f64 = args.na, args.p, args.d, torch.float64
    sigma, rho = math.log(0.01), 6.0
    dev = torch.device("cuda", torch.cuda.current_device())
    db = np.arange(d - args.nb_dims, d, dtype=np.uint32)
    da = [l for l in range(d) if l < d - args.nb_dims]

    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, bench_knots(kinds, args.knots))
    terms = om.selectterms(p)
    t = ob.obmod._Terms(om, terms)
    caps = t.maxlevels()
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    N = na + max(nbs)
    x = torch.empty((d, N), dtype=f64, device=dev)              # column-major N x d
    y = torch.empty((1, N), dtype=f64, device=dev)
    kid = (C.c_int * d)(*[KIND_ID[k] for k in kinds])
    call("obhip_synth_xy_dev", 42, 0, N, d, C.cast(kid, C.c_void_p), x.data_ptr(), y.data_ptr())
    xa = x[da, :na].contiguous()
    acc, rows_acc = ob.NewtonAccumulator(om, t, 1), ob.NewtonAccumulator(om, t, 1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}

    res = {"command": "python " + " ".join(sys.argv),
           "config": {"d": d, "na": na, "nb": nbs, "p": p, "dims_b": db.tolist(), "knots": args.knots, "reps": args.reps,
                      "sigma": sigma, "rho": rho, "layout": ob.product_fit_layout(om, t, db)},
           "source_hash": _lib.lib.obhip_source_hash(0).decode(),
           "gram_source_hash": _lib.lib.obhip_source_hash(1).decode(),
           "device": torch.cuda.get_device_name(0),
           "not_run": "the expanded-row route beyond nb = %d" % args.rows_nb, "nb": {}}

    for nb in nbs:
        xb = x[db.tolist(), na:na + nb].contiguous()
        Y = (torch.cos(2.0 * xa.sum(0))[None, :] * (1.0 + xb.sum(0))[:, None]
             + 0.05 * torch.randn((nb, na), dtype=f64, device=dev, generator=torch.Generator(dev).manual_seed(nb)))
        Y = Y.reshape(1, nb, na).contiguous()

        def add():
            acc.reset()
            acc._product_batch_dev(xa, xb, Y, na, nb, db, na, +1)

        def add_refit():
            add()
            acc._solve_dev(sigma, rho)

        with_rows = nb == args.rows_nb
        if with_rows:
            n = na * nb
            X = torch.empty((d, n), dtype=f64, device=dev)      # row i nb + j = the pair (i, j)
            X[da] = xa.repeat_interleave(nb, dim=1)
            X[db.tolist()] = xb.repeat(1, na)
            Yr = Y[0].T.reshape(1, n).contiguous()

            def rows_refit():
                rows_acc.reset()
                rows_acc._batch_dev(X, Yr, n, +1)
                rows_acc._solve_dev(sigma, rho)

            rows_refit()                                        # warm-up
        add_refit()                                             # warm-up
        ta, tr, tw = [], [], []
        for _ in range(args.reps):
            ta.append(timed(add))
            tr.append(timed(add_refit))
            if with_rows:
                tw.append(timed(rows_refit))
        call("obhip_profile_reset")
        call("obhip_profile_enable", 1)
        add()
        torch.cuda.synchronize()
        parts = {}
        for name in PARTS:
            ln, ms = C.c_uint64(0), C.c_double(0)
            call("obhip_profile_get", name.encode(), C.byref(ln), C.byref(ms))
            parts[name] = {"launches": ln.value, "ms": ms.value}
        call("obhip_profile_enable", 0)
        call("obhip_profile_reset")
        out = {"pairs": na * nb, "add_product": stats(ta), "add_product_and_refit": stats(tr), "parts_one_call": parts}
        line = "nb %6d: add_product %.2f ms, + refit %.2f ms" % (nb, statistics.median(ta), statistics.median(tr))
        if with_rows:
            out["rows_and_refit"] = stats(tw)
            tg = acc._solve_dev(sigma, rho)[0].clone()
            th = rows_acc._solve_dev(sigma, rho)[0]
            torch.cuda.synchronize()
            out["theta_rel_diff_to_rows"] = float((tg - th).abs().max() / th.abs().max())
            out["ratio_rows_over_grid"] = statistics.median(tw) / statistics.median(tr)
            line += "; expanded rows + refit %.2f ms (ratio %.1f)" % (statistics.median(tw), out["ratio_rows_over_grid"])
            del X, Yr
        print(line, flush=True)
        res["nb"][str(nb)] = out
        del xb, Y
    acc.close()
    rows_acc.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {"add_product_ms": v["add_product"]["median_ms"],
                          "add_product_and_refit_ms": v["add_product_and_refit"]["median_ms"],
                          "rows_and_refit_ms": v.get("rows_and_refit", {}).get("median_ms")} for k, v in res["nb"].items()}))


if __name__ == "__main__":
    main()
