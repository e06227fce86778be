"""What the predictor on the product of two input blocks costs, at d = 20 mat25 with the headline term set
(selectterms, p = 4096), dims_b = the last 8 dimensions, na = 1000 field rows, nb in {1e3, 1e4, 1e5} candidates.

One process.  After one fit on 100000 rows (coefficients and diagH of one response) and a warm-up of every leg,
--reps times in turn per nb (device events around each leg):
  (a) obhip_predict_product_dev, mean only
  (b) obhip_predict_product_dev, mean + variance
  (c) obhip_product_loglik_dev with coefficient and observation variances
  (d) the baseline: obhip_predict_dev on the same pairs written out as full-width rows, in chunks of at
      most 1e7 rows (the expansion itself is done before the clock starts and is not counted)
Median and min-max per leg; pairs / s of (a) and (d), their ratio, and 2 p na nb / t of (a) in TFLOP/s -- the
figure that stands next to the Gram's matrix rate.  Writes one JSON (--out).

  timeout -k 10 900 python tools/predict_product_bench.py [--na 1000 --nb 1000 10000 100000 --reps 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--na", type=int, default=1000)
    ap.add_argument("--nb", type=int, nargs="+", default=[1000, 10_000, 100_000])
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--nb-dims", type=int, default=8)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--fit-rows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join("profiles", "predict_product_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib
    from outerbase_amd.driver import HotPath
    call = _lib.call
    d, p, na = args.d, args.p, args.na
    kinds = ["mat25"] * d
    assert max(args.nb) <= args.fit_rows and na <= args.fit_rows

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}

    a = HotPath(kinds, args.knots, p, args.fit_rows)
    a.setup()
    a.step()
    torch.cuda.synchronize()
    dev, f64 = a.x.device, torch.float64
    om, t = a.om._h, a.t._h
    dims_b = np.arange(d - args.nb_dims, d, dtype=np.uint32)
    da = d - args.nb_dims
    mu_a, mu_b, fused = ob.product_layout(a.om, a.t, dims_b)
    cv = (1.0 / a.diagH).contiguous()
    nz = np.asarray(a.terms) > 0
    wa, wb = max(1, int(nz[:, :da].sum(1).max())), max(1, int(nz[:, da:].sum(1).max()))
    xa = a.xnew[:da, :na].contiguous()                       # na x |A| column-major
    y = torch.randn(na, dtype=f64, device=dev)
    ov = 0.01 * (1.0 + torch.rand(na, dtype=f64, device=dev))
    per_nb = {}
    for nb in args.nb:
        xb = a.x[da:, :nb].contiguous()                      # nb x |B| column-major
        mean = torch.empty((nb, na), dtype=f64, device=dev)
        var = torch.empty((nb, na), dtype=f64, device=dev)
        out = torch.empty((2, nb), dtype=f64, device=dev)
        # the baseline's rows, row j na + i = (xa[i], xb[j]), in chunks of whole candidates
        per = max(1, args.chunk // na)
        chunks = []
        for j0 in range(0, nb, per):
            nj = min(per, nb - j0)
            X = torch.empty((d, nj, na), dtype=f64, device=dev)
            X[:da] = xa[:, None, :]
            X[da:] = xb[:, j0:j0 + nj, None]
            chunks.append((X, nj * na))
        rowmean = torch.empty(min(per, nb) * na, dtype=f64, device=dev)

        def run_a():
            call("obhip_predict_product_dev", om, t, a.theta.data_ptr(), 1, dims_b.ctypes.data, dims_b.size, xa.data_ptr(),
                 na, xb.data_ptr(), nb, mean.data_ptr(), na, None, a.sigma, None)

        def run_b():
            call("obhip_predict_product_dev", om, t, a.theta.data_ptr(), 1, dims_b.ctypes.data, dims_b.size, xa.data_ptr(),
                 na, xb.data_ptr(), nb, mean.data_ptr(), na, cv.data_ptr(), a.sigma, var.data_ptr())

        def run_c():
            call("obhip_product_loglik_dev", om, t, a.theta.data_ptr(), dims_b.ctypes.data, dims_b.size, xa.data_ptr(), na,
                 y.data_ptr(), ov.data_ptr(), xb.data_ptr(), nb, cv.data_ptr(), a.sigma, out.data_ptr())

        def run_d():
            for X, rows in chunks:
                call("obhip_predict_dev", om, t, a.theta.data_ptr(), X.data_ptr(), rows, rowmean.data_ptr(), None, a.sigma,
                     None)

        legs = (run_a, run_b, run_c, run_d)
        for fn in legs:
            fn()
        torch.cuda.synchronize()
        # the two routes on the same pairs (the last chunk of the baseline against its part of the product)
        X, rows = chunks[-1]
        run_a()
        ref = rowmean[:rows].reshape(-1, na)
        agree = float((mean[nb - ref.shape[0]:] - ref).abs().max() / ref.abs().max())
        times = [[] for _ in legs]
        for _ in range(args.reps):
            for v, fn in zip(times, legs):
                v.append(timed(fn))
        ta, tb, tc, td = times
        pairs = float(na) * nb
        ma, md = statistics.median(ta), statistics.median(td)
        per_nb[str(nb)] = {"a_product_mean": stats(ta), "b_product_mean_var": stats(tb), "c_product_loglik": stats(tc),
                           "d_rows_mean": stats(td), "pairs": pairs,
                           "a_pairs_per_s": pairs / (ma * 1e-3), "d_pairs_per_s": pairs / (md * 1e-3),
                           "d_over_a": md / ma, "a_tflops": 2.0 * p * pairs / (ma * 1e-3) * 1e-12,
                           "b_tflops": 4.0 * p * pairs / (statistics.median(tb) * 1e-3) * 1e-12,
                           "a_against_d_maxnorm": agree}
        del xb, mean, var, out, chunks, rowmean, X, ref
    res = {"config": {"d": d, "p": p, "na": na, "dims_b": [int(v) for v in dims_b], "knots": args.knots,
                      "fit_rows": args.fit_rows, "reps": args.reps, "chunk_rows": args.chunk, "kinds": "mat25 x d"},
           "source_hash": _lib.lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0),
           "terms": {"mu_a": mu_a, "mu_b": mu_b, "fused_kernel": bool(fused and not os.environ.get("OBHIP_FORCE_GENERIC")),
                     "max_factors_a": wa, "max_factors_b": wb,
                     # predict_product_lds of csrc/kernels_product.hip
                     "lds_bytes": ((mu_a + mu_b) * 64 + 1152 + 512) * 8 + 256 * ((wa + wa % 2) // 2 + (wb + wb % 2) // 2) * 4},
           "nb": per_nb}
    a.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({nb: {k: (round(v["median_ms"], 3) if isinstance(v, dict) else v) for k, v in r.items()}
                      for nb, r in per_nb.items()}))


if __name__ == "__main__":
    main()
