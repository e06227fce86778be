"""What the gradient of the calibration likelihood by the candidate parameters costs, in the setting of
tools/predict_product_bench.py: d = 20 mat25, the headline term set (selectterms, p = 4096), dims_b = the last 8
dimensions (L = 8), na = 1000 field rows, nb in {1e4, 1e5} candidates, coefficient and observation variances on.

One process.  After one fit on 100000 rows and a warm-up of every leg, --reps times in turn per nb (device events
around each leg):
  (g) obhip_product_loglik_grad_dev: the two sums and their 2 L gradient columns
  (v) obhip_product_loglik_dev on the same inputs: the sums alone
  (c) 2 L calls of obhip_product_loglik_dev at xb -+ h e_l: the central-difference route to the same gradient
      (the 2 L shifted copies of xb are made before the clock starts)
Median and min-max per leg, g / v, c / g, and the largest difference between (g)'s gradient and (c)'s, relative to
the gradient's largest entry.  Also view_terms / p, the LDS of the two kernels, and -- given --remarks, the text hipcc
prints for csrc/kernels_product_dx.hip under -Rpass-analysis=kernel-resource-usage -- the registers, scratch and
occupancy of every variant of k_product_grad.

--occupancy LABEL: instead, time the two variants of the kernel whose allocation OBHIP_PG_MIN_BLOCKS sets (pair
gradients with the variance; likelihood gradient without it) at dims_b = the last 2 dimensions, where two
workgroups fit a CU's LDS, and write them under LABEL; --merge FILE .. adds such files, one per build, to the result.

  timeout -k 10 900 python tools/product_grad_bench.py [--nb 10000 100000 --reps 5]
"""
import argparse
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_remarks(path):
    """{kernel variant: {vgprs, agprs, scratch_bytes_per_lane, occupancy_waves_per_simd}} of k_product_grad"""
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            v = re.search(r"k_product_gradILb([01])ELb([01])E", m.group(1))
            cur = "k_product_grad<VAR=%s, LIK=%s>" % v.groups() if v else None
            if cur:
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z\[\]/ ]+): (\d+)", line)
        if cur and m and m.group(1).strip() in keys:
            out[cur][keys[m.group(1).strip()]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--na", type=int, default=1000)
    ap.add_argument("--nb", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--nb-dims", type=int, default=8)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--fit-rows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--h", type=float, default=2.0 ** -20)
    ap.add_argument("--remarks", default=None)
    ap.add_argument("--occupancy", default=None, metavar="LABEL")
    ap.add_argument("--merge", nargs="*", default=[], metavar="FILE")
    ap.add_argument("--out", default=os.path.join("profiles", "product_grad_bench.json"))
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

    def measure(legs):
        for fn in legs:
            fn()
        torch.cuda.synchronize()
        times = [[] for _ in legs]
        for _ in range(args.reps):
            for v, fn in zip(times, legs):
                v.append(timed(fn))
        return times

    a = HotPath(kinds, args.knots, p, args.fit_rows)
    a.setup()
    a.step()
    torch.cuda.synchronize()
    dev, f64 = a.x.device, torch.float64
    om, t = a.om._h, a.t._h
    cv = (1.0 / a.diagH).contiguous()
    y = torch.randn(na, dtype=f64, device=dev)
    ov = 0.01 * (1.0 + torch.rand(na, dtype=f64, device=dev))
    nz = np.asarray(a.terms) > 0

    def split(nb_dims):
        dims_b = np.arange(d - nb_dims, d, dtype=np.uint32)
        da = d - nb_dims
        mu_a, mu_b, view_terms, fused = ob.product_grad_layout(a.om, a.t, dims_b)
        wa, wb = max(1, int(nz[:, :da].sum(1).max())), max(1, int(nz[:, da:].sum(1).max()))
        w2 = (wa + wa % 2) // 2 + (wb + wb % 2) // 2
        lay = {"dims_b": [int(v) for v in dims_b], "mu_a": mu_a, "mu_b": mu_b, "view_terms": view_terms,
               "view_terms_over_p": view_terms / p, "max_factors_a": wa, "max_factors_b": wb,
               "fused_kernel": bool(fused and not os.environ.get("OBHIP_FORCE_GENERIC")),
               # predict_product_lds of csrc/kernels_product.hip, product_grad_lds of csrc/kernels_product_dx.hip
               "lds_bytes_values": ((mu_a + mu_b) * 64 + 1152 + 512) * 8 + 256 * w2 * 4,
               "lds_bytes_gradient": ((mu_a + 2 * mu_b - 1 + nb_dims) * 64 + 1152 + 128 + 512) * 8 + 256 * (w2 + 1) * 4}
        return dims_b, da, lay

    base = {"config": {"d": d, "p": p, "na": na, "knots": args.knots, "fit_rows": args.fit_rows, "reps": args.reps,
                       "kinds": "mat25 x d"},
            "source_hash": _lib.lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0)}

    if args.occupancy:
        dims_b, da, lay = split(2)
        nb = args.nb[0]
        xa, xb = a.xnew[:da, :na].contiguous(), a.x[da:, :nb].contiguous()
        dmean = torch.empty((2, nb, na), dtype=f64, device=dev)
        dvar = torch.empty((2, nb, na), dtype=f64, device=dev)
        out = torch.empty((6, nb), dtype=f64, device=dev)

        def pair_grad_var():
            call("obhip_predict_product_grad_dev", om, t, a.theta.data_ptr(), dims_b.ctypes.data, 2, xa.data_ptr(), na,
                 xb.data_ptr(), nb, dmean.data_ptr(), na, cv.data_ptr(), a.sigma, dvar.data_ptr())

        def loglik_grad_novar():
            call("obhip_product_loglik_grad_dev", om, t, a.theta.data_ptr(), dims_b.ctypes.data, 2, xa.data_ptr(), na,
                 y.data_ptr(), ov.data_ptr(), xb.data_ptr(), nb, None, a.sigma, out.data_ptr())

        tp, tl = measure((pair_grad_var, loglik_grad_novar))
        res = dict(base, label=args.occupancy, nb=nb, split=lay, pair_grad_var=stats(tp), loglik_grad_novar=stats(tl))
        a.close()
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({"label": args.occupancy, "pair_grad_var_ms": round(statistics.median(tp), 3),
                          "loglik_grad_novar_ms": round(statistics.median(tl), 3)}))
        return

    dims_b, da, lay = split(args.nb_dims)
    L = args.nb_dims
    xa = a.xnew[:da, :na].contiguous()                       # na x |A| column-major
    per_nb = {}
    for nb in args.nb:
        xb = a.x[da:, :nb].contiguous()                      # nb x |B| column-major
        g = torch.empty((2 + 2 * L, nb), dtype=f64, device=dev)
        v = torch.empty((2, nb), dtype=f64, device=dev)
        shifted = []
        for l in range(L):
            for sgn in (1.0, -1.0):
                xs = xb.clone()
                xs[l] += sgn * args.h
                shifted.append(xs)
        cd = torch.empty((2 * L, 2, nb), dtype=f64, device=dev)

        def loglik(xs, out):
            call("obhip_product_loglik_dev", om, t, a.theta.data_ptr(), dims_b.ctypes.data, L, xa.data_ptr(), na,
                 y.data_ptr(), ov.data_ptr(), xs.data_ptr(), nb, cv.data_ptr(), a.sigma, out.data_ptr())

        def run_g():
            call("obhip_product_loglik_grad_dev", om, t, a.theta.data_ptr(), dims_b.ctypes.data, L, xa.data_ptr(), na,
                 y.data_ptr(), ov.data_ptr(), xb.data_ptr(), nb, cv.data_ptr(), a.sigma, g.data_ptr())

        def run_v():
            loglik(xb, v)

        def run_c():
            for k, xs in enumerate(shifted):
                loglik(xs, cd[k])

        tg, tv, tc = measure((run_g, run_v, run_c))
        diff = (cd[0::2] - cd[1::2]) / (2 * args.h)          # L x 2 x nb
        fd = torch.cat([diff[:, 0], diff[:, 1]])             # the order of g's gradient columns
        mg, mv, mc = (statistics.median(x) for x in (tg, tv, tc))
        per_nb[str(nb)] = {"g_loglik_grad": stats(tg), "v_loglik": stats(tv), "c_central_differences_2L_calls": stats(tc),
                           "g_over_v": mg / mv, "c_over_g": mc / mg,
                           "values_same_bits": bool(torch.equal(g[:2], v)),
                           "g_against_c_maxnorm": float((g[2:] - fd).abs().max() / g[2:].abs().max())}
        del xb, g, v, shifted, cd, diff, fd
    res = dict(base, split=lay, h=args.h, nb=per_nb)
    if args.remarks:
        res["kernel_resource_usage"] = parse_remarks(args.remarks)
    if args.merge:
        res["workgroups_per_cu"] = {"note": "OBHIP_PG_MIN_BLOCKS of csrc/kernels_product_dx.hip, one build each; "
                                            "dims_b = the last 2 dimensions, where two workgroups fit a CU's LDS"}
        for path in args.merge:
            other = json.load(open(path))
            res["workgroups_per_cu"][other["label"]] = {k: other[k] for k in ("nb", "split", "source_hash",
                                                                               "pair_grad_var", "loglik_grad_novar")}
    a.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({nb: {k: (round(v["median_ms"], 3) if isinstance(v, dict) else v) for k, v in r.items()}
                      for nb, r in per_nb.items()}))


if __name__ == "__main__":
    main()
