"""What the conditional moments cost at d = 20 with the headline term set (selectterms, p = 4096) on n = 1e5 rows.

One process, one GPU.  Timed with device events after a warm-up, three legs alternating three times per case
(|E| in 2, 4, 10; q in 1, 16), the noise measure 64 Gauss-Legendre nodes per dimension:
  (a) obhip_conditional_moments_dev, mean + variance;
  (b) the same with both gradients;
  (c) obhip_predict_multi_dev, the mean-only predictor, on the same rows (full width).
Recorded per case: G, the times and their spread, (a)/(c), (b)/(a), the profile scopes of one call of (b) (cond_coef,
cond_ck, cond_moments, cond_grad) and the share of the FP64 matrix rate the G^2 part reaches, 2 n q Gp^2 flop over the
time of cond_ck.  And the route a user has without the entry: predict_product over the rows times 256 noise points
sampled from the measure, reduced by torch (q = 1), with its time and its sampling error in W against (a).
Writes one JSON.

  python tools/conditional_bench.py [--rows 100000 --p 4096 --d 20 --es 2,4,10 --qs 1,16]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MATRIX_PEAK = 78.6e12  # MI355X data sheet, matrix FP64 flop/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--es", default="2,4,10")
    ap.add_argument("--qs", default="1,16")
    ap.add_argument("--fill", type=float, default=0.6)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "conditional_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib, obmod
    call, lib = _lib.call, _lib.lib
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ob_oracle as O
    n, p, d, f64 = args.rows, args.p, args.d, torch.float64
    kinds = ["mat25"] * d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, O.bench_knots(kinds, args.knots))
    terms = om.selectterms(p)
    t = obmod._terms_of(om, terms)
    dev = torch.device("cuda", 0)
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def timed(fn, fill):
        fn()
        torch.cuda.synchronize()
        out, t0 = [], time.perf_counter()
        while not out or time.perf_counter() - t0 < fill:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": len(v),
                "spread": (max(v) - min(v)) / statistics.median(v)}

    res = {"config": {"d": d, "n": n, "p": p, "knots": args.knots, "noise_nodes": 64},
           "source_hash": lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0), "cases": {}}
    x = torch.empty((d, n), dtype=f64, device=dev)
    ysyn = torch.empty(n, dtype=f64, device=dev)
    call("obhip_synth_xy_dev", 7, 0, n, d, np.zeros(d, dtype=np.int32).ctypes.data, x.data_ptr(), ysyn.data_ptr())
    gl_x, gl_w = ob.uniform_nodes(np.full(d, 0.02), np.full(d, 0.98), order=64)
    mom = ob.input_moments(om, t, gl_x, gl_w)
    rng = np.random.default_rng(9)
    order = (terms > 0).sum(axis=1)
    scopes = ("cond_tables", "cond_coef", "cond_ck", "cond_moments", "cond_grad")
    for ne in [int(v) for v in args.es.split(",")]:
        noise = np.arange(0, 2 * ne, 2)[:ne] if 2 * ne <= d else np.arange(ne)      # interleaved where they fit
        ctrl = np.setdiff1d(np.arange(d), noise)
        lay = ob.conditional_layout(om, t, noise)
        G, Gp, ns = lay["n_groups"], (lay["n_groups"] + 15) // 16 * 16, len(ctrl)
        de = np.ascontiguousarray(noise, dtype=np.uint32)
        xs = x[torch.from_numpy(ctrl).to(dev)].contiguous()
        for q in [int(v) for v in args.qs.split(",")]:
            Theta = rng.standard_normal((p, q)) * (0.5 ** order)[:, None]
            dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
            mean = torch.empty((q, n), dtype=f64, device=dev)
            var = torch.empty((q, n), dtype=f64, device=dev)
            gm = torch.empty((q, ns, n), dtype=f64, device=dev)
            gv = torch.empty((q, ns, n), dtype=f64, device=dev)
            pm = torch.empty((q, n), dtype=f64, device=dev)

            def leg(grad):
                call("obhip_conditional_moments_dev", om._h, t._h, dth.data_ptr(), q, de.ctypes.data, de.size,
                     mom.mean_dev.data_ptr(), mom.cov_dev.data_ptr(), xs.data_ptr(), n, 0, mean.data_ptr(),
                     var.data_ptr(), gm.data_ptr() if grad else None, gv.data_ptr() if grad else None)

            def predictor():
                call("obhip_predict_multi_dev", om._h, t._h, dth.data_ptr(), q, x.data_ptr(), n, pm.data_ptr(), None,
                     0.0, None)
            ta, tb, tc = [], [], []
            for _ in range(3):                                                       # alternating
                ta += timed(lambda: leg(False), args.fill / 3)
                tb += timed(lambda: leg(True), args.fill / 3)
                tc += timed(predictor, args.fill / 3)
            call("obhip_profile_enable", 1)
            call("obhip_profile_reset")
            leg(True)
            torch.cuda.synchronize()
            sc = {}
            for name in scopes:
                cnt, ms = C.c_uint64(0), C.c_double(0.0)
                call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
                sc[name] = {"launches": cnt.value, "ms": ms.value}
            call("obhip_profile_enable", 0)
            sa, sb, sc_ = stats(ta), stats(tb), stats(tc)
            flop = 2.0 * n * q * Gp * Gp
            case = {"G": G, "Gp": Gp, "mu_s": lay["mu_s"], "fused": lay["fused"], "mean_var": sa, "with_gradients": sb,
                    "predict_multi": sc_, "a_over_c": sa["median_ms"] / sc_["median_ms"],
                    "b_over_a": sb["median_ms"] / sa["median_ms"], "scopes_of_one_call_with_gradients": sc,
                    "g2_flop": flop,
                    "share_of_fp64_matrix_peak": (flop / (sc["cond_ck"]["ms"] * 1e-3) / FP64_MATRIX_PEAK)
                    if sc["cond_ck"]["ms"] > 0 else None}
            res["cases"]["E=%d q=%d" % (ne, q)] = case
            print("|E|=%d q=%d G=%d: (a) %.2f ms, (b) %.2f ms, (c) %.2f ms, (a)/(c) %.2f, (b)/(a) %.2f, scopes %s" % (
                ne, q, G, sa["median_ms"], sb["median_ms"], sc_["median_ms"], case["a_over_c"], case["b_over_a"],
                {k: round(v["ms"], 2) for k, v in sc.items()}), flush=True)
        # the route a user has today, q = 1: the rows times sampled noise points through predict_product
        wn = gl_w / gl_w.sum(axis=0)[None, :]
        pts = np.stack([gl_x[rng.choice(64, size=args.samples, p=wn[:, l]), l] for l in noise], axis=1)
        Theta = rng.standard_normal((p, 1)) * (0.5 ** order)[:, None]
        leg_theta = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
        mean1 = torch.empty((1, n), dtype=f64, device=dev)
        var1 = torch.empty((1, n), dtype=f64, device=dev)
        call("obhip_conditional_moments_dev", om._h, t._h, leg_theta.data_ptr(), 1, de.ctypes.data, de.size,
             mom.mean_dev.data_ptr(), mom.cov_dev.data_ptr(), xs.data_ptr(), n, 0, mean1.data_ptr(), var1.data_ptr(),
             None, None)
        from outerbase_amd import product
        xa_h = xs.cpu().numpy().T
        keep = {}

        def sampled():
            m, _ = product.predict_product_dev(om, t, Theta, xa_h, pts, de, None, 0.0)   # q x nb x na on the device
            keep["mean"], keep["var"] = m.mean(dim=1), m.var(dim=1, unbiased=True)
        ts = timed(sampled, 0.0)
        rel = ((keep["var"][0] - var1[0]).abs() / var1[0].abs()).cpu().numpy()
        res["cases"]["E=%d sampled route q=1" % ne] = {
            "samples": args.samples, "time": stats(ts), "includes_host_upload_of_rows": True,
            "relative_error_of_W_median": float(np.median(rel)), "relative_error_of_W_max": float(rel.max())}
        print("|E|=%d: %d sampled noise points through predict_product %.1f ms, relative error of W median %.3g" % (
            ne, args.samples, statistics.median(ts), float(np.median(rel))), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v.get("a_over_c") for k, v in res["cases"].items() if "a_over_c" in v}))


if __name__ == "__main__":
    main()
