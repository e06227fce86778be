"""What Thompson picks cost at d = 20 with the headline term set (selectterms, p = 4096): the optimum of S = 64,
256 and 1024 posterior draws over m = 1e6 candidates, alternating in one process

  (a) obhip_posterior_extremum_dev on the fused kernel (k_sample_ext: the m x S paths are never stored),
  (b) the yardstick: obhip_posterior_sample_dev into an m x S buffer (8 GB at S = 1024, in one piece) and
      torch.argmin(dim=0) over it,
  (c) obhip_posterior_extremum_dev on the unfused route (OBHIP_FORCE_GENERIC: the column loop over the
      single-response predictor into scratch, k_sample_colext).

Timed with device events after a warm-up, --reps runs each; min ... max are reported.  Also recorded: one
launch_predict_multi pass of 64 columns alone (obhip_predict_multi_dev with 65 responses: one by the single
predictor, 64 batched; scope predict_multi), the fused kernel's time per pass (64 draws at S = 64, 128 beyond
where the wider pass fits the LDS) and k_draw's per launch from the library's own event scopes (sample_ext,
draw), and whether the three routes return the same indices.

The GPU part runs as a child process under its own `timeout -k 10`.

  python tools/sample_bench.py [--rows 1000000 --p 4096 --d 20 --draws 64,256,1024]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 900      # seconds the GPU part may take


def scope(lib, name):
    cnt, ms = C.c_uint64(0), C.c_double(0.0)
    lib.call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
    return {"launches": cnt.value, "ms": ms.value}


def spread(v):
    return {"min": min(v), "max": max(v), "runs": list(v)}


def part(args):
    import numpy as np
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib as lib
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ob_oracle as O
    kinds = ["mat25"] * args.d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, O.bench_knots(kinds, args.knots))
    terms = om.selectterms(args.p)
    dev = torch.device("cuda", 0)
    f64 = torch.float64
    lib.call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def synth(seed, n):
        x = torch.empty((args.d, n), dtype=f64, device=dev)
        y = torch.empty((1, n), dtype=f64, device=dev)
        lib.call("obhip_synth_xy_dev", seed, 0, n, args.d, np.zeros(args.d, dtype=np.int32).ctypes.data, x.data_ptr(),
                 y.data_ptr())
        return x, y
    acc = ob.NewtonAccumulator(om, terms, 1)
    xf, yf = synth(3, args.fit_rows)
    acc._batch_dev(xf, yf, args.fit_rows, +1)
    theta = acc._solve_dev(args.sigma, args.rho, None)[0][0].clone()
    post = acc.posterior(args.sigma, args.rho)
    m, p = args.rows, args.p
    xc, _ = synth(7, m)
    draws = [int(s) for s in args.draws.split(",")]
    smax = max(draws)
    Z = torch.randn((smax, p), dtype=f64, device=dev, generator=torch.Generator(dev).manual_seed(5))
    path = torch.empty((smax, m), dtype=f64, device=dev)
    index = torch.empty(smax, dtype=torch.int64, device=dev)
    value = torch.empty(smax, dtype=f64, device=dev)
    res = {"config": {"d": args.d, "p": p, "m": m, "draws": draws, "fit_rows": args.fit_rows, "sigma": args.sigma,
                      "rho": args.rho, "reps": args.reps, "yardstick_form": "one m x S buffer, torch.argmin(dim=0)"},
           "source_hash": lib.lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0)}

    def timed(f):
        lib.call("obhip_profile_reset")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def extremum(S, generic):
        if generic:
            os.environ["OBHIP_FORCE_GENERIC"] = "1"
        else:
            os.environ.pop("OBHIP_FORCE_GENERIC", None)
        ms, _ = timed(lambda: lib.call("obhip_posterior_extremum_dev", post._h, theta.data_ptr(), Z.data_ptr(), p, S,
                                       xc.data_ptr(), m, None, 0, index.data_ptr(), value.data_ptr()))
        os.environ.pop("OBHIP_FORCE_GENERIC", None)
        out = {"ms": ms, "index": index[:S].cpu().numpy().tolist()}
        for name in ("sample_ext", "draw", "sample_colext", "predict"):
            out[name] = scope(lib, name)
        return out

    def yardstick(S):
        os.environ.pop("OBHIP_FORCE_GENERIC", None)

        def f():
            lib.call("obhip_posterior_sample_dev", post._h, theta.data_ptr(), Z.data_ptr(), p, S, xc.data_ptr(), m,
                     path.data_ptr())
            return torch.argmin(path[:S], dim=1)
        ms, idx = timed(f)
        return {"ms": ms, "index": idx.cpu().numpy().tolist(), "predict_multi": scope(lib, "predict_multi"),
                "draw": scope(lib, "draw")}
    theta65 = torch.randn((65, p), dtype=f64, device=dev)
    mean65 = torch.empty((65, m), dtype=f64, device=dev)

    def predictor_pass():
        os.environ.pop("OBHIP_FORCE_GENERIC", None)
        lib.call("obhip_profile_reset")
        lib.call("obhip_predict_multi_dev", om._h, acc._t._h, theta65.data_ptr(), 65, xc.data_ptr(), m, mean65.data_ptr(),
                 None, args.sigma, None)
        torch.cuda.synchronize()
        a = scope(lib, "predict_multi")
        assert a["launches"] == 1, "the 65-response call did not take launch_predict_multi"
        return a["ms"]
    lib.call("obhip_profile_enable", 1)
    yard = []
    for S in draws:
        runs = {"fused": [], "yardstick": [], "unfused": []}
        extremum(S, False), yardstick(S), args.no_unfused or extremum(S, True), predictor_pass()    # warm-up
        for _ in range(args.reps):                                               # alternating
            runs["fused"].append(extremum(S, False))
            runs["yardstick"].append(yardstick(S))
            runs["unfused"].append(runs["fused"][-1] if args.no_unfused else extremum(S, True))
            yard.append(predictor_pass())
        ref = runs["fused"][0]["index"]
        fa = runs["fused"]
        e = {"S": S, "same_indices": all(a["index"] == ref for v in runs.values() for a in v),
             "distinct_picks": len(set(ref)),
             "fused_ms": spread([a["ms"] for a in fa]),
             "yardstick_ms": spread([a["ms"] for a in runs["yardstick"]]),
             "unfused_ms": None if args.no_unfused else spread([a["ms"] for a in runs["unfused"]]),
             "sample_ext_ms_per_pass": spread([a["sample_ext"]["ms"] / a["sample_ext"]["launches"] for a in fa]),
             "sample_ext_passes": fa[0]["sample_ext"]["launches"],
             "draw_ms_per_launch": spread([a["draw"]["ms"] / a["draw"]["launches"] for a in fa]),
             "yardstick_predict_multi_ms": spread([a["predict_multi"]["ms"] for a in runs["yardstick"]])}
        e["draws_per_pass"] = S / e["sample_ext_passes"]
        e["sample_ext_ms_per_64_draws_min"] = e["sample_ext_ms_per_pass"]["min"] * 64.0 / e["draws_per_pass"]
        e["fused_over_yardstick_min"] = e["fused_ms"]["min"] / e["yardstick_ms"]["min"]
        res["S%d" % S] = e
        print(json.dumps(e), flush=True)
    res["predict_multi_64_column_pass_ms"] = spread(yard)
    # at the same column count: the 64-draw pass (S = 64) beside the predictor's 64-column pass; the wider pass
    # (128 draws where its LDS fits) per 64 draws beside the same
    res["fused_64_draw_pass_over_predictor_pass"] = (res["S64"]["sample_ext_ms_per_pass"]["min"] / min(yard)
                                                     if "S64" in res and res["S64"]["draws_per_pass"] == 64 else None)
    res["fused_per_64_draws_over_predictor_pass"] = res["S%d" % draws[-1]]["sample_ext_ms_per_64_draws_min"] / min(yard)
    print("predict_multi 64-column pass", json.dumps(res["predict_multi_64_column_pass_ms"]),
          "fused 64-draw pass / predictor pass:", res["fused_64_draw_pass_over_predictor_pass"],
          "fused per 64 draws / predictor pass: %.3f" % res["fused_per_64_draws_over_predictor_pass"], flush=True)
    lib.call("obhip_profile_enable", 0)
    post.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--draws", default="64,256,1024")
    ap.add_argument("--fit-rows", type=int, default=20_000)
    ap.add_argument("--sigma", type=float, default=-2.302585092994046)
    ap.add_argument("--rho", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-unfused", action="store_true", help="leave route (c) out (its column loop takes seconds)")
    ap.add_argument("--part", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "sample_bench.json"))
    args = ap.parse_args()
    if args.part:
        with open(args.out, "w") as fh:
            json.dump(part(args), fh, indent=1)
        return
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--part", "--out", args.out]
    for key in ("rows", "p", "d", "knots", "draws", "fit_rows", "sigma", "rho", "reps"):
        cmd.append("--%s=%s" % (key.replace("_", "-"), getattr(args, key)))
    if args.no_unfused:
        cmd.append("--no-unfused")
    rc = subprocess.call(cmd)
    if rc != 0:
        sys.exit("sample_bench: the GPU part ended with status %d" % rc)
    print(json.dumps({"sample_bench": args.out}))


if __name__ == "__main__":
    main()
