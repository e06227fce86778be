"""What the sequential design costs at d = 20 with the headline term set (selectterms, p = 4096): k = 64 greedy
picks among m = 1e6 candidates, both criteria (r = 1e4 reference rows for imse), on the fused step kernel and
on the unfused route (predictor to scratch, then k_design_update), alternating in one process.

Timed with device events after a warm-up.  Per call: the whole obhip_design_select_dev; from the library's own
event scopes (obhip_profile_get) the k + 1 passes over the candidates (design_step, or predict and
design_update under OBHIP_FORCE_GENERIC), and the p-space kernels between them (design_pspace).  The yardstick
of a pass is the multi-response predictor at the same shape, a kernel this change does not touch, timed in the
same process and alternating with the selections: launch_predict_multi is reached through
obhip_predict_multi_dev from nine responses on (one by the single predictor, eight batched), and its one
16-column pass costs the same products for 1 to 16 columns, so the scope predict_multi of that call stands for
the two-column pass (it writes eight n-vectors where two columns would write two).  The "before" figure is
today's host loop over 8 picks: MultiFit.predict(var=True) on all candidates, argmax on the host,
NewtonAccumulator.add of the row, refit.

Every GPU part runs as a child process under its own `timeout -k 10`; the first part that fails ends the run.

  python tools/design_bench.py [--rows 1000000 --p 4096 --d 20 --k 64 --ref 10000]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = {"select": 900, "hostloop": 600}      # seconds each part may take


def setup(args):
    import numpy as np
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ob_oracle as O
    kinds = ["mat25"] * args.d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, O.bench_knots(kinds, args.knots))
    terms = om.selectterms(args.p)
    dev = torch.device("cuda", 0)
    _lib.call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def synth(seed, n):
        x = torch.empty((args.d, n), dtype=torch.float64, device=dev)
        y = torch.empty((1, n), dtype=torch.float64, device=dev)
        _lib.call("obhip_synth_xy_dev", seed, 0, n, args.d, np.zeros(args.d, dtype=np.int32).ctypes.data, x.data_ptr(),
                  y.data_ptr())
        return x, y
    acc = ob.NewtonAccumulator(om, terms, 1)
    xf, yf = synth(3, args.fit_rows)
    acc._batch_dev(xf, yf, args.fit_rows, +1)
    return dict(ob=ob, lib=_lib, om=om, terms=terms, dev=dev, synth=synth, acc=acc, torch=torch, np=np)


def scope(lib, name):
    cnt, ms = C.c_uint64(0), C.c_double(0.0)
    lib.call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
    return {"launches": cnt.value, "ms": ms.value}


def part_select(args):
    s = setup(args)
    torch, np, lib = s["torch"], s["np"], s["lib"]
    m, k, r, f64 = args.rows, args.k, args.ref, torch.float64
    xc, _ = s["synth"](7, m)
    xr, _ = s["synth"](11, r)
    post = s["acc"].posterior(args.sigma, args.rho)
    index = torch.empty(k, dtype=torch.int64, device=s["dev"])
    score = torch.empty(k, dtype=f64, device=s["dev"])
    var = torch.empty(m, dtype=f64, device=s["dev"])
    trace = torch.empty(k + 1, dtype=f64, device=s["dev"])
    res = {"config": {"d": args.d, "p": args.p, "m": m, "k": k, "r": r, "fit_rows": args.fit_rows, "sigma": args.sigma,
                      "rho": args.rho, "reps": args.reps},
           "source_hash": lib.lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0)}

    def select(crit, generic):
        if generic:
            os.environ["OBHIP_FORCE_GENERIC"] = "1"
        else:
            os.environ.pop("OBHIP_FORCE_GENERIC", None)
        n = C.c_uint64(0)
        lib.call("obhip_profile_reset")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.call("obhip_design_select_dev", post._h, xc.data_ptr(), m, crit, xr.data_ptr() if crit else None, r, None, None,
                 k, 0, index.data_ptr(), score.data_ptr(), var.data_ptr(), trace.data_ptr(), C.byref(n))
        e1.record()
        e1.synchronize()
        out = {"total_ms": e0.elapsed_time(e1), "n_picked": n.value, "index": index.cpu().numpy()[:n.value].tolist()}
        for name in ("design_step", "design_update", "design_pspace", "predict_multi", "predict", "getmat"):
            out[name] = scope(lib, name)
        return out
    theta = torch.randn((9, args.p), dtype=f64, device=s["dev"])
    mean9 = torch.empty((9, m), dtype=f64, device=s["dev"])

    def yardstick():
        os.environ.pop("OBHIP_FORCE_GENERIC", None)
        lib.call("obhip_profile_reset")
        lib.call("obhip_predict_multi_dev", s["om"]._h, s["acc"]._t._h, theta.data_ptr(), 9, xc.data_ptr(), m,
                 mean9.data_ptr(), None, args.sigma, None)
        torch.cuda.synchronize()
        a = scope(lib, "predict_multi")
        assert a["launches"] == 1, "the nine-response call did not take launch_predict_multi"
        return a["ms"]
    lib.call("obhip_profile_enable", 1)
    yard = []
    for crit, cname in ((0, "maxvar"), (1, "imse")):
        runs = {"fused": [], "unfused": []}
        select(crit, False), select(crit, True), yardstick()                # warm-up of every shape
        for _ in range(args.reps):                                          # alternating
            runs["fused"].append(select(crit, False))
            runs["unfused"].append(select(crit, True))
            yard.append(yardstick())
        entry = {"same_picks": all(a["index"] == runs["fused"][0]["index"] for v in runs.values() for a in v),
                 "n_picked": runs["fused"][0]["n_picked"], "first_picks": runs["fused"][0]["index"][:8]}
        for route, v in runs.items():
            pass_name = "design_step" if route == "fused" else "design_update"
            e = {"total_ms": [a["total_ms"] for a in v]}
            for name in ("design_step", "design_update", "design_pspace", "predict_multi", "predict"):
                per = [a[name]["ms"] / a[name]["launches"] for a in v if a[name]["launches"]]
                if per:
                    e[name + "_ms_per_launch"] = {"median": statistics.median(per), "min": min(per), "max": max(per),
                                                  "launches": v[0][name]["launches"]}
            e["pass_scope"] = pass_name
            entry[route] = e
        entry["step_over_predict_multi_pass"] = (entry["fused"]["design_step_ms_per_launch"]["median"]
                                                 / statistics.median(yard))
        res[cname] = entry
        print(cname, json.dumps({kk: vv for kk, vv in entry.items() if kk not in ("fused", "unfused")}), flush=True)
        for route in ("fused", "unfused"):
            print(" ", route, json.dumps(entry[route]), flush=True)
    res["predict_multi_pass_ms"] = {"median": statistics.median(yard), "min": min(yard), "max": max(yard), "reps": len(yard)}
    print("predict_multi pass", json.dumps(res["predict_multi_pass_ms"]), flush=True)
    lib.call("obhip_profile_enable", 0)
    os.environ.pop("OBHIP_FORCE_GENERIC", None)
    post.close()
    return res


def part_hostloop(args):
    """today's loop: variances back to the host, one pick, acc.add, refit"""
    s = setup(args)
    torch, np, acc = s["torch"], s["np"], s["acc"]
    xc, _ = s["synth"](7, args.rows)
    x = xc.cpu().numpy().T.copy()
    per = []
    fit = acc.fit(args.sigma, args.rho)
    fit.predict(x[:1000], var=True)
    torch.cuda.synchronize()
    for _ in range(8):
        t0 = time.perf_counter()
        _, v = fit.predict(x, var=True)
        j = int(np.argmax(v[:, 0]))
        acc.add(x[j:j + 1], np.zeros((1, 1)))
        fit = acc.fit(args.sigma, args.rho)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3)
    print("host loop: %.1f ms per pick (median of 8)" % statistics.median(per), flush=True)
    return {"host_loop_ms_per_pick": per, "host_loop_median_ms": statistics.median(per),
            "what": "MultiFit.predict(var=True) on all candidates from host memory, argmax, NewtonAccumulator.add, fit"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--ref", type=int, default=10_000)
    ap.add_argument("--fit-rows", type=int, default=20_000)
    ap.add_argument("--sigma", type=float, default=-2.302585092994046)
    ap.add_argument("--rho", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--part", choices=sorted(PARTS))
    ap.add_argument("--out", default=os.path.join("profiles", "design_bench.json"))
    args = ap.parse_args()
    if args.part:
        res = {"select": part_select, "hostloop": part_hostloop}[args.part](args)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        return
    merged = {}
    for part, limit in PARTS.items():
        tmp = args.out + "." + part
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part, "--out", tmp]
        for key in ("rows", "p", "d", "knots", "k", "ref", "fit_rows", "sigma", "rho", "reps"):
            cmd.append("--%s=%s" % (key.replace("_", "-"), getattr(args, key)))
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit("design_bench: part %s ended with status %d; nothing more is started" % (part, rc))
        merged[part] = json.load(open(tmp))
        os.remove(tmp)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(merged, fh, indent=1)
    print(json.dumps({"design_bench": args.out}))


if __name__ == "__main__":
    main()
