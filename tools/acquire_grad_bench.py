"""What the gradient of the full-covariance variance and of an acquisition criterion costs at d = 20 with the headline
term set (selectterms, p = 4096) on n = 1e5 rows, alternating in one process with two yardsticks on the same rows:

  (a) obhip_posterior_var_dev: the variance alone, from the triangular L^-T (code this entry does not touch);
  (b) obhip_posterior_var_grad_dev: the variance and its gradient;
  (c) obhip_acquire_grad_dev with EI and all six outputs;
  (d) obhip_predict_grad_dev, mean and gradient: the input-gradient predictor's own pass.

The record is (b) / (a) and (c) / (a) against d + 1 = 21, what one-sided differences through (a) would cost.  Timed
with device events after a warm-up (which also forms the handle's inv(H)); from the library's own event scopes
(obhip_profile_get) the stored product Y = S B^T (acquire_dx_product) and the kernel (acquire_dx) per launch.

The GPU part runs as a child process under its own `timeout -k 10`.

  python tools/acquire_grad_bench.py [--rows 100000 --p 4096 --d 20]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = 600
SCOPES = ("acquire_dx_product", "acquire_dx", "predict_std_gemm", "predict_dx")


def scope(lib, name):
    cnt, ms = C.c_uint64(0), C.c_double(0.0)
    lib.call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
    return {"launches": cnt.value, "ms": ms.value}


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "reps": len(v)}


def part(args):
    from design_bench import setup
    s = setup(args)
    torch, np, lib = s["torch"], s["np"], s["lib"]
    n, d, f64, dev = args.rows, args.d, torch.float64, s["dev"]
    x, _ = s["synth"](7, n)
    fit = s["acc"].fit(args.sigma, args.rho)
    post = s["acc"].posterior(args.sigma, args.rho)
    tm = s["acc"]._t
    theta = torch.from_numpy(np.ascontiguousarray(fit.coeff[:, 0])).to(dev)
    score, mean, var = (torch.empty(n, dtype=f64, device=dev) for _ in range(3))
    grad, gmean, gvar = (torch.empty((d, n), dtype=f64, device=dev) for _ in range(3))
    fused, lds, chunk = post.acquire_grad_layout()
    res = {"config": {"d": d, "p": args.p, "n": n, "fit_rows": args.fit_rows, "sigma": args.sigma, "rho": args.rho,
                      "reps": args.reps, "criterion": "ei", "fused": fused, "lds_bytes": lds, "chunk_rows": chunk,
                      "view_entries": int((s["terms"] > 0).sum())},
           "source_hash": lib.lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0)}
    lib.call("obhip_profile_enable", 1)

    def timed(fn):
        lib.call("obhip_profile_reset")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out = {"total_ms": e0.elapsed_time(e1)}
        out.update({name: scope(lib, name) for name in SCOPES})
        return out
    lib.call("obhip_predict_dev", s["om"]._h, tm._h, theta.data_ptr(), x.data_ptr(), n, mean.data_ptr(), None, args.sigma,
             None)
    best = float(np.quantile(mean.cpu().numpy(), 0.001))
    par = (C.c_double * 4)(best, 0.0, 1.96, 0.0)
    calls = {
        "a_posterior_var": lambda: lib.call("obhip_posterior_var_dev", post._h, x.data_ptr(), n, var.data_ptr(), 0),
        "b_var_grad": lambda: lib.call("obhip_posterior_var_grad_dev", post._h, x.data_ptr(), n, 0, 0, var.data_ptr(),
                                       gvar.data_ptr()),
        "c_acquire_grad_ei": lambda: lib.call("obhip_acquire_grad_dev", post._h, theta.data_ptr(), x.data_ptr(), n, 0, par,
                                              0, 0, score.data_ptr(), grad.data_ptr(), mean.data_ptr(), gmean.data_ptr(),
                                              var.data_ptr(), gvar.data_ptr()),
        "d_predict_grad": lambda: lib.call("obhip_predict_grad_dev", s["om"]._h, tm._h, theta.data_ptr(), x.data_ptr(), n,
                                           mean.data_ptr(), gmean.data_ptr(), None, args.sigma, None, None),
    }
    runs = {k: [] for k in calls}
    for fn in calls.values():                                               # warm-up of every shape; forms inv(H)
        fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):                                              # alternating
        for k, fn in calls.items():
            runs[k].append(timed(fn))
    med = {k: statistics.median([a["total_ms"] for a in v]) for k, v in runs.items()}
    for k, v in runs.items():
        res[k] = {"total_ms": [a["total_ms"] for a in v]}
    for k in ("b_var_grad", "c_acquire_grad_ei"):
        for name in ("acquire_dx_product", "acquire_dx"):
            res[k][name + "_ms_per_launch"] = stats([a[name]["ms"] / a[name]["launches"] for a in runs[k]])
            res[k][name + "_launches"] = runs[k][0][name]["launches"]
            res[k][name + "_ms"] = statistics.median([a[name]["ms"] for a in runs[k]])
    res["a_posterior_var"]["predict_std_gemm_ms"] = statistics.median([a["predict_std_gemm"]["ms"] for a in runs["a_posterior_var"]])
    res["d_predict_grad"]["predict_dx_ms"] = statistics.median([a["predict_dx"]["ms"] for a in runs["d_predict_grad"]])
    res["ratios"] = {"b_over_a": med["b_var_grad"] / med["a_posterior_var"],
                     "c_over_a": med["c_acquire_grad_ei"] / med["a_posterior_var"],
                     "d_over_a": med["d_predict_grad"] / med["a_posterior_var"], "bound_d_plus_1": d + 1}
    print(json.dumps(res), flush=True)
    lib.call("obhip_profile_enable", 0)
    post.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--fit-rows", type=int, default=20_000)
    ap.add_argument("--sigma", type=float, default=-2.302585092994046)
    ap.add_argument("--rho", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--part", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "acquire_grad_bench.json"))
    args = ap.parse_args()
    if args.part:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        res = part(args)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        return
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--part", "--out", args.out]
    for key in ("rows", "p", "d", "knots", "fit_rows", "sigma", "rho", "reps"):
        cmd.append("--%s=%s" % (key.replace("_", "-"), getattr(args, key)))
    rc = subprocess.call(cmd)
    if rc != 0:
        sys.exit("acquire_grad_bench: the GPU part ended with status %d" % rc)
    print(json.dumps({"acquire_grad_bench": args.out}))


if __name__ == "__main__":
    main()
