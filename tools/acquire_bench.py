"""What an acquisition pick costs at d = 20 with the headline term set (selectterms, p = 4096): k = 64 picks among
m = 1e6 candidates by each of the four criteria (constant liar, so that both downdates run), alternating in one
process with the two yardsticks:

  the one-response predictor's own pass on the same rows (obhip_predict_dev without variance: launch_predict, a
  kernel this entry calls and does not touch) -- a step is that pass plus k_acq_update plus k_acq_pick, and the
  record is their sum over the pass;
  Posterior.select's max-variance picks with the same k (obhip_design_select_dev), per pick.

Timed with device events after a warm-up.  Per call: the whole obhip_acquire_dev, and from the library's own event
scopes (obhip_profile_get) the predictor passes (predict), the update (acq_update), the pick (acq_pick) and the
p-space kernels between two steps (design_pspace).

The GPU part runs as a child process under its own `timeout -k 10`.

  python tools/acquire_bench.py [--rows 1000000 --p 4096 --d 20 --k 64]
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
LIMIT = 900
SCOPES = ("predict", "acq_update", "acq_pick", "design_pspace", "design_step")


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
    m, k, f64, dev = args.rows, args.k, torch.float64, s["dev"]
    xc, _ = s["synth"](7, m)
    fit = s["acc"].fit(args.sigma, args.rho)
    post = s["acc"].posterior(args.sigma, args.rho)
    theta = torch.from_numpy(np.ascontiguousarray(fit.coeff[:, 0])).to(dev)
    index = torch.empty(k, dtype=torch.int64, device=dev)
    score = torch.empty(k, dtype=f64, device=dev)
    score0, mean, var = (torch.empty(m, dtype=f64, device=dev) for _ in range(3))
    trace = torch.empty(k + 1, dtype=f64, device=dev)
    res = {"config": {"d": args.d, "p": args.p, "m": m, "k": k, "fit_rows": args.fit_rows, "sigma": args.sigma,
                      "rho": args.rho, "reps": args.reps, "lie": "constant"},
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

    def yardstick():
        out = timed(lambda: lib.call("obhip_predict_dev", s["om"]._h, s["acc"]._t._h, theta.data_ptr(), xc.data_ptr(), m,
                                     mean.data_ptr(), None, args.sigma, None))
        assert out["predict"]["launches"] == 1
        return out["predict"]["ms"]
    yardstick()
    mu = mean.cpu().numpy()
    best, level = float(np.quantile(mu, 0.001)), float(np.median(mu))
    par = (C.c_double * 4)(best, 0.0, 1.96, level)

    def acquire(crit):
        n = C.c_uint64(0)
        out = timed(lambda: lib.call("obhip_acquire_dev", post._h, theta.data_ptr(), xc.data_ptr(), m, crit, par, 0, 1, best,
                                     None, k, index.data_ptr(), score.data_ptr(), score0.data_ptr(), mean.data_ptr(),
                                     var.data_ptr(), C.byref(n)))
        out.update(n_picked=n.value, index=index.cpu().numpy()[:n.value].tolist())
        return out

    def select():
        n = C.c_uint64(0)
        out = timed(lambda: lib.call("obhip_design_select_dev", post._h, xc.data_ptr(), m, 0, None, 0, None, None, k, 0,
                                     index.data_ptr(), score.data_ptr(), var.data_ptr(), trace.data_ptr(), C.byref(n)))
        out["n_picked"] = n.value
        return out
    names = ("ei", "pi", "lcb", "straddle")
    runs, yard, sel = {c: [] for c in names}, [], []
    for ci in range(4):                                                     # warm-up of every shape
        acquire(ci)
    select()
    for _ in range(args.reps):                                              # alternating
        for ci, cname in enumerate(names):
            runs[cname].append(acquire(ci))
            yard.append(yardstick())
        sel.append(select())
    ypass = statistics.median(yard)
    spick = statistics.median([a["total_ms"] / a["n_picked"] for a in sel])
    res["predict_pass_ms"] = stats(yard)
    res["select_maxvar"] = {"total_ms": [a["total_ms"] for a in sel], "ms_per_pick": spick,
                            "design_step_ms_per_launch": stats([a["design_step"]["ms"] / a["design_step"]["launches"] for a in sel])}
    for cname, v in runs.items():
        e = {"total_ms": [a["total_ms"] for a in v], "n_picked": v[0]["n_picked"], "first_picks": v[0]["index"][:8],
             "same_picks": all(a["index"] == v[0]["index"] for a in v)}
        per = {}
        for name in ("predict", "acq_update", "acq_pick", "design_pspace"):
            per[name] = statistics.median([a[name]["ms"] / a[name]["launches"] for a in v])
            e[name + "_ms_per_launch"] = stats([a[name]["ms"] / a[name]["launches"] for a in v])
            e[name + "_launches"] = v[0][name]["launches"]
        e["step_ms"] = per["predict"] + per["acq_update"] + per["acq_pick"]
        e["step_over_predict_pass"] = e["step_ms"] / ypass
        e["ms_per_pick"] = statistics.median([a["total_ms"] / a["n_picked"] for a in v])
        e["select_ms_per_pick_over_ms_per_pick"] = spick / e["ms_per_pick"]
        res[cname] = e
        print(cname, json.dumps(e), flush=True)
    print("predict pass", json.dumps(res["predict_pass_ms"]), "select(maxvar)", json.dumps(res["select_maxvar"]), flush=True)
    lib.call("obhip_profile_enable", 0)
    post.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--fit-rows", type=int, default=20_000)
    ap.add_argument("--sigma", type=float, default=-2.302585092994046)
    ap.add_argument("--rho", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--part", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "acquire_bench.json"))
    args = ap.parse_args()
    if args.part:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        res = part(args)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        return
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--part", "--out", args.out]
    for key in ("rows", "p", "d", "knots", "k", "fit_rows", "sigma", "rho", "reps"):
        cmd.append("--%s=%s" % (key.replace("_", "-"), getattr(args, key)))
    rc = subprocess.call(cmd)
    if rc != 0:
        sys.exit("acquire_bench: the GPU part ended with status %d" % rc)
    print(json.dumps({"acquire_bench": args.out}))


if __name__ == "__main__":
    main()
