"""What a pick over several responses costs at d = 20 with the headline term set (selectterms, p = 4096): k = 16 picks
among m = 1e6 candidates, constant liar, for

  constrained expected improvement with 0, 4 and 15 constraints (q = 1, 5, 16 responses of one 16-response fit),
  the expected hypervolume improvement of two objectives with an initial front of 0, 64 and 1024 points,

alternating in one process with the yardstick, the one-response obhip_acquire_dev with expected improvement on the
same candidates.  Timed with device events after a warm-up, medians over the repetitions; per call the whole entry
and, from the library's own event scopes (obhip_profile_get), the predictor passes (predict), the update
(macq_update / acq_update), the pick kernel (macq_pick / acq_pick) and the p-space kernels between two steps.  For
the hypervolume cases the update per front point and row is reported beside the count of erfc / exp evaluations,
4 (F + 1) per row.  The clocks are whatever the device runs at: the record holds its name and the times only.

Baseline, per pick: today's only alternative, MultiFit.predict(var=True) of the 16 responses on the same candidates
and the constrained expected improvement with 15 constraints in NumPy / torch on the host (diagonal variance).

The GPU part runs as a child process under its own `timeout -k 10`.

  python tools/acquire_multi_bench.py [--rows 1000000 --p 4096 --d 20 --k 16]
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
LIMIT = 900
Q = 16
SCOPES = ("predict", "predict_multi", "macq_update", "macq_pick", "acq_update", "acq_pick", "design_pspace")


def scope(lib, name):
    cnt, ms = C.c_uint64(0), C.c_double(0.0)
    lib.call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
    return {"launches": cnt.value, "ms": ms.value}


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "reps": len(v)}


def part(args):
    from design_bench import setup
    s = setup(args)
    torch, np, lib, ob = s["torch"], s["np"], s["lib"], s["ob"]
    m, k, f64, dev = args.rows, args.k, torch.float64, s["dev"]
    xc, _ = s["synth"](7, m)
    xf, yf = s["synth"](3, args.fit_rows)
    gen = torch.Generator(dev).manual_seed(5)                               # 16 responses: the synthetic one, mixed with noise
    mix = torch.linspace(1.0, 0.3, Q, dtype=f64, device=dev)[:, None]
    Y = mix * yf + (1.0 - mix) * yf.std() * torch.randn(Q, args.fit_rows, dtype=f64, device=dev, generator=gen)
    acc = ob.NewtonAccumulator(s["om"], s["terms"], Q)
    acc._batch_dev(xf, Y.contiguous(), args.fit_rows, +1)
    fit = acc.fit(args.sigma, args.rho)
    post = acc.posterior(args.sigma, args.rho)
    Theta = torch.from_numpy(np.ascontiguousarray(fit.coeff.T)).to(dev)      # column-major p x Q
    index = torch.empty(k, dtype=torch.int64, device=dev)
    score = torch.empty(k, dtype=f64, device=dev)
    score0, pof0, var = (torch.empty(m, dtype=f64, device=dev) for _ in range(3))
    mean = torch.empty((Q, m), dtype=f64, device=dev)
    res = {"config": {"d": args.d, "p": args.p, "m": m, "k": k, "fit_rows": args.fit_rows, "sigma": args.sigma,
                      "rho": args.rho, "reps": args.reps, "lie": "constant", "responses": Q},
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
    lib.call("obhip_predict_multi_dev", s["om"]._h, acc._t._h, Theta.data_ptr(), Q, xc.data_ptr(), m, mean.data_ptr(), None,
             args.sigma, None)
    torch.cuda.synchronize()
    mu = mean.cpu().numpy()                                                  # Q x m, standardised
    qt = lambda j, a: float(np.quantile(mu[j, ::97], a))
    lies = np.array([qt(j, 0.5) for j in range(Q)])

    def multi(crit, q, roles, signs, limits, front):
        n, nf, bo = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
        F0 = len(front)
        fout = np.zeros((F0 + k, 2))
        roles = np.ascontiguousarray(roles, dtype=np.int32)
        signs, limits, front = (np.ascontiguousarray(v, dtype=np.float64) for v in (signs, limits, front))
        out = timed(lambda: lib.call("obhip_acquire_multi_dev", post._h, Theta.data_ptr(), q, xc.data_ptr(), m, crit,
                                     roles.ctypes.data, signs.ctypes.data, limits.ctypes.data, 0.0,
                                     front.ctypes.data if F0 else None, F0, 1, lies.ctypes.data, None, k, index.data_ptr(),
                                     score.data_ptr(), score0.data_ptr(), pof0.data_ptr(), mean.data_ptr(), var.data_ptr(),
                                     fout.ctypes.data, C.byref(nf), C.byref(bo), C.byref(n)))
        out.update(n_picked=n.value, n_front=nf.value, index=index.cpu().numpy()[:n.value].tolist())
        return out

    def cei(ncon):
        q = 1 + ncon
        roles = [0] + [1] * ncon
        signs = [1.0] + [1.0 if j % 2 else -1.0 for j in range(ncon)]
        limits = [qt(0, 0.001)] + [qt(1 + j, 0.7 if signs[1 + j] > 0 else 0.3) for j in range(ncon)]
        return multi(0, q, roles, signs, limits, np.zeros((0, 2)))

    def ehvi(F0):
        # a staircase of F0 undominated points between the good and the poor quantiles of the two objectives
        t = (np.arange(F0) + 0.5) / max(F0, 1)
        u = qt(0, 0.001) + t * (qt(0, 0.5) - qt(0, 0.001))
        c = qt(1, 0.5) - t * (qt(1, 0.5) - qt(1, 0.001))
        return multi(3, 2, [0, 0], [1.0, 1.0], [qt(0, 0.9), qt(1, 0.9)], np.column_stack([u, c]))

    def single():
        n = C.c_uint64(0)
        par = (C.c_double * 4)(qt(0, 0.001), 0.0, 1.96, 0.0)
        out = timed(lambda: lib.call("obhip_acquire_dev", post._h, Theta.data_ptr(), xc.data_ptr(), m, 0, par, 0, 1, float(lies[0]),
                                     None, k, index.data_ptr(), score.data_ptr(), score0.data_ptr(), mean.data_ptr(),
                                     var.data_ptr(), C.byref(n)))
        out["n_picked"] = n.value
        return out
    cases = [("cei_0", lambda: cei(0)), ("cei_4", lambda: cei(4)), ("cei_15", lambda: cei(15)),
             ("ehvi_F0_0", lambda: ehvi(0)), ("ehvi_F0_64", lambda: ehvi(64)), ("ehvi_F0_1024", lambda: ehvi(1024))]
    runs, yard = {name: [] for name, _ in cases}, []
    for _, fn in cases:                                                      # warm-up of every shape
        fn()
    single()
    for _ in range(args.reps):                                               # alternating
        for name, fn in cases:
            runs[name].append(fn())
            yard.append(single())

    def per_launch(v, name):
        return [a[name]["ms"] / a[name]["launches"] for a in v if a[name]["launches"]]
    y = {"total_ms": [a["total_ms"] for a in yard], "ms_per_pick": statistics.median([a["total_ms"] / a["n_picked"] for a in yard])}
    for name in ("predict", "acq_update", "acq_pick", "design_pspace"):
        y[name + "_ms_per_launch"] = stats(per_launch(yard, name))
    res["acquire_ei"] = y
    ypass, yupd = y["predict_ms_per_launch"]["median"], y["acq_update_ms_per_launch"]["median"]
    for name, v in runs.items():
        e = {"total_ms": [a["total_ms"] for a in v], "n_picked": v[0]["n_picked"], "n_front": v[0]["n_front"],
             "first_picks": v[0]["index"][:8], "same_picks": all(a["index"] == v[0]["index"] for a in v),
             "ms_per_pick": statistics.median([a["total_ms"] / a["n_picked"] for a in v])}
        for sc in ("predict", "macq_update", "macq_pick", "design_pspace"):
            e[sc + "_ms_per_launch"] = stats(per_launch(v, sc))
            e[sc + "_launches"] = v[0][sc]["launches"]
        upd = e["macq_update_ms_per_launch"]["median"]
        e["step_ms"] = e["predict_ms_per_launch"]["median"] + upd + e["macq_pick_ms_per_launch"]["median"]
        e["update_over_predict_pass"] = upd / ypass
        e["update_over_acq_update"] = upd / yupd
        if name.startswith("ehvi"):
            F = int(name.rsplit("_", 1)[1])
            e["update_ns_per_row_and_strip"] = 1e6 * upd / (m * (F + 1))      # (the front changes with the picks: F0 + 1 strips at the start)
            e["erfc_exp_pairs_per_row"] = 2 * (F + 1)
        res[name] = e
        print(name, json.dumps(e), flush=True)
    print("acquire ei", json.dumps(y), flush=True)
    lib.call("obhip_profile_enable", 0)

    # the baseline: the host loop, per pick
    xh = xc.cpu().numpy().T.copy()                                           # m x d
    signs = np.array([1.0] + [1.0 if j % 2 else -1.0 for j in range(15)])
    cen, sca = fit.y_cent, fit.y_sca
    lim = np.array([qt(0, 0.001)] + [qt(1 + j, 0.7 if signs[1 + j] > 0 else 0.3) for j in range(15)]) * sca + cen
    base = []
    for _ in range(args.base_reps):
        t0 = time.perf_counter()
        mean_h, var_h = fit.predict(xh, var=True)
        t1 = time.perf_counter()
        mt, sd = torch.from_numpy(mean_h), torch.from_numpy(np.sqrt(np.maximum(var_h, 0.0)))
        u = (lim[0] - mt[:, 0]) / sd[:, 0]
        sc = (lim[0] - mt[:, 0]) * torch.special.ndtr(u) + sd[:, 0] * torch.exp(-0.5 * u * u) * 0.3989422804014327
        for j in range(1, Q):
            sc = sc * torch.special.ndtr(torch.from_numpy(signs[j:j + 1]) * (lim[j] - mt[:, j]) / sd[:, j])
        pick = int(torch.argmax(sc))
        t2 = time.perf_counter()
        base.append({"predict_ms": 1e3 * (t1 - t0), "criterion_ms": 1e3 * (t2 - t1), "pick": pick})
    res["host_loop_per_pick"] = {"predict_ms": stats([b["predict_ms"] for b in base]),
                                 "criterion_ms": stats([b["criterion_ms"] for b in base]),
                                 "ms_per_pick": statistics.median([b["predict_ms"] + b["criterion_ms"] for b in base]),
                                 "note": "without the add and the refit a real loop also pays per pick"}
    print("host loop", json.dumps(res["host_loop_per_pick"]), flush=True)
    post.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--fit-rows", type=int, default=20_000)
    ap.add_argument("--sigma", type=float, default=-2.302585092994046)
    ap.add_argument("--rho", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--base-reps", type=int, default=3)
    ap.add_argument("--part", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "acquire_multi_bench.json"))
    args = ap.parse_args()
    if args.part:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        res = part(args)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        return
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--part", "--out", args.out]
    for key in ("rows", "p", "d", "knots", "k", "fit_rows", "sigma", "rho", "reps", "base_reps"):
        cmd.append("--%s=%s" % (key.replace("_", "-"), getattr(args, key)))
    rc = subprocess.call(cmd)
    if rc != 0:
        sys.exit("acquire_multi_bench: the GPU part ended with status %d" % rc)
    print(json.dumps({"acquire_multi_bench": args.out}))


if __name__ == "__main__":
    main()
