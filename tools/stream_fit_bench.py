"""What rows that arrive later, and K-fold cross-validation, cost with a NewtonAccumulator next to
the one-shot fit, at the headline model (d = 20, p = 4096) with 10^6 resident rows.

One process, one response.  The rows come from obhip_synth_xy_dev and stay on the device.
  baseline   the existing one-shot path on all resident rows, as fit_newton_multi runs it on the
             device: obhip_standardise_multi_dev, obhip_basis_create_dev,
             obhip_fit_newton_multi_dev, obhip_basis_destroy;
  load       the resident rows into the accumulator in --load-chunk row batches (once);
  add        for every batch size in --add: basis of the batch, obhip_normal_acc_add_dev and the
             refit obhip_normal_acc_solve_dev on all rows; the batch is taken out again (timed on its
             own) before the next repetition;
  cv         cv_newton_multi, --folds folds over a 3 x 3 (sigma, rho) grid, wall clock of the whole
             call from host arrays (fold assignment and uploads included), beside
             folds x 9 one-shot fits counted as the baseline's median x 45.
Every timing is a host clock around work that ends in a device synchronise, after a warm-up of the
same work; --reps repetitions, the baseline and the adds alternating; median, min, max and all
values are written (--out) with the command line.  No speed-up is asserted anywhere.

  python tools/stream_fit_bench.py [--rows 1000000 --p 4096 --d 20 --add 1000,10000,100000 --reps 5]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--add", default="1000,10000,100000")
    ap.add_argument("--load-chunk", type=int, default=250_000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cv-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "stream_fit_bench.json"))
    args = ap.parse_args()
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib
    from outerbase_amd.driver import KIND_ID, bench_knots
    call = _lib.call
    kinds = ["mat25"] * args.d
    adds = [int(v) for v in args.add.split(",")]
    n, p, f64 = args.rows, args.p, torch.float64
    sigma, rho = math.log(0.01), 6.0
    dev = torch.device("cuda", torch.cuda.current_device())

    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, bench_knots(kinds, args.knots))
    terms = om.selectterms(p)
    t = ob.obmod._Terms(om, terms)
    caps = t.maxlevels()
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    N = n + max(adds)
    x = torch.empty((args.d, N), dtype=f64, device=dev)        # column-major N x d
    y = torch.empty((1, N), dtype=f64, device=dev)
    kid = (C.c_int * args.d)(*[KIND_ID[k] for k in kinds])
    call("obhip_synth_xy_dev", 42, 0, N, args.d, C.cast(kid, C.c_void_p), x.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}

    # ---- the one-shot path on the resident rows ----------------------------------------------
    xr, yr = x[:, :n].contiguous(), y[:, :n].contiguous()
    wsb = C.c_uint64(0)
    call("obhip_newton_multi_workspace_bytes", p, 1, C.byref(wsb))
    ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
    H = torch.empty((p, p), dtype=f64, device=dev)
    rhs, theta0, diagH = (torch.empty(p, dtype=f64, device=dev) for _ in range(3))
    ys = torch.empty_like(yr)
    meansd = torch.empty((1, 3), dtype=f64, device=dev)

    def one_shot():
        call("obhip_standardise_multi_dev", None, yr.data_ptr(), n, 1, n, ys.data_ptr(), meansd.data_ptr())
        basis = C.c_void_p()
        call("obhip_basis_create_dev", C.byref(basis), om._h, xr.data_ptr(), n, caps.ctypes.data)
        try:
            call("obhip_fit_newton_multi_dev", None, basis, t._h, om._h, ys.data_ptr(), 1, n, sigma, rho, H.data_ptr(),
                 rhs.data_ptr(), theta0.data_ptr(), diagH.data_ptr(), None, 0, ws.data_ptr(), wsb.value)
            torch.cuda.synchronize()
        finally:
            call("obhip_basis_destroy", basis)

    one_shot()                                                  # warm-up
    res = {"command": "python " + " ".join(sys.argv),
           "config": {"d": args.d, "rows": n, "p": p, "knots": args.knots, "reps": args.reps, "folds": args.folds,
                      "load_chunk": args.load_chunk, "sigma": sigma, "rho": rho},
           "source_hash": _lib.lib.obhip_source_hash(0).decode(),
           "gram_source_hash": _lib.lib.obhip_source_hash(1).decode(),
           "device": torch.cuda.get_device_name(0)}

    # ---- the accumulator ---------------------------------------------------------------------
    acc = ob.NewtonAccumulator(om, t, 1)
    load = []
    for a in range(0, n, args.load_chunk):
        b = min(n, a + args.load_chunk)
        xa, ya = x[:, a:b].contiguous(), y[:, a:b].contiguous()
        load.append(timed(lambda: acc._batch_dev(xa, ya, b - a, +1)))
        del xa, ya
    assert acc.rows == n
    res["load"] = {"chunks_ms": load, "total_ms": sum(load)}
    refit = [timed(lambda: acc._solve_dev(sigma, rho)) for _ in range(args.reps + 1)][1:]
    res["refit_only"] = stats(refit)
    th = acc._solve_dev(sigma, rho)[0]
    torch.cuda.synchronize()
    res["theta_rel_diff_to_one_shot"] = float((th[0] - theta0).abs().max() / theta0.abs().max())

    base, per_add = [], {}
    for nb in adds:
        xa, ya = x[:, n:n + nb].contiguous(), y[:, n:n + nb].contiguous()

        def add_and_refit():
            acc._batch_dev(xa, ya, nb, +1)
            acc._solve_dev(sigma, rho)

        def take_out():
            acc._batch_dev(xa, ya, nb, -1)

        add_and_refit()                                         # warm-up of both
        take_out()
        ta, tr = [], []
        for _ in range(args.reps):
            base.append(timed(one_shot))
            ta.append(timed(add_and_refit))
            tr.append(timed(take_out))
        per_add[str(nb)] = {"add_and_refit": stats(ta), "remove": stats(tr)}
        print("add %7d rows + refit: %.2f ms (remove %.2f ms); one-shot fit of %d rows: %.2f ms"
              % (nb, statistics.median(ta), statistics.median(tr), n, statistics.median(base)), flush=True)
        assert acc.rows == n
    res["one_shot_fit"] = stats(base)
    res["add"] = per_add
    acc.close()
    del H, ws, xr, ys
    call("obhip_trim_pool")
    torch.cuda.empty_cache()

    # ---- cross-validation --------------------------------------------------------------------
    xh = x[:, :n].T.cpu().numpy()
    yh = y[:, :n].T.cpu().numpy()
    sigmas = (math.log(0.005), math.log(0.01), math.log(0.02))
    rhos = (5.0, 6.0, 7.0)

    def cv():
        return ob.cv_newton_multi(om, t, xh, yh, folds=args.folds, sigmas=sigmas, rhos=rhos, seed=0)

    r = cv()                                                    # warm-up
    tcv = [timed(cv) for _ in range(args.cv_reps)]
    fits = args.folds * len(sigmas) * len(rhos)
    res["cv"] = {"wall": stats(tcv), "fits": fits, "one_shot_fits_equivalent_ms": fits * res["one_shot_fit"]["median_ms"],
                 "best": {"sigma": r.sigma, "rho": r.rho}, "rmse": r.rmse.tolist(),
                 "note": "wall clock of cv_newton_multi from host arrays: fold assignment, uploads and the "
                         "full fit at the best candidate included"}
    T1 = res["one_shot_fit"]["median_ms"]
    res["summary"] = {"one_shot_fit_ms": T1, "one_shot_spread_ms": res["one_shot_fit"]["max_ms"] - res["one_shot_fit"]["min_ms"],
                      "refit_only_ms": res["refit_only"]["median_ms"], "cv_wall_ms": res["cv"]["wall"]["median_ms"],
                      "cv_as_one_shot_fits_ms": fits * T1}
    for nb in adds:
        res["summary"]["add_%d_and_refit_ms" % nb] = per_add[str(nb)]["add_and_refit"]["median_ms"]
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"]))


if __name__ == "__main__":
    main()
