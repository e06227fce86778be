"""What the Sobol indices cost at d = 20 with the headline term set (selectterms, p = 4096).

One process.  Timed with device events after a warm-up, over enough repetitions to fill --fill seconds:
  (a) obhip_dim_moments_dev on n = 1e6 empirical rows and on 64 Gauss-Legendre nodes per dimension;
  (b) obhip_sobol_dev at q = 1, 8, 64;
  (c) beside (b), alternating three times in the same run, a torch float64 restatement of the pair sums in
      row blocks on the same GPU -- written here, and checked against the kernel to the stage-2 tolerance
      gamma_{p^2+3d+4} sum |theta theta'| |C_l| prod |A_i| (the absolute sums come from the same restatement).
Recorded with the times and their spread: the bytes the moments pass reads (8 n d, 160 MB), the operation model
of the pair sum, p (p + 1) / 2 . (7 d + 2 (d + 1) q), and its share of the FP64 vector peak.  Writes one JSON.

  python tools/sobol_bench.py [--rows 1000000 --p 4096 --d 20 --qs 1,8,64]
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

FP64_VECTOR_PEAK = 78.6e12  # MI355X data sheet, vector FP64 flop/s
U = 2.0 ** -53


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--qs", default="1,8,64")
    ap.add_argument("--fill", type=float, default=0.5)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "sobol_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib, obmod
    call, lib = _lib.call, _lib.lib
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ob_oracle as O
    n, p, d, f64 = args.rows, args.p, args.d, torch.float64
    qs = [int(v) for v in args.qs.split(",")]
    kinds = ["mat25"] * d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, O.bench_knots(kinds, args.knots))
    terms = om.selectterms(p)
    t = obmod._terms_of(om, terms)
    dev = torch.device("cuda", 0)
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    levels = (t.maxlevels() + 1).astype(np.int64)
    nm, nc = int(levels.sum()), int((levels ** 2).sum())

    def timed(fn, fill=args.fill):
        """fn repeated until `fill` seconds are full -> per-call milliseconds of every repetition"""
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

    res = {"config": {"d": d, "n": n, "p": p, "knots": args.knots, "levels": levels.tolist()},
           "source_hash": lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0)}
    # (a) the moments
    x = torch.empty((d, n), dtype=f64, device=dev)
    ysyn = torch.empty(n, dtype=f64, device=dev)
    call("obhip_synth_xy_dev", 7, 0, n, d, np.zeros(d, dtype=np.int32).ctypes.data, x.data_ptr(), ysyn.data_ptr())
    mean = torch.empty(nm, dtype=f64, device=dev)
    cov = torch.empty(nc, dtype=f64, device=dev)
    gl_x, gl_w = ob.uniform_nodes(np.full(d, 0.02), np.full(d, 0.98), order=64)
    dgx = torch.from_numpy(np.ascontiguousarray(gl_x.T)).to(dev)
    dgw = torch.from_numpy(np.ascontiguousarray(gl_w.T)).to(dev)
    v = timed(lambda: call("obhip_dim_moments_dev", om._h, t._h, dgx.data_ptr(), 64, 64, dgw.data_ptr(), 64,
                           mean.data_ptr(), cov.data_ptr()))
    res["moments_gauss_legendre_64"] = stats(v)
    v = timed(lambda: call("obhip_dim_moments_dev", om._h, t._h, x.data_ptr(), n, n, None, 0, mean.data_ptr(),
                           cov.data_ptr()))
    nbytes = 8.0 * n * d
    res["moments_empirical"] = dict(stats(v), bytes_read=nbytes, passes=2,
                                    GB_per_s=2 * nbytes / (statistics.median(v) * 1e-3) / 1e9)
    print("moments: %d rows %.3f ms (%.0f GB/s over two passes), 64 nodes %.3f ms" % (
        n, res["moments_empirical"]["median_ms"], res["moments_empirical"]["GB_per_s"],
        res["moments_gauss_legendre_64"]["median_ms"]), flush=True)
    # (b), (c) the sums on the empirical tables
    mtab, ctab = mean.clone(), cov.clone()
    om_ = np.concatenate([[0], np.cumsum(levels)])
    oc_ = np.concatenate([[0], np.cumsum(levels ** 2)])
    lev = torch.from_numpy(terms.astype(np.int64)).to(dev)
    Cl = [ctab[oc_[l]:oc_[l + 1]] for l in range(d)]
    ml = [mtab[om_[l]:om_[l + 1]] for l in range(d)]
    Al = [(Cl[l].view(levels[l], levels[l]) + torch.outer(ml[l], ml[l])).reshape(-1) for l in range(d)]

    def restatement(Th, absolute=False):
        """(VT (d x q), V (q)) of the pair sums, row blocks of --block terms against all p"""
        q = Th.shape[1]
        VT, V = torch.zeros((d, q), dtype=f64, device=dev), torch.zeros(q, dtype=f64, device=dev)
        fix = torch.abs if absolute else (lambda a: a)
        for k0 in range(0, p, args.block):
            k1 = min(p, k0 + args.block)
            a, c, mm = [], [], []
            for l in range(d):
                idx = lev[k0:k1, l][:, None] * int(levels[l]) + lev[:, l][None, :]
                a.append(fix(Al[l][idx])), c.append(fix(Cl[l][idx]))
                mm.append(fix(torch.outer(ml[l][lev[k0:k1, l]], ml[l][lev[:, l]])))
            sa = [None] * (d + 1)
            sa[d] = torch.ones_like(a[0])
            for l in range(d - 1, -1, -1):
                sa[l] = sa[l + 1] * a[l]
            pa, D = torch.ones_like(a[0]), torch.zeros_like(a[0])
            for l in range(d):
                pc = pa * c[l]
                VT[l] += (Th[k0:k1] * ((pc * sa[l + 1]) @ Th)).sum(dim=0)
                D = mm[l] * D + pc
                pa = pa * a[l]
            V += (Th[k0:k1] * (D @ Th)).sum(dim=0)
        return VT, V

    rng = np.random.default_rng(9)
    order = (terms > 0).sum(axis=1)
    res["sobol"] = {}
    for q in qs:
        Theta = rng.standard_normal((p, q)) * (0.5 ** order)[:, None]
        dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)        # p x q column-major
        Th = torch.from_numpy(Theta).to(dev)
        wsb = C.c_uint64(0)
        call("obhip_sobol_workspace_bytes", p, d, q, C.byref(wsb))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
        out = torch.empty((q, 2 + 2 * d), dtype=f64, device=dev)

        def kernel():
            call("obhip_sobol_dev", t._h, dth.data_ptr(), q, mtab.data_ptr(), ctab.data_ptr(), out.data_ptr(), None,
                 ws.data_ptr(), wsb.value)
        tk, tr = [], []
        for _ in range(3):                                                   # alternating
            tk += timed(kernel, args.fill / 3)
            tr += timed(lambda: restatement(Th), args.fill / 3)
        VT, V = restatement(Th)
        aVT, aV = restatement(Th, absolute=True)
        gq = (p * p + 3 * d + 4) * U / (1 - (p * p + 3 * d + 4) * U)
        got = out.cpu()
        r = max(float(((got[:, 2 + d:].T - VT.cpu()).abs() / (gq * aVT.cpu())).max()),
                float(((got[:, 1] - V.cpu()).abs() / (gq * aV.cpu())).max()))
        ops = p * (p + 1) / 2 * (7 * d + 2 * (d + 1) * q)
        sk, sr = stats(tk), stats(tr)
        res["sobol"]["q=%d" % q] = {
            "kernel": sk, "torch_restatement": sr, "restatement_over_kernel": sr["median_ms"] / sk["median_ms"],
            "kernel_vs_restatement_err_over_tolerance": r, "operations_model": ops,
            "share_of_fp64_vector_peak": ops / (sk["median_ms"] * 1e-3) / FP64_VECTOR_PEAK}
        print("q=%d: kernel %.3f ms (spread %.2f), restatement %.1f ms (spread %.2f), err/tolerance %.3g, %.1f%% of the "
              "FP64 vector peak" % (q, sk["median_ms"], sk["spread"], sr["median_ms"], sr["spread"], r,
                                    100 * res["sobol"]["q=%d" % q]["share_of_fp64_vector_peak"]), flush=True)
        assert r < 1, "the kernel and the restatement disagree beyond the stage-2 tolerance"
    call("obhip_profile_enable", 1)
    call("obhip_profile_reset")
    kernel()
    torch.cuda.synchronize()
    res["scopes_last_q"] = {}
    for name in ("sobol_first", "sobol_pairs"):
        cnt, ms = C.c_uint64(0), C.c_double(0.0)
        call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
        res["scopes_last_q"][name] = {"launches": cnt.value, "ms": ms.value}
    call("obhip_profile_enable", 0)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v["restatement_over_kernel"] for k, v in res["sobol"].items()}))


if __name__ == "__main__":
    main()
