"""What the Shapley effects cost at d = 20 with the headline term set (selectterms, p = 4096).

One process.  Timed with device events after a warm-up, over enough repetitions to fill --fill seconds, alternating
three times in the same run at q = 1, 8, 64:
  (a) obhip_shapley_dev, every dimension its own player (P = 20, 10 Gauss-Legendre nodes);
  (b) the untouched obhip_sobol_dev on the same tables;
  (c) a torch float64 restatement of the same pair sum in row blocks on the same GPU -- written here, and checked
      against the kernel to --agree of the stage-2 tolerance (gamma_{p^2+3d+2G+4} + (P - 1) 2^-52) sum |summands|
      (the absolute sums come from the same restatement).
Also timed at the first q: the players grouped in two halves (P = 2, one node).  Recorded with the times and their
spread: the operation models of the two pair sums and their ratio beside the measured ratio, the ratio to the
restatement, and the resource usage of the new kernels as the compiler reports it
(-Rpass-analysis=kernel-resource-usage, gfx950).  Writes one JSON.

  python tools/shapley_bench.py [--rows 100000 --p 4096 --d 20 --qs 1,8,64]
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
# SGPRs, VGPRs, AGPRs, scratch bytes per lane, waves per SIMD (compiler remarks, gfx950); no instantiation spills
RESOURCES = {"k_shapley_pairs<8 slots, 2 responses>": [48, 122, 0, 0, 4],
             "k_shapley_pairs<24 slots, 2 responses>": [51, 256, 87, 0, 1],
             "k_shapley_pairs<40 slots, 1 response>": [55, 256, 230, 0, 1],
             "k_shapley_pairs<40 slots, 1 response, d > 40>": [74, 256, 234, 0, 1],
             "k_shapley_reduce": [32, 9, 0, 0, 8]}


def ops_sobol(p, d, q):
    """DESIGN.md section 19"""
    return p * (p + 1) / 2 * (7 * d + 2 * (d + 1) * q)


def ops_shapley(p, d, P, q):
    """per term pair 6 d for the player recursion, then per node and player a fused
    multiply-add and a product on the way back, a fused multiply-add and three products on the way forward, and one
    fused multiply-add per response"""
    G = (P + 1) // 2
    return p * (p + 1) / 2 * (6 * d + G * P * (8 + 2 * q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--qs", default="1,8,64")
    ap.add_argument("--fill", type=float, default=0.5)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--agree", type=float, default=1e-2, help="kernel vs restatement, as a share of the tolerance")
    ap.add_argument("--out", default=os.path.join("profiles", "shapley_bench.json"))
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
    P, G = d, (d + 1) // 2
    nodes, weights = (C.c_double * G)(), (C.c_double * G)()
    call("obhip_gauss_legendre01", G, nodes, weights)
    nodes, weights = list(nodes), list(weights)

    def timed(fn, fill):
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

    res = {"config": {"d": d, "n": n, "p": p, "knots": args.knots, "levels": levels.tolist(), "players": P, "nodes": G},
           "source_hash": lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0),
           "kernel_resources_sgpr_vgpr_agpr_scratch_waves": RESOURCES}
    # the tables of n empirical rows
    x = torch.empty((d, n), dtype=f64, device=dev)
    ysyn = torch.empty(n, dtype=f64, device=dev)
    call("obhip_synth_xy_dev", 7, 0, n, d, np.zeros(d, dtype=np.int32).ctypes.data, x.data_ptr(), ysyn.data_ptr())
    mtab = torch.empty(nm, dtype=f64, device=dev)
    ctab = torch.empty(nc, dtype=f64, device=dev)
    call("obhip_dim_moments_dev", om._h, t._h, x.data_ptr(), n, n, None, 0, mtab.data_ptr(), ctab.data_ptr())
    om_ = np.concatenate([[0], np.cumsum(levels)])
    oc_ = np.concatenate([[0], np.cumsum(levels ** 2)])
    lev = torch.from_numpy(terms.astype(np.int64)).to(dev)
    Cl = [ctab[oc_[l]:oc_[l + 1]] for l in range(d)]
    Ml = [torch.outer(mtab[om_[l]:om_[l + 1]], mtab[om_[l]:om_[l + 1]]).reshape(-1) for l in range(d)]

    def restatement(Th, absolute=False):
        """Sh (d x q) of the pair sum, every dimension a player, row blocks of --block terms against all p"""
        q = Th.shape[1]
        Sh = torch.zeros((d, q), dtype=f64, device=dev)
        fix = torch.abs if absolute else (lambda a: a)
        for k0 in range(0, p, args.block):
            k1 = min(p, k0 + args.block)
            c, mm = [], []
            for l in range(d):
                idx = lev[k0:k1, l][:, None] * int(levels[l]) + lev[:, l][None, :]
                c.append(fix(Cl[l][idx])), mm.append(fix(Ml[l][idx]))
            F = [torch.zeros_like(c[0]) for _ in range(d)]
            for s, w in zip(nodes, weights):
                v = [mm[l] + s * c[l] for l in range(d)]
                suf = [None] * d
                suf[d - 1] = torch.ones_like(c[0])
                for l in range(d - 1, 0, -1):
                    suf[l - 1] = suf[l] * v[l]
                pre = torch.full_like(c[0], w)
                for l in range(d):
                    F[l] += c[l] * (pre * suf[l])
                    pre = pre * v[l]
            for l in range(d):
                Sh[l] += (Th[k0:k1] * (F[l] @ Th)).sum(dim=0)
        return Sh

    rng = np.random.default_rng(9)
    order = (terms > 0).sum(axis=1)
    halves = np.array([0] * (d // 2) + [1] * (d - d // 2), dtype=np.int32)
    res["shapley"] = {}
    for q in qs:
        Theta = rng.standard_normal((p, q)) * (0.5 ** order)[:, None]
        dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)        # p x q column-major
        Th = torch.from_numpy(Theta).to(dev)
        wsb, wsbs = C.c_uint64(0), C.c_uint64(0)
        call("obhip_sobol_workspace_bytes", p, d, q, C.byref(wsb))
        call("obhip_shapley_workspace_bytes", p, d, q, C.byref(wsbs))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
        wss = torch.empty(wsbs.value, dtype=torch.uint8, device=dev)
        out = torch.empty((q, 2 + 2 * d), dtype=f64, device=dev)
        outs = torch.empty((q, P), dtype=f64, device=dev)
        out2 = torch.empty((q, 2), dtype=f64, device=dev)

        def shapley():
            call("obhip_shapley_dev", t._h, None, dth.data_ptr(), q, mtab.data_ptr(), ctab.data_ptr(), outs.data_ptr(),
                 wss.data_ptr(), wsbs.value)

        def shapley_halves():
            call("obhip_shapley_dev", t._h, halves.ctypes.data, dth.data_ptr(), q, mtab.data_ptr(), ctab.data_ptr(),
                 out2.data_ptr(), wss.data_ptr(), wsbs.value)

        def sobol():
            call("obhip_sobol_dev", t._h, dth.data_ptr(), q, mtab.data_ptr(), ctab.data_ptr(), out.data_ptr(), None,
                 ws.data_ptr(), wsb.value)
        ts, t1, tr = [], [], []
        for _ in range(3):                                                   # alternating
            ts += timed(shapley, args.fill / 3)
            t1 += timed(sobol, args.fill / 3)
            tr += timed(lambda: restatement(Th), args.fill / 3)
        Sh, aSh = restatement(Th), restatement(Th, absolute=True)
        K = p * p + 3 * d + 2 * G + 4
        tol = (K * U / (1 - K * U) + (P - 1) * 2 * U) * aSh.cpu()
        shapley()
        torch.cuda.synchronize()
        got = outs.cpu().T
        r = float(((got - Sh.cpu()).abs() / tol).max())
        V = out.cpu()[:, 1]
        ss, s1, sr = stats(ts), stats(t1), stats(tr)
        opss, ops1 = ops_shapley(p, d, P, q), ops_sobol(p, d, q)
        rec = {"shapley_dev": ss, "sobol_dev": s1, "torch_restatement": sr,
               "shapley_over_sobol": ss["median_ms"] / s1["median_ms"], "operations_model_ratio": opss / ops1,
               "restatement_over_shapley": sr["median_ms"] / ss["median_ms"],
               "kernel_vs_restatement_err_over_tolerance": r,
               "column_sum_vs_sobol_V_relative": float(((got.sum(dim=0) - V).abs() / V.abs()).max()),
               "workspace_bytes": wsbs.value, "operations_model": opss,
               "share_of_fp64_vector_peak": opss / (ss["median_ms"] * 1e-3) / FP64_VECTOR_PEAK}
        if q == qs[0]:
            rec["shapley_dev_two_players"] = stats(timed(shapley_halves, args.fill / 3))
        res["shapley"]["q=%d" % q] = rec
        print("q=%d: shapley %.3f ms (spread %.2f), sobol %.3f ms (spread %.2f): ratio %.2f, model %.2f; restatement "
              "%.1f ms (spread %.2f): %.1f x; err/tolerance %.3g" % (
                  q, ss["median_ms"], ss["spread"], s1["median_ms"], s1["spread"], ss["median_ms"] / s1["median_ms"],
                  opss / ops1, sr["median_ms"], sr["spread"], sr["median_ms"] / ss["median_ms"], r), flush=True)
        assert r < args.agree, "the kernel and the restatement disagree beyond the stated share of the tolerance"
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v["shapley_over_sobol"] for k, v in res["shapley"].items()}))


if __name__ == "__main__":
    main()
