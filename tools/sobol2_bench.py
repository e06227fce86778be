"""What the pairwise Sobol quantities cost at d = 20 with the headline term set (selectterms, p = 4096).

One process.  Timed with device events after a warm-up, over enough repetitions to fill --fill seconds, alternating
three times in the same run at q = 1, 8, 64:
  (a) obhip_sobol2_dev (G_ij, V2_ij, VT2_ij of all 190 pairs);
  (b) the untouched obhip_sobol_dev on the same tables;
  (c) a torch float64 restatement of the VT2 pair sums in row blocks on the same GPU -- written here, and checked
      against the kernel to --agree of the stage-2 tolerance gamma_{p^2+3d+4} sum |theta theta'| |C_i| |C_j| prod |A_l|
      (the absolute sums come from the same restatement).
Recorded with the times and their spread: the operation models of the two pair sums and their ratio beside the
measured ratio, the ratio to the restatement, and the resource usage of the new kernels as the compiler reports it
(-Rpass-analysis=kernel-resource-usage, gfx950).  Writes one JSON.

  python tools/sobol2_bench.py [--rows 100000 --p 4096 --d 20 --qs 1,8,64]
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
T = 5                       # kSobol2T: dimensions per block of the output triangle
# VGPRs, AGPRs, scratch bytes per lane, waves per SIMD (compiler remarks, gfx950)
RESOURCES = {"k_sobol2_second": [48, 0, 0, 8], "k_block_reduce<5, 2, no diagonal>": [8, 0, 0, 8],
             "k_interaction_effect": [129, 0, 0, 3],
             "k_block_pairs<Sobol2Op, 8, diagonal>": [88, 0, 0, 5],
             "k_block_pairs<Sobol2Op, 8, off-diagonal>": [179, 0, 0, 2],
             "k_block_pairs<Sobol2Op, 24, diagonal>": [125, 0, 0, 4],
             "k_block_pairs<Sobol2Op, 24, off-diagonal>": [207, 0, 0, 2]}


def ops_sobol(p, d, q):
    """DESIGN.md section 19"""
    return p * (p + 1) / 2 * (7 * d + 2 * (d + 1) * q)


def ops_sobol2(p, d, q):
    """per term pair, nb diagonal passes (outside product d - T, row and column factors 4 T,
    T (T - 1) for the outputs; per response 1 + T (T - 1)) and nb (nb - 1) / 2 off-diagonal ones (d - 2 T, 8 T, T^2;
    per response 1 + 2 T^2)"""
    nb = (d + T - 1) // T
    noff = nb * (nb - 1) // 2
    per_pair = nb * (max(d - T, 0) + 4 * T + T * (T - 1)) + noff * (max(d - 2 * T, 0) + 8 * T + T * T)
    per_resp = nb * (1 + T * (T - 1)) + noff * (1 + 2 * T * T)
    return p * (p + 1) / 2 * (per_pair + q * per_resp)


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
    ap.add_argument("--out", default=os.path.join("profiles", "sobol2_bench.json"))
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
    pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
    npairs = len(pairs)

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

    res = {"config": {"d": d, "n": n, "p": p, "knots": args.knots, "levels": levels.tolist(), "pairs": npairs},
           "source_hash": lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0),
           "kernel_resources_vgpr_agpr_scratch_waves": RESOURCES}
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
    ml = [mtab[om_[l]:om_[l + 1]] for l in range(d)]
    Al = [(Cl[l].view(levels[l], levels[l]) + torch.outer(ml[l], ml[l])).reshape(-1) for l in range(d)]

    def restatement(Th, absolute=False):
        """VT2 (n_pairs x q) of the pair sums, row blocks of --block terms against all p"""
        q = Th.shape[1]
        VT2 = torch.zeros((npairs, q), dtype=f64, device=dev)
        fix = torch.abs if absolute else (lambda a: a)
        for k0 in range(0, p, args.block):
            k1 = min(p, k0 + args.block)
            a, c = [], []
            for l in range(d):
                idx = lev[k0:k1, l][:, None] * int(levels[l]) + lev[:, l][None, :]
                a.append(fix(Al[l][idx])), c.append(fix(Cl[l][idx]))
            suf = [None] * d
            suf[d - 1] = torch.ones_like(a[0])
            for l in range(d - 1, 0, -1):
                suf[l - 1] = suf[l] * a[l]
            pre, o = torch.ones_like(a[0]), 0
            for i in range(d):
                row = pre * c[i]
                for j in range(i + 1, d):
                    VT2[o] += (Th[k0:k1] * ((row * c[j] * suf[j]) @ Th)).sum(dim=0)
                    row = row * a[j]
                    o += 1
                pre = pre * a[i]
        return VT2

    rng = np.random.default_rng(9)
    order = (terms > 0).sum(axis=1)
    res["sobol2"] = {}
    for q in qs:
        Theta = rng.standard_normal((p, q)) * (0.5 ** order)[:, None]
        dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)        # p x q column-major
        Th = torch.from_numpy(Theta).to(dev)
        wsb, wsb2 = C.c_uint64(0), C.c_uint64(0)
        call("obhip_sobol_workspace_bytes", p, d, q, C.byref(wsb))
        call("obhip_sobol2_workspace_bytes", p, d, q, C.byref(wsb2))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
        ws2 = torch.empty(wsb2.value, dtype=torch.uint8, device=dev)
        out = torch.empty((q, 2 + 2 * d), dtype=f64, device=dev)
        out2 = torch.empty((q, 2 * npairs), dtype=f64, device=dev)

        def kernel2():
            call("obhip_sobol2_dev", t._h, dth.data_ptr(), q, mtab.data_ptr(), ctab.data_ptr(), out2.data_ptr(), None,
                 ws2.data_ptr(), wsb2.value)

        def kernel1():
            call("obhip_sobol_dev", t._h, dth.data_ptr(), q, mtab.data_ptr(), ctab.data_ptr(), out.data_ptr(), None,
                 ws.data_ptr(), wsb.value)
        t2, t1, tr = [], [], []
        for _ in range(3):                                                   # alternating
            t2 += timed(kernel2, args.fill / 3)
            t1 += timed(kernel1, args.fill / 3)
            tr += timed(lambda: restatement(Th), args.fill / 3)
        VT2, aVT2 = restatement(Th), restatement(Th, absolute=True)
        gq = (p * p + 3 * d + 4) * U / (1 - (p * p + 3 * d + 4) * U)
        got = out2.cpu()[:, npairs:].T
        r = float(((got - VT2.cpu()).abs() / (gq * aVT2.cpu())).max())
        s2, s1, sr = stats(t2), stats(t1), stats(tr)
        ops2, ops1 = ops_sobol2(p, d, q), ops_sobol(p, d, q)
        res["sobol2"]["q=%d" % q] = {
            "sobol2_dev": s2, "sobol_dev": s1, "torch_restatement_vt2": sr,
            "sobol2_over_sobol": s2["median_ms"] / s1["median_ms"], "operations_model_ratio": ops2 / ops1,
            "restatement_over_sobol2": sr["median_ms"] / s2["median_ms"],
            "kernel_vs_restatement_err_over_tolerance": r, "workspace_bytes": wsb2.value,
            "operations_model": ops2, "share_of_fp64_vector_peak": ops2 / (s2["median_ms"] * 1e-3) / FP64_VECTOR_PEAK}
        print("q=%d: sobol2 %.3f ms (spread %.2f), sobol %.3f ms (spread %.2f): ratio %.2f, model %.2f; restatement "
              "%.1f ms (spread %.2f): %.1f x; err/tolerance %.3g" % (
                  q, s2["median_ms"], s2["spread"], s1["median_ms"], s1["spread"], s2["median_ms"] / s1["median_ms"],
                  ops2 / ops1, sr["median_ms"], sr["spread"], sr["median_ms"] / s2["median_ms"], r), flush=True)
        assert r < args.agree, "the kernel and the restatement disagree beyond the stated share of the tolerance"
    call("obhip_profile_enable", 1)
    call("obhip_profile_reset")
    kernel2()
    torch.cuda.synchronize()
    res["scopes_last_q"] = {}
    for name in ("sobol2_second", "sobol2_pairs"):
        cnt, ms = C.c_uint64(0), C.c_double(0.0)
        call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
        res["scopes_last_q"][name] = {"launches": cnt.value, "ms": ms.value}
    call("obhip_profile_enable", 0)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v["restatement_over_sobol2"] for k, v in res["sobol2"].items()}))


if __name__ == "__main__":
    main()
