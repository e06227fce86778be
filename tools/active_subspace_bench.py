"""What C = E[grad f grad f^T] costs in closed form at d = 20 with the headline term set (selectterms, p = 4096).

One process.  Timed with device events after a warm-up, over enough repetitions to fill --fill seconds, alternating
three times in the same run:
  tables  obhip_dim_grad_moments_dev beside the untouched obhip_dim_moments_dev on the same inputs, at --rows
          empirical rows and at 64 Gauss-Legendre nodes per dimension;
  sums    at q = 1, 8, 64:
          (a) obhip_active_dev (gbar and the 210 entries of C);
          (b) a torch float64 restatement of the pair sums in row blocks on the same GPU -- written here, and checked
              against the kernel to --agree of the stage-2 tolerance gamma_{p^2+3d+4} sum |theta theta'| |X| |X| prod |A|
              (the absolute sums come from the same restatement);
          (c) the Monte-Carlo route: obhip_predict_jac_multi_dev on N rows drawn from the product of the empirical
              marginals plus one J J^T / N per response, at the N (doubling from 1000) at which the eigenvalues of
              response 0 that exceed 1 % of the largest are all within 1 % of the closed form's.
Recorded with the times and their spread: the operation model of the pair sum, the ratios, and the resource usage of
the new kernels as the compiler reports it (-Rpass-analysis=kernel-resource-usage, gfx950).  Writes one JSON.

  python tools/active_subspace_bench.py [--rows 1000000 --p 4096 --d 20 --qs 1,8,64]
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
T = 5                       # kActiveT: dimensions per block of the output triangle
# VGPRs, AGPRs, scratch bytes per lane, waves per SIMD (compiler remarks, gfx950)
RESOURCES = {"k_moments<DerivMeans>": [154, 0, 0, 3], "k_moments<DerivCross>": [256, 2, 0, 1],
             "k_moments<DerivProducts>": [256, 2, 0, 1], "k_moments_fin<one tile|all pairs|lower pairs>": [22, 0, 0, 8],
             "k_active_gbar": [20, 0, 0, 8], "k_block_reduce<5, 2, with diagonal>": [8, 0, 0, 8],
             "k_block_pairs<ActiveOp, 8, diagonal>": [146, 0, 0, 3],
             "k_block_pairs<ActiveOp, 8, off-diagonal>": [203, 0, 0, 2],
             "k_block_pairs<ActiveOp, 24, diagonal>": [163, 0, 0, 3],
             "k_block_pairs<ActiveOp, 24, off-diagonal>": [235, 0, 0, 2]}


def ops_active(p, d, q):
    """per term pair, nb diagonal passes (outside product d - T; suffix products and the two
    column factors 3 T; per row the diagonal entry 3 and the two row factors 2; per output above the diagonal 3 and 2
    for the running middle products; per response 1 + T (T + 1) / 2) and nb (nb - 1) / 2 off-diagonal ones (d - 2 T;
    prefix, suffix and the two oriented factors of the row and of the column block 5 T each; 3 T^2 for the outputs;
    per response 1 + T^2)"""
    nb = (d + T - 1) // T
    noff = nb * (nb - 1) // 2
    per_pair = nb * (max(d - T, 0) + 3 * T + 5 * T + 5 * T * (T - 1) // 2) + noff * (max(d - 2 * T, 0) + 10 * T + 3 * T * T)
    per_resp = nb * (1 + T * (T + 1) // 2) + noff * (1 + T * T)
    return p * (p + 1) / 2 * (per_pair + q * per_resp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--qs", default="1,8,64")
    ap.add_argument("--fill", type=float, default=0.5)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--mc-max", type=int, default=1 << 21)
    ap.add_argument("--agree", type=float, default=1e-2, help="kernel vs restatement, as a share of the tolerance")
    ap.add_argument("--out", default=os.path.join("profiles", "active_subspace_bench.json"))
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
    iu = np.triu_indices(d)
    ntri = len(iu[0])

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

    res = {"config": {"d": d, "n": n, "p": p, "knots": args.knots, "levels": levels.tolist(), "entries_of_C": ntri},
           "source_hash": lib.obhip_source_hash(0).decode(), "device": torch.cuda.get_device_name(0),
           "kernel_resources_vgpr_agpr_scratch_waves": RESOURCES}
    # ---- the tables: n empirical rows, then 64 Gauss-Legendre nodes on the box of those rows ----------------
    x = torch.empty((d, n), dtype=f64, device=dev)
    ysyn = torch.empty(n, dtype=f64, device=dev)
    call("obhip_synth_xy_dev", 7, 0, n, d, np.zeros(d, dtype=np.int32).ctypes.data, x.data_ptr(), ysyn.data_ptr())
    mtab, dmtab = (torch.empty(nm, dtype=f64, device=dev) for _ in range(2))
    ctab, xtab, ddtab = (torch.empty(nc, dtype=f64, device=dev) for _ in range(3))
    lo, hi = x.min(dim=1).values.cpu().numpy(), x.max(dim=1).values.cpu().numpy()
    gz, gw = ob.uniform_nodes(lo, hi, 64)
    dgz = torch.from_numpy(np.ascontiguousarray(gz.T)).to(dev)
    dgw = torch.from_numpy(np.ascontiguousarray(gw.T)).to(dev)
    res["tables"] = {}
    for name, nodes, wts, rows in (("gauss_legendre_64", dgz, dgw, 64), ("empirical_rows", x, None, n)):
        wp = None if wts is None else wts.data_ptr()

        def grad_tables():
            call("obhip_dim_grad_moments_dev", om._h, t._h, nodes.data_ptr(), rows, rows, wp, rows, dmtab.data_ptr(),
                 xtab.data_ptr(), ddtab.data_ptr())

        def tables():
            call("obhip_dim_moments_dev", om._h, t._h, nodes.data_ptr(), rows, rows, wp, rows, mtab.data_ptr(),
                 ctab.data_ptr())
        tg, tm = [], []
        for _ in range(3):                                                       # alternating
            tg += timed(grad_tables, args.fill / 3)
            tm += timed(tables, args.fill / 3)
        sg, sm = stats(tg), stats(tm)
        res["tables"][name] = {"rows": rows, "dim_grad_moments_dev": sg, "dim_moments_dev": sm,
                               "grad_over_moments": sg["median_ms"] / sm["median_ms"]}
        print("%s (%d rows): gradient tables %.3f ms (spread %.2f), moment tables %.3f ms (spread %.2f): ratio %.2f" % (
            name, rows, sg["median_ms"], sg["spread"], sm["median_ms"], sm["spread"], sg["median_ms"] / sm["median_ms"]),
            flush=True)
    # (the tables of the empirical rows stay in the buffers: the sums below are taken on them)
    om_ = np.concatenate([[0], np.cumsum(levels)])
    oc_ = np.concatenate([[0], np.cumsum(levels ** 2)])
    lev = torch.from_numpy(terms.astype(np.int64)).to(dev)
    ml = [mtab[om_[l]:om_[l + 1]] for l in range(d)]
    Al = [(ctab[oc_[l]:oc_[l + 1]].view(levels[l], levels[l]) + torch.outer(ml[l], ml[l])).reshape(-1) for l in range(d)]
    Xl = [xtab[oc_[l]:oc_[l + 1]] for l in range(d)]
    Dl = [ddtab[oc_[l]:oc_[l + 1]] for l in range(d)]

    def restatement(Th, absolute=False):
        """the packed upper triangle of C (ntri x q): row blocks of --block terms against all p, every ordered pair"""
        q = Th.shape[1]
        out = torch.zeros((ntri, q), dtype=f64, device=dev)
        fix = torch.abs if absolute else (lambda a: a)
        for k0 in range(0, p, args.block):
            k1 = min(p, k0 + args.block)
            a, xf, xb, dg = [], [], [], []
            for l in range(d):
                L = int(levels[l])
                idx = lev[k0:k1, l][:, None] * L + lev[:, l][None, :]
                idt = lev[:, l][None, :] * L + lev[k0:k1, l][:, None]
                a.append(fix(Al[l][idx])), xf.append(fix(Xl[l][idx])), xb.append(fix(Xl[l][idt])), dg.append(fix(Dl[l][idx]))
            suf = [None] * (d + 1)
            suf[d] = torch.ones_like(a[0])
            for l in range(d - 1, -1, -1):
                suf[l] = suf[l + 1] * a[l]
            pre, o = torch.ones_like(a[0]), 0
            for i in range(d):
                out[o] += (Th[k0:k1] * ((pre * dg[i] * suf[i + 1]) @ Th)).sum(dim=0)
                o += 1
                row = pre * xf[i]
                for j in range(i + 1, d):
                    out[o] += (Th[k0:k1] * ((row * xb[j] * suf[j + 1]) @ Th)).sum(dim=0)
                    row = row * a[j]
                    o += 1
                pre = pre * a[i]
        return out

    rng = np.random.default_rng(9)
    order = (terms > 0).sum(axis=1)
    nout = d + ntri
    res["active"] = {}
    for q in qs:
        Theta = rng.standard_normal((p, q)) * (0.5 ** order)[:, None]
        dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)        # p x q column-major
        Th = torch.from_numpy(Theta).to(dev)
        wsb = C.c_uint64(0)
        call("obhip_active_workspace_bytes", p, d, q, C.byref(wsb))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
        out = torch.empty((q, nout), dtype=f64, device=dev)

        def kernel():
            call("obhip_active_dev", t._h, dth.data_ptr(), q, mtab.data_ptr(), ctab.data_ptr(), dmtab.data_ptr(),
                 xtab.data_ptr(), ddtab.data_ptr(), out.data_ptr(), ws.data_ptr(), wsb.value)
        kernel()
        torch.cuda.synchronize()
        Cpk = out.cpu().numpy()[:, d:]                                         # q x ntri
        # the Monte-Carlo route: N from the eigenvalues of response 0
        Cm = np.zeros((d, d))
        Cm[iu] = Cpk[0]
        Cm = Cm + np.triu(Cm, 1).T
        lam = np.linalg.eigvalsh(Cm)[::-1]
        big = lam >= 1e-2 * lam[0]
        N, mc_err, gen = 500, None, torch.Generator(device=dev)
        gen.manual_seed(q)
        while True:
            N *= 2
            pick = torch.randint(0, n, (d, N), device=dev, generator=gen)
            xmc = torch.gather(x, 1, pick).contiguous()                      # the product of the empirical marginals
            jac = torch.empty((q, d, N), dtype=f64, device=dev)

            def monte_carlo():
                call("obhip_predict_jac_multi_dev", om._h, t._h, dth.data_ptr(), q, xmc.data_ptr(), N, None, jac.data_ptr())
                return torch.bmm(jac, jac.transpose(1, 2)) / N
            lam_mc = np.linalg.eigvalsh(monte_carlo()[0].cpu().numpy())[::-1]
            mc_err = float(np.max(np.abs(lam_mc[big] - lam[big]) / lam[big]))
            if mc_err < 1e-2 or 2 * N > args.mc_max:
                break
        ta, tr, tmc = [], [], []
        for _ in range(3):                                                   # alternating
            ta += timed(kernel, args.fill / 3)
            tr += timed(lambda: restatement(Th), args.fill / 3)
            tmc += timed(monte_carlo, args.fill / 3)
        Cr, aCr = restatement(Th), restatement(Th.abs(), absolute=True)
        gq = (p * p + 3 * d + 4) * U / (1 - (p * p + 3 * d + 4) * U)
        r = float(((torch.from_numpy(Cpk).T - Cr.cpu()).abs() / (gq * aCr.cpu())).max())
        sa, sr, smc = stats(ta), stats(tr), stats(tmc)
        ops = ops_active(p, d, q)
        res["active"]["q=%d" % q] = {
            "active_dev": sa, "torch_restatement": sr, "monte_carlo": smc, "monte_carlo_rows": N,
            "monte_carlo_eigenvalue_error": mc_err, "eigenvalues_compared": int(big.sum()),
            "restatement_over_active": sr["median_ms"] / sa["median_ms"],
            "monte_carlo_over_active": smc["median_ms"] / sa["median_ms"],
            "kernel_vs_restatement_err_over_tolerance": r, "workspace_bytes": wsb.value, "operations_model": ops,
            "share_of_fp64_vector_peak": ops / (sa["median_ms"] * 1e-3) / FP64_VECTOR_PEAK}
        print("q=%d: active %.3f ms (spread %.2f); restatement %.1f ms (spread %.2f): %.1f x; Monte Carlo at N=%d "
              "(eigenvalue error %.3g) %.3f ms (spread %.2f): %.2f x; err/tolerance %.3g" % (
                  q, sa["median_ms"], sa["spread"], sr["median_ms"], sr["spread"], sr["median_ms"] / sa["median_ms"], N,
                  mc_err, smc["median_ms"], smc["spread"], smc["median_ms"] / sa["median_ms"], r), flush=True)
        assert r < args.agree, "the kernel and the restatement disagree beyond the stated share of the tolerance"
    call("obhip_profile_enable", 1)
    call("obhip_profile_reset")
    kernel()
    torch.cuda.synchronize()
    res["scopes_last_q"] = {}
    for name in ("active_pairs",):
        cnt, ms = C.c_uint64(0), C.c_double(0.0)
        call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
        res["scopes_last_q"][name] = {"launches": cnt.value, "ms": ms.value}
    call("obhip_profile_enable", 0)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v["restatement_over_active"] for k, v in res["active"].items()}))


if __name__ == "__main__":
    main()
