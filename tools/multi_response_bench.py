"""What q responses cost next to q single fits, at BASELINE configs[2] (d=20, n=1e6, p=4096).

One process.  For every q in --q the parent path (a) HotPath.step() and (b) MultiHotPath.step() at
that q alternate --reps times after a warm-up of both (device events around each step); then one
profiled step of each gives the per-scope times (obhip_profile_get).  The existing single-column
pieces the batched kernels replace are timed on their own: obhip_basis_tmm_dev (events), and the
`backsolve` and `predict` scopes of the parent's step.  Writes one JSON (--out).

  python tools/multi_response_bench.py [--rows 1000000 --p 4096 --d 20 --q 1,2,4,8,16,32 --reps 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCOPES = ["gram", "materialize_B", "cholesky", "backsolve", "predict", "aty_multi", "trsm_multi",
          "predict_multi", "form_hessian"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--q", default="1,2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "multi_response_bench.json"))
    args = ap.parse_args()
    import torch
    from outerbase_amd import _lib
    from outerbase_amd.driver import HotPath, MultiHotPath
    call = _lib.call
    kinds = ["mat25"] * args.d
    qs = [int(v) for v in args.q.split(",")]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def scopes(fn):
        call("obhip_profile_enable", 1)
        call("obhip_profile_reset")
        fn()
        torch.cuda.synchronize()
        out = {}
        for name in SCOPES:
            cnt, ms = C.c_uint64(0), C.c_double(0.0)
            call("obhip_profile_get", name.encode(), C.byref(cnt), C.byref(ms))
            if cnt.value:
                out[name] = {"launches": cnt.value, "ms": ms.value}
        call("obhip_profile_enable", 0)
        return out

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "all_ms": v}

    a = HotPath(kinds, args.knots, args.p, args.rows)
    a.setup()
    a.step()
    a.step()
    torch.cuda.synchronize()
    res = {"config": {"d": args.d, "n": args.rows, "p": args.p, "knots": args.knots, "reps": args.reps},
           "source_hash": _lib.lib.obhip_source_hash(0).decode(),
           "gram_source_hash": _lib.lib.obhip_source_hash(1).decode(),
           "device": torch.cuda.get_device_name(0), "per_q": {}}
    # the single-column pieces on their own
    out = torch.empty(args.p, dtype=torch.float64, device=a.x.device)
    tmm = [timed(lambda: call("obhip_basis_tmm_dev", a.basis, a.t._h, a.y.data_ptr(), out.data_ptr(), 0))
           for _ in range(args.reps + 1)][1:]
    res["single"] = {"tmm_dev": stats(tmm), "scopes_of_one_step": scopes(a.step)}
    t_a_all = []
    for q in qs:
        b = MultiHotPath(kinds, args.knots, args.p, args.rows, responses=q)
        b.setup()
        b.step()
        a.step()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(a.step))
            tb.append(timed(b.step))
        t_a_all += ta
        res["per_q"][str(q)] = {"parent_step": stats(ta), "multi_step": stats(tb),
                                "multi_scopes": scopes(b.step), "parent_scopes": scopes(a.step)}
        print("q=%2d  parent %.2f ms  multi %.2f ms" % (q, statistics.median(ta), statistics.median(tb)), flush=True)
        b.close()
        del b
        call("obhip_trim_pool")
        torch.cuda.empty_cache()
    a.close()
    Ta = statistics.median(t_a_all)
    res["parent_step_all"] = stats(t_a_all)
    res["spread_ms"] = max(t_a_all) - min(t_a_all)
    one = res["single"]["scopes_of_one_step"]
    summ = {"T_a_ms": Ta}
    for q in qs:
        r = res["per_q"][str(q)]
        summ["T_%d_over_%d_T_a" % (q, q)] = r["multi_step"]["median_ms"] / (q * Ta)
    if "16" in res["per_q"]:
        sc = res["per_q"]["16"]["multi_scopes"]
        n, p = args.rows, args.p
        p_pad = (p + 255) // 256 * 256
        aty = sc.get("aty_multi", {}).get("ms")
        trsm = sc.get("trsm_multi", {}).get("ms")
        prm = sc.get("predict_multi", {}).get("ms")
        pr0 = sc.get("predict", {}).get("ms", 0.0)
        if aty:
            summ["aty_multi_q16_ms"] = aty
            summ["aty_over_16_tmm"] = aty / (16 * statistics.median(tmm))
            summ["aty_B_bytes_per_s"] = 8.0 * n * p_pad / (aty * 1e-3)
        if trsm:
            summ["trsm_multi_q16_ms"] = trsm
            summ["trsm_over_16_backsolve"] = trsm / (16 * one["backsolve"]["ms"])
        if prm:
            summ["predict_q16_ms"] = prm + pr0
            summ["predict_over_16_single"] = (prm + pr0) / (16 * one["predict"]["ms"])
            summ["predict_multi_fp64_flops"] = 2.0 * n * p * 15 / (prm * 1e-3)
    res["summary"] = summ
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(summ))


if __name__ == "__main__":
    main()
