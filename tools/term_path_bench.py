"""What the term-count path costs at d = 20 with the headline term set (selectterms, p = 4096), step 16 (K = 256
sizes), 20 000 rows in the fit and 1e5 hold-out rows, q = 1 and 16 responses, alternating in one process with two
yardsticks on the same rows:

  (a) the score pass, obhip_posterior_path_scores_dev, beside obhip_posterior_var_dev: the same matrix product
      Z = B L^-T without the path (row norms in the product's epilogue, Z never stored; code this entry does not
      touch).  The record is scores / var per q, and from the library's own event scopes the stored product
      (term_path_gemm) and the walk over it (term_path_walk) beside the row-norm product (predict_std_gemm).
  (b) the whole path -- a new accumulator, the fit rows added, NewtonAccumulator.term_path with the hold-out rows --
      beside refitting 8 of the 256 sizes the existing way (fit_newton_multi on terms[:k], obhip_predict_multi_dev on
      the hold-out rows, obhip_cv_score_dev), that time scaled by 256 / 8.  The 8 sizes are spread evenly, k = 512,
      1024, ..., 4096, so their mean cost stands for the mean over all sizes of a cost that grows with k.  A size
      that fit_newton_multi refuses (OBHIP_ERR_NUMERIC) is listed under "refit_refused" with the library's message and
      left out; the time of the sizes that were fitted ("refit_sizes") is then scaled by 256 / their number.

Timed with a host clock around calls that end in a device synchronise, after a warm-up of every shape.

The GPU part runs as a child process under its own `timeout -k 10`.

  python tools/term_path_bench.py [--rows 100000 --p 4096 --d 20 --step 16]
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
SCOPES = ("term_path_gemm", "term_path_walk", "predict_std_gemm")


def part(args):
    from design_bench import scope, setup
    s = setup(args)
    torch, np, lib, ob, om, terms = s["torch"], s["np"], s["lib"], s["ob"], s["om"], s["terms"]
    n, nf, p, step, f64, dev = args.rows, args.fit_rows, args.p, args.step, torch.float64, s["dev"]
    xf, yf = s["synth"](3, nf)
    xh, yh = s["synth"](7, n)
    rng = np.random.default_rng(5)

    def responses(y, q):
        """q columns: the synthetic response, then seeded mixtures of it with noise (host, n x q)"""
        y = y.cpu().numpy()[0]
        cols = [y] + [y * (1 + 0.1 * j) + 0.05 * y.std() * rng.standard_normal(len(y)) for j in range(1, q)]
        return np.stack(cols, axis=1)
    xf_h, xh_h = xf.cpu().numpy().T.copy(), xh.cpu().numpy().T.copy()
    K = C.c_uint64(0)
    lib.call("obhip_term_path_layout", p, 1, step, n, 0, C.byref(K), None, None)
    K = K.value
    res = {"config": {"d": args.d, "p": p, "rows": n, "fit_rows": nf, "step": step, "K": K, "sigma": args.sigma,
                      "rho": args.rho, "reps": args.reps},
           "source_hash": lib.lib.obhip_source_hash(0).decode(), "gram_hash": lib.lib.obhip_source_hash(1).decode(),
           "device": torch.cuda.get_device_name(0)}
    lib.call("obhip_profile_enable", 1)

    def timed(fn):
        lib.call("obhip_profile_reset")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out = {"total_ms": 1e3 * (time.perf_counter() - t0)}
        out.update({name: scope(lib, name) for name in SCOPES})
        return out

    sizes8 = [p * (i + 1) // 8 for i in range(8)]
    for q in args.q:
        Yf, Yh = responses(yf, q), responses(yh, q)
        dYh = torch.from_numpy(np.ascontiguousarray(Yh.T)).to(dev)
        with ob.NewtonAccumulator(om, terms, q) as acc:
            acc.add(xf_h, Yf)
            post = acc.posterior(args.sigma, args.rho)
            dG = torch.empty((q, p), dtype=f64, device=dev)
            dms = torch.empty((q, 3), dtype=f64, device=dev)
            lib.call("obhip_normal_acc_rhs_dev", acc._h, None, args.sigma, dG.data_ptr(), dms.data_ptr())
            dU = torch.empty_like(dG)
            lib.call("obhip_posterior_path_coef_dev", post._h, dG.data_ptr(), q, dU.data_ptr())
        var = torch.empty(n, dtype=f64, device=dev)
        scores = torch.empty((K, q, 3), dtype=f64, device=dev)
        sumv = torch.empty(K, dtype=f64, device=dev)
        mean = torch.empty((q, n), dtype=f64, device=dev)
        cv = torch.empty((q, 2), dtype=f64, device=dev)

        def whole_path():
            with ob.NewtonAccumulator(om, terms, q) as a:
                a.add(xf_h, Yf)
                with a.term_path(args.sigma, args.rho, step=step, x=xh_h, Y=Yh) as path:
                    return path.best("lpd")

        refused, used = {}, []

        def choose_sizes():
            """the nominal sizes the library fits; one it refuses is recorded and left out, never replaced"""
            for k in sizes8:
                try:
                    ob.fit_newton_multi(om, terms[:k], xf_h, Yf, sigma=args.sigma, rho=args.rho)
                    used.append(k)
                except ob.ObhipError as e:
                    if e.code != 5:
                        raise
                    refused[k] = str(e)
            if not used:
                raise RuntimeError("none of the sizes could be fitted")

        def refit8():
            for k in used:
                fit = ob.fit_newton_multi(om, terms[:k], xf_h, Yf, sigma=args.sigma, rho=args.rho)
                th = torch.from_numpy(np.ascontiguousarray(fit.coeff.T)).to(dev)
                ms = torch.from_numpy(np.ascontiguousarray(fit._meansd)).to(dev)
                lib.call("obhip_predict_multi_dev", om._h, fit._t._h, th.data_ptr(), q, xh.data_ptr(), n, mean.data_ptr(),
                         None, args.sigma, None)
                lib.call("obhip_cv_score_dev", mean.data_ptr(), dYh.data_ptr(), n, q, n, ms.data_ptr(), cv.data_ptr())

        calls = {
            "a_posterior_var": lambda: lib.call("obhip_posterior_var_dev", post._h, xh.data_ptr(), n, var.data_ptr(), 0),
            "a_path_scores": lambda: lib.call("obhip_posterior_path_scores_dev", post._h, dU.data_ptr(), q, xh.data_ptr(),
                                              n, dYh.data_ptr(), n, dms.data_ptr(), step, 0, 0, scores.data_ptr(),
                                              sumv.data_ptr()),
            "b_whole_path": whole_path,
            "b_refit_8_sizes": refit8,
        }
        choose_sizes()
        for fn in calls.values():                                           # warm-up of every shape
            fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in calls}
        for _ in range(args.reps):                                          # alternating
            for k, fn in calls.items():
                runs[k].append(timed(fn))
        med = {k: statistics.median([a["total_ms"] for a in v]) for k, v in runs.items()}
        r = {k: {"total_ms": [a["total_ms"] for a in v]} for k, v in runs.items()}
        for name in ("term_path_gemm", "term_path_walk"):
            r["a_path_scores"][name + "_ms"] = statistics.median([a[name]["ms"] for a in runs["a_path_scores"]])
            r["a_path_scores"][name + "_launches"] = runs["a_path_scores"][0][name]["launches"]
        r["a_posterior_var"]["predict_std_gemm_ms"] = statistics.median(
            [a["predict_std_gemm"]["ms"] for a in runs["a_posterior_var"]])
        r["best_by_lpd"] = whole_path()
        r["refit_sizes"] = used
        r["refit_refused"] = {str(k): e for k, e in refused.items()}
        r["ratios"] = {"a_scores_over_var": med["a_path_scores"] / med["a_posterior_var"],
                       "b_refit_scaled_to_K_ms": med["b_refit_8_sizes"] * K / len(used),
                       "b_refit_scaled_over_whole_path": med["b_refit_8_sizes"] * K / len(used) / med["b_whole_path"]}
        res["q%d" % q] = r
        post.close()
    print(json.dumps(res), flush=True)
    lib.call("obhip_profile_enable", 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--p", type=int, default=4096)
    ap.add_argument("--d", type=int, default=20)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--q", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--knots", type=int, default=40)
    ap.add_argument("--fit-rows", type=int, default=20_000)
    ap.add_argument("--sigma", type=float, default=-2.302585092994046)
    ap.add_argument("--rho", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--part", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "term_path_bench.json"))
    args = ap.parse_args()
    if args.part:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        res = part(args)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        return
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--part", "--out", args.out]
    for key in ("rows", "p", "d", "step", "knots", "fit_rows", "sigma", "rho", "reps"):
        cmd.append("--%s=%s" % (key.replace("_", "-"), getattr(args, key)))
    cmd += ["--q"] + [str(v) for v in args.q]
    rc = subprocess.call(cmd)
    if rc != 0:
        sys.exit("term_path_bench: the GPU part ended with status %d" % rc)
    print(json.dumps({"term_path_bench": args.out}))


if __name__ == "__main__":
    main()
