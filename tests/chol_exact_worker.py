"""Worker of tests/test_gpu_chol.py: the schedule switches of the Cholesky (OBHIP_CHOL_PANELS, _M8, _M4,
_T64) are read once per process, so every environment runs in a process of its own.  The parent builds
every matrix and every bound; this process only loads, calls the library and writes back what came out.
Usage: chol_exact_worker.py <directory>; <directory>/jobs.json lists the jobs in ascending size:

  {"name", "kind": "solve" | "multi" | "npd", "p", "q", "rho", "G": file, "R": file (q x p), "terms": file | null}

Per job it writes <name>_L.npy (the p x p matrix the call left in d_G), <name>_theta.npy (q x p),
<name>_diag.npy (d_diagH) and <name>_guard.npy (the sentinel bytes behind the workspace); for "npd" the
error text in <name>_msg.txt.  It prints "done <name>" per job and stops at the first error."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import outerbase_amd as ob  # noqa: E402
from conftest import knots_for  # noqa: E402
from outerbase_amd._lib import call  # noqa: E402
from posterior_ref import KINDS, NKNOTS  # noqa: E402

GUARD_BYTES = 4096
SENTINEL = 0xA5


def main(d):
    with open(os.path.join(d, "jobs.json")) as f:
        jobs = json.load(f)
    om = ob.outermod()
    ob.setcovfs(om, KINDS)
    ob.setknot(om, knots_for(KINDS, NKNOTS))
    for job in jobs:
        name, p, q = job["name"], int(job["p"]), int(job["q"])
        terms = om.selectterms(p) if job["terms"] is None else np.load(os.path.join(d, job["terms"]))
        t = ob.obmod._Terms(om, terms)
        G = torch.from_numpy(np.load(os.path.join(d, job["G"]))).cuda()
        R = torch.from_numpy(np.load(os.path.join(d, job["R"]))).cuda()
        assert G.shape == (p, p) and R.shape == (q, p) and G.is_contiguous() and R.is_contiguous()
        wsb = C.c_uint64(0)
        if job["kind"] == "multi":
            call("obhip_newton_multi_workspace_bytes", p, q, C.byref(wsb))
        else:
            call("obhip_newton_workspace_bytes", p, C.byref(wsb))
        ws = torch.full((wsb.value + GUARD_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda")
        th = torch.full((q, p), float("nan"), dtype=torch.float64, device="cuda")
        dH = torch.full((p,), float("nan"), dtype=torch.float64, device="cuda")
        if job["kind"] == "multi":
            args = ("obhip_newton_multi_solve_dev", om._h, t._h, G.data_ptr(), R.data_ptr(), q, 0.0, job["rho"],
                    th.data_ptr(), dH.data_ptr(), ws.data_ptr(), wsb.value)
        else:
            args = ("obhip_newton_solve_dev", om._h, t._h, G.data_ptr(), R.data_ptr(), 0.0, job["rho"],
                    th.data_ptr(), dH.data_ptr(), ws.data_ptr(), wsb.value)
        if job["kind"] == "npd":
            try:
                call(*args)
                msg = "no error"
            except ob.ObhipError as e:
                msg = str(e)
            torch.cuda.synchronize()
            with open(os.path.join(d, name + "_msg.txt"), "w") as f:
                f.write(msg)
        else:
            call(*args)
            torch.cuda.synchronize()
            np.save(os.path.join(d, name + "_L.npy"), G.cpu().numpy())
            np.save(os.path.join(d, name + "_theta.npy"), th.cpu().numpy())
            np.save(os.path.join(d, name + "_diag.npy"), dH.cpu().numpy())
        np.save(os.path.join(d, name + "_guard.npy"), ws[wsb.value:].cpu().numpy())
        print("done", name, flush=True)
        del G, R, ws, th, dH


if __name__ == "__main__":
    main(sys.argv[1])
