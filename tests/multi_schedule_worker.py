"""Worker of test_multi_solve_under_forced_cholesky_schedules (and home of the backward-error
helper of tests/test_gpu_multi_response.py): OBHIP_CHOL_PANELS is read once per process, so every
schedule runs in a process of its own.
Usage: multi_schedule_worker.py <q> <p> [<p> ...]; prints per size
"ok|BAD <p> <largest eta_multi / allowed> <largest eta_multi> <largest eta_single>"."""
import ctypes as C
import math
import os
import sys

import numpy as np

U = 2.0 ** -53


def backward_errors(H, Theta, R):
    """eta_j = ||H theta_j - r_j||_inf / (||H||_inf ||theta_j||_inf + ||r_j||_inf) per column, in
    extended precision on the host (H p x p, Theta and R p x q)."""
    Hl = np.asarray(H, dtype=np.longdouble)
    Tl = np.asarray(Theta, dtype=np.longdouble)
    Rl = np.asarray(R, dtype=np.longdouble)
    res = np.abs(Hl @ Tl - Rl).max(axis=0)
    hn = np.abs(Hl).sum(axis=1).max()
    return np.asarray(res / (hn * np.abs(Tl).max(axis=0) + np.abs(Rl).max(axis=0)), dtype=np.float64)


def solve_case(om, p, q, ncheck=None, seed=None):
    """Random SPD G (the recipe of tests/chol_schedule_worker.py) and q right-hand sides through
    obhip_newton_multi_solve_dev, and column by column through obhip_newton_solve_dev.
    -> (eta_multi (q), eta_single (ncheck), ncheck)"""
    import torch
    import outerbase_amd as ob
    from outerbase_amd._lib import call
    terms = om.selectterms(p)
    t = ob.obmod._Terms(om, terms)
    torch.manual_seed(p if seed is None else seed)
    A = torch.randn((p, p + 3), dtype=torch.float64, device="cuda")
    G = A @ A.T + 0.5 * torch.eye(p, dtype=torch.float64, device="cuda")
    del A
    Rt = torch.randn((q, p), dtype=torch.float64, device="cuda")      # column-major p x q
    sigma, rho = 0.3, 2.0
    e2 = math.exp(-2 * sigma)
    prec = 1.0 / (om.getvar(terms) * math.exp(2 * rho))
    H = e2 * G.cpu().numpy()
    H[np.diag_indices(p)] += prec
    R = e2 * Rt.cpu().numpy().T
    wsb = C.c_uint64(0)
    call("obhip_newton_multi_workspace_bytes", p, q, C.byref(wsb))
    ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
    Th = torch.full((q, p), float("nan"), dtype=torch.float64, device="cuda")
    dH = torch.empty(p, dtype=torch.float64, device="cuda")
    Gc = G.clone()
    call("obhip_newton_multi_solve_dev", om._h, t._h, Gc.data_ptr(), Rt.data_ptr(), q, sigma, rho,
         Th.data_ptr(), dH.data_ptr(), ws.data_ptr(), wsb.value)
    torch.cuda.synchronize()
    assert np.allclose(dH.cpu().numpy(), np.diag(H), rtol=1e-14)
    eta_m = backward_errors(H, Th.cpu().numpy().T, R)
    ncheck = q if ncheck is None else min(q, ncheck)
    # the single solve on the columns the batched substitution handled first (1, 2, ...); column 0
    # of the batch IS the single solve
    cols = [(1 + i) % q for i in range(ncheck)]
    th1 = torch.empty(p, dtype=torch.float64, device="cuda")
    Ts = np.empty((p, ncheck))
    for i, j in enumerate(cols):
        Gc.copy_(G)
        call("obhip_newton_solve_dev", om._h, t._h, Gc.data_ptr(), Rt[j].data_ptr(), sigma, rho,
             th1.data_ptr(), dH.data_ptr(), ws.data_ptr(), wsb.value)
        torch.cuda.synchronize()
        Ts[:, i] = th1.cpu().numpy()
    eta_s = backward_errors(H, Ts, R[:, cols])
    return eta_m, eta_s, cols


def allowed(eta_m, eta_s, cols, p):
    """eta_j <= max(4 eta_single_j, p 2^-53); the columns whose single solve was not run are held
    to the smallest eta_single that was."""
    lim = np.full(len(eta_m), 4 * eta_s.min())
    lim[cols] = 4 * eta_s
    return np.maximum(lim, p * U)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import outerbase_amd as ob
    from conftest import knots_for
    kinds = ["mat25"] * 6
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 40))
    q = int(sys.argv[1])
    for p in [int(v) for v in sys.argv[2:]]:
        em, es, cols = solve_case(om, p, q)
        ratio = float(np.max(em / allowed(em, es, cols, p)))
        print("ok" if ratio <= 1.0 and np.all(np.isfinite(em)) else "BAD", p, ratio, em.max(), es.max(), flush=True)
